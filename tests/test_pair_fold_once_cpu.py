"""Census of the fold-once path of k_mbest_step1_pair on the case table of pair_fold_once_cases.py: every case is followed
sweep by sweep with the oracle, the path rule of the kernel is restated in numpy on exact values, and the table as a whole
must take every path at least once -- so that test_gpu_pair_fold_once.py can say which paths it ran.  No GPU."""

import numpy as np
import pytest

import pair_fold_once_cases as fc
from oracle import period_oracle as po

REQUIRED = (
    "fold: m <= block",  # one column per thread
    "fold: m > block",  # two columns for some threads
    "fold: first sweep (source is the input)",
    "fold: later sweep (in place)",
    "fold: no divisor listed",
    "fold: divisors thinned from the column sums",
    "fallback: exact tie",
    "fallback: near tie",
    "fallback: divisors of a skipped top period listed",
    "fallback: two top periods",
    "fallback: short winner",
    "exact_all",
    "action 0",
    "action 1",
    "action 2",
)


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c["name"])
def test_every_case_is_admitted_and_follows_the_oracle(case):
    """No window-sweep of the case hangs on the float screen's rounding (trace raises Ambiguous otherwise), and the
    restated step 1 picks the oracle's periods."""
    x = fc.windows(case)
    for w, tr in enumerate(fc.traces(case)):
        assert tr, (case["name"], w)
        picks = []
        for rec in tr:
            if rec["action"] == 1:
                picks.append(rec["winner"])
        trc = {}
        try:
            with np.errstate(all="ignore"):
                po.m_best(x[w], case["num"], max_length=case["max_length"], min_length=case["min_length"], gamma=case["gamma"], trace=trc)
        except TypeError:  # the reference runs out of candidates (Periods.py:520/537)
            assert tr[-1]["winner"] == 0, (case["name"], w)
            continue
        assert picks == [int(p) for p in trc["step1_periods"]], (case["name"], w)


def test_the_table_takes_every_path():
    got = {}
    for case in fc.CASES:
        for label in fc.labels(case):
            got.setdefault(label, []).append(case["name"])
    for label in sorted(got):
        print(f"{label}: {got[label]}")
    missing = [label for label in REQUIRED if label not in got]
    assert not missing, missing


def test_the_lengths_reach_their_shapes():
    by = fc.BY_NAME
    # N = 1024, max_length = 341: top periods of 4 ... 6 rows on both sides of kPairSmallP, folded and not
    c = by["n1024_341"]
    ms = {rec["m"] for tr in fc.traces(c) for rec in tr if rec["path"].startswith("fold")}
    assert {fc.rows(1024, m) for m in ms} >= {4} and min(ms) > fc.K_PAIR_SMALL_P
    assert {fc.rows(1024, q) for q in range(171, 342)} == {4, 5, 6}
    assert "fallback: short winner" in fc.labels(c)
    # max_length = 700: two rows
    ms = {rec["m"] for tr in fc.traces(by["n1024_700"]) for rec in tr if rec["path"].startswith("fold")}
    assert {2} <= {fc.rows(1024, m) for m in ms} <= {2, 3}
    # N = 4096 is the only length with a top period above the block, and its batch has an odd number of windows
    for c in fc.CASES:
        assert ("fold: m > block" in fc.labels(c)) == (c["n"] == 4096), c["name"]
    assert len(by["n4096"]["windows"]) == 7
    # m_best_gamma: no cover logic, a single listed period folds
    g = fc.labels(by["n1024_341_gamma"])
    assert "fold: no divisor listed" in g and "fold: divisors thinned from the column sums" not in g


def test_the_near_ties_sit_on_both_sides_of_the_thinning_threshold():
    c = fc.BY_NAME["n1024_341"]
    x, trs = fc.windows(c), fc.traces(c)
    for kind, want, ratio in (("near:150:300:5e-10", "fallback: tie", 5e-10), ("near:150:300:2e-9", "fold: m <= block", 2e-9)):
        w = c["windows"].index(kind)
        first = trs[w][0]
        assert first["path"] == want and first["m"] == 300 and 150 in first["listed"], (kind, first)
        e_m, e_d = fc.exact_value(x[w], 300), fc.exact_value(x[w], 150)
        assert abs((e_m - e_d) / e_m - ratio) < 0.02 * ratio, (kind, (e_m - e_d) / e_m)
        assert first["winner"] == 300  # 5e-10 is far outside an fp64 tie: every kernel takes 300
    # the exact tie: an integer window of period 256 whose folds at 256 and 512 have power-of-two counts
    c = fc.BY_NAME["n1024_700"]
    w = c["windows"].index("int:256")
    first = fc.traces(c)[w][0]
    assert first["path"] == "fallback: tie" and first["lead"] == 0.0 and first["m"] == 512 and first["winner"] == 256
    assert fc.exact_value(fc.windows(c)[w], 512) == fc.exact_value(fc.windows(c)[w], 256) == float(np.sum(fc.windows(c)[w] ** 2))


def test_the_margin_rule_rejects_a_window_on_the_float_radius():
    """Two top periods 1e-6 (relative) apart are inside ten radii and outside the certain tie: not admitted."""
    n = 1024
    lo, hi = fc.pair_crossing(n)
    with pytest.raises(fc.Ambiguous):
        fc.sweep_path(fc.pair_planted(n, hi * (1 + 1e-6)), set(), 2, n // 3, False)
    assert fc.sweep_path(fc.pair_planted(n, hi * (1 + 2e-10)), set(), 2, n // 3, False)["path"] == "fallback: two top periods"
    # and the bound behind it: ten radii of the two periods are far above the 1e-9 tie and below any gap the table relies on
    assert 10 * 2 * fc.pair_radius(n, 305) < 1e-4 and fc.thin_band(n) == 5 * fc.cover_slack(n)


def test_a_long_period_is_skipped_on_the_path_and_its_divisors_meet_the_divisibility_test():
    """n500_skip: action 0 occurs on a fold-once sweep (the new update loop with nothing to store), and a skipped top period
    lists a divisor beside a top period m > kPairSmallP that it does not divide -- a list on which `m > kPairSmallP` and
    "exactly one top period" both hold, so the kernel's divisibility test alone decides."""
    tr = fc.traces(fc.BY_NAME["n500_skip"])[0]
    skipped = [rec for rec in tr if rec["action"] == 0]
    assert skipped and all(rec["path"].startswith("fold") and rec["m"] == rec["winner"] > fc.K_PAIR_SMALL_P for rec in skipped), skipped
    guard = [rec for rec in tr if rec["path"] == "fallback: divisors of a skipped top period listed"]
    assert guard
    for rec in guard:
        tops = [q for q in rec["listed"] if q > 312 // 2]
        assert tops == [rec["m"]] and rec["m"] > fc.K_PAIR_SMALL_P, rec
        assert any(rec["m"] % d for d in rec["listed"]), rec
    # every case of the table: the label never hides behind the short-winner rule only
    ms = {rec["m"] for c in fc.CASES for t in fc.traces(c) for rec in t if rec["path"] == "fallback: divisors of a skipped top period listed"}
    assert max(ms) > fc.K_PAIR_SMALL_P and min(ms) <= fc.K_PAIR_SMALL_P

