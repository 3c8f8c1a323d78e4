"""The best_correlation census on the CPU: what tests/bc_cases.py reaches, and what its expected values rest on.

k_best_correlation and k_best_correlation_pair (ph_bc.h) pick the code of a round by the plan variant, by the pass that
produces a period, by how many periods the screen lists (kCandCap = 256 and three ballot trips in the one-window kernel,
kPairListCap = 96 in the pair kernel), by whether the float image of the pair kernel can be screened at all, whether it
went stale, and by the status of the window and of its partner.  bc_cases restates them; `test_table_reaches_every_class`
asserts that the table reaches every label of bc_cases.CLASSES and that every case reaches what its entry claims, and
prints every label with the cases that reach it (-s).

Expected values: the reference's own answers where the table names a fixture tag (tests/golden/best_correlation_edges.npz:
the non-finite, scaled, impulse, near-tie and max_length windows), the oracle's everywhere.  The oracle passes over NaN
column sums like the reference's strict '>' does: on a window with one NaN or Inf sample it returns zeros, where
np.argmax alone would have picked the NaN and raised.

Measured: 64 cases (131 windows), 37 labels; this module 3 s.  The margin rule leaves out 0 of the float64 windows and 0
of the float32 ones (smallest lead of a window that is not exact: 3.0e-8, the planted near ties); the 18 exact windows
have leads of 0 (ties) and 2^-51 and are compared whatever the rule says.
"""

import collections
import os

import numpy as np
import pytest

import bc_cases as bc
from oracle import period_oracle as po

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "best_correlation_edges.npz")


@pytest.fixture(scope="module")
def fixture():
    return bc.load_fixture(GOLDEN)


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


def test_table_reaches_every_class():
    carriers = collections.defaultdict(list)
    for case in bc.CASES:
        labels = bc.classify(case)
        missing = [c for c in case["claims"] if c not in labels]
        assert not missing, (case["name"], "does not reach what its entry claims", missing)
        for label in labels:
            carriers[label].append(case["name"])
    for label in bc.CLASSES:
        names = carriers[label]
        print(f"{len(names):3d}  {label}: {', '.join(names)}")
    assert not set(carriers) - set(bc.CLASSES), set(carriers) - set(bc.CLASSES)
    missing = [label for label in bc.CLASSES if not carriers[label]]
    assert not missing, missing
    assert len(set(bc.CLASSES)) == len(bc.CLASSES)
    # no window that is the only carrier of a label is left out of the period comparison
    for label in bc.CLASSES:
        if len(carriers[label]) == 1:
            case = bc.BY_NAME[carriers[label][0]]
            assert all(bc.admitted(case, w) for w in range(len(case["kinds"]))), (label, case["name"])
    assert max(c["n"] for c in bc.CASES) <= 1024 and max(len(c["kinds"]) for c in bc.CASES) <= 9


def test_margin_rule_caps():
    """Period lists are compared at a lead of MARGIN64 / MARGIN32 and more; the share of windows left out stays under
    CAP64 / CAP32.  Exact windows are never left out.  Every window whose smallest lead is below 1e-6 is reported."""
    for dtype, cap in ((np.float64, bc.CAP64), (np.float32, bc.CAP32)):
        wins = [(c, w) for c in bc.CASES if c["dtype"] == dtype for w in range(len(c["kinds"]))]
        out = [(c["name"], w) for c, w in wins if not bc.admitted(c, w)]
        inexact = [bc.ref(c)[w]["margin"] for c, w in wins if not c["exact"][w] and bc.ref(c)[w]["rounds"]]
        print(f"{np.dtype(dtype).name}: {len(out)} of {len(wins)} windows left out {out}, smallest margin of an inexact window {min(inexact):.2e}")
        assert len(wins) >= 4 and len(out) <= cap * len(wins), (np.dtype(dtype).name, out)
        assert not any(c["exact"][w] for c, w in wins if not bc.admitted(c, w))
    for c in bc.CASES:
        for w, r in enumerate(bc.ref(c)):
            if r["rounds"] and r["margin"] < 1e-6:
                how = "exact arithmetic" if c["exact"][w] else "knife edge of the ratio" if c["knife"] else "margin rule"
                print(f"{c['name']}[{w}] {c['kinds'][w]}: leads {[float('%.3g' % rd['lead']) for rd in r['rounds']]} "
                      f"ties {[len(rd['ties']) for rd in r['rounds']]} margin {r['margin']:.2e} ({how})")


def test_rounds_are_the_oracle():
    """bc_cases.rounds restates the oracle's loop with more bookkeeping: same periods, norms and bases bit for bit, and
    TypeError exactly where it reports a round without a period."""
    for case in bc.CASES:
        x = bc.windows(case).astype(np.float64)
        for w, r in enumerate(bc.ref(case)):
            kw = dict(num=case["num"], max_length=bc.max_length_of(case), ratio=case["ratio"], trunc=case["trunc"], orth=case["orth"])
            if r["raised"] is not None:
                with pytest.raises(TypeError):
                    po.best_correlation(x[w], **kw)
                continue
            per, nr, bs = po.best_correlation(x[w], **kw)
            assert np.array_equal(per, r["periods"]) and np.array_equal(nr, r["norms"]) and np.array_equal(bs, r["bases"]), (case["name"], w)


def test_oracle_equals_the_fixture(fixture):
    seen = set()
    for case in bc.CASES:
        for w, tag in enumerate(case["fixture"]):
            if tag is None:
                continue
            seen.add(tag)
            f, r = fixture[tag], bc.ref(case)[w]
            assert np.array_equal(f[-1], bc.windows(case)[w].astype(np.float64), equal_nan=True), tag
            if f[0] == "raises":
                assert f[1] == "TypeError" and r["raised"] is not None, tag
                continue
            assert r["raised"] is None and np.array_equal(f[1], r["periods"]), (tag, f[1], r["periods"])
            assert np.max(np.abs(f[2] - r["norms"])) <= bc.TOL * np.max(np.abs(f[2]), initial=0.0), tag
            assert np.max(np.abs(f[3] - r["bases"])) <= bc.TOL * np.max(np.abs(f[3]), initial=0.0), tag
    assert seen == set(fixture) and len(seen) >= 30
    # what the reference does with the degenerate windows
    for k in bc.ZEROS_REF + ("2^510",):
        f = fixture["deg_" + k]
        assert f[0] == "ok" and not f[1].any() and not f[2].any() and not f[3].any(), k
    for k in bc.RAISES_REF:
        assert fixture["deg_" + k][:2] == ("raises", "TypeError"), k
    for k in ("2^400", "2^-400", "2^-530"):
        assert list(fixture["deg_" + k][1]) == list(fixture["deg_2^400"][1]) and np.all(fixture["deg_" + k][1] != 0), k
    assert all(fixture[f"ml2_w{w}"][0] == "raises" for w in range(3)) and all(fixture[f"ml3_w{w}"][0] == "ok" for w in range(3))
    for name, _, _, _ in bc.NEARTIES:
        assert fixture[name][0] == "ok" and np.array_equal(fixture[name][2], bc.ref(bc.BY_NAME[name])[0]["norms"]), name  # bit for bit
        assert np.array_equal(fixture[name][3], bc.ref(bc.BY_NAME[name])[0]["bases"]), name


def test_nan_sums_are_passed_over_and_trace_is_unchanged():
    case = bc.BY_NAME["deg_nan_second"]
    x = bc.windows(case)
    per, nr, bs = po.best_correlation(x[1])
    assert not per.any() and not nr.any() and not bs.any()
    tr_a, tr_b = [], []
    a = po.best_correlation(x[0], trace=tr_a)
    b = po.best_correlation(x[0])
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and len(tr_a) == 5
    r = bc.rounds(x[0], 5, len(x[0]) // 3, 0.01)[0]
    for (lead, gap, best), rd in zip(tr_a, r):
        assert best == rd["best"] and lead == rd["lead"] and gap == abs(rd["gain"] - 0.01)
    assert tr_b == []


def test_exact_windows_are_exact():
    """Impulse and near-tie windows: every class sum of every compared round is exact in fp64 in any order, and every base
    is the correctly rounded quotient of exact numbers (Fraction arithmetic).  The impulse's round 0 is a tie of ALL
    periods, its round 1 another tie; the near ties lead by 2^-51."""
    n = 0
    for case in bc.CASES:
        for w, exact in enumerate(case["exact"]):
            if not exact:
                continue
            n += 1
            r = bc.ref(case)[w]
            assert r["raised"] is None and len(r["rounds"]) == case["num"] and all(bc.exact_rounds(case, w)), (case["name"], w)
            P = bc.max_length_of(case) - 2
            if case["kinds"][w].startswith("impulse:"):
                assert r["rounds"][0]["ties"] == list(range(2, P + 2)) and r["rounds"][0]["best"] == 1.0 and r["periods"][0] == 2
                if case["num"] == 2:
                    assert len(r["rounds"][1]["ties"]) >= 4 and r["periods"][1] == min(r["rounds"][1]["ties"]) > 2
            else:
                assert 2.0 ** -52 < r["rounds"][0]["lead"] <= 2.0 ** -51 and r["rounds"][0]["best"] == 2.0 + bc.EPS and r["periods"][0] != 0
    assert n == 18
    # the counts either side of the caps
    got = {c["name"]: bc.one_ncand_exact(bc.ref(c)[0]["rounds"][0], bc.max_length_of(c) - 2) for c in bc.CASES if c["name"].startswith("impulse_")}
    assert got == {"impulse_pair_98": 96, "impulse_pair_99": 97, "impulse_one_66": 64, "impulse_one_258": 256, "impulse_one_259": 257}
    assert bc.K_PAIR_LIST_CAP == 96 and bc.K_CAND_CAP == 256
    # winners by producer: 179 alone, 101 with 202, 67 with 134 and 268, 61 in a chain / on its own; the mirror's 2
    want = {"neartie_179": (179, "m = 1", "m = 1"), "neartie_m2": (101, "m = 2", "m = 2"), "neartie_m4": (67, "m = 4", "m = 4"),
            "neartie_short": (61, "chain", "m = 0"), "neartie_mirror": (2, "chain", "m = 0")}
    for name, (p, pair, one) in want.items():
        assert bc.ref(bc.BY_NAME[name])[0]["periods"][0] == p
        assert bc.build_plan(2, 340, True)[p] == pair and bc.build_plan(2, 340, False)[p] == one


def test_planted_near_ties():
    seeds = bc.tie2_seeds()
    assert len(seeds) == 8
    up = 0
    for s in seeds:
        y, p1, p2, lead = bc.planted_near_tie(s)
        tr = []
        per, _, _ = po.best_correlation(y, num=1, max_length=bc.TIE2_ML, ratio=0.0, trace=tr)
        assert per[0] == p2 != p1 and p1 % p2 and p2 % p1 and 1e-8 <= tr[0][0] <= 1e-7 and tr[0][0] == lead, (s, per, tr)
        up += p2 > p1
        print(f"seed {s}: {p1} -> {p2}, lead {lead:.3e}")
    assert 3 <= up <= 5


def test_collapse_rounds():
    """Round 0 takes p0 with a gain of 1 - 1e-11, every sum of it exact (integers below 2^53); the residual is then 2^-36
    of the window, which makes the float image stale, and rounds 1 and 2 are kept with gains of 1e-12."""
    for p0 in (2, 8, 64):
        case = bc.BY_NAME[f"collapse_{p0}"]
        r = bc.ref(case)[0]
        assert bc.sums_exact(bc.windows(case)[0], bc.max_length_of(case))
        rd = r["rounds"]
        assert rd[0]["p"] == p0 and 1 - 1e-10 < rd[0]["gain"] < 1 and rd[0]["lead"] > 0.1
        assert bc.stale(rd[0]["after_rsq"], bc.pick_scale(rd[0]["rsq"], case["n"]), case["n"]) and rd[1]["rmax"] < 2.0 ** -30 * rd[0]["rmax"]
        assert all(p != 0 for p in r["periods"]) and all(1e-13 < g < 1e-11 for g in r["norms"][1:]) and r["margin"] > 1e-3


def test_knife_edges():
    for i in range(len(bc.KNIFE_SOURCES)):
        kept, rej = bc.ref(bc.BY_NAME[f"knife_{i}_kept"])[0], bc.ref(bc.BY_NAME[f"knife_{i}_rejected"])[0]
        g = kept["rounds"][0]["gain"]
        assert kept["periods"][0] == kept["rounds"][0]["p"] != 0 and kept["norms"][0] == g
        assert rej["periods"][0] == 0 and not rej["bases"][0].any() and rej["rounds"][0]["gain"] == g
        assert np.any(rej["periods"][1:] != 0)  # the residual was reduced all the same, and a later round is kept
        assert np.array_equal(rej["rounds"][1]["base"], kept["rounds"][1]["base"])  # on the same residual
        assert rej["norms"][1] != kept["norms"][1]  # measured from the norm before the rejected pick
        assert 0.5e-9 < abs(bc.BY_NAME[f"knife_{i}_kept"]["ratio"] - g) / g < 2e-9


def test_restatements():
    f64, f32, E = np.float64, np.float32, bc.ENGINES
    assert bc.plan_variant(f64, False, 1024, 341) == "pair" and bc.plan_variant(f32, False, 1024, 341) == "one"
    assert bc.plan_variant(f64, True, 1024, 341) == "one" and bc.plan_variant(f64, False, 1024, 341, E["one"]) == "one"
    assert bc.plan_variant(f64, False, 130, 2) == "one" and bc.plan_variant(f64, False, 130, 3) == "pair"
    assert bc.plan_variant(f64, False, 130, 130) == "pair" and bc.plan_variant(f64, False, 130, 131) == "one"
    assert all(bc.plan_variant(f64, False, 1024, 341, E[k]) == "one" for k in ("one", "one256", "hbm"))
    assert bc.pair_lds_bytes(1024) == 2 * 8 * 1280 + 256 + 128 + 64 + 768 + 32 + 80
    for chains in (False, True):
        for hi in (2, 3, 63, 64, 65, 97, 128, 257, 340, 399):
            plan = bc.build_plan(2, hi, chains)
            assert sorted(plan) == list(range(2, hi + 1)), (chains, hi)  # every period once
            assert all((v == "chain") == (chains and p <= 64) and (v == "m = 0") == (not chains and p < 64) for p, v in plan.items())
    plan = bc.build_plan(2, 340, True)
    assert plan[65] == plan[130] == plan[260] == "m = 4" and plan[86] == plan[172] == "m = 2" and plan[171] == "m = 1"
    assert bc.build_plan(2, 340, False)[64] == "m = 4"  # 64 itself is no row-split pass without the chains
