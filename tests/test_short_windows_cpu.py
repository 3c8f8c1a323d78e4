"""Census of the short-window case table (short_windows_cases.py), on the CPU: what the oracle does at every window
length from 1 to 200 -- where it raises, how far its decisions are from flipping -- and that the table contains the
lengths at which the kernels enter a code path for the first time.  test_gpu_short_windows.py runs the same table
through the library.

The raising lengths are pinned as literals; the shares of cases the margin rule leaves out of the period comparison
are CONDITIONS (at most 2 % for float64 input, 10 % for float32 input, per op); every figure is printed."""

import numpy as np
import pytest

import short_windows_cases as sw

ALL = list(sw.DENSE)
# lengths at which the oracle raises, per op and window kind (d: zeros, e: constant raise wherever the op needs a
# second pick from a residual that is exactly zero); default parameters of sw.CENSUS
RAISING = {
    "m_best": {"a": list(range(1, 12)), "b": list(range(1, 12)), "c": list(range(1, 12)), "d": ALL, "e": ALL},
    "m_best_gamma": {"a": list(range(1, 12)), "b": list(range(1, 12)), "c": list(range(1, 12)), "d": ALL, "e": ALL},
    "small_to_large": {"a": [], "b": [], "c": [], "d": [], "e": []},
    "best_correlation": {"a": list(range(1, 9)) + [10], "b": list(range(1, 9)), "c": list(range(1, 9)), "d": ALL, "e": ALL},
    "best_frequency": {
        "a": [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 19, 22, 23, 33, 48, 55, 66, 71, 75, 80, 83, 94, 97, 100, 111, 137, 161,
              175],
        "b": [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13],
        "c": [1, 2, 3, 4, 5, 6, 7, 8, 11, 13, 18, 19, 20, 21, 26, 30, 36, 42, 51, 65, 81, 85, 95, 104, 106, 110, 111, 116, 138,
              153, 154, 161, 171, 180, 182],
        "d": ALL, "e": ALL,
    },
    "qo_find_periods": {"a": [], "b": [], "c": [], "d": [], "e": []},
}


def _lengths(name, dtype):
    lens = sw.DENSE if dtype == np.float64 else sw.FLAGS
    return [n for n in lens if not (name == "qo_find_periods" and n < 6)]


@pytest.mark.parametrize("name", list(sw.CENSUS))
def test_where_the_oracle_raises(name):
    for kind in sw.KINDS:
        got = [n for n in _lengths(name, np.float64) if sw.census_ref(name, n, kind)[0].startswith("raises")]
        if kind in "abc":
            print(f"{name} ({kind}): the oracle raises at N = {got}")
        assert got == RAISING[name][kind], (name, kind)


@pytest.mark.parametrize("name", list(sw.CENSUS))
def test_share_of_cases_without_a_clear_margin(name):
    """Windows (a)-(c): the dense set in float64 at 1e-9, the flag subset rounded to float32 at 1e-3."""
    for dtype, bar, cap in ((np.float64, sw.MARGIN64, sw.CAP64), (np.float32, sw.MARGIN32, sw.CAP32)):
        margins = []
        for n in _lengths(name, dtype):
            for kind in "abc":
                st, _, m = sw.census_ref(name, n, kind, dtype)
                if st == "ok":
                    margins.append((m, n, kind))
        out = [c for c in margins if c[0] < bar]
        print(f"{name} {np.dtype(dtype).name}: {len(out)} of {len(margins)} cases below {bar:g} "
              f"({100 * len(out) / len(margins):.2f} %, cap {100 * cap:g} %): {[(n, k) for _, n, k in out]}")
        assert len(out) <= cap * len(margins), (name, dtype)


FLAG_SETS = ((True, False), (False, True), (True, True))
SECOND = ("m_best", "m_best_gamma", "m_best_mid", "m_best_mid_gamma", "small_to_large", "best_correlation", "best_frequency")


def _share(op, cases, dtype, bar):
    """(cases answered, of them below `bar`) over windows (a)-(c); cases: (n, kwargs)."""
    margins = [m for n, kw in cases for kind in "abc" for st, _, m in [sw.ref(op, n, kind, dtype, **kw)] if st == "ok"]
    return len(margins), sum(m < bar for m in margins)


@pytest.mark.parametrize("name", SECOND)
def test_share_without_a_clear_margin_second_parameter_sets(name):
    """The further parameter sets of the GPU file under the same caps: float64 on the dense set, float32 on the subset.
    One set is exempt and pinned instead: m_best with min_length=1, max_length=N-1 without gamma.  Once period N - 1 is
    taken the residual is two spikes, every p > N / 2 then has the same norm, and the oracle's step-1 gap is exactly 0 --
    more than 90 % of its cases are ties whatever the windows are, so no seed meets the cap.  The GPU test holds its rows to
    status, to the oracle's values wherever the list agrees and to a replay where it does not, and runs the set
    "m_best_mid" (min_length=2, max_length=N // 2: the same first periods of 64 and more, at N = 128) under the cap."""
    op = "m_best" if name.startswith("m_best") else name
    gamma = dict(gamma=name.endswith("gamma")) if op == "m_best" else {}
    key = name[:-6] if name.endswith("_gamma") and name != "m_best_gamma" else name
    for dtype, lens, bar, cap in ((np.float64, sw.DENSE, sw.MARGIN64, sw.CAP64), (np.float32, sw.FLAGS, sw.MARGIN32, sw.CAP32)):
        cases = [(n, {**sw.second_set(key, n), **gamma}) for n in lens if sw.second_set(key, n) is not None]
        tot, low = _share(op, cases, dtype, bar)
        print(f"{name} second set {np.dtype(dtype).name}: {low} of {tot} cases below {bar:g} ({100 * low / tot:.2f} %)")
        if name == "m_best":
            assert low >= 0.8 * tot, (low, tot)  # the set of ties
        else:
            assert low <= cap * tot, (name, dtype, low, tot)


@pytest.mark.parametrize("name", ["m_best", "m_best_gamma", "small_to_large", "best_correlation", "best_frequency"])
def test_share_without_a_clear_margin_under_the_flags(name):
    """trunc, orth and both with the default parameters on the flag subset, float64 and float32, under the same caps."""
    op = "m_best" if name == "m_best_gamma" else name
    for dtype, bar, cap in ((np.float64, sw.MARGIN64, sw.CAP64), (np.float32, sw.MARGIN32, sw.CAP32)):
        cases = [(n, dict(sw.CENSUS[name], trunc=t, orth=o)) for n in sw.FLAGS for t, o in FLAG_SETS]
        tot, low = _share(op, cases, dtype, bar)
        print(f"{name} flags {np.dtype(dtype).name}: {low} of {tot} cases below {bar:g} ({100 * low / tot:.2f} %)")
        assert low <= cap * tot, (name, dtype, low, tot)


def test_windows_are_what_the_table_says():
    for n in (1, 2, 7, 64, 200):
        x = sw.windows(n)
        assert x.shape == (5, n) and not x[3].any() and np.all(x[4] == sw.CONST)
        assert np.array_equal(sw.windows(n, np.float32), x.astype(np.float32))
        q = max(2, n // 4)
        if n > 2 * q:  # (c) is periodic up to its noise
            assert np.abs(x[2][q:] - x[2][:-q]).max() < 6 * 0.2 * np.sqrt(2) + 1e-12
    assert set(sw.FLAGS) <= set(sw.DENSE) and len(sw.DENSE) == 200
    # k copies of the constant add up exactly: its projections are exact and the residual after the first is exactly zero
    assert all(float(np.sum(np.full(k, sw.CONST))) == k * sw.CONST for k in range(1, 201))


def test_first_entry_lengths_are_in_the_table():
    """The lengths at which a kernel path is entered for the first time, from the defaults' arithmetic on N
    (n_periods = N // 2, max_length = N // 3, the Ramanujan ranges of the GPU test: q_hi = N // 2 and N // 3)."""
    first = {
        "n_periods >= 64 (small_to_large)": min(n for n in range(1, 1000) if n // 2 >= 64),
        "max_length - 1 >= 64 (best_correlation)": min(n for n in range(1, 1000) if n // 3 - 1 >= 64),
        "max_length >= 64 (m_best)": min(n for n in range(1, 1000) if n // 3 >= 64),
        "q_hi >= 64 (ramanujan, q_hi = N // 2)": min(n for n in range(1, 1000) if n // 2 >= 64),
        "q_hi >= 64 (ramanujan, q_hi = N // 3)": min(n for n in range(1, 1000) if n // 3 >= 64),
        "max_length >= 64 with max_length = N - 1": 65,
    }
    print("first-entry lengths:", first)
    assert first == {"n_periods >= 64 (small_to_large)": 128, "max_length - 1 >= 64 (best_correlation)": 195,
                     "max_length >= 64 (m_best)": 192, "q_hi >= 64 (ramanujan, q_hi = N // 2)": 128,
                     "q_hi >= 64 (ramanujan, q_hi = N // 3)": 192, "max_length >= 64 with max_length = N - 1": 65}
    for name, n in first.items():
        assert n in sw.DENSE and n - 1 in sw.DENSE, name  # the length before the entry too
    assert {128, 192} <= set(sw.FLAGS)
    assert any(n < 64 for n in sw.DENSE) and {63, 64, 65} <= set(sw.FLAGS)
    # fewer periods than the 16 wavefronts of the queue kernel: n_periods = N // 2 < 16
    few = [n for n in sw.DENSE if n // 2 < 16]
    print("n_periods below 16 wavefronts at N =", few[0], "...", few[-1])
    assert few == list(range(1, 32)) and set(range(1, 25)) | {31} <= set(sw.FLAGS)


def test_picks_on_rounding_noise():
    """Cases in which a later pick of best_correlation or qo_find_periods runs on the rounding noise of an exactly fitted
    window (sw.noisy): at these lengths the range holds too few periods for `num` picks.  They are left out of the period
    comparison beside the margin rule, and pinned here so that the set cannot grow unnoticed."""
    want = {
        "qo_find_periods": [(n, k) for n in range(6, 15) for k in "abc" if (n, k) not in ((13, "a"), (13, "b"))],
    }
    # best_correlation, N = 9 .. 11 (max_length = 3: period 2 alone): whether the second round finds sums of 1e-17 or
    # exact zeros (then the oracle raises, "raises late") differs between the float64 window and its float32 rounding
    bc = {np.float64: [(9, "a"), (9, "b"), (9, "c"), (10, "b"), (10, "c"), (11, "a"), (11, "b"), (11, "c")],
          np.float32: [(9, "b"), (9, "c"), (10, "a"), (10, "b"), (10, "c"), (11, "a"), (11, "b"), (11, "c")]}
    for dtype in (np.float64, np.float32):
        want["best_correlation"] = bc[dtype]
        for name in want:
            got = [(n, k) for n in _lengths(name, dtype) for k in "abc" if sw.census_ref(name, n, k, dtype, fn=sw.noisy)]
            print(f"{name} {np.dtype(dtype).name}: picks on rounding noise at", got)
            assert got == want[name], (name, dtype)


def test_m_best_picks_on_rounding_noise():
    """m_best over all three parameter sets of the GPU file: the cases in which a step-1 winner of the oracle has a norm at
    the rounding noise of an exactly fitted window (the range holds too few periods for three picks, so a period that
    is already exhausted wins again with 1e-17).  Whether the reference then returns or raises hangs on that noise; the
    GPU test accepts a status for these rows, and they are pinned here."""
    want = {False: [("mid", 8, "a"), ("default", 12, "a"), ("default", 12, "b"), ("default", 12, "c"), ("default", 13, "c"),
                    ("default", 14, "a"), ("default", 14, "c")],
            True: [("default", 12, "a"), ("default", 12, "b"), ("default", 12, "c"), ("default", 13, "c")]}
    for dtype, lens in ((np.float64, sw.DENSE), (np.float32, sw.FLAGS)):
        for gamma in (False, True):
            got = []
            for n in lens:
                for tag, kw in (("default", dict(num=3)), ("wide", sw.second_set("m_best", n)), ("mid", sw.second_set("m_best_mid", n))):
                    if kw is not None:
                        got += [(tag, n, k) for k in "abc" if sw.noisy("m_best", n, k, dtype, **{**kw, "gamma": gamma})]
            print(f"m_best gamma={gamma} {np.dtype(dtype).name}: step-1 picks on rounding noise at", got)
            assert got == want[gamma], (dtype, gamma)
