"""m_best through the window-pair screen with shared-load passes (pair_pass_duo in ph_pair.h): a period p with 3 ... 6
rows is folded together with p + 64 from one set of LDS reads where both have the same row count.

Three engines -- shared loads on (default), off (PH_PAIR_DUO=0: one pass per period, the kernel as it was) and the
one-window fp64 kernel (PH_STEP1_PAIR=0) -- must give identical periods, status and sweep counts and bit-identical bases,
powers within 1e-13 of each other; against the oracle periods equal, powers and bases within 1e-10 (the inputs are sums
of sinusoids and planted periodic components, whose picks lie far above rounding noise).
"""

import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch

pytestmark = pytest.mark.gpu
TOL = 1e-10  # against the oracle
KTOL = 1e-13  # powers, kernel against kernel (test_gpu_cover.py)
W = 5  # one workgroup has a missing partner


def _engine(**env):
    from pyperiod_amd import PeriodEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return PeriodEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge

    ge.build()
    duo = _engine(PH_STEP1_PAIR="1", PH_PAIR_DUO="1")
    off = _engine(PH_STEP1_PAIR="1", PH_PAIR_DUO="0")
    single = _engine(PH_STEP1_PAIR="0")
    yield duo, off, single
    for e in (duo, off, single):
        e.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _np(out):
    return [o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in out]


def _same(a, b, what):
    """periods, status, sweeps identical; bases bit for bit; powers within KTOL."""
    ok = a[3] == 0  # (what a window whose step 1 failed leaves in its rows is no contract)
    print(what, "periods", np.array_equal(a[0], b[0]), "status", np.array_equal(a[3], b[3]), "sweeps", np.array_equal(a[4], b[4]),
          "bases", np.array_equal(a[2][ok], b[2][ok]), "powers rel", rel_err(b[1][ok], a[1][ok]) if ok.any() else None)
    assert np.array_equal(a[0], b[0]), (what, np.nonzero((a[0] != b[0]).any(1))[0][:10])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), what
    assert np.array_equal(a[2][ok], b[2][ok]), what
    assert not ok.any() or rel_err(b[1][ok], a[1][ok]) < KTOL, what


def _three(engines, x, what, oracle_rows=(0,), **kw):
    duo, off, single = engines
    a = _np(duo.m_best(x, want_sweeps=True, **kw))
    b = _np(off.m_best(x, want_sweeps=True, **kw))
    c = _np(single.m_best(x, want_sweeps=True, **kw))
    _same(b, a, f"{what} duo/off")
    _same(c, a, f"{what} duo/one-window")
    okw = {k: v for k, v in kw.items() if k != "num"}
    for w in oracle_rows:
        want = po.m_best(x[w], kw.get("num", 5), **okw)
        assert a[3][w] == 0 and np.array_equal(a[0][w].astype(np.int64), np.asarray(want[0]).astype(np.int64)), (what, w, a[0][w], want[0])
        assert rel_err(a[1][w], want[1]) < TOL and rel_err(a[2][w], want[2]) < TOL, (what, w)
    return a


def _rows(n, p):
    return -(-n // p)


def _plan(n, lo, hi):
    """The pairing rule of the host plan over the screened periods [lo, hi]: -> (bases of shared passes, singles)."""
    covered, duo, single = set(), [], []
    for p in range(lo, hi + 1):
        if p in covered:
            continue
        r = _rows(n, p)
        if p >= 64 and p + 64 <= hi and 3 <= r <= 6 and -(-p // 64) > r and _rows(n, p + 64) == r:
            covered.add(p + 64)
            duo.append(p)
        else:
            single.append(p)
    return duo, single


def test_screen_info(engines):
    duo, off, single = engines
    assert duo.m_best_info(4096, 10) == (2, 8) and off.m_best_info(4096, 10) == (2, 8) and single.m_best_info(4096, 10) == (1, 8)
    # what bench.py multiplies by stays the number of periods folded
    assert duo.m_best_plan_info(4096, 10) == (683, 1364) and off.m_best_plan_info(4096, 10) == (683, 1364)
    ent, scr, elems = duo.m_best_screen_info(4096, 10)
    ent0, scr0, elems0 = off.m_best_screen_info(4096, 10)
    print("screen info: duo", (ent, scr, elems), "single passes", (ent0, scr0, elems0), "ratio", elems / elems0)
    assert (ent0, scr0) == (683, 683) and elems0 == 64 * 45281
    assert scr == 683 and ent <= 393 and elems <= 0.65 * elems0
    pairs, singles = _plan(4096, 683, 1365)
    assert ent == len(pairs) + len(singles) == 393
    # m_best_gamma runs the full plan; its few-row singles are paired by the same rule
    g_ent, g_scr, g_el = duo.m_best_screen_info(4096, 10, gamma=True)
    g_ent0, g_scr0, g_el0 = off.m_best_screen_info(4096, 10, gamma=True)
    assert g_scr == g_scr0 == 1364 and g_ent < g_ent0 and g_el < g_el0
    # a screened range shorter than 64 has no pair
    assert duo.m_best_screen_info(4096, 10, max_length=100) == off.m_best_screen_info(4096, 10, max_length=100)


@pytest.mark.parametrize("n", [1000, 1200, 4095, 4096, 4097])
def test_window_lengths(engines, n):
    pairs, _ = _plan(n, (n // 3) // 2 + 1, n // 3)
    assert pairs, n  # the default range has shared passes at every one of these lengths
    x = multi_sinusoid_batch(300 + n, W, n)
    _three(engines, x, f"N={n}", oracle_rows=(4,), num=4)


@pytest.mark.parametrize("lo,hi,npairs", [
    (2, 100, 0),        # screened range 51 ... 100: shorter than 64, no pair
    (1301, 1365, 1),    # exactly 65 long: the one pair 1301 / 1365, which ends at nfull = 1
    (780, 900, None),   # crosses the row classes 6 | 5 at 819 / 820
    (990, 1100, None),  # crosses 5 | 4 at 1023 / 1024 and contains 1024 (nfull = q, no short part)
    (1024, 1088, 1),    # base 1024 itself
    (2, 2047, None),    # three-row periods (1366 ... 2047) in pairs next to singles
])
def test_period_ranges(engines, lo, hi, npairs):
    n = 4096
    scr = max(lo, hi // 2 + 1)
    pairs, singles = _plan(n, scr, hi)
    if npairs is not None:
        assert len(pairs) == npairs, pairs
    assert engines[0].m_best_screen_info(n, 4, max_length=hi, min_length=lo)[0] == len(pairs) + len(singles)
    rng = np.random.default_rng(lo + hi)
    t = np.arange(n)
    mid = (scr + hi) // 2
    x = np.stack([2.0 * rng.standard_normal(hi)[t % hi] + 1.5 * rng.standard_normal(mid)[t % mid] +
                  1.0 * rng.standard_normal(scr)[t % scr] + 0.1 * rng.standard_normal(n) for _ in range(W)])
    _three(engines, x, f"range {lo}..{hi}", oracle_rows=(0,), num=3, min_length=lo, max_length=hi)


def test_winners_from_both_outputs_of_one_pass(engines):
    """Periodic components planted at the base AND at the partner of one shared pass (1160 and 1224 at N = 4096: rows 4,
    1152 ... 1215 are bases), in either order of strength, and at a pair of the five- and six-row classes."""
    n = 4096
    pairs, _ = _plan(n, 683, 1365)
    rng = np.random.default_rng(8)
    t = np.arange(n)
    rows = []
    for q, wa, wb in ((1160, 3.0, 2.0), (1160, 2.0, 3.0), (830, 3.0, 2.0), (700, 2.0, 3.0), (1301, 2.0, 3.0)):
        assert q in pairs
        rows.append(wa * rng.standard_normal(q)[t % q] + wb * rng.standard_normal(q + 64)[t % (q + 64)] + 0.05 * rng.standard_normal(n))
    x = np.stack(rows)
    a = _three(engines, x, "planted pairs", oracle_rows=(0, 1, 3), num=3)
    for w, q in enumerate((1160, 1160, 830, 700, 1301)):
        assert {q, q + 64} <= set(a[0][w].tolist()), (w, a[0][w])
    assert a[0][0][0] == 1160 and a[0][1][0] == 1224


def test_gamma(engines):
    duo, off, single = engines
    for n, kw in ((4096, dict(num=5)), (1200, dict(num=4))):
        x = multi_sinusoid_batch(80 + n, W, n)
        a = _np(duo.m_best(x, gamma=True, want_sweeps=True, **kw))
        b = _np(off.m_best(x, gamma=True, want_sweeps=True, **kw))
        c = _np(single.m_best(x, gamma=True, want_sweeps=True, **kw))
        _same(b, a, f"gamma N={n} duo/off")
        _same(c, a, f"gamma N={n} duo/one-window")
        want = po.m_best(x[0], kw["num"], gamma=True)
        assert np.array_equal(a[0][0], want[0]) and rel_err(a[1][0], want[1]) < TOL and rel_err(a[2][0], want[2]) < TOL
    # m_best and m_best_gamma in alternation on one context: each gets its own plan
    x = multi_sinusoid_batch(3, W, 4096)
    first = [_np(duo.m_best(x, 4, gamma=g, want_sweeps=True)) for g in (False, True)]
    for g in (False, True):
        again = _np(duo.m_best(x, 4, gamma=g, want_sweeps=True))
        for k in range(5):
            assert np.array_equal(again[k], first[int(g)][k]), (g, k)


def test_a_window_of_zeros(engines):
    x = multi_sinusoid_batch(17, W, 4096)
    x[1] = 0.0  # shares its workgroup with window 0
    a = _three(engines, x, "zeros in window 1", oracle_rows=(0, 2), num=4)
    assert a[3][1] == 1 and (a[3][[0, 2, 3, 4]] == 0).all()
