"""ph_period_path / ShortTime.period_map / ShortTime.contour without a GPU: the numpy restatement that
tests/test_gpu_period_path.py holds k_period_path to (tests/period_path_cases.py) against an exhaustive search, its
tie-break order, forbidden entries and band width; what the path buys on the glide signal of the issue; the new C-ABI
symbols, every refusal of the entry point and the argument errors of period_map / contour."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from period_path_cases import (PH_ST_NO_PERIOD, PH_ST_OK, brute_force, glide_signal, period_path_ref, random_cost,
                               tie_cost, with_dead_frame, with_forbidden)


# ------------------------------------------------------------------ the restatement against all paths
@pytest.mark.parametrize("band", [0, 1, 2, 3])
def test_restatement_against_exhaustive_search(band):
    """Integer costs and dyadic jumps: every sum is exact, so the scores must be equal, and the paths wherever the
    optimum is unique."""
    unique = 0
    for W in range(1, 6):
        for P in range(1, 5):
            for seed, jump in ((0, 0.0), (1, 0.25), (2, 0.5), (3, 2.0)):
                c = np.random.default_rng(1000 * W + 100 * P + 10 * band + seed).integers(-4, 5, (W, P)).astype(np.float64)
                if seed == 3 and W * P > 2:
                    c = with_forbidden(c, seed + W + P, frac=0.3)
                want, paths = brute_force(c, band, jump)
                path, values, score, status = period_path_ref(c, band, jump)
                assert score == want, (W, P, band, jump)
                if not paths:
                    assert status == PH_ST_NO_PERIOD and np.all(path == -1) and np.all(values == 0.0)
                    continue
                assert status == PH_ST_OK and tuple(path) in paths
                assert np.array_equal(values, c[np.arange(W), path])
                if len(paths) == 1:
                    unique += 1
                    assert tuple(path) == paths[0]
    assert unique >= 10  # (the comparison of paths is not vacuous)


def test_tie_break_order():
    # every candidate ties: the state stays, and the end state is the lowest
    path, _, score, _ = period_path_ref(np.ones((4, 5)), 2, 0.0)
    assert path.tolist() == [0, 0, 0, 0] and score == 4.0
    # -1 before +1
    path, _, _, _ = period_path_ref(np.array([[0, 1, 0, 1, 0], [0, 0, 5, 0, 0.0]]), 1, 0.0)
    assert path.tolist() == [1, 2]
    # stay before -1 and +1
    path, _, _, _ = period_path_ref(np.array([[0, 1, 1, 1, 0], [0, 0, 5, 0, 0.0]]), 1, 0.0)
    assert path.tolist() == [2, 2]
    # -1 before -2 and +2; -2 before +2
    path, _, _, _ = period_path_ref(np.array([[1, 1, 0, 0, 1], [0, 0, 5, 0, 0.0]]), 2, 0.0)
    assert path.tolist() == [1, 2]
    path, _, _, _ = period_path_ref(np.array([[1, 0, 0, 0, 1], [0, 0, 5, 0, 0.0]]), 2, 0.0)
    assert path.tolist() == [0, 2]
    # a strictly greater candidate wins over an earlier one, a penalty can reverse that
    c = np.array([[0, 0, 0, 0, 3], [0, 0, 5, 0, 0.0]])
    assert period_path_ref(c, 2, 0.0)[0].tolist() == [4, 2]
    assert period_path_ref(c, 2, 1.0)[0].tolist() == [4, 2] and period_path_ref(c, 2, 1.0)[2] == 6.0
    assert period_path_ref(c, 2, 2.0)[0].tolist() == [2, 2]  # 3 - 2 * 2 < 0: stay
    # the lowest of several equal end states
    assert period_path_ref(np.array([[0, 0, 0.0], [1, 7, 7.0]]), 1, 0.0)[0].tolist() == [1, 1]


def test_forbidden_entries():
    c = random_cost(5, 12, 9)
    base = period_path_ref(c, 2, 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        d = c.copy()
        d[4, base[0][4]] = bad  # the best path loses a cell: the new path avoids it, whatever the kind
        path, values, score, status = period_path_ref(d, 2, 0.1)
        assert status == PH_ST_OK and path[4] != base[0][4] and np.all(np.isfinite(values)) and score < base[2]
    same = [period_path_ref(np.where(np.isfinite(d), d, k), 2, 0.1) for k in (np.nan, np.inf, -np.inf)]
    assert all(np.array_equal(s[0], same[0][0]) and s[2] == same[0][2] for s in same)
    # a sprinkled table: the path only visits finite cells
    d = with_forbidden(random_cost(6, 40, 30), 7)
    path, values, score, status = period_path_ref(d, 3, 0.05)
    assert status == PH_ST_OK and np.all(np.isfinite(values)) and np.array_equal(values, d[np.arange(40), path])
    # a wholly forbidden frame, first, middle and last: status, the -1 path, zero values, score -inf
    for frame in (0, 20, 39):
        path, values, score, status = period_path_ref(with_dead_frame(d, frame), 3, 0.05)
        assert status == PH_ST_NO_PERIOD and np.all(path == -1) and np.all(values == 0.0) and score == -np.inf
    # finite cells in every frame, but no two within the band of each other
    c = np.full((3, 9), np.nan)
    c[0, 0] = c[1, 8] = c[2, 0] = 1.0
    assert period_path_ref(c, 7, 0.0)[3] == PH_ST_NO_PERIOD
    assert period_path_ref(c, 8, 0.0)[0].tolist() == [0, 8, 0]


def test_band_of_P_or_more_is_the_unbanded_programme():
    for seed, (W, P) in enumerate([(7, 1), (9, 2), (30, 13), (12, 40)]):
        for c in (random_cost(seed, W, P), tie_cost(seed, W, P)):
            for jump in (0.0, 0.25, 1e-3):
                full = period_path_ref(c, max(P - 1, 0), jump)
                for band in (P, P + 5, 64 + P):
                    got = period_path_ref(c, band, jump)
                    assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1]) and got[2] == full[2]
                if P > 2:  # and a narrower band is a different programme somewhere
                    assert period_path_ref(c, 1, jump)[2] <= full[2]


def glide_map():
    """The gamma-norm map of the glide signal by the oracle: N = 256, hop = 64, whole frames, rectangular window,
    periods 8 .. 85.  -> (map (61, 78), true period per frame)."""
    from oracle import period_oracle as po

    x, period_at = glide_signal()
    N, hop, lo, hi = 256, 64, 8, 85
    W = 1 + (x.size - N) // hop
    m = np.stack([po.sweep_norms(x[f * hop : f * hop + N], lo, hi, gamma=True) for f in range(W)])
    truth = np.array([round(period_at(hop * f + N // 2)) for f in range(W)])
    return m, truth, lo


def test_glide_signal_path_tracks_where_the_argmax_does_not():
    m, truth, lo = glide_map()
    assert m.shape == (61, 78)
    path, values, score, status = period_path_ref(m, 2, 0.002)
    assert status == PH_ST_OK
    assert np.all(np.abs(lo + path - truth) <= 1)  # every frame
    argmax = lo + np.argmax(m, axis=1)
    assert np.mean(np.abs(argmax - truth) > 1) >= 0.25  # a map that needs tracking


# ------------------------------------------------------------------ the C ABI without a GPU
def test_symbols_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for name, n_args in (("ph_period_path", 13), ("ph_period_path_plan_info", 5)):
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args and len(_ffi.SIGNATURES[name]) == n_args
        for arg, have in zip(args, _ffi.SIGNATURES[name]):
            if "*" in arg:
                assert have in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), arg
            else:
                assert have is ctype[arg.rsplit(" ", 1)[0]], arg


def test_entry_point_rejects_bad_arguments_without_gpu():
    """Every refusal comes before the first HIP call: a block of zeros stands in for the context, and the arrays are
    never read."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    ctx = ctypes.addressof((ctypes.c_char * 8192)())
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    good = dict(ctx=ctx, cost=buf, R=2, W=3, P=5, ld=5, band=2, jump=0.5, flags=0, path=buf, value=buf, score=buf,
                status=buf)

    def call(**change):
        a = dict(good, **change)
        return lib.ph_period_path(a["ctx"], a["cost"], a["R"], a["W"], a["P"], a["ld"], a["band"], a["jump"], a["flags"],
                                  a["path"], a["value"], a["score"], a["status"])

    def said(word):
        return word in lib.ph_last_error()

    for dev in (0, _ffi.PH_FLAG_DEVICE):
        assert call(ctx=None, flags=dev) == E and said(b"ctx")
        for name in ("cost", "path", "score", "status"):
            assert call(flags=dev, **{name: None}) == E and said(b"NULL"), name
        for P in (0, -1, 8193, 2**31 - 1):
            assert call(flags=dev, P=P, ld=max(P, 1)) == E and said(b"P="), P
        for band in (-1, 65, 2**31 - 1):
            assert call(flags=dev, band=band) == E and said(b"band"), band
        for jump in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
            assert call(flags=dev, jump=jump) == E and said(b"jump"), jump
        for W in (0, -1, -2**63):
            assert call(flags=dev, W=W) == E and said(b"W="), W
        for R in (-1, 2**31, 2**63 - 1):
            assert call(flags=dev, R=R) == E and said(b"R="), R
        for ld in (4, 0, -1, -2**63):
            assert call(flags=dev, ld=ld) == E and said(b"ld="), ld
        big = 2**63 - 1
        assert call(flags=dev, W=big) == E and said(b"64 bits")
        assert call(flags=dev, ld=big) == E and said(b"64 bits")
        assert call(flags=dev, R=2**31 - 1, W=2**40, ld=2**10) == E and said(b"64 bits")
    # the plan query: NULL arguments, and the same limits on P
    n = ctypes.c_int(0)
    assert lib.ph_period_path_plan_info(None, 64, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E
    assert lib.ph_period_path_plan_info(ctx, 64, None, ctypes.byref(n), ctypes.byref(n)) == E
    for P in (0, 8193):
        assert lib.ph_period_path_plan_info(ctx, P, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E and said(b"P=")


def test_period_map_and_contour_validate_before_touching_the_gpu(monkeypatch):
    import sys

    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)
    st = ShortTime(96, 24)
    x = np.zeros(300)
    for call in (st.period_map, st.contour):
        for kind in ("power", "", None, "Gamma", 3):
            with pytest.raises(ValueError, match="kind"):
                call(x, kind=kind)
        for lo in (0, -1):
            with pytest.raises(ValueError, match="min_length"):
                call(x, min_length=lo)
        with pytest.raises(ValueError, match="max_length"):
            call(x, min_length=9, max_length=8)
        with pytest.raises(ValueError, match="max_length"):
            ShortTime(4, 2).period_map(x) if call == st.period_map else ShortTime(4, 2).contour(x)  # 4 // 3 < 2
        with pytest.raises(ValueError, match="Ramanujan"):
            call(x, kind="ramanujan", max_length=30030)
        for bad in (0, -3, 1.5, True):
            with pytest.raises(ValueError, match="block_frames"):
                call(x, block_frames=bad)
        for flags in (dict(trunc_to_integer_multiple=True), dict(orthogonalize=True)):
            flagged = ShortTime(96, 24, **flags)
            for kind in ("orth", "ramanujan"):
                with pytest.raises(ValueError, match="no projection"):
                    (flagged.period_map if call == st.period_map else flagged.contour)(x, kind=kind)
    for band in (-1, 65, 1.0, None, True):
        with pytest.raises(ValueError, match="band"):
            st.contour(x, band=band)
    for jump in (-0.1, np.inf, np.nan, None, "1", True):
        with pytest.raises(ValueError, match="jump"):
            st.contour(x, jump=jump)
    with pytest.raises(ValueError, match="8192"):
        st.contour(x, min_length=1, max_length=8193)
    # what passes the checks reaches the engine
    for call in (lambda: st.period_map(x), lambda: st.contour(x), lambda: st.contour(x, kind="orth", band=0, jump=0),
                 lambda: st.period_map(x, kind="ramanujan", max_length=30029), lambda: st.contour(x, max_length=8193)):
        with pytest.raises(AssertionError, match="the GPU was touched"):
            call()


def test_engine_period_path_argument_errors_without_gpu():
    from test_short_time_cpu import cpu_engine

    eng, Reached = cpu_engine()
    for bad in (np.zeros(5), np.zeros((2, 2, 2, 2)), 3.0, None):
        with pytest.raises(ValueError, match="shape"):
            eng.period_path(bad)
    with pytest.raises(TypeError, match="float64"):
        eng.period_path(np.zeros((4, 5), dtype=np.float32))
