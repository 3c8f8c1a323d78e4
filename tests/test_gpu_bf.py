"""ph_best_frequency's three spectrum kernels (k_bf_fft, k_bf_chirp, k_bf_spectrum) and the argmax, rounding and status
logic of k_bf_update, pinned to the reference at their edges.

  * the reference fixtures of tests/golden/best_frequency_edges.npz (round-half-even, zero padding, truncation, the
    Nyquist bin, the flags, p > N) through every variant: the natural one (FFT for a power-of-two win_size, chirp
    otherwise), the direct DFT forced with PH_BF_DIRECT, and both again on an engine that keeps windows in HBM;
  * two tones planted so that their bins differ by 1e-9, and by 1e-11, (relative) in magnitude, to either side of the
    crossing: the only observable of the spectrum is its argmax, so the argmax is made sensitive.  The expected pick is
    numpy's, which a long-double direct DFT of the two bins confirms 100 to 1000 times more closely;
  * a batch in which some windows die (DC peak, NaN, exactly zero residual) while others go on;
  * windows scaled by 2^+-300, 2^+-520 and 2^-560, where |X|^2 leaves the range of a double but np.abs does not;
  * float32 windows, and a device tensor on torch's current stream;
  * the best_correlation cases of the same fixture file (flags with an explicit max_length, picks that `ratio` rejects).
"""

import contextlib
import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from test_bf_cpu import NAME, bc_case, bf_case

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL32 = 1e-4


def _engine(**env):
    """A fresh engine created with `env` set (the variables are read by ph_create) and restored right after."""
    from pyperiod_amd import PeriodEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return PeriodEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def forced_direct(on=True):
    """PH_BF_DIRECT is read when a call is planned: inside this block every call takes the direct DFT."""
    old = os.environ.get("PH_BF_DIRECT")
    if on:
        os.environ["PH_BF_DIRECT"] = "1"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["PH_BF_DIRECT"]
            else:
                os.environ["PH_BF_DIRECT"] = old


@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    assert "PH_BF_DIRECT" not in os.environ
    hbm = _engine(PH_HBM_WINDOW=1)
    try:
        yield default_engine(), hbm
    finally:
        hbm.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def spectrum_plan(eng, n, L, dtype=np.float64):
    """(variant of the spectrum kernel, placement of the update kernel's window) the next call would take."""
    recs = eng.plan_info("best_frequency", n, (L,), dtype)
    return recs[0].variant, recs[1].window


def natural_variant(L):
    from pyperiod_amd import _ffi

    return _ffi.PH_PLAN_FFT if L & (L - 1) == 0 else _ffi.PH_PLAN_CHIRP


def runs(engines, n, L, dtype=np.float64):
    """(name, engine, direct forced) of the four ways a window of n samples is run, each with its plan asserted: a
    planning change cannot silently turn the variants into one."""
    from pyperiod_amd import _ffi

    eng, hbm = engines
    out = []
    for name, e, direct, place in (("natural", eng, False, _ffi.PH_PLAN_LDS), ("direct", eng, True, _ffi.PH_PLAN_LDS),
                                   ("hbm", hbm, False, _ffi.PH_PLAN_HBM), ("hbm-direct", hbm, True, _ffi.PH_PLAN_HBM)):
        with forced_direct(direct):
            want = _ffi.PH_PLAN_DIRECT if direct else natural_variant(L)
            assert spectrum_plan(e, n, L, dtype) == (want, place), (name, n, L)
        out.append((name, e, direct))
    return out


# ---------------------------------------------------------------------------- reference fixtures, every variant
def _bf_tags():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", NAME + ".npz"))
    return [str(t) for t in g["bf_tags"]]


@pytest.mark.parametrize("tag", _bf_tags())
def test_reference_fixture_through_every_variant(engines, golden, tag):
    x, L, num, trunc, orth, per, pw, bs = bf_case(golden(NAME), tag)
    got = {}
    for name, e, direct in runs(engines, len(x), L):
        with forced_direct(direct):
            p, w, b, st = e.best_frequency(x[None, :], L, num, trunc, orth)
        assert st[0] == 0 and np.array_equal(p[0], per), (tag, name, p[0], per)
        assert rel_err(w[0], pw) < TOL and rel_err(b[0], bs) < TOL, (tag, name)
        got[name] = (p[0], b[0])
    for name, (p, b) in got.items():
        assert np.array_equal(p, got["natural"][0]) and rel_err(b, got["natural"][1]) < 1e-12, (tag, name)


# ---------------------------------------------------------------------------- planted near-tie
K1, K2 = 37, 91


def _two_tones(n, L, b, seed=5):
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return np.cos(2 * np.pi * K1 * t / L + 0.4) + b * np.cos(2 * np.pi * K2 * t / L + 1.1) + 1e-3 * rng.standard_normal(n)


def _gap_numpy(x, L):
    """(|X[K2]| - |X[K1]|) / |X[K1]| on the reference's own spectrum; the two bins are its two largest."""
    mags = np.abs(np.fft.rfft(x, L))
    assert set(np.argsort(mags)[-2:]) == {K1, K2}
    return (mags[K2] - mags[K1]) / mags[K1]


def _gap_longdouble(x, L):
    """The same gap from a direct DFT of the two bins in long double, the phase k n mod L reduced in integers."""
    ld = np.longdouble
    m = min(len(x), L)
    two_pi = 8 * np.arctan(ld(1))
    mags = []
    for k in (K1, K2):
        ang = two_pi * ((k * np.arange(m, dtype=np.int64)) % L).astype(ld) / ld(L)
        xv = x[:m].astype(ld)
        mags.append(np.sqrt(np.sum(xv * np.cos(ang)) ** 2 + np.sum(xv * np.sin(ang)) ** 2))
    return float((mags[1] - mags[0]) / mags[0])


@pytest.mark.parametrize("n,L,direct", [(1024, 1024, False), (700, 1024, False), (1000, 1000, False), (1500, 1000, False),
                                        (1000, 1000, True), (6000, 6000, False)])
def test_two_bins_1e9_apart(engines, n, L, direct):
    """Bins 37 and 91 carry the two tones; the amplitude of the second is tuned by bisection on np.abs(np.fft.rfft(x, L))
    until the two magnitudes cross, then set 1e-9 (relative) to either side: the project's figure for this construction
    (tests/test_gpu_pair.py).  The reference's own gap agrees with a long-double DFT within 1e-12, 1000 times less.

    A table rounded through float perturbs every entry by up to 6e-8, but a bin sums a thousand of them with signs that
    average out: the bin moves by about 6e-8 / sqrt(N), 1e-9 for these lengths, and a gap of 1e-9 may or may not flip.
    So the same crossing is also approached to 1e-11.  That is still decided by fp64 arithmetic: N fused multiply-adds
    of the direct DFT are off by at most N 2^-53 sum|x| / |X| < 1.4e-12 at N = 6000 (2e-13 at N = 1000), the FFT stages
    by a few log2(M) 2^-53 < 1e-14, and numpy agrees with the long-double DFT within 1e-13 (asserted; 1e-16 seen).  An
    error above 1e-11 in the difference of the two bins flips one of the two sides."""
    from pyperiod_amd import _ffi

    eng, _ = engines
    want_variant = {(1024, 1024, False): _ffi.PH_PLAN_FFT, (700, 1024, False): _ffi.PH_PLAN_FFT,
                    (1000, 1000, False): _ffi.PH_PLAN_CHIRP, (1500, 1000, False): _ffi.PH_PLAN_CHIRP,
                    (1000, 1000, True): _ffi.PH_PLAN_DIRECT, (6000, 6000, False): _ffi.PH_PLAN_DIRECT}[(n, L, direct)]
    lo, hi = 0.5, 2.0
    assert _gap_numpy(_two_tones(n, L, lo), L) < 0 < _gap_numpy(_two_tones(n, L, hi), L)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if _gap_numpy(_two_tones(n, L, mid), L) < 0:
            lo = mid
        else:
            hi = mid
    for rel, ref_tol in ((1e-9, 1e-12), (1e-11, 1e-13)):
        picks = []
        for b in (lo * (1 - rel), hi * (1 + rel)):
            x = _two_tones(n, L, b)
            g_np, g_ld = _gap_numpy(x, L), _gap_longdouble(x, L)
            print(f"n={n} L={L} direct={direct} b={b!r}: gap numpy {g_np:.6e} long double {g_ld:.6e}")
            assert 0.5 * rel < abs(g_np) < 2 * rel and g_np * g_ld > 0 and abs(g_np - g_ld) < ref_tol
            rper, rpw, rbs = po.best_frequency(x, L, 2)
            with forced_direct(direct):
                assert spectrum_plan(eng, n, L)[0] == want_variant
                per, pw, bs, st = eng.best_frequency(x[None, :], L, 2)
            assert st[0] == 0 and np.array_equal(per[0], rper), (n, L, direct, rel, b, per[0], rper)
            assert rel_err(pw[0], rpw) < TOL and rel_err(bs[0], rbs) < TOL
            picks.append(int(rper[0]))
        assert picks == [int(np.round(2 * L / K1)), int(np.round(2 * L / K2))] and picks[0] != picks[1]


# ---------------------------------------------------------------------------- windows that die next to windows that live
@pytest.mark.parametrize("direct", [False, True])
def test_mixed_fate_batch(engines, golden, direct):
    """One call, five windows: live, dead at round 0 (DC peak), live at round 0 and dead from round 1 (the k = 1 window
    is its own base at p = 2 N, the residual is exactly zero), dead at round 0 (NaN), live."""
    from pyperiod_amd import Periods, _ffi

    g = golden(NAME)
    eng, _ = engines
    names = ["live_a", "offset", "p_gt_n", "nan", "live_b"]
    x = np.stack([g[f"{t}_x"] for t in names])
    n, num = x.shape[1], 3
    with forced_direct(direct):
        assert spectrum_plan(eng, n, n)[0] == (_ffi.PH_PLAN_DIRECT if direct else _ffi.PH_PLAN_CHIRP)
        per, pw, bs, st = eng.best_frequency(x, None, num)
        assert _ffi.PH_ST_NO_PERIOD == 1 and st.tolist() == [0, 1, 1, 1, 0]
        for w in (0, 4):  # the batch does not change a live window's result by a bit, and it is the reference's
            p1, w1, b1, s1 = eng.best_frequency(x[w:w + 1], None, num)
            assert s1[0] == 0 and np.array_equal(per[w], p1[0]) and np.array_equal(pw[w], w1[0])
            assert np.array_equal(bs[w], b1[0])
            _, _, _, _, _, rper, rpw, rbs = bf_case(g, names[w])
            assert np.array_equal(per[w], rper) and rel_err(pw[w], rpw) < TOL and rel_err(bs[w], rbs) < TOL
        with pytest.raises(OverflowError):
            Periods().best_frequency(x, None, num)
    for w in (1, 3):
        assert not per[w].any() and not pw[w].any() and not bs[w].any(), w
    _, _, _, _, _, rper, rpw, rbs = bf_case(g, "p_gt_n")  # the reference's num = 1 answer, then zero rows
    assert per[2].tolist() == [2 * n, 0, 0] and int(rper[0]) == 2 * n
    assert rel_err(pw[2, :1], rpw) < TOL and rel_err(bs[2, 0], rbs[0]) < TOL
    assert not pw[2, 1:].any() and not bs[2, 1:].any()


# ---------------------------------------------------------------------------- power-of-two scaling
@pytest.mark.parametrize("tag,direct", [("nyquist", False), ("live_a", False), ("live_a", True)])
def test_power_of_two_scaling_is_exact(engines, golden, tag, direct):
    """The reference's period list and bases are exactly invariant under x -> 2^e x (np.abs ranks with hypot; sums,
    means and differences scale exactly).  |X|^2 is inf in every bin at e = 520 and 0 in every bin at e = -560: the
    kernels rank on an exactly rescaled spectrum.  Beyond +-500 the reference's own norm overflows or underflows, so
    powers are compared at +-300 only."""
    from pyperiod_amd import _ffi

    eng, _ = engines
    x, L, num, trunc, orth, rper, rpw, rbs = bf_case(golden(NAME), tag)
    want = _ffi.PH_PLAN_DIRECT if direct else natural_variant(L)
    with forced_direct(direct):
        assert spectrum_plan(eng, len(x), L)[0] == want
        per0, pw0, bs0, st0 = eng.best_frequency(x[None, :], L, num)
        assert st0[0] == 0 and np.array_equal(per0[0], rper) and rel_err(bs0[0], rbs) < TOL
        for e in (300, -300, 520, -520, -560):
            s = 2.0 ** e
            y = x * s
            assert np.array_equal(y / s, x)  # the scaling itself is exact
            assert np.array_equal(po.best_frequency(y, L, num)[0], rper)  # and numpy's pick does not move
            per, pw, bs, st = eng.best_frequency(y[None, :], L, num)
            assert st[0] == 0, (tag, direct, e, st, per)
            assert np.array_equal(per[0], per0[0]), (tag, direct, e, per[0], per0[0])
            assert np.array_equal(bs[0], bs0[0] * s), (tag, direct, e)
            if abs(e) == 300:
                assert rel_err(pw[0], pw0[0]) < TOL, (tag, direct, e)


# ---------------------------------------------------------------------------- float32 windows
@pytest.mark.parametrize("tag,variant", [("flags_t0_o0", "CHIRP"), ("flags_t1_o0", "CHIRP"), ("flags_t0_o1", "CHIRP"),
                                         ("flags_t1_o1", "CHIRP"), ("half_dn_k32", "CHIRP"), ("pad_fft", "FFT"),
                                         ("cut_fft", "FFT"), ("nyquist", "FFT")])
def test_float32_windows(engines, golden, tag, variant):
    """The float instantiations of all three spectrum kernels: the flags window and a half-even window (chirp), and the
    zero-padded, truncated and full-length power-of-two windows (FFT), each also with the direct DFT forced.  Judged by
    the oracle on the fp32-rounded input; its runner-up stays below 0.98 of the peak in every round of these windows,
    far outside what a residual stored as float (6e-8 per sample) can move."""
    from pyperiod_amd import _ffi

    x, L, num, trunc, orth, _, _, _ = bf_case(golden(NAME), tag)
    assert natural_variant(L) == getattr(_ffi, "PH_PLAN_" + variant)  # runs() asserts that the call is planned so
    x32 = x.astype(np.float32)
    rper, rpw, rbs = po.best_frequency(x32.astype(np.float64), L, num, trunc, orth)
    work = x32.astype(np.float64)
    for i in range(num):
        mags = np.sort(np.abs(np.fft.rfft(work, L)))
        assert mags[-2] <= 0.98 * mags[-1], (tag, i)
        work = work - rbs[i]
    for name, e, direct in runs(engines, len(x), L, np.float32):
        with forced_direct(direct):
            per, pw, bs, st = e.best_frequency(x32[None, :], L, num, trunc, orth)
        assert bs.dtype == np.float32 and st[0] == 0 and np.array_equal(per[0], rper), (tag, name, per[0], rper)
        assert rel_err(pw[0], rpw) < TOL32 and rel_err(bs[0], rbs) < TOL32, (tag, name)


# ---------------------------------------------------------------------------- device-pointer path
def test_device_tensor_on_torchs_current_stream(engines, golden):
    import torch

    eng, _ = engines
    x, L, num, trunc, orth, rper, _, _ = bf_case(golden(NAME), "flags_t1_o1")
    host = eng.best_frequency(x[None, :], L, num, trunc, orth)
    assert np.array_equal(host[0][0], rper)
    xd = torch.from_numpy(x[None, :]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for stream in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(stream):
            dev = eng.best_frequency(xd, L, num, trunc, orth)
            assert all(t.is_cuda for t in dev)
            dev = [t.cpu().numpy() for t in dev]
        assert dev[0].dtype == np.int32 and host[0].dtype == np.uint32  # torch has no uint32: the same 32 bits
        assert np.array_equal(dev[0].view(np.uint32), host[0])
        for a, b in zip(dev[1:], host[1:]):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------- best_correlation cases of the fixture
def test_best_correlation_reference_fixtures(engines, golden):
    g = golden(NAME)
    for e in engines:
        for tag in (str(t) for t in g["bc_tags"]):
            x, num, max_length, ratio, trunc, orth, per, nr, bs = bc_case(g, tag)
            p, w, b, st = e.best_correlation(x[None, :], num, max_length, ratio, trunc, orth)
            assert st[0] == 0 and np.array_equal(p[0], per), (tag, p[0], per)
            assert rel_err(w[0], nr) < TOL and rel_err(b[0], bs) < TOL, tag
