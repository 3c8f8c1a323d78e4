"""ShortTime on the MI355X: k_frames bit for bit against the numpy restatement (a loop over frames), k_overlap_add and the
round trip against the np.add.at restatement, ShortTime.analyze against the Periods methods on the host-built batch of
the same frames, and the argument checks of both entry points.  The restatements and the bound live in
tests/test_short_time_cpu.py.

Overlap-add bound, per sample: |out - ref| <= (T + 3) * 2^-52 * mag[n] / den[n] with T = K * ceil(N / hop) terms,
mag[n] = sum |ws * y| over them and den = 1 when not normalised -- both sides are float64 sums of at most T terms with one
product rounding each and one division.  Samples with den == 0 must be exactly 0.0."""

import ctypes
import warnings

import numpy as np
import pytest

from pyperiod_amd.synth import readme_window
from test_short_time_cpu import frames_ref, ola_bound, overlap_add_ref, sqrt_hann

pytestmark = pytest.mark.gpu

NS, HOPS, LS = (63, 64, 65), (1, 3, 16, 64, 80), (997, 1000)
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


@pytest.fixture(scope="module")
def torch_dev(eng):
    import torch

    return torch, torch.device("cuda", eng.device)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _count(L, N, hop):
    from pyperiod_amd import ShortTime

    return ShortTime(N, hop).frame_count(L)


def _signal(L, dtype, seed=0):
    return np.random.default_rng(seed + L).standard_normal(L).astype(dtype)


def _window(N):
    """A window without structure (every sample different, both signs), so that a wrong window index shows."""
    return np.random.default_rng(N).uniform(-1.0, 1.0, N)


# ------------------------------------------------------------------ framing
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("N", NS)
def test_frames_bit_exact(eng, torch_dev, N, hop):
    torch, dev = torch_dev
    win = _window(N)
    win_d = torch.as_tensor(win, device=dev)
    for L in LS:
        W = _count(L, N, hop)
        for tin in DTYPES:
            x = _signal(L, tin)
            xd = torch.as_tensor(x, device=dev)
            for tout in DTYPES:
                for w, wd in ((None, None), (win, win_d)):
                    ref = frames_ref(x, N, hop, W, w, tout)
                    got = eng.frames(x, N, hop, W, w, tout)
                    assert got.dtype == ref.dtype and got.shape == (W, N)
                    assert np.array_equal(got, ref), (L, tin, tout, w is not None)
                    got_d = eng.frames(xd, N, hop, W, wd, tout)
                    assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), ref), (L, tin, tout, w is not None)
    # the default count is the padded one, the default dtype the signal's
    x = _signal(LS[0], np.float32)
    got = eng.frames(x, N, hop)
    assert got.dtype == np.float32 and np.array_equal(got, frames_ref(x, N, hop, _count(LS[0], N, hop)))


@pytest.mark.parametrize("L,N,hop,W", [(64, 64, 16, 1), (50, 64, 7, 1), (40, 64, 16, 3), (130, 64, 33, 4), (1, 1, 1, 1),
                                       (9, 1, 2, 5), (70, 3, 1, 70)])
def test_frames_edges(eng, L, N, hop, W):
    """L == N, L < N padded (one frame, and more frames than the padded count asks for), a partial last frame, N below
    the vector width."""
    for tin in DTYPES:
        x = _signal(L, tin, 7)
        for tout in DTYPES:
            assert np.array_equal(eng.frames(x, N, hop, W, None, tout), frames_ref(x, N, hop, W, None, tout))
            w = _window(N)
            assert np.array_equal(eng.frames(x, N, hop, W, w, tout), frames_ref(x, N, hop, W, w, tout))


def test_frames_past_the_16_bit_grid_limit(eng, torch_dev):
    torch, dev = torch_dev
    W, N, hop = 70_000, 8, 1
    x = _signal(W + N - 1, np.float64, 3)
    ref = frames_ref(x, N, hop, W)
    assert np.array_equal(eng.frames(x, N, hop, W), ref)
    got = eng.frames(torch.as_tensor(x.astype(np.float32), device=dev), N, hop, W, None, np.float64)
    assert np.array_equal(got.cpu().numpy(), frames_ref(x.astype(np.float32), N, hop, W, None, np.float64))
    assert eng.frames(x, N, hop, 0).shape == (0, N)  # W == 0: no call


def test_frames_unaligned_pointers(eng, torch_dev):
    """A signal that starts 4 or 8 bytes into an allocation (the source vector loads must fall back), and through the C ABI
    an output that is not 16-byte aligned (the scalar variant)."""
    from pyperiod_amd import _ffi

    torch, dev = torch_dev
    L, N, hop = 1000, 64, 16
    W = _count(L, N, hop)
    for tin, code in ((np.float64, _ffi.PH_F64), (np.float32, _ffi.PH_F32)):
        x = _signal(L + 3, tin, 11)
        xd = torch.as_tensor(x, device=dev)
        for off in (1, 2, 3):
            got = eng.frames(xd[off : off + L], N, hop, W, None, np.float64)
            assert np.array_equal(got.cpu().numpy(), frames_ref(x[off : off + L], N, hop, W, None, np.float64))
        for tout, ocode, tt in ((np.float64, _ffi.PH_F64, torch.float64), (np.float32, _ffi.PH_F32, torch.float32)):
            buf = torch.zeros(W * N + 1, dtype=tt, device=dev)
            torch.cuda.synchronize()
            rc = eng._call(_stream_of(torch, xd), W, eng._lib.ph_frames, xd.data_ptr(), code, L, N, hop, W, None, ocode,
                           _ffi.PH_FLAG_DEVICE, buf.data_ptr() + buf.element_size())
            assert rc == _ffi.PH_OK
            torch.cuda.synchronize()
            assert np.array_equal(buf[1:].cpu().numpy().reshape(W, N), frames_ref(x[:L], N, hop, W, None, tout))
            assert buf[0].item() == 0.0


def _stream_of(torch, t):
    from pyperiod_amd import _ffi
    from pyperiod_amd.engine import _Out

    mk = _Out(t)
    mk.stream = torch.cuda.current_stream(t.device).cuda_stream or _ffi.PH_STREAM_DEFAULT
    return mk


# ------------------------------------------------------------------ overlap-add
def _check_ola(got, y, hop, L, counts, wa, ws, normalize, what):
    ref, mag, den = overlap_add_ref(y, hop, L, counts, wa, ws, normalize)
    K, N = (1, y.shape[1]) if y.ndim == 2 else y.shape[1:]
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (L,)
    pos = den > 0
    err, bound = np.abs(got - ref), ola_bound(mag, den, K, N, hop)
    assert np.all(np.isfinite(got)), what
    assert np.all(err[pos] <= bound[pos]), (what, float(np.max(err[pos] - bound[pos])))
    assert np.all(got[~pos] == 0.0), what
    return pos


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("N", NS)
def test_overlap_add_against_restatement(eng, torch_dev, N, hop):
    torch, dev = torch_dev
    hann = sqrt_hann(N) ** 2  # first sample exactly zero
    assert hann[0] == 0.0
    for L in LS:
        W = _count(L, N, hop)
        rng = np.random.default_rng(N * 100 + hop + L)
        for K in (1, 3):
            y = rng.standard_normal((W, K, N))
            for normalize in (False, True):
                got = eng.overlap_add(y, hop, L, normalize=normalize)
                _check_ola(got, y, hop, L, None, None, None, normalize, (L, K, normalize))
            if K == 1:  # (W, N) input
                assert np.array_equal(eng.overlap_add(y[:, 0], hop, L, normalize=False), eng.overlap_add(y, hop, L, normalize=False))
            # counts with zeros and full rows, garbage behind them, a window with a zero
            counts = rng.integers(0, K + 1, W).astype(np.int32)
            counts[0], counts[-1] = K, 0
            if W > 2:
                counts[1] = 0
            bad = y.copy()
            bad[np.arange(K)[None, :] >= counts[:, None]] = np.nan
            got = eng.overlap_add(bad, hop, L, counts, hann, hann, True)
            pos = _check_ola(got, y, hop, L, counts, hann, hann, True, (L, K, "counts"))
            if hop >= N:
                assert not pos[0] and (hop == N or not pos[N])  # the window's zero, and the gap behind a frame
            # two runs and the device-tensor call give the same bits
            again = eng.overlap_add(bad, hop, L, counts, hann, hann, True)
            assert np.array_equal(got, again)
            got_d = eng.overlap_add(torch.as_tensor(bad, device=dev), hop, L, torch.as_tensor(counts, device=dev),
                                    torch.as_tensor(hann, device=dev), torch.as_tensor(hann, device=dev), True)
            assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), got)
            # different analysis and synthesis windows, float32 y
            y32 = y.astype(np.float32)
            wa = _window(N) ** 2 + 0.1
            got = eng.overlap_add(y32, hop, L, None, wa, hann, True)
            _check_ola(got, y32, hop, L, None, wa, hann, True, (L, K, "float32"))
            # a count outside [0, K] is clipped
            wild = counts.copy()
            wild[0], wild[-1] = K + 5, -3
            assert np.array_equal(eng.overlap_add(bad, hop, L, wild, hann, hann, True), again)


def test_overlap_add_many_frames_and_empty(eng):
    """More frames than a 16-bit grid dimension holds, K past the unrolled quads, and W == 0."""
    W, K, N, hop = 70_000, 6, 8, 1
    L = W + N - 1
    y = np.random.default_rng(5).standard_normal((W, K, N))
    _check_ola(eng.overlap_add(y, hop, L, normalize=True), y, hop, L, None, None, None, True, "many frames")
    out = eng.overlap_add(np.zeros((0, 3, N)), hop, 20)
    assert out.shape == (20,) and np.all(out == 0.0)


@pytest.mark.parametrize("L,N,hop", [(1000, 64, 16), (1000, 64, 48), (333, 64, 1), (200, 64, 64), (50, 64, 7),
                                     (1000, 64, 80), (997, 63, 3), (997, 65, 16)])
def test_round_trip(eng, torch_dev, L, N, hop):
    """overlap_add(frames(x)) under a sqrt-Hann window gives x back wherever a frame with a non-zero window covers it."""
    from pyperiod_amd import ShortTime

    torch, dev = torch_dev
    x = _signal(L, np.float64, 21)
    w = sqrt_hann(N)
    st = ShortTime(N, hop, window=w)
    fr = st.frames(x)
    assert np.array_equal(fr, frames_ref(x, N, hop, st.frame_count(L), w))
    out = st.overlap_add(fr, L)
    _, mag, den = overlap_add_ref(fr, hop, L, None, w, w, True)
    pos = den > 0
    assert np.all(np.abs(out - x)[pos] <= ola_bound(mag, den, 1, N, hop)[pos])
    assert np.all(out[~pos] == 0.0)
    # the same chain on device tensors
    fr_d = st.frames(torch.as_tensor(x, device=dev))
    out_d = st.overlap_add(fr_d, L)
    assert fr_d.is_cuda and out_d.is_cuda and np.array_equal(out_d.cpu().numpy(), out)


# ------------------------------------------------------------------ analyze
A_N, A_HOP, A_L = 256, 64, 2000


@pytest.fixture(scope="module")
def analysis(eng):
    from pyperiod_amd import ShortTime

    x = readme_window(A_L, seed=0)
    w = sqrt_hann(A_N)
    st = ShortTime(A_N, A_HOP, window=w)
    batch = frames_ref(x, A_N, A_HOP, st.frame_count(A_L), w)  # the host-built batch of the same frames
    return st, x, w, batch


def _check_analysis(res, x, w, bases, counts=None):
    ref, mag, den = overlap_add_ref(bases, A_HOP, A_L, counts, w, w, True)
    pos = den > 0
    assert res.periodic.dtype == np.float64 and res.periodic.shape == (A_L,)
    err, bound = np.abs(res.periodic - ref), ola_bound(mag, den, bases.shape[1], A_N, A_HOP)
    assert np.all(err[pos] <= bound[pos]), float(np.max(err[pos] - bound[pos]))
    assert np.all(res.periodic[~pos] == 0.0)
    # the residual is float64(signal) - periodic exactly as computed; adding the periodic part back returns the signal
    # to the rounding of that one subtraction and one addition
    x64 = x.astype(np.float64)
    assert np.array_equal(res.residual, x64 - res.periodic)
    assert np.all(np.abs(res.residual + res.periodic - x64) <= 2.0**-52 * (np.abs(x64) + np.abs(res.periodic)))


@pytest.mark.parametrize("method,kwargs", [("m_best", {"num": 3}), ("m_best_gamma", {}), ("best_correlation", {}),
                                           ("best_frequency", {}), ("best_frequency", {"num": 2})])
def test_analyze_against_periods(eng, analysis, method, kwargs):
    """best_frequency with its default num = 5 is a case the reference itself cannot finish on this signal: in frames 8
    and 28 the third spectral peak is bin 0 and Periods.best_frequency raises OverflowError (the CPU oracle agrees).  What
    is equal to `Periods` there is the exception, and analyze names the first such frame; num = 2, which every frame
    completes, carries the value comparison for that method."""
    from pyperiod_amd import Periods

    st, x, w, batch = analysis
    if method == "best_frequency" and not kwargs:
        with pytest.raises(OverflowError):
            Periods().best_frequency(batch)
        first = int(np.flatnonzero(eng.best_frequency(batch)[3])[0])
        assert first == 8
        with pytest.raises(OverflowError, match=f"frame {first}"):
            st.analyze(x, method=method)
        return
    per, pw, bases = getattr(Periods(), method)(batch, **kwargs)
    eng.profile(True)
    try:
        res = st.analyze(x, method=method, **kwargs)
        names = [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)
    assert names.count("k_frames") == 1 and names.count("k_overlap_add") == 1
    assert names[0] == "k_frames" and names[-1] == "k_overlap_add" and len(names) >= 3
    assert isinstance(res.periods, np.ndarray) and isinstance(res.powers, np.ndarray) and res.counts is None
    assert res.periods.dtype == per.dtype and np.array_equal(res.periods, per)
    assert res.powers.dtype == np.float64 and np.array_equal(res.powers, pw)
    _check_analysis(res, x, w, bases)


def test_analyze_small_to_large(eng, analysis):
    from pyperiod_amd import Periods

    st, x, w, batch = analysis
    host = Periods().small_to_large(batch, thresh=0.1)
    res = st.analyze(x, method="small_to_large", thresh=0.1)
    W = batch.shape[0]
    counts = np.array([len(h[0]) for h in host], dtype=np.int32)
    assert res.counts.dtype == np.int32 and np.array_equal(res.counts, counts)
    kmax = max(1, int(counts.max()))
    bases = np.zeros((W, kmax, A_N))
    for f, (per, pw, bs) in enumerate(host):
        k = len(per)
        assert np.array_equal(res.periods[f, :k], np.array(per, dtype=res.periods.dtype))
        assert np.array_equal(res.powers[f, :k], np.array(pw))
        assert np.all(res.periods[f, k:] == 0) and np.all(res.powers[f, k:] == 0.0)
        if k:
            bases[f, :k] = np.stack(bs)
    assert counts.max() > 0
    _check_analysis(res, x, w, bases, counts)


def test_analyze_names_the_bad_frame(eng):
    """An all-zero frame: Periods.best_frequency raises OverflowError (the spectral peak is bin 0); analyze raises the
    same, naming the frame."""
    from pyperiod_amd import Periods, ShortTime

    x = readme_window(A_L, seed=1)
    x[512:1100] = 0.0  # frame 8 (samples 512 .. 767) and frame 9 are all zero
    st = ShortTime(A_N, A_HOP)
    batch = frames_ref(x, A_N, A_HOP, st.frame_count(A_L))
    assert not batch[8].any() and batch[7].any()
    with pytest.raises(OverflowError):  # (num = 1: with more rounds, frames that are only partly zero fail before frame 8)
        Periods().best_frequency(batch, num=1)
    with pytest.raises(OverflowError, match="frame 8"):
        st.analyze(x, method="best_frequency", num=1)
    with pytest.raises(TypeError):
        Periods().m_best(batch, num=2)
    with pytest.raises(TypeError, match="frame 8"):
        st.analyze(x, method="m_best", num=2)
    with pytest.raises(TypeError):
        st.analyze(x, method="m_best", nmu=2)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(eng):
    from pyperiod_amd import _ffi

    lib, ctx = eng._lib, eng._ctx
    sig = np.zeros(100)
    fr = np.zeros((4, 16))
    y = np.zeros((4, 2, 16))
    out = np.zeros(100)
    s, f, yy, o = sig.ctypes.data, fr.ctypes.data, y.ctypes.data, out.ctypes.data
    E = _ffi.PH_E_ARG
    eng.profile(True)
    try:
        for dev in (0, _ffi.PH_FLAG_DEVICE):
            assert lib.ph_frames(ctx, None, 0, 100, 16, 8, 4, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 100, 16, 8, 4, None, 0, dev, None) == E
            assert lib.ph_frames(ctx, s, 2, 100, 16, 8, 4, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 100, 16, 8, 4, None, 5, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 0, 16, 8, 4, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 100, 0, 8, 4, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 100, 16, 0, 4, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 100, 16, 8, 0, None, 0, dev, f) == E
            assert lib.ph_frames(ctx, s, 0, 24, 16, 8, 4, None, 0, dev, f) == E  # (W - 1) hop == L
            assert lib.ph_overlap_add(ctx, None, 0, 4, 2, 16, 8, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 2, 16, 8, 100, None, None, None, dev, None) == E
            assert lib.ph_overlap_add(ctx, yy, 3, 4, 2, 16, 8, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 0, 2, 16, 8, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 0, 16, 8, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 2, 0, 8, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 2, 16, 0, 100, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 2, 16, 8, 0, None, None, None, dev, o) == E
            assert lib.ph_overlap_add(ctx, yy, 0, 4, 2, 16, 8, 24, None, None, None, dev, o) == E
        # the engine turns PH_E_ARG into ValueError
        with pytest.raises(ValueError):
            eng.frames(sig, 16, 0, 4)
        with pytest.raises(ValueError):
            eng.frames(sig, 16, 50, 4)  # frame 2 starts behind the signal
        with pytest.raises(ValueError):
            eng.frames(sig, 0, 8, 4)
        with pytest.raises(ValueError):
            eng.overlap_add(y, 0, 100)
        with pytest.raises(ValueError):
            eng.overlap_add(y, 8, 24)
        with pytest.raises(ValueError):
            eng.overlap_add(y, 8, 100, counts=np.zeros(3, np.int32))
        with pytest.raises(ValueError):
            eng.overlap_add(y, 8, 100, win_s=np.ones(15))
        with pytest.raises(ValueError):
            eng.frames(fr, 16, 8)  # not 1-D
        assert eng.profile_read() == []
        # and a good call is recorded
        eng.frames(sig, 16, 8, 4)
        eng.overlap_add(y, 8, 100)
        assert [n for n, _ in eng.profile_read()] == ["k_frames", "k_overlap_add"]
    finally:
        eng.profile(False)
    assert ctypes.sizeof(ctypes.c_int64) == 8
