"""The blocked overlap-add and ``block_frames`` on the MI355X.

Kernel level: for every partition of the frames into blocks (tests/test_short_time_blocks_ola_cpu.partitions),
k_overlap_add_block per block and one k_overlap_add_finish give THE SAME BITS as k_overlap_add -- with masks, as
k_overlap_add_tracks -- on the whole (W, K, N) array: a lane of a later block continues the walk of its sample where the
block before left it, the same additions in the same order.  Against the numpy restatement of the two kernels the result
stays within the bound tests/test_gpu_short_time.py derives for k_overlap_add, (T + 3) 2^-52 mag / den per sample with
T = K ceil(N / hop) terms.  The blocks of the bit-for-bit sweeps are launched through the C ABI on device pointers (a
block of one frame at hop = 1 makes a thousand launches per partition); the binding's numpy and tensor forms run on two
partitions of every shape.

End to end: ``analyze`` / ``decompose`` with ``block_frames`` against the same call without, field for field and bit for
bit, the kernels either call launches, the exception of a bad frame in a late block, and the peak device memory of a
blocked run."""

import warnings

import numpy as np
import pytest

from pyperiod_amd.synth import readme_window
from test_short_time_blocks_ola_cpu import blocked_ref, overlap_add_finish_ref, partitions
from test_short_time_cpu import ola_bound, overlap_add_ref, sqrt_hann
from test_short_time_tracks_cpu import overlap_add_tracks_ref

pytestmark = pytest.mark.gpu

NS, HOPS, LS, KS = (63, 64, 65), (1, 3, 16, 64, 80), (997, 1000), (1, 3, 5, 9)
DTYPES = (np.float64, np.float32)
SENTINEL = np.float64(-1.2345678901234567e300)


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


def _count(L, N, hop, pad_end=True):
    from pyperiod_amd import ShortTime

    return ShortTime(N, hop, pad_end=pad_end).frame_count(L)


def _stream_of(torch, t):
    from pyperiod_amd import _ffi
    from pyperiod_amd.engine import _Out

    mk = _Out(t)
    mk.stream = torch.cuda.current_stream(t.device).cuda_stream or _ffi.PH_STREAM_DEFAULT
    return mk


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Whole:
    """One (W, K, N) array on the device with its side arrays, and the blocked route over it through the C ABI."""

    def __init__(self, eng, torch_dev, y, hop, L, counts=None, masks=None, wa=None, ws=None):
        from pyperiod_amd import _ffi

        torch, dev = torch_dev
        self.eng, self.torch, self.dev, self.ffi = eng, torch, dev, _ffi
        self.y = torch.as_tensor(np.ascontiguousarray(y), device=dev)
        self.W, self.K, self.N = y.shape
        self.hop, self.L = hop, L
        self.code = _ffi.PH_F64 if y.dtype == np.float64 else _ffi.PH_F32
        self.counts = None if counts is None else torch.as_tensor(counts, device=dev)
        self.masks = masks  # host (T, W) uint64 or None
        self.T = 1 if masks is None else masks.shape[0]
        self.wa = None if wa is None else torch.as_tensor(wa, device=dev)
        self.ws = None if ws is None else torch.as_tensor(ws, device=dev)
        self.mk = _stream_of(torch, self.y)

    def _ptr(self, t):
        return None if t is None else t.data_ptr()

    def blocks(self, cuts, acc):
        """ph_overlap_add_block for every (f0, Wb) of `cuts`, in order, into the device tensor acc (T, L)."""
        lib, fl = self.eng._lib, self.ffi.PH_FLAG_DEVICE
        row = self.K * self.N * self.y.element_size()
        md = None
        if self.masks is not None:  # block-major: the (T, Wb) words of block after block
            md = self.torch.as_tensor(np.concatenate([self.masks[:, f0 : f0 + Wb].ravel() for f0, Wb in cuts]).view(np.int64),
                                      device=self.dev)
        done = 0
        for f0, Wb in cuts:
            rc = self.eng._call(self.mk, Wb, lib.ph_overlap_add_block, self.y.data_ptr() + f0 * row, self.code, Wb, self.K,
                                self.N, self.hop, self.L, f0, None if self.counts is None else self.counts.data_ptr() + 4 * f0,
                                None if md is None else md.data_ptr() + 8 * self.T * done, self.T, self._ptr(self.ws), fl,
                                acc.data_ptr())
            assert rc == self.ffi.PH_OK
            done += Wb
        return acc

    def finish(self, acc, normalize, out):
        rc = self.eng._call(self.mk, self.W, self.eng._lib.ph_overlap_add_finish, acc.data_ptr(), self.T, self.N, self.hop,
                            self.L, self.W, self._ptr(self.wa), self._ptr(self.ws),
                            self.ffi.PH_FLAG_DEVICE | (self.ffi.PH_FLAG_OLA_NORM if normalize else 0), out.data_ptr())
        assert rc == self.ffi.PH_OK
        return out

    def one_launch(self, normalize):
        """The yardstick: ph_overlap_add / ph_overlap_add_tracks on the whole array, (T, L) on the host."""
        if self.masks is None:
            return self.eng.overlap_add(self.y, self.hop, self.L, self.counts, self.wa, self.ws, normalize).cpu().numpy()[None]
        md = self.torch.as_tensor(self.masks.view(np.int64), device=self.dev)
        return self.eng.overlap_add_tracks(self.y, md, self.hop, self.L, self.counts, self.wa, self.ws, normalize).cpu().numpy()

    def check_partitions(self, what):
        """Every partition, not normalised (finish into a second array) and normalised (finish in place), against the
        one-launch kernel, bit for bit.  -> the normalised result."""
        torch = self.torch
        want_raw, want = self.one_launch(False), self.one_launch(True)
        for name, cuts in partitions(self.W).items():
            acc = self.blocks(cuts, torch.zeros((self.T, self.L), dtype=torch.float64, device=self.dev))
            raw = self.finish(acc, False, torch.empty_like(acc)).cpu().numpy()
            got = self.finish(acc, True, acc).cpu().numpy()
            assert _same_bits(raw, want_raw), (what, name, "raw", int((_bits(raw) != _bits(want_raw)).sum()))
            assert _same_bits(got, want), (what, name, "normalised", int((_bits(got) != _bits(want)).sum()))
        return want


def _hann(N):
    w = sqrt_hann(N) ** 2  # first sample exactly zero
    assert w[0] == 0.0
    return w


# ------------------------------------------------------------------ kernel level: bit for bit
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("N", NS)
def test_blocks_equal_overlap_add_bit_for_bit(eng, torch_dev, N, hop, L):
    rng = np.random.default_rng(N * 1000 + hop * 10 + L)
    hann = _hann(N)
    wa = rng.uniform(-1.0, 1.0, N) ** 2 + 0.1
    for K in KS:
        for W in sorted({_count(L, N, hop), _count(L, N, hop, pad_end=False)} if K == 3 else {_count(L, N, hop)}):
            y = rng.standard_normal((W, K, N))
            counts = rng.integers(0, K + 1, W).astype(np.int32)
            counts[0], counts[-1] = K + 5, -3  # clipped to [0, K]
            if W > 2:
                counts[1] = 0
            behind = np.arange(K)[None, :] >= np.clip(counts, 0, K)[:, None]
            for dtype in DTYPES:
                for windowed in (False, True):
                    for counted in (False, True):
                        bad = y.astype(dtype)
                        if counted:
                            bad[behind] = np.nan  # never read
                        whole = Whole(eng, torch_dev, bad, hop, L, counts if counted else None, None,
                                      wa if windowed else None, hann if windowed else None)
                        got = whole.check_partitions((N, hop, L, K, W, np.dtype(dtype).name, windowed, counted))
                        assert np.all(np.isfinite(got))
                        # exact 0.0 where no frame covers the sample or the window product is zero
                        den = overlap_add_finish_ref(np.zeros((1, L)), N, hop, W, wa if windowed else None,
                                                     hann if windowed else None)[1]
                        assert np.all(_bits(got[0][den <= 0]) == 0)
                        if windowed:
                            assert den[0] == 0.0
                        if hop > N:
                            assert den[N] == 0.0  # the gap behind the first frame
                        if W < _count(L, N, hop) and hop <= N:
                            assert den[-1] == 0.0  # pad_end=False: the tail no whole frame covers


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("N", NS)
def test_blocks_equal_overlap_add_tracks_bit_for_bit(eng, torch_dev, N, hop):
    L = LS[0]
    W = _count(L, N, hop)
    rng = np.random.default_rng(N * 100 + hop)
    hann = _hann(N)
    for K in (5, 64):
        for T in (1, 3):
            y = rng.standard_normal((W, K, N))
            # sparse overlapping words, bits at and above K too; bit 63 in every third frame of track 0
            masks = rng.integers(0, 2**64, (T, W), dtype=np.uint64) & rng.integers(0, 2**64, (T, W), dtype=np.uint64)
            masks[0, ::3] |= np.uint64(1) << np.uint64(63)
            if T == 3:
                masks[1] = masks[0] | masks[2]  # overlaps both
            counts = rng.integers(0, K + 1, W).astype(np.int32)
            counts[0], counts[-1] = K + 5, -3
            any_t = np.bitwise_or.reduce(masks, axis=0)
            named = ((any_t[:, None] >> np.arange(K, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
            behind = np.arange(K)[None, :] >= np.clip(counts, 0, K)[:, None]
            for dtype in DTYPES:
                for full in (False, True):  # without / with counts and windows
                    bad = y.astype(dtype)
                    bad[~named] = np.nan  # rows no mask names
                    if full:
                        bad[behind] = np.nan
                    whole = Whole(eng, torch_dev, bad, hop, L, counts if full else None, masks, hann if full else None,
                                  hann if full else None)
                    got = whole.check_partitions((N, hop, K, T, np.dtype(dtype).name, full))
                    assert np.all(np.isfinite(got))
    # an all-ones mask row is the unrouted walk: the same bits as ph_overlap_add
    y = rng.standard_normal((W, 5, N))
    ones = np.full((1, W), 2**64 - 1, np.uint64)
    a = Whole(eng, torch_dev, y, hop, L, None, ones, hann, hann).check_partitions("all ones")
    assert _same_bits(a, Whole(eng, torch_dev, y, hop, L, None, None, hann, hann).one_launch(True))


# ------------------------------------------------------------------ kernel level: the restatement, the span, the binding
@pytest.mark.parametrize("L,N,hop,K", [(997, 63, 1, 3), (1000, 64, 3, 9), (997, 65, 16, 5), (1000, 64, 64, 1),
                                       (997, 64, 80, 5)])
def test_blocks_against_restatement(eng, torch_dev, L, N, hop, K):
    """(T + 3) 2^-52 mag / den per sample, T = K ceil(N / hop): both sides are float64 sums of at most T terms with one
    product rounding each (the kernel's fused multiply-add rounds once where numpy rounds twice) and one division."""
    rng = np.random.default_rng(L + N + hop)
    W = _count(L, N, hop)
    w = sqrt_hann(N)
    masks = rng.integers(0, 2**64, (3, W), dtype=np.uint64)
    counts = rng.integers(0, K + 1, W).astype(np.int32)
    for dtype in DTYPES:
        y = rng.standard_normal((W, K, N)).astype(dtype)
        cuts = partitions(W)["irregular"]
        for msk in (None, masks):
            whole = Whole(eng, torch_dev, y, hop, L, counts, msk, w, w)
            torch = whole.torch
            acc = whole.blocks(cuts, torch.zeros((whole.T, L), dtype=torch.float64, device=whole.dev))
            got = whole.finish(acc, True, acc).cpu().numpy()
            ref = blocked_ref(y, hop, L, cuts, counts, msk, w, w, True)
            if msk is None:
                _, mag, den = overlap_add_ref(y, hop, L, counts, w, w, True)
                mag = mag[None]
            else:
                _, mag, den = overlap_add_tracks_ref(y, msk, hop, L, counts, w, w, True)
            pos = den > 0
            for t in range(whole.T):
                err, bound = np.abs(got[t] - ref[t]), ola_bound(mag[t], den, K, N, hop)
                print((L, N, hop, K, np.dtype(dtype).name, msk is not None, t), "worst err / bound",
                      float(np.max(err[pos] / np.maximum(bound[pos], 1e-300))))
                assert np.all(err[pos] <= bound[pos]), float(np.max(err[pos] - bound[pos]))
                assert np.all(got[t][~pos] == 0.0)


@pytest.mark.parametrize("N,hop", [(64, 16), (63, 1), (64, 80), (65, 64)])
def test_block_touches_its_span_only(eng, torch_dev, N, hop):
    """Samples outside n0 .. n1 - 1 keep their bits (a sentinel no sum produces); inside, the block adds to what is
    there: zeros give the result of a zeroed acc."""
    torch, dev = torch_dev
    L, K, T = 1000, 3, 2
    W = _count(L, N, hop)
    rng = np.random.default_rng(N + hop)
    y = rng.standard_normal((W, K, N))
    masks = rng.integers(0, 8, (T, W)).astype(np.uint64)
    sent = int(_bits(np.array([SENTINEL]))[0])
    for msk in (None, masks):
        whole = Whole(eng, torch_dev, y, hop, L, None, msk, None, None)
        for f0, Wb in ((0, 1), (1, 2), (W // 2, 7), (W - 3, 3), (W - 1, 1), (0, W)):
            n0, n1 = f0 * hop, min(L, (f0 + Wb - 1) * hop + N)
            clean = whole.blocks([(f0, Wb)], torch.zeros((whole.T, L), dtype=torch.float64, device=dev)).cpu().numpy()
            start = np.full((whole.T, L), SENTINEL)
            start[:, n0:n1] = 0.0
            got = whole.blocks([(f0, Wb)], torch.as_tensor(start, device=dev)).cpu().numpy()
            assert np.all(_bits(got[:, :n0]) == sent) and np.all(_bits(got[:, n1:]) == sent), (N, hop, f0, Wb)
            assert _same_bits(got[:, n0:n1], clean[:, n0:n1])
            assert not clean[:, :n0].any() and not clean[:, n1:].any()
            if msk is None and hop <= N:
                assert np.all(clean[0, n0:n1] != 0.0)  # every sample of the span has a term


def test_binding_numpy_and_tensor_forms(eng, torch_dev):
    """PeriodEngine.overlap_add_block / overlap_add_finish: numpy arrays (acc staged both ways) and device tensors, (L,)
    and (T, L) accumulators, finish into a new array, into `out` and in place, an acc 8 bytes off a 16-byte boundary."""
    torch, dev = torch_dev
    rng = np.random.default_rng(2)
    for N, hop, L, K in ((64, 16, 1000, 5), (63, 3, 997, 3), (65, 80, 1000, 9)):
        W = _count(L, N, hop)
        w = sqrt_hann(N)
        y = rng.standard_normal((W, K, N))
        counts = rng.integers(0, K + 1, W).astype(np.int32)
        masks = rng.integers(0, 2**64, (3, W), dtype=np.uint64)
        want = eng.overlap_add(y, hop, L, counts, w, w, True)
        want_t = eng.overlap_add_tracks(y, masks, hop, L, counts, w, w, True)
        y_d, c_d, w_d = (torch.as_tensor(a, device=dev) for a in (y, counts, w))
        m_d = torch.as_tensor(masks.view(np.int64), device=dev)
        for name in ("B=7", "irregular"):
            cuts = partitions(W)[name]
            # numpy
            acc, acc_t = np.zeros(L), np.zeros((3, L))
            for f0, Wb in cuts:
                s = slice(f0, f0 + Wb)
                assert eng.overlap_add_block(y[s], hop, L, f0, acc, counts[s], None, w) is acc
                eng.overlap_add_block(y[s], hop, L, f0, acc_t, counts[s], np.ascontiguousarray(masks[:, s]), w)
            out = eng.overlap_add_finish(acc, N, hop, W, w, w)
            assert out is not acc and out.shape == (L,) and _same_bits(out, want)
            assert _same_bits(eng.overlap_add_finish(acc_t, N, hop, W, w, w, True, out=np.empty((3, L))), want_t)
            assert eng.overlap_add_finish(acc_t, N, hop, W, w, w, out=acc_t) is acc_t and _same_bits(acc_t, want_t)
            # device tensors; the (L,) accumulator misaligned
            buf = torch.zeros(L + 3, dtype=torch.float64, device=dev)
            acc = buf[1 : L + 1] if buf.data_ptr() % 16 == 0 else buf[2 : L + 2]
            assert acc.data_ptr() % 16 == 8
            acc_t = torch.zeros((3, L), dtype=torch.float64, device=dev)
            for f0, Wb in cuts:
                s = slice(f0, f0 + Wb)
                assert eng.overlap_add_block(y_d[s], hop, L, f0, acc, c_d[s], None, w_d) is acc
                eng.overlap_add_block(y_d[s], hop, L, f0, acc_t, c_d[s], m_d[:, s], w_d)
            assert eng.overlap_add_finish(acc, N, hop, W, w_d, w_d, out=acc) is acc
            assert _same_bits(acc.cpu().numpy(), want) and not buf[0].item() and not buf[L + 2].item()
            got_t = eng.overlap_add_finish(acc_t, N, hop, W, w_d, w_d)
            assert got_t.is_cuda and got_t.data_ptr() != acc_t.data_ptr() and _same_bits(got_t.cpu().numpy(), want_t)
    # (W, N) input is K = 1; an empty block adds nothing; what the library refuses is a ValueError
    y1 = rng.standard_normal((4, 16))
    a, b = np.zeros(40), np.zeros(40)
    eng.overlap_add_block(y1, 8, 40, 0, a)
    eng.overlap_add_block(y1[:, None, :], 8, 40, 0, b)
    eng.overlap_add_block(y1[:0], 8, 40, 2, b)
    assert _same_bits(a, b) and _same_bits(eng.overlap_add_finish(a, 16, 8, 4), eng.overlap_add(y1, 8, 40))
    with pytest.raises(ValueError):
        eng.overlap_add_block(y1, 8, 40, 2, a)  # frame 5 starts at sample 40
    with pytest.raises(ValueError):
        eng.overlap_add_block(y1, 8, 40, -1, a)
    with pytest.raises(ValueError):
        eng.overlap_add_finish(a, 16, 8, 6)
    with pytest.raises(ValueError):
        eng.overlap_add_block(np.zeros((2, 65, 16)), 8, 40, 0, np.zeros((1, 40)), masks=np.zeros((1, 2), np.uint64))


def test_many_frames_in_blocks_of_4096(eng, torch_dev):
    """70 000 frames: more than a 16-bit grid dimension holds, f0 * K * N past 2^23 elements, blocks of 4 096."""
    torch, dev = torch_dev
    W, K, N, hop, B = 70_000, 2, 64, 16, 4096
    L = (W - 1) * hop + N
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    y = torch.randn((W, K, N), dtype=torch.float64, device=dev, generator=gen)
    w = torch.as_tensor(sqrt_hann(N), device=dev)
    want = eng.overlap_add(y, hop, L, None, w, w, True)
    acc = torch.zeros(L, dtype=torch.float64, device=dev)
    for f0 in range(0, W, B):
        eng.overlap_add_block(y[f0 : f0 + B], hop, L, f0, acc, None, None, w)
    eng.overlap_add_finish(acc, N, hop, W, w, w, out=acc)
    assert bool(torch.equal(acc.view(torch.int64), want.view(torch.int64)))
    assert bool(torch.isfinite(acc).all()) and float(acc.abs().max()) > 0.0


def test_bad_arguments_launch_nothing(eng):
    from pyperiod_amd import _ffi

    lib, ctx = eng._lib, eng._ctx
    y, acc = np.zeros((4, 2, 16)), np.zeros((3, 100))
    masks = np.ones((3, 4), np.uint64)
    yy, a, m = y.ctypes.data, acc.ctypes.data, masks.ctypes.data
    E = _ffi.PH_E_ARG
    eng.profile(True)
    try:
        for dev in (0, _ffi.PH_FLAG_DEVICE):
            def block(y=yy, dt=0, Wb=4, K=2, N=16, hop=8, L=100, f0=3, masks=m, T=3, acc=a):
                return lib.ph_overlap_add_block(ctx, y, dt, Wb, K, N, hop, L, f0, None, masks, T, None, dev, acc)

            def finish(acc=a, T=3, N=16, hop=8, L=100, W=12, out=a):
                return lib.ph_overlap_add_finish(ctx, acc, T, N, hop, L, W, None, None, dev, out)

            for bad in (dict(y=None), dict(acc=None), dict(dt=3), dict(Wb=0), dict(K=0), dict(N=0), dict(hop=0), dict(L=0),
                        dict(f0=-1), dict(f0=10), dict(f0=9, L=96), dict(masks=None), dict(masks=None, T=0), dict(T=0),
                        dict(K=65)):
                assert block(**bad) == E, bad
            for bad in (dict(acc=None), dict(out=None), dict(T=0), dict(N=0), dict(hop=0), dict(L=0), dict(W=0), dict(W=14)):
                assert finish(**bad) == E, bad
        assert eng.profile_read() == []
        # and good calls are recorded: K = 65 without masks is fine
        eng.overlap_add_block(np.zeros((4, 65, 16)), 8, 100, 9, np.zeros(100))
        eng.overlap_add_block(y, 8, 100, 3, acc, masks=masks)
        eng.overlap_add_finish(acc, 16, 8, 13)
        assert [n for n, _ in eng.profile_read()] == ["k_overlap_add_block", "k_overlap_add_block", "k_overlap_add_finish"]
    finally:
        eng.profile(False)


# ------------------------------------------------------------------ end to end
E_N, E_HOP, E_W = 96, 24, 240
E_L = E_N + E_HOP * (E_W - 1) - 5  # the last frame is zero-padded
METHODS = [("m_best", {"num": 3}), ("m_best_gamma", {}), ("best_correlation", {}), ("best_frequency", {"num": 2}),
           ("small_to_large", {"thresh": 0.1})]


def _recording(method=None):
    """Two sinusoids of periods 12 and 17 under a little noise: every method completes on every frame (no frame without a
    positive norm, no spectrum whose peak is bin 0), and the periods fit a frame of 96 samples several times."""
    n = np.arange(E_L)
    return (np.sin(2 * np.pi * n / 12.0) + 0.7 * np.sin(2 * np.pi * n / 17.0 + 1.0)
            + 0.05 * np.random.default_rng(1).standard_normal(E_L))


def _short_time():
    from pyperiod_amd import ShortTime

    st = ShortTime(E_N, E_HOP, window=sqrt_hann(E_N))
    assert st.frame_count(E_L) == E_W
    return st


def _same_fields(got, want, what):
    assert type(got) is type(want)
    for name, g, w in zip(want._fields, got, want):
        if w is None or isinstance(w, list):
            assert g == w, (what, name)
            continue
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)  # bit for bit, NaN and -0.0 included


@pytest.mark.parametrize("method,kwargs", METHODS)
def test_analyze_in_blocks_is_analyze(eng, method, kwargs):
    st, x = _short_time(), _recording(method)
    want = st.analyze(x, method=method, **kwargs)
    assert want.periods.shape[0] == E_W and np.any(want.periodic != 0.0)
    for B in (1, 3, E_W - 1, E_W + 5):
        _same_fields(st.analyze(x, method=method, block_frames=B, **kwargs), want, (method, B))
    _same_fields(st.analyze(x.astype(np.float32), method=method, block_frames=np.int64(50), **kwargs),
                 st.analyze(x.astype(np.float32), method=method, **kwargs), (method, "float32 signal"))


def test_analyze_in_blocks_float32_frames_no_window_and_num_zero(eng):
    from pyperiod_amd import ShortTime

    x = _recording("m_best")
    st = ShortTime(E_N, 100, dtype=np.float32, pad_end=False)  # hop > N: gaps, and whole frames only
    _same_fields(st.analyze(x, "m_best", 7, num=2), st.analyze(x, "m_best", num=2), "float32 frames")
    st = _short_time()
    _same_fields(st.analyze(x, "m_best", block_frames=7, num=0), st.analyze(x, "m_best", num=0), "num = 0")
    _same_fields(st.decompose(x, "m_best", tracks=[12], block_frames=7, num=0), st.decompose(x, "m_best", tracks=[12], num=0),
                 "num = 0, tracks")


def _launches(eng, call):
    eng.profile(True)
    try:
        res = call()
        return res, [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)


@pytest.mark.parametrize("method,kwargs", [("m_best", {"num": 3}), ("small_to_large", {"thresh": 0.1})])
def test_decompose_in_blocks_is_decompose(eng, method, kwargs):
    st, x = _short_time(), _recording(method)
    tracks = [12, (17, 34), 5]
    want_t, names = _launches(eng, lambda: st.decompose(x, method=method, tracks=tracks, **kwargs))
    want_r = st.decompose(x, method=method, max_tracks=4, **kwargs)
    assert names[0] == "k_frames" and names.count("k_frames") == 1 and "k_overlap_add_block" not in names
    # a kernel of the method that one run of it launches once
    first = next(n for n in names[1:] if names.count(n) == 1 and not n.startswith("k_overlap_add"))
    assert np.any(want_t.tracks != 0.0) and np.any(want_r.tracks != 0.0) and len(want_r.track_periods) == 4
    for B in (1, 3, E_W - 1, E_W + 5):
        _same_fields(st.decompose(x, method=method, tracks=tracks, block_frames=B, **kwargs), want_t, (method, B, "tracks"))
        _same_fields(st.decompose(x, method=method, max_tracks=4, block_frames=B, **kwargs), want_r, (method, B, "ranked"))
    # the launches (the profile keeps the first 256: few blocks): with tracks the method runs once per block and every
    # block is added twice, (L) and (T + 1, L); the ranking costs a second run of the method and no third overlap-add
    for B in (E_W - 1, 64):
        nb = -(-E_W // B)
        _, names = _launches(eng, lambda: st.decompose(x, method=method, tracks=tracks, block_frames=B, **kwargs))
        assert len(names) < 256
        assert names.count("k_frames") == nb and names.count(first) == nb
        assert names.count("k_overlap_add_block") == 2 * nb and names.count("k_overlap_add_finish") == 2
        assert "k_overlap_add" not in names and "k_overlap_add_tracks" not in names
        _, names = _launches(eng, lambda: st.decompose(x, method=method, max_tracks=4, block_frames=B, **kwargs))
        assert len(names) < 256
        assert names.count("k_frames") == 2 * nb and names.count(first) == 2 * nb
        assert names.count("k_overlap_add_block") == 2 * nb and names.count("k_overlap_add_finish") == 2
        _, names = _launches(eng, lambda: st.analyze(x, method=method, block_frames=B, **kwargs))
        assert names.count("k_frames") == nb and names.count(first) == nb
        assert names.count("k_overlap_add_block") == nb and names.count("k_overlap_add_finish") == 1


@pytest.mark.parametrize("method,kwargs", [("m_best", {"num": 3}), ("small_to_large", {"thresh": 0.1})])
def test_unblocked_calls_launch_one_block_and_no_block_kernel(eng, method, kwargs):
    """Without ``block_frames``: one k_frames, one run of the method, the one-launch overlap-adds (decompose: the routed
    one first) and neither block kernel -- with ranked tracks too, which need no second run of the method."""
    st, x = _short_time(), _recording(method)
    blocked = {"k_overlap_add_block", "k_overlap_add_finish"}
    _, names = _launches(eng, lambda: st.analyze(x, method=method, **kwargs))
    assert len(names) < 256
    assert names[0] == "k_frames" and names.count("k_frames") == 1
    assert names[-1] == "k_overlap_add" and names.count("k_overlap_add") == 1
    assert "k_overlap_add_tracks" not in names and not blocked & set(names)
    # a kernel of the method that one run of it launches once
    first = next(n for n in names[1:] if names.count(n) == 1 and not n.startswith("k_overlap_add"))
    for kw in ({"tracks": [12, (17, 34), 5]}, {"max_tracks": 4}):
        _, got = _launches(eng, lambda: st.decompose(x, method=method, **kw, **kwargs))
        assert len(got) < 256
        assert got[0] == "k_frames" and got.count("k_frames") == 1 and got.count(first) == 1, kw
        assert got[-2:] == ["k_overlap_add_tracks", "k_overlap_add"], kw
        assert got.count("k_overlap_add_tracks") == 1 and got.count("k_overlap_add") == 1 and not blocked & set(got), kw
        assert got[1:-2] == names[1:-1], kw  # the method's kernels once, as analyze launches them: not twice


def test_bad_frame_in_a_late_block_raises_what_the_unblocked_call_raises(eng):
    st = _short_time()
    x = _recording()
    bad = 200  # frames 200 and 201 are all zero; blocks of 16: block 12
    x[bad * E_HOP : bad * E_HOP + E_N + E_HOP] = 0.0
    for call, kw in ((st.analyze, {}), (st.decompose, {}), (st.decompose, {"tracks": [12]})):
        with pytest.raises(TypeError, match=f"frame {bad}$") as want:  # (the partly zero frames before it complete)
            call(x, method="m_best", num=2, **kw)
        for B in (16, 1, E_W):
            with pytest.raises(TypeError) as got:
                call(x, method="m_best", num=2, block_frames=B, **kw)
            assert str(got.value) == str(want.value)
    with pytest.raises(OverflowError) as want:
        st.analyze(x, method="best_frequency", num=1)
    with pytest.raises(OverflowError) as got:
        st.analyze(x, method="best_frequency", num=1, block_frames=16)
    assert str(got.value) == str(want.value) and "frame" in str(want.value)


def test_blocked_run_holds_one_block_on_the_device(eng, torch_dev):
    """m_best with num = 8, N = 256, hop = 64, 400 frames, blocks of 16.  Torch's peak allocation of the blocked run,
    less its fixed arrays (the signal, the window, the running sum; the per-frame results live on the host), is at most
    3 x one block's frames plus bases: the factor covers the method's own results and temporaries and one block not yet
    released.  That is under a quarter of the (W, num, N) bases, which the unblocked run is seen to allocate."""
    from pyperiod_amd import ShortTime

    torch, dev = torch_dev
    N, hop, W, num, B = 256, 64, 400, 8, 16
    L = N + hop * (W - 1)
    st = ShortTime(N, hop, window=sqrt_hann(N))
    assert st.frame_count(L) == W
    x = readme_window(L, seed=0)

    def peak(**kw):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        res = st.analyze(x, "m_best", num=num, **kw)
        torch.cuda.synchronize(dev)
        return res, torch.cuda.max_memory_allocated(dev) - base

    want, unblocked = peak()
    got, blocked = peak(block_frames=B)
    _same_fields(got, want, "memory shape")
    bases = W * num * N * 8
    block = B * N * 8 + B * num * N * 8
    fixed = L * 8 + N * 8 + L * 8
    print("peak bytes: unblocked", unblocked, "blocked", blocked, "fixed", fixed, "one block", block, "bases", bases)
    assert unblocked >= bases
    assert blocked - fixed <= 3 * block
    assert 3 * block < bases / 4
