"""The blocked overlap-add without a GPU: numpy restatements of k_overlap_add_block / k_overlap_add_finish as loops in the
kernels' order, which tests/test_gpu_short_time_blocks.py holds the kernels to; the partitions both files walk; the
refusals of ``block_frames``; the two new C-ABI symbols and every refusal of their entry points.

Order.  A lane of k_overlap_add_block owns one (t, n): it loads the running sum, walks the block's frames that cover n in
ascending f and their rows in ascending k, and stores it back.  ``overlap_add_block_ref`` loops over f, then k, and adds a
whole row at a time: the samples of one row are distinct, so every sample sees exactly the lane's order.  A later block
continues where the one before stopped, hence on float data any partition gives the bits of one block.  The one-launch
restatements of test_short_time_cpu.py / test_short_time_tracks_cpu.py add in another order (k outside f), so the
comparison with them runs on integer-valued data under an integer window, where every sum is exact."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_short_time_cpu import cpu_engine, overlap_add_ref
from test_short_time_tracks_cpu import overlap_add_tracks_ref


# ------------------------------------------------------------------ restatements
def overlap_add_block_ref(acc, y, hop, L, f0, counts=None, masks=None, ws=None):
    """acc (T, L) float64 += the frames f0 .. f0 + Wb - 1: y (Wb, K, N), counts (Wb), masks (T, Wb) block-local.  In
    place; -> (n0, n1), the span of samples the kernel may touch."""
    y = np.asarray(y)
    if y.ndim == 2:
        y = y[:, None, :]
    Wb, K, N = y.shape
    T = acc.shape[0]
    assert acc.shape == (T, L) and (masks is not None or T == 1) and (f0 + Wb - 1) * hop < L
    ws = np.ones(N) if ws is None else ws
    if masks is not None:
        masks = np.asarray(masks).view(np.uint64)
        assert masks.shape == (T, Wb) and K <= 64
    for t in range(T):
        for fb in range(Wb):
            lo = (f0 + fb) * hop
            n = min(N, L - lo)
            kf = K if counts is None else min(max(int(counts[fb]), 0), K)
            for k in range(kf):
                if masks is not None and not (int(masks[t, fb]) >> k) & 1:
                    continue
                acc[t, lo : lo + n] += ws[:n] * y[fb, k, :n].astype(np.float64)
    return f0 * hop, min(L, (f0 + Wb - 1) * hop + N)


def overlap_add_finish_ref(acc, N, hop, W, wa=None, ws=None, normalize=True):
    """-> (out, den): acc (T, L) over the overlap-added window product of all W frames (ascending f), 0.0 where that is
    not positive; acc itself when not normalised."""
    T, L = acc.shape
    wa = np.ones(N) if wa is None else wa
    ws = np.ones(N) if ws is None else ws
    den = np.zeros(L)
    for f in range(W):
        n = min(N, L - f * hop)
        den[f * hop : f * hop + n] += (wa * ws)[:n]
    if not normalize:
        return acc.copy(), np.ones(L)
    out = np.zeros((T, L))
    pos = den > 0
    out[:, pos] = acc[:, pos] / den[pos]
    return out, den


def partitions(W):
    """The partitions of W frames into blocks [(f0, Wb), ...]: all blocks of 1, 2, 7, W - 1, W and W + 3 frames, and
    one irregular one (1, 5, 2, the rest)."""
    out = {}
    for B in (1, 2, 7, W - 1, W, W + 3):
        if B >= 1:
            out[f"B={B}"] = [(f0, min(B, W - f0)) for f0 in range(0, W, B)]
    cuts, f0 = [], 0
    for Wb in (1, 5, 2, W):
        Wb = min(Wb, W - f0)
        if Wb > 0:
            cuts.append((f0, Wb))
            f0 += Wb
    out["irregular"] = cuts
    return out


def blocked_ref(y, hop, L, cuts, counts=None, masks=None, wa=None, ws=None, normalize=True):
    """overlap_add_block_ref over `cuts`, then overlap_add_finish_ref: -> (T, L)."""
    W = y.shape[0]
    assert sorted(f for f0, Wb in cuts for f in range(f0, f0 + Wb)) == list(range(W))  # every frame exactly once
    T = 1 if masks is None else masks.shape[0]
    acc = np.zeros((T, L))
    for f0, Wb in cuts:
        overlap_add_block_ref(acc, y[f0 : f0 + Wb], hop, L, f0, None if counts is None else counts[f0 : f0 + Wb],
                              None if masks is None else masks[:, f0 : f0 + Wb], ws)
    return overlap_add_finish_ref(acc, y.shape[-1], hop, W, wa, ws, normalize)[0]


def frame_count(L, N, hop):
    from pyperiod_amd import ShortTime

    return ShortTime(N, hop).frame_count(L)


SHAPES = [(997, 63, 1, 3), (1000, 64, 3, 5), (997, 65, 16, 9), (1000, 64, 64, 1), (997, 64, 80, 4), (200, 64, 16, 64)]


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("L,N,hop,K", SHAPES)
def test_integer_data_equals_the_one_launch_restatements(L, N, hop, K):
    rng = np.random.default_rng(L + 10 * N + hop)
    W = frame_count(L, N, hop)
    y = rng.integers(-8, 9, (W, K, N)).astype(np.float64)
    win = rng.integers(0, 4, N).astype(np.float64)
    win[0] = 0.0
    counts = rng.integers(-1, K + 2, W).astype(np.int32)
    masks = rng.integers(0, 2**63, (3, W)).astype(np.uint64) | (np.uint64(1) << np.uint64(63))
    for normalize in (False, True):
        for cnt, wa, ws in ((None, None, None), (counts, win, win), (counts, win + 1.0, win)):
            want = overlap_add_ref(y, hop, L, cnt, wa, ws, normalize)[0]
            want_t = overlap_add_tracks_ref(y, masks, hop, L, cnt, wa, ws, normalize)[0] if K <= 64 else None
            for name, cuts in partitions(W).items():
                got = blocked_ref(y, hop, L, cuts, cnt, None, wa, ws, normalize)
                assert np.array_equal(got[0], want), (name, normalize)
                if name in ("B=1", "B=7", "irregular"):  # (the routed walk is slow in python: three partitions)
                    got_t = blocked_ref(y, hop, L, cuts, cnt, masks, wa, ws, normalize)
                    assert np.array_equal(got_t, want_t), (name, normalize)


@pytest.mark.parametrize("L,N,hop,K", SHAPES[:5])
def test_float_data_any_partition_gives_the_bits_of_one_block(L, N, hop, K):
    rng = np.random.default_rng(7 * L + N + hop)
    W = frame_count(L, N, hop)
    y = rng.standard_normal((W, K, N))
    win = rng.uniform(-1.0, 1.0, N)
    counts = rng.integers(0, K + 1, W).astype(np.int32)
    masks = rng.integers(0, 2**63, (2, W)).astype(np.uint64)
    parts = partitions(W)
    one = blocked_ref(y, hop, L, parts[f"B={W}"], counts, None, win, win, True)
    one_t = blocked_ref(y, hop, L, parts[f"B={W}"], counts, masks, win, win, True)
    for name, cuts in parts.items():
        assert np.array_equal(blocked_ref(y, hop, L, cuts, counts, None, win, win, True), one), name
        if name in ("B=2", "irregular"):
            assert np.array_equal(blocked_ref(y, hop, L, cuts, counts, masks, win, win, True), one_t), name
    # and the one-launch restatement agrees to rounding (another order of the same terms)
    ref = overlap_add_ref(y, hop, L, counts, win, win, True)[0]
    assert np.allclose(one[0], ref, rtol=1e-9, atol=1e-12)


def test_block_touches_its_span_only():
    L, N, hop, K = 300, 16, 5, 2
    W = frame_count(L, N, hop)
    y = np.ones((W, K, N))
    for f0, Wb in ((0, 3), (4, 1), (W - 2, 2)):
        acc = np.full((1, L), 7.0)
        n0, n1 = overlap_add_block_ref(acc, y[f0 : f0 + Wb], hop, L, f0)
        assert np.all(acc[0, :n0] == 7.0) and np.all(acc[0, n1:] == 7.0) and np.all(acc[0, n0:n1] > 7.0)
        assert n0 == f0 * hop and n1 <= L


def test_partitions_cover_every_frame_once():
    for W in (1, 2, 3, 8, 9, 60):
        parts = partitions(W)
        assert "irregular" in parts and f"B={W}" in parts and f"B={W + 3}" in parts
        assert parts[f"B={W}"] == parts[f"B={W + 3}"] == [(0, W)]
        for cuts in parts.values():
            assert [f for f0, Wb in cuts for f in range(f0, f0 + Wb)] == list(range(W))


def test_block_frames_is_refused_before_the_gpu(monkeypatch):
    import sys

    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)
    st = ShortTime(64, 16)
    x = np.zeros(400)
    for bad in (True, False, 0, -1, -7, 2.0, 1.5, "4", np.float64(3), [4], np.array([4])):
        with pytest.raises(ValueError, match="block_frames"):
            st.analyze(x, block_frames=bad)
        with pytest.raises(ValueError, match="block_frames"):
            st.decompose(x, block_frames=bad)
        with pytest.raises(ValueError, match="block_frames"):
            st.decompose(x, tracks=[12], block_frames=bad)
    # what analyze / decompose refuse without blocks they refuse with them, still without a GPU
    with pytest.raises(ValueError):
        st.analyze(x, method="find_periods", block_frames=4)
    with pytest.raises(TypeError):
        st.analyze(x, block_frames=4, nmu=2)
    with pytest.raises(ValueError):
        st.decompose(x, tracks=[], block_frames=4)
    with pytest.raises(ValueError):
        st.decompose(x, num=65, block_frames=np.int64(4))
    # a good value gets as far as the engine
    for good in (1, 4, np.int32(9), 10**6):
        with pytest.raises(AssertionError, match="GPU was touched"):
            st.analyze(x, block_frames=good)
        with pytest.raises(AssertionError, match="GPU was touched"):
            st.decompose(x, block_frames=good)


def test_symbols_in_binding_header_and_library():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "pyperiod_amd", "libperiod_hip.so"))
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint}
    for name, arity in (("ph_overlap_add_block", 15), ("ph_overlap_add_finish", 11)):
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == arity and len(_ffi.SIGNATURES[name]) == arity
        for arg, have in zip(args, _ffi.SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]]
            assert have is want, (name, arg)
        assert getattr(lib, name)  # exported by the built library
        assert getattr(_ffi.load(), name).argtypes == _ffi.SIGNATURES[name]


def test_entry_points_reject_bad_arguments_without_gpu():
    """Every refusal comes before the first HIP call and before the context is looked at: a block of zeros stands in
    for the context, and the arrays are never read."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    ctx = ctypes.addressof((ctypes.c_char * 4096)())
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    big = 2**63 - 1

    good = dict(ctx=ctx, y=buf, dtype=0, Wb=4, K=2, N=16, hop=8, L=100, f0=3, counts=None, masks=None, T=1, ws=None,
                flags=0, acc=buf)

    def block(**change):
        a = dict(good, **change)
        return lib.ph_overlap_add_block(a["ctx"], a["y"], a["dtype"], a["Wb"], a["K"], a["N"], a["hop"], a["L"], a["f0"],
                                        a["counts"], a["masks"], a["T"], a["ws"], a["flags"], a["acc"])

    for dev in (0, _ffi.PH_FLAG_DEVICE):
        assert block(ctx=None, flags=dev) == E and b"ctx" in lib.ph_last_error()
        for name in ("y", "acc"):
            assert block(flags=dev, **{name: None}) == E and b"NULL" in lib.ph_last_error()
        for dt in (2, 7, -1):
            assert block(flags=dev, dtype=dt) == E and b"dtype" in lib.ph_last_error()
        for name in ("Wb", "K", "N", "hop", "L"):
            for v in (0, -1):
                assert block(flags=dev, **{name: v}) == E, (name, v)
        assert block(flags=dev, f0=-1) == E and b"f0" in lib.ph_last_error()
        assert block(flags=dev, f0=big) == E and b"behind" in lib.ph_last_error()
        assert block(flags=dev, f0=10) == E and b"behind" in lib.ph_last_error()  # (10 + 3) * 8 = 104 >= 100
        assert block(flags=dev, f0=9, L=96) == E and b"behind" in lib.ph_last_error()  # (f0 + Wb - 1) hop == L
        assert block(flags=dev, f0=0, L=24) == E and b"behind" in lib.ph_last_error()
        assert block(flags=dev, Wb=big, f0=big) == E
        for T in (0, 2, 3, -1, big):
            assert block(flags=dev, T=T) == E and b"T=" in lib.ph_last_error(), T  # no masks: T must be 1
        for T in (0, -1):
            assert block(flags=dev, masks=buf, T=T) == E and b"T=" in lib.ph_last_error()
        assert block(flags=dev, masks=buf, T=3, K=65) == E and b"K=65" in lib.ph_last_error()
        assert block(flags=dev, masks=buf, T=3, K=2**31 - 1) == E
        # the 64-bit size products: Wb K N 8, T L 8, T Wb 8
        assert block(flags=dev, Wb=big // 2, K=64, N=2**31 - 1, hop=1, L=big, f0=0) == E
        assert b"W * K * N" in lib.ph_last_error()
        assert block(flags=dev, masks=buf, T=3, L=big // 16) == E and b"T * L" in lib.ph_last_error()
        assert block(flags=dev, masks=buf, T=big) == E
        assert block(flags=dev, masks=buf, T=1 << 21, Wb=1 << 40, K=1, N=1, hop=1, L=1 << 41, f0=5) == E

    fgood = dict(ctx=ctx, acc=buf, T=3, N=16, hop=8, L=100, W=12, wa=None, ws=None, flags=0, out=buf)

    def finish(**change):
        a = dict(fgood, **change)
        return lib.ph_overlap_add_finish(a["ctx"], a["acc"], a["T"], a["N"], a["hop"], a["L"], a["W"], a["wa"], a["ws"],
                                         a["flags"], a["out"])

    for dev in (0, _ffi.PH_FLAG_DEVICE, _ffi.PH_FLAG_DEVICE | _ffi.PH_FLAG_OLA_NORM):
        assert finish(ctx=None, flags=dev) == E and b"ctx" in lib.ph_last_error()
        for name in ("acc", "out"):
            assert finish(flags=dev, **{name: None}) == E and b"NULL" in lib.ph_last_error()
        for name in ("T", "N", "hop", "L", "W"):
            for v in (0, -1):
                assert finish(flags=dev, **{name: v}) == E, (name, v)
        assert finish(flags=dev, W=14, L=104) == E and b"behind" in lib.ph_last_error()  # (W - 1) hop == L
        assert finish(flags=dev, L=big // 16) == E and b"T * L" in lib.ph_last_error()
        assert finish(flags=dev, T=big) == E
        assert finish(flags=dev, W=1 << 40, N=1, hop=1, L=1 << 40, T=1 << 21) == E


def test_binding_checks_its_arrays_before_the_library():
    """acc is written in place, so the binding takes it as it is or not at all; with torch input every side array is a
    tensor on the device of y."""
    import torch

    eng, Reached = cpu_engine()
    y, masks = torch.zeros((4, 2, 16), dtype=torch.float64), torch.ones((3, 4), dtype=torch.int64)
    acc1, acc3 = torch.zeros(40, dtype=torch.float64), torch.zeros((3, 40), dtype=torch.float64)
    with pytest.raises(Reached):
        eng.overlap_add_block(y, 4, 40, 2, acc1)
    with pytest.raises(Reached):
        eng.overlap_add_block(y, 4, 40, 2, acc3, torch.ones(4, dtype=torch.int32), masks, torch.ones(16, dtype=torch.float64))
    with pytest.raises(Reached):
        eng.overlap_add_finish(acc3, 16, 4, 7, out=acc3)
    for call in (lambda: eng.overlap_add_block(y, 4, 40, 2, acc1.numpy()),
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc1.to(torch.float32)),
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc3, masks=masks.numpy()),
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc1, counts=np.ones(4, np.int32)),
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc1, win_s=np.ones(16)),
                 lambda: eng.overlap_add_finish(acc3, 16, 4, 7, win_a=np.ones(16)),
                 lambda: eng.overlap_add_finish(acc3, 16, 4, 7, out=np.zeros((3, 40)))):
        with pytest.raises(TypeError, match="on the device of"):
            call()
    for call in (lambda: eng.overlap_add_block(y, 4, 40, 2, acc3),  # T = 3 without masks
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc1, masks=masks),  # T = 1 with three mask rows
                 lambda: eng.overlap_add_block(y, 4, 41, 2, acc1),  # another length
                 lambda: eng.overlap_add_block(y, 4, 40, 2, torch.zeros((3, 80), dtype=torch.float64)[:, ::2], masks=masks),
                 lambda: eng.overlap_add_block(y, 4, 40, 2, acc3, masks=masks[:, :3]),
                 lambda: eng.overlap_add_finish(acc3, 16, 4, -1),
                 lambda: eng.overlap_add_finish(acc3, 16, 4, 7, out=acc1),
                 lambda: eng.overlap_add_finish(acc3, 16, 4, 7, win_s=torch.ones(15, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()
    # numpy: a float64 C-contiguous array or nothing (a copy would lose the sum)
    yn = np.zeros((4, 2, 16))
    for bad in (np.zeros(40, np.float32), [0.0] * 40):
        with pytest.raises(TypeError):
            PeriodEngineless().overlap_add_block(yn, 4, 40, 2, bad)
    with pytest.raises(ValueError):
        PeriodEngineless().overlap_add_block(yn, 4, 40, 2, np.zeros(80)[::2])


def PeriodEngineless():
    """A PeriodEngine without a context for numpy input: reaching the library is an error."""
    from pyperiod_amd.engine import PeriodEngine

    def call(*a, **k):
        raise AssertionError("the library was reached")

    eng = object.__new__(PeriodEngine)
    eng._call, eng._lib = call, type("Lib", (), {"__getattr__": lambda self, name: name})()
    return eng
