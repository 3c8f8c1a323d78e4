"""ShortTime.decompose_qo without a GPU: the numpy restatement of the routed overlap-add of periodic segments that
tests/test_gpu_short_time_qo.py holds k_overlap_add_periodic to, its agreement with the dense restatement of
tests/test_short_time_tracks_cpu.py on explicitly tiled rows, the new C-ABI symbol, every refusal of the entry point
and the argument errors of decompose_qo.

The restatement walks the frames in ascending f and a frame's blocks in ascending a -- the order of the kernel -- and
honours its stop rule: the blocks of a frame from the first with p < 1 or off + p > ccap on contribute nothing.  Its
per-sample bound is test_short_time_cpu.ola_bound with K the largest number of blocks one (track, frame) routes: both
sides are float64 sums of the same at most K * ceil(N / hop) terms."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_short_time_cpu import cpu_engine, ola_bound, sqrt_hann
from test_short_time_tracks_cpu import overlap_add_tracks_ref


# ------------------------------------------------------------------ restatement
def block_walk(periods, counts, ccap):
    """-> (valid (W, pcap) bool, off (W, pcap) int64): the blocks the kernel's walk reaches and their offsets."""
    periods = np.asarray(periods, dtype=np.int64)
    W, pcap = periods.shape
    valid, offs = np.zeros((W, pcap), bool), np.zeros((W, pcap), np.int64)
    for f in range(W):
        off = 0
        for a in range(min(max(int(counts[f]), 0), pcap, 64)):
            p = int(periods[f, a])
            if p < 1 or off + p > ccap:
                break
            valid[f, a], offs[f, a] = True, off
            off += p
    return valid, offs


def routed_blocks(periods, counts, masks, ccap):
    """(T, W, pcap) bool: block a of frame f is added to track t."""
    valid, _ = block_walk(periods, counts, ccap)
    masks = np.asarray(masks).view(np.uint64)
    pcap = valid.shape[1]
    bits = np.zeros(masks.shape + (pcap,), bool)
    for a in range(min(pcap, 64)):
        bits[:, :, a] = ((masks >> np.uint64(a)) & np.uint64(1)) != 0
    return bits & valid[None, :, :]


def ola_periodic_ref(seg, periods, counts, masks, N, hop, L, wa=None, ws=None, normalize=True):
    """-> (out, mag, den, K): out and mag (T, L) -- the routed overlap-add of the tiled segments and the sum of
    |ws * value| over the same terms --, den (L) the overlap-added window product (ones when not normalised) and K the
    largest number of blocks one (track, frame) routes (at least 1)."""
    seg = np.asarray(seg, dtype=np.float64)
    periods = np.asarray(periods, dtype=np.int64)
    W, ccap = seg.shape
    valid, offs = block_walk(periods, counts, ccap)
    routed = routed_blocks(periods, counts, masks, ccap)
    T = routed.shape[0]
    wa = np.ones(N) if wa is None else wa
    ws = np.ones(N) if ws is None else ws
    num, mag, den = np.zeros((T, L)), np.zeros((T, L)), np.zeros(L)
    i = np.arange(N)
    for f in range(W):  # ascending f for every sample, ascending a inside a frame: the kernel's order
        lo = f * hop
        n = min(N, L - lo)
        if n <= 0:
            continue
        den[lo : lo + n] += (wa * ws)[:n]
        for a in np.flatnonzero(routed[:, f, :].any(axis=0)):
            p = int(periods[f, a])
            term = ws * seg[f, offs[f, a] + i % p]  # the segment tiled to N
            for t in np.flatnonzero(routed[:, f, a]):
                num[t, lo : lo + n] += term[:n]
                mag[t, lo : lo + n] += np.abs(term[:n])
    K = max(1, int(routed.sum(axis=2).max())) if routed.size else 1
    if not normalize:
        return num, mag, np.ones(L), K
    out = np.zeros((T, L))
    pos = den > 0
    out[:, pos] = num[:, pos] / den[pos]
    return out, mag, den, K


def tile_segments(seg, periods, counts, N):
    """The dense (W, pcap, N) rows the segments stand for (blocks the walk does not reach: zeros) and their mask."""
    seg = np.asarray(seg, dtype=np.float64)
    valid, offs = block_walk(periods, counts, seg.shape[1])
    W, pcap = valid.shape
    y = np.zeros((W, pcap, N))
    for f, a in zip(*np.nonzero(valid)):
        y[f, a] = seg[f, offs[f, a] + np.arange(N) % int(periods[f][a])]
    return y, valid


def random_case(rng, W, pcap, N, ccap=None, integer=False):
    """Segments, periods and counts of W frames: periods 1, N, above N and primes among them, counts 0 .. pcap + 2."""
    pool = np.array([1, 2, 3, 5, 7, 13, N, N + 3, max(2, N // 3)])
    periods = rng.choice(pool, (W, pcap)).astype(np.int32)
    counts = rng.integers(0, pcap + 3, W).astype(np.int32)
    need = int(periods.astype(np.int64).sum(axis=1).max())
    ccap = need if ccap is None else ccap
    seg = rng.integers(-8, 9, (W, ccap)).astype(np.float64) if integer else rng.standard_normal((W, ccap))
    return seg, periods, counts


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("N,hop,pcap,T", [(37, 5, 4, 3), (64, 64, 64, 2), (48, 61, 3, 3), (16, 3, 1, 1)])
def test_restatement_against_dense_restatement(N, hop, pcap, T):
    from pyperiod_amd import ShortTime

    L = 333
    rng = np.random.default_rng(N * 100 + hop)
    W = ShortTime(N, hop).frame_count(L)
    w = sqrt_hann(N)
    masks = rng.integers(0, 2**64, (T, W), dtype=np.uint64)
    # integers, no window, no division: every sum is exact, so the two orders of summation give the same bits
    seg, periods, counts = random_case(rng, W, pcap, N, integer=True)
    y, valid = tile_segments(seg, periods, counts, N)
    got, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, normalize=False)
    dense, dmag, _ = overlap_add_tracks_ref(y, masks, hop, L, counts, None, None, False)
    assert np.array_equal(got, dense) and np.array_equal(mag, dmag) and np.all(den == 1.0)
    assert 1 <= K <= min(pcap, 64)
    # real values under a window, normalised: the same terms in two orders, within the bound of one such sum
    seg, periods, counts = random_case(rng, W, pcap, N)
    y, valid = tile_segments(seg, periods, counts, N)
    got, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, w, w, True)
    dense, dmag, dden = overlap_add_tracks_ref(y, masks, hop, L, counts, w, w, True)
    assert np.array_equal(den, dden)
    pos = den > 0
    for t in range(T):
        bound = ola_bound(mag[t], den, K, N, hop)
        assert np.all(np.abs(got[t] - dense[t])[pos] <= bound[pos])
        assert np.all(got[t][~pos] == 0.0)


def test_restatement_stop_rule_and_unread_elements():
    rng = np.random.default_rng(9)
    W, pcap, N, hop, L, ccap = 6, 4, 12, 4, 32, 20
    periods = np.array([[3, 5, 7, 2], [3, 0, 7, 2], [3, 5, 13, 2], [20, 1, 1, 1], [5, 5, 5, 5], [21, 1, 1, 1]], np.int32)
    counts = np.array([4, 4, 4, 4, 9, 4], np.int32)
    valid, offs = block_walk(periods, counts, ccap)
    assert valid.tolist() == [[True, True, True, True], [True, False, False, False], [True, True, False, False],
                              [True, False, False, False], [True, True, True, True], [False, False, False, False]]
    assert offs[0].tolist() == [0, 3, 8, 15] and offs[4].tolist() == [0, 5, 10, 15]
    seg = rng.standard_normal((W, ccap))
    bad = seg.copy()
    bad[0, 17:] = np.nan  # behind sum p
    bad[1, 3:] = np.nan  # behind the block with p = 0
    bad[2, 8:] = np.nan  # behind the block that overruns ccap
    bad[5, :] = np.nan  # the first block overruns: nothing of the row is read
    masks = np.full((2, W), 2**64 - 1, np.uint64)
    masks[1] = 0b0101
    bad[4, 5:10] = np.nan  # block 1 of frame 4 is in no mask of track 1 ...
    out, mag, den, K = ola_periodic_ref(bad, periods, counts, masks[1:], N, hop, L, normalize=False)
    assert np.all(np.isfinite(out)) and K == 2
    bad[4, 5:10] = seg[4, 5:10]  # ... and in track 0's
    out2, _, _, K2 = ola_periodic_ref(bad, periods, counts, masks, N, hop, L, normalize=False)
    assert np.all(np.isfinite(out2)) and K2 == 4 and np.array_equal(out2[1], out[0])
    want = np.zeros(L)
    y, _ = tile_segments(seg, periods, counts, N)
    for f in range(W):
        for a in range(pcap):
            want[f * hop : f * hop + N] += y[f, a][: L - f * hop]
    assert np.allclose(out2[0], want, rtol=0, atol=1e-12)


def test_symbol_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint ph_overlap_add_periodic\s*\(([^;]*)\);", text)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16 and len(_ffi.SIGNATURES["ph_overlap_add_periodic"]) == 16
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint}
    for arg, have in zip(args, _ffi.SIGNATURES["ph_overlap_add_periodic"]):
        want = ctypes.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]]
        assert have is want, arg


def test_entry_point_rejects_bad_arguments_without_gpu():
    """Every refusal comes before the first HIP call and before the context is looked at: a block of zeros stands in
    for the context, and the arrays are never read."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    assert lib.ph_version() == 100
    ctx = ctypes.addressof((ctypes.c_char * 4096)())
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    good = dict(ctx=ctx, seg=buf, periods=buf, counts=buf, masks=buf, W=4, pcap=2, ccap=16, T=3, N=16, hop=8, L=100,
                wa=None, ws=None, flags=0, out=buf)

    def call(**change):
        a = dict(good, **change)
        return lib.ph_overlap_add_periodic(a["ctx"], a["seg"], a["periods"], a["counts"], a["masks"], a["W"], a["pcap"],
                                           a["ccap"], a["T"], a["N"], a["hop"], a["L"], a["wa"], a["ws"], a["flags"], a["out"])

    for dev in (0, _ffi.PH_FLAG_DEVICE):
        assert call(ctx=None, flags=dev) == E and b"ctx" in lib.ph_last_error()
        for name in ("seg", "periods", "counts", "masks", "out"):
            assert call(flags=dev, **{name: None}) == E, name
            assert b"NULL" in lib.ph_last_error()
        for name in ("W", "N", "hop", "T", "pcap", "ccap", "L"):
            for v in (0, -1):
                assert call(flags=dev, **{name: v}) == E, (name, v)
        assert call(flags=dev, pcap=(1 << 20) + 1) == E and b"pcap" in lib.ph_last_error()
        assert call(flags=dev, ccap=(1 << 24) + 1) == E and b"ccap" in lib.ph_last_error()
        assert call(flags=dev, L=24) == E and b"behind" in lib.ph_last_error()  # (W - 1) hop == L
        assert call(flags=dev, W=14, L=104) == E  # (W - 1) hop == L again
        big = 2**63 - 1
        assert call(flags=dev, L=big // 16) == E and b"T * L" in lib.ph_last_error()  # T L 8
        assert call(flags=dev, T=big) == E
        assert call(flags=dev, W=1 << 40, N=1, hop=1, L=1 << 40, T=1 << 21) == E  # T W 8
        assert call(flags=dev, W=1 << 40, N=1, hop=1, L=1 << 40, T=1, ccap=1 << 24) == E  # W ccap 8
        assert b"W * ccap" in lib.ph_last_error()
        assert call(flags=dev, W=1 << 42, N=1, hop=1, L=1 << 42, T=1, ccap=1, pcap=1 << 20) == E  # W pcap 4


def test_numpy_side_array_next_to_a_tensor_is_a_type_error():
    import torch

    eng, Reached = cpu_engine()
    seg, masks = torch.zeros((4, 8), dtype=torch.float64), torch.ones((3, 4), dtype=torch.int64)
    per, cnt = torch.ones((4, 2), dtype=torch.int32), torch.ones(4, dtype=torch.int32)
    with pytest.raises(Reached):
        eng.overlap_add_periodic(seg, per, cnt, masks, 16, 4, 28)
    for call in (lambda: eng.overlap_add_periodic(seg, per.numpy(), cnt, masks, 16, 4, 28),
                 lambda: eng.overlap_add_periodic(seg, per, cnt.numpy(), masks, 16, 4, 28),
                 lambda: eng.overlap_add_periodic(seg, per, None, masks, 16, 4, 28),
                 lambda: eng.overlap_add_periodic(seg, per, cnt, masks.numpy(), 16, 4, 28),
                 lambda: eng.overlap_add_periodic(seg, per, cnt, masks, 16, 4, 28, win_a=np.ones(16))):
        with pytest.raises(TypeError, match="on the device of"):
            call()


def test_merge_repeats_against_a_loop():
    """ShortTime._merge_repeats is plain tensor arithmetic: on CPU tensors against a loop over the blocks -- repeated
    periods (twice and three times), frames without a block, unused entries that repeat a used period."""
    import torch

    from pyperiod_amd import ShortTime

    rng = np.random.default_rng(21)
    W, P, Kc, max_block = 40, 6, 70, 12
    per = rng.integers(1, 6, (W, P)).astype(np.int32) * 2  # few distinct values: many repeats
    nb = rng.integers(0, P + 1, W).astype(np.int32)
    nb[0], nb[1], nb[2] = 0, P, 1
    per[1] = [4, 6, 4, 4, 8, 6]
    keeps = np.minimum(rng.integers(1, 13, (W, P)), per).astype(np.int32)
    wts = rng.standard_normal((W, Kc))
    got = ShortTime._merge_repeats(torch, *(torch.as_tensor(a) for a in (per, keeps, nb, wts)), max_block)
    g_per, g_rows, g_nb, g_wts = (t.numpy() for t in got)
    for f in range(W):
        merged, read = {}, 0
        for b in range(nb[f]):
            q, r = int(per[f, b]), int(keeps[f, b])
            v = np.zeros(q)
            v[:r] = wts[f, read : read + r]
            read += r
            have = merged.get(q, (np.zeros(q), 0))
            merged[q] = (have[0] + v, max(have[1], r))
        n = len(merged)
        assert g_nb[f] == n and g_per[f, :n].tolist() == list(merged) and np.all(g_per[f, n:] == 0), f
        assert g_rows[f, :n].tolist() == [r for _, r in merged.values()] and np.all(g_rows[f, n:] == 0), f
        flat = np.concatenate([v[:r] for v, r in merged.values()]) if n else np.zeros(0)
        assert np.array_equal(g_wts[f, : flat.size], flat) and np.all(g_wts[f, flat.size :] == 0.0), f
    # nothing repeats: the tensors come back as they are
    per2 = np.tile(np.arange(1, P + 1, dtype=np.int32), (W, 1))
    args = [torch.as_tensor(a) for a in (per2, np.minimum(keeps, per2), nb, wts)]
    back = ShortTime._merge_repeats(torch, *args, max_block)
    assert all(a is b for a, b in zip(args, back))


def test_decompose_qo_validates_before_touching_the_gpu(monkeypatch):
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
    for bad in (0, 65, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            st.decompose_qo(x, bad, 0.1)
    with pytest.raises(TypeError):
        st.decompose_qo(x)  # num is required
    with pytest.raises(ValueError):
        ShortTime(96, 24, orthogonalize=True).decompose_qo(x, 3, 0.1)
    for bad in ([], [0], [12, (17, 12)], [()], 12, [1.5], "12"):
        with pytest.raises(ValueError):
            st.decompose_qo(x, 3, 0.1, tracks=bad)
    with pytest.raises(ValueError):
        st.decompose_qo(x, 3, 0.1, max_tracks=-1)
    with pytest.raises(ValueError):
        st.decompose_qo(x, 3, 0.1, max_rows=0)
