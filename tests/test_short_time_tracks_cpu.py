"""ShortTime.decompose without a GPU: the numpy restatement of the routed overlap-add that
tests/test_gpu_short_time_tracks.py holds k_overlap_add_tracks to, the two host statics (rank_periods, track_masks),
argument validation and the new C-ABI symbol.

The restatement adds, per track, the rows a mask names with np.add.at in ascending k and ascending f -- the order of the
kernel and of overlap_add_ref.  Its per-sample bound is the one of test_short_time_cpu.ola_bound over the track's own
terms: (K * ceil(N / hop) + 3) * 2^-52 * mag_t / den, mag_t = sum |ws * y| over the rows routed to track t."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_short_time_cpu import cpu_engine, ola_bound, overlap_add_ref, sqrt_hann


# ------------------------------------------------------------------ restatement
def overlap_add_tracks_ref(y, masks, hop, L, counts=None, wa=None, ws=None, normalize=True):
    """-> (out, mag, den): out and mag (T, L) -- the routed overlap-add of y (W, K, N) and the sum of |ws * y| over the
    same terms -- and den (L), the overlap-added window product (ones when not normalised)."""
    y = np.asarray(y)
    if y.ndim == 2:
        y = y[:, None, :]
    W, K, N = y.shape
    masks = np.asarray(masks).view(np.uint64)
    T = masks.shape[0]
    assert masks.shape == (T, W) and K <= 64
    wa = np.ones(N) if wa is None else wa
    ws = np.ones(N) if ws is None else ws
    num, mag, den = np.zeros((T, L)), np.zeros((T, L)), np.zeros(L)
    idx = np.arange(W)[:, None] * hop + np.arange(N)[None, :]  # sample of element (f, i)
    ok = idx < L
    kf = np.full(W, K) if counts is None else np.clip(np.asarray(counts, dtype=np.int64), 0, K)
    np.add.at(den, idx[ok], np.broadcast_to(wa * ws, (W, N))[ok])
    for t in range(T):
        for k in range(K):  # np.add.at adds in index order: ascending f for every sample
            bit = ((masks[t] >> np.uint64(k)) & np.uint64(1)) != 0
            use = ok & ((k < kf) & bit)[:, None]
            if not use.any():
                continue  # (rows nobody names may hold anything, NaN included)
            term = ws[None, :] * y[:, k].astype(np.float64)
            np.add.at(num[t], idx[use], term[use])
            np.add.at(mag[t], idx[use], np.abs(term)[use])
    if not normalize:
        return num, mag, np.ones(L)
    out = np.zeros((T, L))
    pos = den > 0
    out[:, pos] = num[:, pos] / den[pos]
    return out, mag, den


def partition_masks(rng, T, W, K):
    """Masks that put every row (f, k) into exactly one of T tracks."""
    label = rng.integers(0, T, (W, K))
    masks = np.zeros((T, W), np.uint64)
    for k in range(K):
        for t in range(T):
            masks[t, label[:, k] == t] |= np.uint64(1) << np.uint64(k)
    return masks


def brute_rank(periods, powers, counts, max_tracks):
    score = {}
    W, K = np.asarray(periods).shape
    for f in range(W):
        kf = K if counts is None else min(max(int(counts[f]), 0), K)
        for k in range(kf):
            p = int(periods[f][k])
            if p == 0:
                continue
            v = float(powers[f][k])
            score[p] = score.get(p, 0.0) + (0.0 if v != v else v)
    return sorted(score, key=lambda p: (-score[p], p))[:max_tracks]


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("N,hop,K,T", [(64, 16, 5, 3), (63, 1, 1, 1), (64, 80, 64, 3), (63, 16, 64, 2)])
def test_partition_sums_to_overlap_add(N, hop, K, T):
    from pyperiod_amd import ShortTime

    L = 997
    rng = np.random.default_rng(N * 1000 + hop * 10 + K)
    W = ShortTime(N, hop).frame_count(L)
    y = rng.standard_normal((W, K, N))
    counts = rng.integers(-1, K + 2, W).astype(np.int32)
    w = sqrt_hann(N)
    masks = partition_masks(rng, T, W, K)
    out, mag, den = overlap_add_tracks_ref(y, masks, hop, L, counts, w, w, True)
    ref, mag_all, den_all = overlap_add_ref(y, hop, L, counts, w, w, True)
    assert np.array_equal(den, den_all)
    pos = den > 0
    # every term is in exactly one track: the magnitudes add up (sums of non-negative terms may differ by the order,
    # so compare to rounding) and the tracks add up to the whole within the sum of the per-track bounds -- ola_bound
    # already covers two float64 evaluations of one sum, and it is linear in mag, so this is the bound of the whole
    assert np.allclose(mag.sum(0), mag_all, rtol=1e-12, atol=0)
    bound = sum(ola_bound(mag[t], den, K, N, hop) for t in range(T))
    err = np.abs(out.sum(0) - ref)
    print("worst err / bound", float(np.max(err[pos] / np.maximum(bound[pos], 1e-300))))
    assert np.all(err[pos] <= bound[pos])
    assert np.all(out[:, ~pos] == 0.0)
    # a single all-ones mask is overlap_add_ref itself, bit for bit
    one, mag1, _ = overlap_add_tracks_ref(y, np.full((1, W), 2**64 - 1, np.uint64), hop, L, counts, w, w, True)
    assert np.array_equal(one[0], ref) and np.array_equal(mag1[0], mag_all)


def test_restatement_ignores_unrouted_rows_and_takes_int64_masks():
    rng = np.random.default_rng(3)
    W, K, N, hop, L = 10, 64, 16, 8, 88
    y = rng.standard_normal((W, K, N))
    masks = np.zeros((2, W), np.uint64)
    masks[0] = np.uint64(1) << np.uint64(63)
    masks[1, ::2] = np.uint64(0b101)
    bad = y.copy()
    bad[:, 1] = np.nan
    bad[:, 3:63] = np.nan
    out, mag, den = overlap_add_tracks_ref(bad, masks.view(np.int64), hop, L, None, None, None, False)
    assert np.all(np.isfinite(out))
    assert np.array_equal(out[0], overlap_add_ref(y[:, 63], hop, L, normalize=False)[0])
    half = y[:, 0] + 0.0
    half[1::2] = 0.0
    two = y[:, 2] + 0.0
    two[1::2] = 0.0
    want = overlap_add_ref(np.stack([half, two], axis=1), hop, L, normalize=False)[0]
    assert np.array_equal(out[1], want)


def test_rank_periods_against_brute_force():
    from pyperiod_amd import ShortTime

    rng = np.random.default_rng(11)
    for trial in range(20):
        W, K = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        periods = rng.integers(0, 7, (W, K)).astype(np.uint32 if trial % 2 else np.int32)
        powers = rng.integers(0, 4, (W, K)).astype(np.float64)  # small integers: many exact ties
        powers[rng.random((W, K)) < 0.1] = np.nan
        counts = None if trial % 3 == 0 else rng.integers(-1, K + 2, W).astype(np.int32)
        for mt in (0, 1, 3, 8):
            got = ShortTime.rank_periods(periods, powers, counts, mt)
            assert got == brute_rank(periods, powers, counts, mt), (trial, mt)
            assert all(isinstance(p, int) and p > 0 for p in got)
    # real-valued powers, in the flattened order both sides add in
    periods = rng.integers(1, 30, (50, 5))
    powers = rng.standard_normal((50, 5)) ** 2
    assert ShortTime.rank_periods(periods, powers) == brute_rank(periods, powers, None, 8)
    # ties go to the smaller period; zeros are no period; entries behind counts do not count
    assert ShortTime.rank_periods([[9, 4, 0], [4, 9, 7]], [[1.0, 2.0, 50.0], [1.0, 2.0, 99.0]], [3, 2]) == [4, 9]
    assert ShortTime.rank_periods(np.zeros((3, 2), int), np.ones((3, 2))) == []
    assert ShortTime.rank_periods([[5, 6]], [[np.nan, np.nan]]) == [5, 6]


def test_track_masks():
    from pyperiod_amd import ShortTime

    W, K = 4, 64
    periods = np.zeros((W, K), np.uint32)
    periods[:, 63] = 12  # bit 63
    periods[:, 0] = 17
    periods[1, 1] = 34
    periods[2, 5] = 99  # in no track
    periods[3, 2] = 12
    counts = np.array([64, 64, 64, 3], np.int32)  # frame 3: row 63 is behind counts
    masks = ShortTime.track_masks(periods, counts, [(12,), (17, 34)])
    assert masks.dtype == np.uint64 and masks.shape == (3, W)
    top = 1 << 63
    assert [int(m) for m in masks[0]] == [top, top, top, 1 << 2]
    assert [int(m) for m in masks[1]] == [1, 0b11, 1, 1]
    full = (1 << 64) - 1
    assert int(masks[2, 0]) == full & ~top & ~1  # period-0 rows land in the last row
    assert int(masks[2, 1]) == full & ~top & ~0b11
    assert int(masks[2, 2]) == full & ~top & ~1  # 99 stays in `other`
    assert int(masks[2, 3]) == 0b010  # rows at or above counts are in no row
    # the rows of every frame partition its used entries
    for f in range(W):
        kf = int(counts[f])
        used = (1 << kf) - 1
        assert int(masks[0, f]) | int(masks[1, f]) | int(masks[2, f]) == used
        assert int(masks[0, f]) & int(masks[1, f]) == 0 and int(masks[0, f]) & int(masks[2, f]) == 0
    # counts None: all K; counts outside [0, K] are clipped; a track that never occurs is all zero
    m2 = ShortTime.track_masks(periods, None, [(5,)])
    assert np.all(m2[0] == 0) and np.all(m2[1] == np.uint64(full))
    m3 = ShortTime.track_masks(periods, [70, -2, 0, 1], [(17,)])
    assert [int(m) for m in m3[0]] == [1, 0, 0, 1] and int(m3[1, 1]) == 0 and int(m3[1, 0]) == full & ~1
    # no track at all: one row, everything in it
    m4 = ShortTime.track_masks(periods, counts, [])
    assert m4.shape == (1, W) and int(m4[0, 3]) == 0b111
    with pytest.raises(ValueError):
        ShortTime.track_masks(np.zeros((2, 65), np.int32), None, [(3,)])
    with pytest.raises(ValueError):
        ShortTime.track_masks(periods, counts, [(12,), (12, 17)])


def test_decompose_validates_before_touching_the_gpu(monkeypatch):
    import sys

    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime, ShortTimeTracks

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)
    st = ShortTime(64, 16)
    x = np.zeros(200)
    for bad in ([], [0], [12, -3], [12, (17, 12)], [()], [12, []], [(3, 4), 4], 12, [1.5], ["12"], "12", [(3, "4")],
                np.array(12), [np.array(0)], [None]):
        with pytest.raises(ValueError):
            st.decompose(x, tracks=bad)
    with pytest.raises(ValueError):
        st.decompose(x, method="find_periods")
    with pytest.raises(ValueError):
        st.decompose(x, max_tracks=-1)
    with pytest.raises(ValueError):  # K > 64 rows per frame, before any launch
        st.decompose(x, method="m_best", num=65)
    with pytest.raises(ValueError):
        st.decompose(x, method="best_frequency", num=100, tracks=[12])
    assert ShortTimeTracks._fields == ("periods", "powers", "periodic", "residual", "track_periods", "tracks", "other",
                                       "activity", "counts")
    assert ShortTime._track_list([12, (17, 34), {5}, np.int64(7), [8, 8], np.array(9),
                                  np.array([3, 6])]) == [(12,), (17, 34), (5,), (7,), (8,), (9,), (3, 6)]


def test_numpy_side_array_next_to_a_tensor_is_a_type_error():
    import torch

    eng, Reached = cpu_engine()
    y, masks = torch.zeros((4, 2, 16), dtype=torch.float64), torch.ones((3, 4), dtype=torch.int64)
    with pytest.raises(Reached):
        eng.overlap_add_tracks(y, masks, 4, 28, torch.ones(4, dtype=torch.int32))
    for call in (lambda: eng.overlap_add_tracks(y, masks.numpy(), 4, 28),
                 lambda: eng.overlap_add_tracks(y, masks.to(torch.int32), 4, 28),
                 lambda: eng.overlap_add_tracks(y, masks, 4, 28, counts=np.ones(4, np.int32)),
                 lambda: eng.overlap_add_tracks(y, masks, 4, 28, win_s=np.ones(16))):
        with pytest.raises(TypeError, match="on the device of"):
            call()


def test_symbol_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint ph_overlap_add_tracks\s*\(([^;]*)\);", text)
    assert m
    assert len(m.group(1).split(",")) == 15
    assert len(_ffi.SIGNATURES["ph_overlap_add_tracks"]) == 15


def test_entry_point_rejects_bad_arguments_without_gpu():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    assert lib.ph_overlap_add_tracks(None, buf, 0, 2, 1, 8, 4, 12, None, buf, 1, None, None, 0, buf) == E
    assert b"ctx" in lib.ph_last_error()
