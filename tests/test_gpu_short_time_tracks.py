"""ShortTime.decompose on the MI355X: k_overlap_add_tracks against the np.add.at restatement of
tests/test_short_time_tracks_cpu.py, at large indices, ShortTime.decompose against the host route (Periods on the
host-built frames, track_masks, the restatement), a recording whose two tracks mean something, and the refusals of the
entry point through a live context.

Bound, per sample of track t: |out - ref| <= (K * ceil(N / hop) + 3) * 2^-52 * mag_t[n] / den[n] -- test_short_time_cpu's
ola_bound with mag_t = sum |ws * y| over the rows routed to t: both sides are float64 sums of at most K * ceil(N / hop) terms
with one product rounding each and one division (den = 1 when not normalised).  Samples with den == 0 and samples where the
track has no term must be exactly 0.0.
Sum of the tracks against the whole: when the masks partition the used rows, `tracks.sum(0) + other` is held to the
summed per-track bounds, sum_t b_t with b_t the bound above -- which is the bound of `periodic` itself, b being linear in
mag and mag_all = sum_t mag_t.  One b covers both sides of a comparison of two float64 evaluations of the same sum, so a
device value is within half of it of the exact value: the device tracks add up to within sum_t b_t / 2 of the exact
periodic part and the device `periodic` is within b_all / 2 of it.  Adding the T + 1 rows in the test is not charged."""

import warnings

import numpy as np
import pytest

from pyperiod_amd.synth import readme_window
from test_short_time_cpu import frames_ref, ola_bound, sqrt_hann
from test_short_time_tracks_cpu import overlap_add_tracks_ref, partition_masks

pytestmark = pytest.mark.gpu

L0 = 997


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


def _check(got, ref, mag, den, K, N, hop, what):
    """Every track within its bound, exact zeros where den == 0 or the track has no term."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), what
    pos = den > 0
    for t in range(ref.shape[0]):
        err, bound = np.abs(got[t] - ref[t]), ola_bound(mag[t], den, K, N, hop)
        worst = float(np.max(err[pos] - bound[pos])) if pos.any() else 0.0
        print(what, "track", t, "max err", float(err[pos].max()) if pos.any() else 0.0, "max err - bound", worst)
        assert np.all(err[pos] <= bound[pos]), (what, t, worst)
        assert np.all(got[t][~pos] == 0.0), (what, t)
        assert np.all(got[t][mag[t] == 0.0] == 0.0), (what, t)


def _random_masks(rng, T, W):
    """Sparse random 64-bit words (a quarter of the bits, bit 63 among them, bits at and above K too): tracks overlap,
    some rows are in no track; of three tracks the middle one is empty."""
    masks = rng.integers(0, 2**64, (T, W), dtype=np.uint64) & rng.integers(0, 2**64, (T, W), dtype=np.uint64)
    masks[0, ::3] |= np.uint64(1) << np.uint64(63)
    masks[0, 1::3] &= ~(np.uint64(1) << np.uint64(63))
    if T == 3:
        masks[1] = 0
    return masks


def _named(masks, K):
    """(W, K) bool: row k of frame f is in at least one track."""
    any_t = np.bitwise_or.reduce(masks, axis=0)
    return ((any_t[:, None] >> np.arange(K, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0


# ------------------------------------------------------------------ the kernel against the restatement
@pytest.mark.parametrize("hop", (1, 16, 80))
@pytest.mark.parametrize("N", (63, 64))
def test_tracks_against_restatement(eng, torch_dev, N, hop):
    torch, dev = torch_dev
    L = L0
    W = _count(L, N, hop)
    w = sqrt_hann(N)
    w_d = torch.as_tensor(w, device=dev)
    rng = np.random.default_rng(N * 100 + hop)
    for K in (1, 5, 64):
        for T in (1, 3):
            y = rng.standard_normal((W, K, N))
            masks = _random_masks(rng, T, W)
            if K == 64:
                assert (masks[0] >> np.uint64(63)).any()
            counts = rng.integers(0, K + 1, W).astype(np.int32)
            counts[0], counts[-1] = K + 5, -3  # clipped to [0, K]
            if W > 2:
                counts[1] = K
            named = _named(masks, K)
            behind = np.arange(K)[None, :] >= np.clip(counts, 0, K)[:, None]
            for dtype in (np.float64, np.float32):
                yt = y.astype(dtype)
                for windowed in (True, False):
                    wa, ws, wd = (w, w, w_d) if windowed else (None, None, None)
                    cnt = counts if windowed else None
                    normalize = windowed or dtype == np.float32
                    bad = yt.copy()  # NaN wherever the kernel must not read
                    bad[~named] = np.nan
                    if cnt is not None:
                        bad[behind] = np.nan
                    what = (N, hop, K, T, np.dtype(dtype).name, windowed)
                    ref, mag, den = overlap_add_tracks_ref(yt, masks, hop, L, cnt, wa, ws, normalize)
                    got = eng.overlap_add_tracks(bad, masks, hop, L, cnt, wa, ws, normalize)
                    _check(got, ref, mag, den, K, N, hop, what)
                    if T == 3:
                        assert np.all(got[1] == 0.0)  # the empty track
                    # two runs, int64 masks and the device-tensor call give the same bits
                    assert np.array_equal(eng.overlap_add_tracks(bad, masks.view(np.int64), hop, L, cnt, wa, ws, normalize), got)
                    got_d = eng.overlap_add_tracks(torch.as_tensor(bad, device=dev),
                                                   torch.as_tensor(masks.view(np.int64), device=dev), hop, L,
                                                   None if cnt is None else torch.as_tensor(cnt, device=dev), wd, wd, normalize)
                    assert got_d.is_cuda and got_d.shape == (T, L) and np.array_equal(got_d.cpu().numpy(), got), what
            if K == 1:  # (W, N) input
                assert np.array_equal(eng.overlap_add_tracks(y[:, 0], masks, hop, L), eng.overlap_add_tracks(y, masks, hop, L))
    # one all-ones mask is k_overlap_add: the same terms in the same order, so the same bits
    y = rng.standard_normal((W, 5, N))
    counts = rng.integers(0, 6, W).astype(np.int32)
    ones = np.full((1, W), 2**64 - 1, np.uint64)
    assert np.array_equal(eng.overlap_add_tracks(y, ones, hop, L, counts, w, w, True)[0], eng.overlap_add(y, hop, L, counts, w, w, True))
    # W == 0 or L == 0: no call, zeros
    out = eng.overlap_add_tracks(np.zeros((0, 3, N)), np.zeros((2, 0), np.uint64), hop, 20)
    assert out.shape == (2, 20) and np.all(out == 0.0)
    assert eng.overlap_add_tracks(y, ones, hop, 0).shape == (1, 0)


def test_tracks_many_frames(eng):
    """More frames than a 16-bit grid dimension holds."""
    W, K, N, hop, T = 70_000, 2, 16, 1, 2
    L = W + N - 1
    rng = np.random.default_rng(5)
    y = rng.standard_normal((W, K, N))
    masks = rng.integers(0, 4, (T, W)).astype(np.uint64)
    ref, mag, den = overlap_add_tracks_ref(y, masks, hop, L)
    _check(eng.overlap_add_tracks(y, masks, hop, L), ref, mag, den, K, N, hop, "many frames")


def test_tracks_second_trip_of_the_stride_loop(eng):
    """T * L just above the num_cu * 64 workgroups of 256 lanes the flat grid is capped at."""
    N = hop = 64
    K, T = 1, 5
    cap = eng.num_cu * 64 * 256
    L = cap // T + 70  # T * L = cap + 350 - (cap mod 5): the second trip ends inside the last track
    assert T * L > cap and T * (L - 70) <= cap
    W = _count(L, N, hop)
    rng = np.random.default_rng(6)
    y = rng.standard_normal((W, K, N))
    masks = partition_masks(rng, T, W, K)
    ref, mag, den = overlap_add_tracks_ref(y, masks, hop, L, normalize=False)
    got = eng.overlap_add_tracks(y, masks, hop, L, normalize=False)
    _check(got, ref, mag, den, K, N, hop, "second trip")
    assert np.array_equal(got, ref)  # one term per sample and no division: nothing to round
    assert np.array_equal(got.sum(0), eng.overlap_add(y, hop, L, normalize=False))


# ------------------------------------------------------------------ decompose
D_N, D_HOP, D_L = 256, 64, 3000


def _recording(method):
    """best_frequency: two sinusoids of periods 12 and 17 under a little noise -- it completes on every frame under both
    windows (no spectrum whose peak is bin 0), and under the rectangular window a period repeats inside a frame.  The
    other methods: the README's recording, on which small_to_large accepts 5 or 6 periods per frame under both windows."""
    if method != "best_frequency":
        return readme_window(D_L, seed=0)
    n = np.arange(D_L)
    return (np.sin(2 * np.pi * n / 12.0) + 0.7 * np.sin(2 * np.pi * n / 17.0 + 1.0)
            + 0.05 * np.random.default_rng(1).standard_normal(D_L))


def _activity_ref(per, pw, counts, groups):
    W, K = per.shape
    act = np.zeros((len(groups), W))
    for t, group in enumerate(groups):
        for f in range(W):
            kf = K if counts is None else int(counts[f])
            s = 0.0
            for k in range(kf):
                if int(per[f, k]) in group:
                    s += pw[f, k]
            act[t, f] = s
    return act


def _host_route(method, kwargs, batch):
    """-> periods (W, K), powers (W, K), bases (W, K, N), counts (W) or None, by Periods on the host-built frames."""
    from pyperiod_amd import Periods

    if method != "small_to_large":
        per, pw, bases = getattr(Periods(), method)(batch, **kwargs)
        return per, pw, bases, None
    host = Periods().small_to_large(batch, **kwargs)
    W = batch.shape[0]
    counts = np.array([len(h[0]) for h in host], dtype=np.int32)
    kmax = max(1, int(counts.max()))
    per, pw, bases = np.zeros((W, kmax), np.int32), np.zeros((W, kmax)), np.zeros((W, kmax, batch.shape[1]))
    for f, (p, q, bs) in enumerate(host):
        k = len(p)
        if k:
            per[f, :k], pw[f, :k], bases[f, :k] = p, q, np.stack(bs)
    return per, pw, bases, counts


@pytest.mark.parametrize("windowed", (True, False))
@pytest.mark.parametrize("method,kwargs", [("m_best", {"num": 3}), ("best_frequency", {"num": 4}),
                                           ("small_to_large", {"thresh": 0.1})])
def test_decompose_against_host_route(eng, torch_dev, method, kwargs, windowed):
    from pyperiod_amd import ShortTime, ShortTimeTracks

    torch, dev = torch_dev
    x = _recording(method)
    w = sqrt_hann(D_N) if windowed else None
    st = ShortTime(D_N, D_HOP, window=w)
    W = st.frame_count(D_L)
    batch = frames_ref(x, D_N, D_HOP, W, w)
    per, pw, bases, counts = _host_route(method, kwargs, batch)
    K = per.shape[1]
    if method == "best_frequency" and not windowed:  # a period can repeat inside a frame
        assert any(len(set(row.tolist())) < K for row in per)
    if method == "small_to_large":
        assert counts.min() < counts.max()  # ragged
    eng.profile(True)
    try:
        res = st.decompose(x, method=method, **kwargs)
        names = [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)
    assert isinstance(res, ShortTimeTracks)
    assert names[0] == "k_frames" and names[-2:] == ["k_overlap_add_tracks", "k_overlap_add"]
    assert names.count("k_frames") == 1 and names.count("k_overlap_add_tracks") == 1 and names.count("k_overlap_add") == 1
    # periods, powers, counts: bit for bit
    if counts is None:
        assert res.counts is None and res.periods.dtype == per.dtype
        assert np.array_equal(res.periods, per) and np.array_equal(res.powers, pw)
    else:
        assert res.counts.dtype == np.int32 and np.array_equal(res.counts, counts)
        assert np.array_equal(res.periods[:, :K], per) and np.array_equal(res.powers[:, :K], pw)
        assert np.all(res.periods[:, K:] == 0) and np.all(res.powers[:, K:] == 0.0)
    # periodic and residual: the launches of analyze, so its bits
    ana = st.analyze(x, method=method, **kwargs)
    assert np.array_equal(res.periodic, ana.periodic) and np.array_equal(res.residual, ana.residual)
    # the default tracks are the strongest periods, one each
    groups = [(p,) for p in ShortTime.rank_periods(per, pw, counts, 8)]
    assert 1 <= len(groups) <= 8 and res.track_periods == groups
    T = len(groups)
    masks = ShortTime.track_masks(per, counts, groups)
    ref, mag, den = overlap_add_tracks_ref(bases, masks, D_HOP, D_L, counts, w, w, True)
    assert res.tracks.shape == (T, D_L) and res.other.shape == (D_L,) and res.activity.shape == (T, W)
    got = np.concatenate([res.tracks, res.other[None, :]])
    _check(got, ref, mag, den, K, D_N, D_HOP, (method, windowed))
    # the tracks and `other` add up to the periodic part
    pos = den > 0
    bound = sum(ola_bound(mag[t], den, K, D_N, D_HOP) for t in range(T + 1))
    err = np.abs(got.sum(0) - res.periodic)
    print((method, windowed), "sum of the tracks against periodic: worst err / bound",
          float(np.max(err[pos] / np.maximum(bound[pos], 1e-300))))
    assert np.all(err[pos] <= bound[pos])
    assert np.array_equal(res.activity, _activity_ref(per, pw, counts, groups))
    # a 1-D device tensor gives the same result
    res_d = st.decompose(torch.as_tensor(x, device=dev), method=method, **kwargs)
    for a, b in zip(res, res_d):
        assert (a is None and b is None) or (a == b if isinstance(a, list) else np.array_equal(a, b))
    # explicit tracks: a group of two periods, a period that never occurs, and the rest in `other`
    if method == "m_best":
        assert T >= 2
        explicit = [(groups[0][0], groups[-1][0]), 251]
        res_e = st.decompose(x, method=method, tracks=explicit, **kwargs)
        want = [explicit[0], (251,)]
        assert res_e.track_periods == want
        masks_e = ShortTime.track_masks(per, counts, want)
        ref_e, mag_e, den_e = overlap_add_tracks_ref(bases, masks_e, D_HOP, D_L, counts, w, w, True)
        _check(np.concatenate([res_e.tracks, res_e.other[None, :]]), ref_e, mag_e, den_e, K, D_N, D_HOP, "explicit")
        assert np.all(res_e.tracks[1] == 0.0) and np.all(res_e.activity[1] == 0.0)
        assert np.array_equal(res_e.periodic, res.periodic)
        assert np.array_equal(res_e.activity, _activity_ref(per, pw, counts, want))
        # num == 0: nothing ran, nothing periodic
        res_0 = st.decompose(x, method=method, num=0, tracks=[12])
        assert res_0.periods.shape == (W, 0) and res_0.tracks.shape == (1, D_L) and not res_0.tracks.any()
        assert not res_0.other.any() and np.array_equal(res_0.residual, x) and res_0.track_periods == [(12,)]


def test_tracks_that_mean_something(eng):
    """A recording that repeats with period 12 in its first half and with period 17 in its second: the two tracks carry
    their half and nothing of the other.  The figures of the CPU oracle's m_best on the same frames: track 0 / signal
    energy 0.999998 in the first half and exactly 0 in the second, track 1 / signal 1.0000014 in the second half and
    exactly 0 in the first, `other` exactly 0 in both (on [N, L/2 - N) and [L/2 + N, L - N))."""
    from pyperiod_amd import ShortTime

    rng = np.random.default_rng(7)
    L, N, hop = 3072, 256, 64
    h = L // 2
    first = np.tile(rng.integers(-8, 9, 12), h // 12 + 1)[:h]
    second = np.tile(rng.integers(-8, 9, 17), h // 17 + 1)[:h]
    x = np.concatenate([first, second]).astype(np.float64) + 1e-3 * rng.standard_normal(L)
    # step 2 of m_best splits 12 into 6 and 12, so the divisors belong to the first group
    tracks = [sorted({2, 3, 4, 6} | set(range(12, 85, 12))), list(range(17, 86, 17))]
    res = ShortTime(N, hop).decompose(x, method="m_best", num=2, tracks=tracks)
    assert res.track_periods == [tuple(tracks[0]), tuple(tracks[1])]
    halves = (slice(N, h - N), slice(h + N, L - N))
    ratio = [[float(np.sum(part[sl] ** 2) / np.sum(x[sl] ** 2)) for sl in halves] for part in (*res.tracks, res.other)]
    print("energy ratios [track 0, track 1, other] x [first, second]:", ratio)
    assert 0.99 <= ratio[0][0] <= 1.01 and 0.99 <= ratio[1][1] <= 1.01
    assert ratio[0][1] <= 1e-6 and ratio[1][0] <= 1e-6
    assert ratio[2][0] <= 1e-6 and ratio[2][1] <= 1e-6
    assert np.all(res.activity[0, : (h - N) // hop] > 0) and np.all(res.activity[1, : (h - N) // hop] == 0)


# ------------------------------------------------------------------ refusals
def test_bad_arguments_launch_nothing(eng):
    from pyperiod_amd import _ffi

    lib, ctx = eng._lib, eng._ctx
    y = np.zeros((4, 2, 16))
    y65 = np.zeros((4, 65, 16))
    masks = np.ones((3, 4), np.uint64)
    out = np.zeros((3, 100))
    yy, y6, mm, o = y.ctypes.data, y65.ctypes.data, masks.ctypes.data, out.ctypes.data
    E = _ffi.PH_E_ARG
    eng.profile(True)
    try:
        for dev in (0, _ffi.PH_FLAG_DEVICE):
            call = lib.ph_overlap_add_tracks
            assert call(ctx, yy, 0, 4, 2, 16, 8, 100, None, mm, 0, None, None, dev, o) == E  # T = 0
            assert b"T=0" in lib.ph_last_error()
            assert call(ctx, y6, 0, 4, 65, 16, 8, 100, None, mm, 3, None, None, dev, o) == E  # K = 65
            assert b"K=65" in lib.ph_last_error()
            assert call(ctx, yy, 0, 4, 2, 16, 8, 100, None, None, 3, None, None, dev, o) == E  # NULL masks
            assert b"masks" in lib.ph_last_error()
            assert call(ctx, yy, 0, 4, 2, 16, 8, 24, None, mm, 3, None, None, dev, o) == E  # (W - 1) hop == L
            assert b"behind" in lib.ph_last_error()
            assert call(ctx, None, 0, 4, 2, 16, 8, 100, None, mm, 3, None, None, dev, o) == E
            assert call(ctx, yy, 0, 4, 2, 16, 8, 100, None, mm, 3, None, None, dev, None) == E
            assert call(ctx, yy, 3, 4, 2, 16, 8, 100, None, mm, 3, None, None, dev, o) == E
        # the engine turns PH_E_ARG into ValueError, and refuses masks that are no 64-bit words
        with pytest.raises(ValueError):
            eng.overlap_add_tracks(y, np.zeros((0, 4), np.uint64), 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_tracks(y65, masks, 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_tracks(y, masks, 8, 24)
        with pytest.raises(ValueError):
            eng.overlap_add_tracks(y, np.ones((3, 5), np.uint64), 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_tracks(y, masks, 8, 100, counts=np.zeros(3, np.int32))
        for bad in (masks.astype(np.float64), masks.astype(np.int32), masks.tolist()):
            with pytest.raises(TypeError):
                eng.overlap_add_tracks(y, bad, 8, 100)
        assert eng.profile_read() == []
        # and a good call is recorded
        eng.overlap_add_tracks(y, masks, 8, 100)
        assert [n for n, _ in eng.profile_read()] == ["k_overlap_add_tracks"]
    finally:
        eng.profile(False)
