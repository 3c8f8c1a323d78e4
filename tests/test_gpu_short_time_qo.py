"""ShortTime.decompose_qo on the MI355X: k_overlap_add_periodic against the restatement of
tests/test_short_time_qo_cpu.py (ola_periodic_ref) and against the dense route (torch tiling + k_overlap_add_tracks) in
the same process, decompose_qo against the host route (ShortTime.frames -> the batched QOPeriods.find_periods ->
get_periods -> numpy tiling -> the restatement), the host fallback, the kernels one call launches and a recording whose
tracks mean something.

Bound, per sample of track t: |out - ref| <= (K * ceil(N / hop) + 3) * 2^-52 * mag_t[n] / den[n] -- test_short_time_cpu's
ola_bound with K the largest number of blocks one (track, frame) routes and mag_t = sum |ws * value| over the track's
terms: both sides are float64 sums of the same at most K * ceil(N / hop) terms, one product rounding each, and one
division (den = 1 when not normalised).  Samples with den == 0 and samples where the track has no term must be exactly
0.0.  Where the masks partition the blocks in use, the rows are held to the summed per-track bounds against the
all-blocks row, as tests/test_gpu_short_time_tracks.py argues for the dense kernel."""

import warnings

import numpy as np
import pytest

from test_short_time_cpu import ola_bound, sqrt_hann
from test_short_time_qo_cpu import block_walk, ola_periodic_ref, routed_blocks, tile_segments

pytestmark = pytest.mark.gpu

L0 = 997  # not a multiple of 64: with T = 3 wavefronts straddle two tracks


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


def _count(L, N, hop):
    from pyperiod_amd import ShortTime

    return ShortTime(N, hop).frame_count(L)


def _check(got, ref, mag, den, K, N, hop, what):
    """Every track within its bound, exact zeros where den == 0 or the track has no term, no NaN."""
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


def _unread(periods, counts, masks, ccap, N, hop, L):
    """(W, ccap) bool: the elements of seg the kernel must not read -- behind sum p, in blocks behind counts, behind a
    block that ends the walk, in blocks no mask names, and the tail of a block longer than the samples its frame has."""
    W = periods.shape[0]
    _, offs = block_walk(periods, counts, ccap)
    named = routed_blocks(periods, counts, masks, ccap).any(axis=0)
    read = np.zeros((W, ccap), bool)
    for f, a in zip(*np.nonzero(named)):
        n = min(N, L - f * hop, int(periods[f, a]))
        read[f, offs[f, a] : offs[f, a] + n] = True
    return ~read


def _kernel_case(rng, W, N, pcap, T):
    """Periods 1, N, above N and primes; counts of 0, of pcap and above pcap; a frame whose second block has p = 0 and one
    whose blocks overrun ccap; overlapping masks with bit 63 in use where pcap = 64."""
    pool = np.array([1, 1, 2, 3, 5, 7, 13, 31, N, N + 3, N + 29])
    periods = rng.choice(pool, (W, pcap)).astype(np.int32)
    counts = rng.integers(0, pcap + 1, W).astype(np.int32)
    counts[0], counts[1], counts[-1] = pcap + 5, pcap, 0
    if W > 6:
        counts[4], counts[5] = 0, -3
    ccap = int(periods.astype(np.int64).sum(axis=1).max()) + 7  # every row has elements behind sum p
    if W > 3:
        counts[2] = counts[3] = pcap
        periods[2, 1] = 0  # the walk of frame 2 ends behind its first block
        periods[3, min(5, pcap - 1)] = ccap  # off + p > ccap (off > 0 when pcap > 1)
    masks = rng.integers(0, 2**64, (T, W), dtype=np.uint64) & rng.integers(0, 2**64, (T, W), dtype=np.uint64)
    masks[0, ::2] |= np.uint64(1) << np.uint64(63)
    masks[T - 1, 1] = np.uint64(2**64 - 1)
    masks[0, 2] |= np.uint64(1)
    seg = rng.standard_normal((W, ccap))
    return seg, periods, counts, masks, ccap


# ------------------------------------------------------------------ (a) the kernel against the restatement
@pytest.mark.parametrize("N,hop", [(37, 5), (64, 64), (48, 61)])
def test_periodic_against_restatement(eng, torch_dev, N, hop):
    torch, dev = torch_dev
    L, T, pcap = L0, 3, 64
    W = _count(L, N, hop)
    w = sqrt_hann(N)
    w_d = torch.as_tensor(w, device=dev)
    rng = np.random.default_rng(N * 100 + hop)
    seg, periods, counts, masks, ccap = _kernel_case(rng, W, N, pcap, T)
    routed = routed_blocks(periods, counts, masks, ccap)
    assert routed[:, :, 63].any()  # bit 63 routes a block
    assert not routed[:, 2, 1:].any() and routed[:, 2, 0].any()  # the stop rule at p = 0
    assert not routed[:, 3, 5:].any()  # and at the overrun
    bad = seg.copy()
    unread = _unread(periods, counts, masks, ccap, N, hop, L)
    bad[unread] = np.nan
    assert unread[:, -7:].all() and not unread.all()
    per_d, cnt_d = torch.as_tensor(periods, device=dev), torch.as_tensor(counts, device=dev)
    bad_d, masks_d = torch.as_tensor(bad, device=dev), torch.as_tensor(masks.view(np.int64), device=dev)
    for windowed in (True, False):
        for normalize in (True, False):
            wa, wd = (w, w_d) if windowed else (None, None)
            what = (N, hop, windowed, normalize)
            ref, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, wa, wa, normalize)
            got = eng.overlap_add_periodic(bad, periods, counts, masks, N, hop, L, wa, wa, normalize)
            _check(got, ref, mag, den, K, N, hop, what)
            if hop > N and normalize:
                assert (den == 0).any()  # the gaps between the frames
            # two runs, int64 masks and the device-tensor call give the same bits
            assert np.array_equal(eng.overlap_add_periodic(bad, periods, counts, masks.view(np.int64), N, hop, L, wa, wa,
                                                           normalize), got), what
            got_d = eng.overlap_add_periodic(bad_d, per_d, cnt_d, masks_d, N, hop, L, wd, wd, normalize)
            assert got_d.is_cuda and got_d.shape == (T, L) and np.array_equal(got_d.cpu().numpy(), got), what
    # a small pcap, one track
    seg, periods, counts, masks, ccap = _kernel_case(rng, W, N, 3, 1)
    ref, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, w, w, True)
    bad = seg.copy()
    bad[_unread(periods, counts, masks, ccap, N, hop, L)] = np.nan
    _check(eng.overlap_add_periodic(bad, periods, counts, masks, N, hop, L, w, w, True), ref, mag, den, K, N, hop, "pcap 3")
    # W == 0 or L == 0: no call, zeros
    out = eng.overlap_add_periodic(np.zeros((0, 5)), np.zeros((0, 2), np.int32), np.zeros(0, np.int32),
                                   np.zeros((2, 0), np.uint64), N, hop, 20)
    assert out.shape == (2, 20) and np.all(out == 0.0)
    assert eng.overlap_add_periodic(seg, periods, counts, masks, N, hop, 0).shape == (1, 0)


def test_periodic_second_trip_of_the_stride_loop(eng):
    """T * L just above the num_cu * 64 workgroups of 256 lanes the flat grid is capped at."""
    N = hop = 64
    pcap, T = 2, 5
    cap = eng.num_cu * 64 * 256
    L = cap // T + 70  # T * L = cap + 350 - (cap mod 5): the second trip ends inside the last track
    assert T * L > cap and T * (L - 70) <= cap
    W = _count(L, N, hop)
    rng = np.random.default_rng(6)
    periods = rng.choice(np.array([1, 3, 7, 64, 70]), (W, pcap)).astype(np.int32)
    counts = rng.integers(0, pcap + 1, W).astype(np.int32)
    seg = rng.integers(-8, 9, (W, 140)).astype(np.float64)
    masks = rng.integers(0, 4, (T, W)).astype(np.uint64)
    ref, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, normalize=False)
    got = eng.overlap_add_periodic(seg, periods, counts, masks, N, hop, L, normalize=False)
    _check(got, ref, mag, den, K, N, hop, "second trip")
    assert np.array_equal(got, ref)  # small integers and no division: nothing to round
    assert got[:, -70:].any()


# ------------------------------------------------------------------ (b) the kernel against the dense route
def test_periodic_against_dense_route(eng, torch_dev):
    torch, dev = torch_dev
    N, hop, L, T, pcap = 64, 16, L0, 3, 6
    W = _count(L, N, hop)
    w = sqrt_hann(N)
    rng = np.random.default_rng(12)
    periods = rng.choice(np.array([1, 2, 3, 5, 7, 13, 31, N, N + 3]), (W, pcap)).astype(np.int32)
    counts = rng.integers(0, pcap + 1, W).astype(np.int32)
    ccap = int(periods.astype(np.int64).sum(axis=1).max())
    seg = rng.standard_normal((W, ccap))
    masks = rng.integers(0, 2**pcap, (T, W)).astype(np.uint64)
    ref, mag, den, K = ola_periodic_ref(seg, periods, counts, masks, N, hop, L, w, w, True)
    seg_d, per_d, cnt_d = (torch.as_tensor(a, device=dev) for a in (seg, periods, counts))
    masks_d, w_d = torch.as_tensor(masks.view(np.int64), device=dev), torch.as_tensor(w, device=dev)
    got = eng.overlap_add_periodic(seg_d, per_d, cnt_d, masks_d, N, hop, L, w_d, w_d, True).cpu().numpy()
    # the dense route: tile every block to N samples with torch, then k_overlap_add_tracks
    off = torch.cumsum(per_d.to(torch.int64), dim=1) - per_d
    idx = off[:, :, None] + torch.arange(N, device=dev)[None, None, :] % per_d[:, :, None]
    y = torch.gather(seg_d[:, None, :].expand(W, pcap, ccap), 2, idx)
    assert np.array_equal(y.cpu().numpy(), tile_segments(seg, periods, np.full(W, pcap), N)[0])
    dense = eng.overlap_add_tracks(y, masks_d, hop, L, cnt_d, w_d, w_d, True).cpu().numpy()
    _check(got, ref, mag, den, K, N, hop, "periodic")
    _check(dense, ref, mag, den, K, N, hop, "dense")
    print("k_overlap_add_periodic and the dense route agree bit for bit:", bool(np.array_equal(got, dense)))


# ------------------------------------------------------------------ (c) - (f) decompose_qo
Q_N, Q_HOP, Q_L, Q_NUM, Q_THRESH = 96, 24, 1003, 3, 0.05
Q_PERIODS = (23, 29, 31)
Q_ON = (((0, 380), (660, 840)), ((200, 380), (620, 840)), ((620, 1003),))  # where each component is switched on
Q_SILENT = (380, 620)  # no component and no noise: the frames that start at 384 .. 504 are all zero
Q_ALL = (660, 840)  # all three on


def _recording():
    """Three periodic components that switch on and off, small noise, a silent stretch and a ragged end
    ((Q_L - Q_N) is no multiple of Q_HOP).  On Q_ALL all three are on: 23 + 29 + 31 - 2 dictionary rows."""
    rng = np.random.default_rng(2024)
    x = 0.01 * rng.standard_normal(Q_L)
    for p, spans in zip(Q_PERIODS, Q_ON):
        wave = rng.integers(-8, 9, p) / 4.0
        tiled = np.tile(wave - wave.mean(), Q_L // p + 1)[:Q_L]
        for lo, hi in spans:
            x[lo:hi] += tiled[lo:hi]
    x[Q_SILENT[0] : Q_SILENT[1]] = 0.0
    return x


_HOST = {}


def _host_route(uw=True, trunc=False, dtype=np.float64):
    """-> (x, per (W, pcap), counts (W), seg (W, ccap), powers (W, pcap), silent (W), rows (W)): the frames of the recording through the
    batched QOPeriods.find_periods and get_periods.  An all-zero frame -- the fixed answer {"1": N} with weight 0 -- and
    an empty dictionary count as no block.  Computed once per setting and shared."""
    key = (uw, trunc, np.dtype(dtype).name)
    if key in _HOST:
        return _HOST[key]
    from pyperiod_amd import QOPeriods, ShortTime

    x = _recording()
    st = ShortTime(Q_N, Q_HOP, window=sqrt_hann(Q_N), dtype=dtype, trunc_to_integer_multiple=trunc)
    batch = st.frames(x)
    W = batch.shape[0]
    qo = QOPeriods(trunc_to_integer_multiple=trunc)
    silent = np.abs(batch.astype(np.float64)).sum(axis=1) <= 1e-16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if uw:
            fits = qo.find_periods(batch, Q_NUM, Q_THRESH, 2, None, True)
            live = [f for f in range(W) if not silent[f] and len(fits[f][0]["basis_dictionary"])]
            dicts = [fits[f][0]["basis_dictionary"] for f in live]
            weights = [fits[f][0]["weights"] for f in live]
        else:
            # The fixed-weight loop fits a period again whenever it is the strongest of the residual, and once more when
            # the test stops it; the dictionary of the class keeps one entry per period, so the blocks are taken from the
            # engine call the class makes (the same capacity) and the blocks of one period are added, zero-padded to
            # the period, in ascending block order: the tiles of a sum are the sum of the tiles.
            from pyperiod_amd import _ffi, default_engine

            p, _, k, c, wt, _, s = default_engine().qo_find_periods(batch, Q_NUM, Q_THRESH, 2, Q_N // 3, 128, trunc=trunc,
                                                                    update_weights=False)
            live = [f for f in range(W) if not silent[f] and c[f, 1] > 0]
            assert all(s[f] == _ffi.PH_ST_OK for f in live)
            dicts, weights, repeats = [], [], 0
            for f in live:
                merged, read = {}, 0
                for b in range(int(c[f, 1])):
                    q = int(p[f, b])
                    r = int(k[f, b]) or q  # (0 stands for `period` rows)
                    v = np.zeros(q)
                    v[:r] = wt[f, read : read + r]
                    read += r
                    repeats += q in merged
                    have = merged.get(q, (np.zeros(q), 0))
                    merged[q] = (have[0] + v, max(have[1], r))
                dicts.append({str(q): r for q, (v, r) in merged.items()})
                weights.append(np.concatenate([v[:r] for v, r in merged.values()]))
            assert repeats > 0  # the case this is about
        waves = qo.get_periods(weights, dicts)
    keys = {f: [int(q) for q in d.keys()] for f, d in zip(live, dicts)}
    pcap = max([Q_NUM] + [len(k) for k in keys.values()])
    ccap = max(1, max(sum(k) for k in keys.values()))
    per, counts = np.zeros((W, pcap), np.int32), np.zeros(W, np.int32)
    seg, powers = np.zeros((W, ccap)), np.zeros((W, pcap))
    for f, ws in zip(live, waves):
        counts[f] = len(keys[f])
        per[f, : counts[f]] = keys[f]
        seg[f, : sum(keys[f])] = np.concatenate(ws)
        powers[f, : counts[f]] = [np.mean(v * v) for v in ws]
    nrows = np.zeros(W, np.int64)  # dictionary rows of every frame
    nrows[live] = [sum(int(r) for r in d.values()) for d in dicts]
    _HOST[key] = (x, per, counts, seg, powers, silent, nrows)
    return _HOST[key]


def _against_host(res, host, groups=None):
    """decompose_qo's result against the host route of the same setting."""
    from pyperiod_amd import ShortTime, ShortTimeTracks

    x, per, counts, seg, powers, silent, _ = host
    W = per.shape[0]
    w = sqrt_hann(Q_N)
    assert isinstance(res, ShortTimeTracks)
    assert res.counts.dtype == np.int32 and np.array_equal(res.counts, counts)
    assert res.periods.shape == per.shape and np.array_equal(res.periods, per)
    assert np.allclose(res.powers, powers, rtol=1e-12, atol=0)  # the same squares, summed in another order
    if groups is None:
        groups = [(p,) for p in ShortTime.rank_periods(per, powers, counts, 8)]
    assert res.track_periods == groups
    T = len(groups)
    masks = np.zeros((T + 2, W), np.uint64)
    masks[: T + 1] = ShortTime.track_masks(per, counts, groups)
    masks[T + 1] = (np.uint64(1) << counts.astype(np.uint64)) - np.uint64(1)
    ref, mag, den, K = ola_periodic_ref(seg, per, counts, masks, Q_N, Q_HOP, Q_L, w, w, True)
    got = np.concatenate([res.tracks, res.other[None, :], res.periodic[None, :]])
    _check(got, ref, mag, den, K, Q_N, Q_HOP, "decompose_qo")
    pos = den > 0
    # the tracks and `other` partition the blocks: they add up to the periodic part within the summed bounds
    bound = sum(ola_bound(mag[t], den, K, Q_N, Q_HOP) for t in range(T + 1))
    err = np.abs(got[: T + 1].sum(0) - res.periodic)
    print("sum of the tracks against periodic: worst err / bound", float(np.max(err[pos] / np.maximum(bound[pos], 1e-300))))
    assert np.all(err[pos] <= bound[pos])
    # residual = x - periodic, one rounding
    assert np.array_equal(res.residual, x - res.periodic)
    back = np.abs(res.periodic + res.residual - x)
    assert np.all(back <= 2.0**-52 * np.maximum(np.abs(x), np.abs(res.periodic)))
    # activity: the powers of the track's blocks, ascending a
    act = np.zeros((T, W))
    for a in range(per.shape[1]):
        for t, g in enumerate(groups):
            act[t] += np.where((a < counts) & np.isin(per[:, a], g), res.powers[:, a], 0.0)
    assert np.array_equal(res.activity, act)
    # silent frames have no block and nothing periodic under them
    assert silent.sum() >= 2 and np.all(counts[silent] == 0)
    heard = np.zeros(Q_L, bool)
    for f in np.flatnonzero(~silent):
        heard[f * Q_HOP : f * Q_HOP + Q_N] = True
    assert (~heard).sum() >= Q_HOP and np.all(got[:, ~heard] == 0.0)
    return groups


@pytest.mark.parametrize("setting", [dict(), dict(uw=False), dict(trunc=True), dict(dtype=np.float32)],
                         ids=["default", "fixed_weights", "trunc", "float32"])
def test_decompose_qo_against_host_route(eng, torch_dev, setting):
    from pyperiod_amd import ShortTime

    torch, dev = torch_dev
    uw, trunc, dtype = setting.get("uw", True), setting.get("trunc", False), setting.get("dtype", np.float64)
    host = _host_route(uw, trunc, dtype)
    x, per, counts = host[0], host[1], host[2]
    assert counts.max() == Q_NUM and counts.min() == 0  # ragged
    st = ShortTime(Q_N, Q_HOP, window=sqrt_hann(Q_N), dtype=dtype, trunc_to_integer_multiple=trunc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = st.decompose_qo(x, Q_NUM, Q_THRESH, update_weights=uw)
        groups = _against_host(res, host)
        if setting:
            return
        # a 1-D device tensor gives the same result
        res_d = st.decompose_qo(torch.as_tensor(x, device=dev), Q_NUM, Q_THRESH)
        for a, b in zip(res, res_d):
            assert a == b if isinstance(a, list) else np.array_equal(a, b)
        # explicit tracks: a group of two periods, a period that never occurs, the rest in `other`
        explicit = [(groups[0][0], groups[-1][0]), 95]
        res_e = st.decompose_qo(x, Q_NUM, Q_THRESH, tracks=explicit)
        _against_host(res_e, host, [explicit[0], (95,)])
        assert np.all(res_e.tracks[1] == 0.0) and np.all(res_e.activity[1] == 0.0)
        assert np.array_equal(res_e.periodic, res.periodic)


def test_decompose_qo_fallback(eng):
    """max_rows = 64: a frame whose dictionary needs more rows (the host route says which) stays PH_ST_CAP and runs
    through the 1-D call -- with the result of the unrestricted run, and a warning that names it."""
    from pyperiod_amd import ShortTime

    host = _host_route()
    x = host[0]
    st = ShortTime(Q_N, Q_HOP, window=sqrt_hann(Q_N))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = st.decompose_qo(x, Q_NUM, Q_THRESH, max_rows=64)
    said = [str(c.message) for c in caught if "not finished by the device loop" in str(c.message)]
    assert len(said) == 1
    named = [int(v) for v in said[0].split("[")[1].split("]")[0].split(",")]
    nrows = host[6]
    print("frames handed to the host:", named, "their dictionary rows", nrows[named].tolist())
    assert named and all(0 <= f < nrows.size for f in named)
    assert (nrows > 64).any() and set(np.flatnonzero(nrows > 64).tolist()) <= set(named)  # what 64 rows cannot hold
    _against_host(res, host)


def test_decompose_qo_kernels_launched(eng):
    from pyperiod_amd import ShortTime

    x = _host_route()[0]
    st = ShortTime(Q_N, Q_HOP, window=sqrt_hann(Q_N))
    for uw, fit in ((True, "k_qo_find"), (False, "k_qo_greedy")):
        eng.profile(True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                st.decompose_qo(x, Q_NUM, Q_THRESH, update_weights=uw)
            names = [n for n, _ in eng.profile_read()]
        finally:
            eng.profile(False)
        print(uw, names)
        # num * max_length = 96 rows fit the first capacity (128): one capacity step
        assert names[0] == "k_frames" and names.count("k_frames") == 1
        assert names.count(fit) == 1
        assert names.count("k_qo_extract") == 1
        assert names.count("k_overlap_add_periodic") == 1 and names[-1] == "k_overlap_add_periodic"
        assert not [n for n in names if n.startswith("k_overlap_add") and n != "k_overlap_add_periodic"]


def test_decompose_qo_capacity_steps(eng):
    """A dictionary beyond the first capacity: num * max_length = 5 * 512 > 2048 starts the re-solved loop at 512 rows;
    the frames that hold two long periods need more, end PH_ST_CAP and are re-run -- gathered, at 1024 rows, and
    scattered back -- while the others keep their first result.  Against the batched class on the same frames, which
    steps the same way."""
    from pyperiod_amd import QOPeriods, ShortTime

    N, hop, num, thresh = 1536, 768, 5, 0.05
    L = 6 * hop + N
    rng = np.random.default_rng(77)
    x = 0.01 * rng.standard_normal(L)
    for p, (lo, hi) in ((389, (0, L)), (467, (3 * hop, L))):
        wave = rng.integers(-8, 9, p) / 4.0
        x[lo:hi] += np.tile(wave - wave.mean(), L // p + 1)[lo:hi]
    st = ShortTime(N, hop)
    if not eng.qo_feasible(N, np.float64, 1024, N // 3):
        pytest.fail("the capacity step this test is about is not feasible for N = 1536")
    batch = st.frames(x)
    qo = QOPeriods()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fits = qo.find_periods(batch, num, thresh)
        eng.profile(True)
        try:
            res = st.decompose_qo(x, num, thresh)
            names = [n for n, _ in eng.profile_read()]
        finally:
            eng.profile(False)
    print(names, res.periods.tolist(), res.counts.tolist())
    assert names.count("k_qo_find") >= 2  # the first capacity and at least one step (a 1-D fallback adds its own)
    assert names.count("k_frames") == 1 and names.count("k_overlap_add_periodic") == 1
    W = batch.shape[0]
    dicts = [fits[f][0]["basis_dictionary"] for f in range(W)]
    waves = qo.get_periods([fits[f][0]["weights"] for f in range(W)], dicts)
    rows = [sum(int(v) for v in d.values()) for d in dicts]
    assert min(rows) <= 512 < max(rows)  # both kinds of frame
    pcap = res.periods.shape[1]
    ccap = max(sum(int(q) for q in d) for d in dicts)
    per, counts, seg = np.zeros((W, pcap), np.int32), np.zeros(W, np.int32), np.zeros((W, ccap))
    for f, (d, ws) in enumerate(zip(dicts, waves)):
        counts[f] = len(d)
        per[f, : len(d)] = [int(q) for q in d]
        seg[f, : sum(per[f])] = np.concatenate(ws)
    assert np.array_equal(res.periods, per) and np.array_equal(res.counts, counts)
    groups = res.track_periods
    T = len(groups)
    masks = np.zeros((T + 2, W), np.uint64)
    masks[: T + 1] = ShortTime.track_masks(per, counts, groups)
    masks[T + 1] = (np.uint64(1) << counts.astype(np.uint64)) - np.uint64(1)
    ref, mag, den, K = ola_periodic_ref(seg, per, counts, masks, N, hop, L, None, None, True)
    got = np.concatenate([res.tracks, res.other[None, :], res.periodic[None, :]])
    _check(got, ref, mag, den, K, N, hop, "capacity steps")


def test_qo_tracks_that_mean_something(eng):
    """tracks=[23, 31] on the planted recording: component 23 is on over [0, 400) and [600, 800), component 31 from 560
    on.  Over the stretches where a component is on alone or with others, its track carries its energy; where it is
    off, the track is (nearly) empty.  Asserted: at least 0.9 of a track's energy lies where its component is on --
    far above an even spread over the recording (0.56 and 0.38 of the samples lie in the two components' spans) and
    with room below what the host route (find_periods -> get_periods -> ola_periodic_ref on the frames of this recording) gives,
    measured on an MI355X: 0.99908 for track 23 and 1.0 for track 31, and the same figures from decompose_qo."""
    from pyperiod_amd import ShortTime

    host = _host_route()
    x = host[0]
    st = ShortTime(Q_N, Q_HOP, window=sqrt_hann(Q_N))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = st.decompose_qo(x, Q_NUM, Q_THRESH, tracks=[23, 31])
    assert res.track_periods == [(23,), (31,)]
    _, per, counts, seg, _, _, _ = host
    masks = ShortTime.track_masks(per, counts, [(23,), (31,)])
    w = sqrt_hann(Q_N)
    ref = ola_periodic_ref(seg, per, counts, masks, Q_N, Q_HOP, Q_L, w, w, True)[0]
    on = np.zeros((2, Q_L), bool)
    for t, spans in enumerate((Q_ON[0], Q_ON[2])):
        for lo, hi in spans:
            on[t, lo:hi] = True
    for name, tr in (("host route", ref[:2]), ("decompose_qo", res.tracks)):
        share = [float(np.sum(tr[t][on[t]] ** 2) / np.sum(tr[t] ** 2)) for t in range(2)]
        print(name, "share of each track's energy where its component is on:", share)
        assert min(share) >= 0.9  # measured: 0.99908 and 1.0 on both routes
    # (activity is not held to the same figure frame by frame: in some frames of a component's span the greedy loop
    # explains it by another period, and the track is silent there)
    act = [float(res.activity[t][[f for f in range(per.shape[0])
                                  if any(lo < f * Q_HOP + Q_N and f * Q_HOP < hi for lo, hi in spans)]].sum()
                 / res.activity[t].sum()) for t, spans in enumerate((Q_ON[0], Q_ON[2]))]
    print("share of each track's activity in the frames that touch its component's spans:", act)


# ------------------------------------------------------------------ refusals through a live context
def test_bad_arguments_launch_nothing(eng, torch_dev):
    torch, dev = torch_dev
    seg, per, cnt = np.zeros((4, 16)), np.full((4, 2), 3, np.int32), np.full(4, 2, np.int32)
    masks = np.ones((3, 4), np.uint64)
    eng.profile(True)
    try:
        with pytest.raises(ValueError):  # a 64-bit mask names 64 blocks
            eng.overlap_add_periodic(np.zeros((4, 70)), np.ones((4, 65), np.int32), cnt, masks, 16, 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per, cnt, masks, 16, 8, 24)  # (W - 1) hop == L
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per, cnt, np.zeros((0, 4), np.uint64), 16, 8, 100)  # T = 0
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per, cnt, np.ones((3, 5), np.uint64), 16, 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per, np.zeros(3, np.int32), masks, 16, 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per[:3], cnt, masks, 16, 8, 100)
        with pytest.raises(ValueError):
            eng.overlap_add_periodic(seg, per, cnt, masks, 16, 8, 100, win_s=np.ones(15))
        with pytest.raises(TypeError):
            eng.overlap_add_periodic(seg.astype(np.float32), per, cnt, masks, 16, 8, 100)
        for bad in (masks.astype(np.float64), masks.astype(np.int32), masks.tolist()):
            with pytest.raises(TypeError):
                eng.overlap_add_periodic(seg, per, cnt, bad, 16, 8, 100)
        seg_d = torch.as_tensor(seg, device=dev)
        with pytest.raises(TypeError):  # device segments need device lists
            eng.overlap_add_periodic(seg_d, per, cnt, masks, 16, 8, 100)
        with pytest.raises(TypeError):
            eng.overlap_add_periodic(seg_d, torch.as_tensor(per, device=dev).to(torch.int64), torch.as_tensor(cnt, device=dev),
                                     torch.as_tensor(masks.view(np.int64), device=dev), 16, 8, 100)
        assert eng.profile_read() == []
        eng.overlap_add_periodic(seg, per, cnt, masks, 16, 8, 100)
        assert [n for n, _ in eng.profile_read()] == ["k_overlap_add_periodic"]
    finally:
        eng.profile(False)
