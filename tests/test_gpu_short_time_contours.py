"""k_follow_residual (PeriodEngine.follow_residual) and ShortTime.contours on the GPU.

The kernel is held, bit for bit, to the numpy restatement of ph_follow_residual's definition (peel_ref,
tests/contours_cases.py) on the case table of ph_follow, on the default engine (states in LDS) and on one created under
PH_HBM_WINDOW=1 (states in a workspace of the context); to ph_frames where no track is named; to k_follow's own segments
subtracted from ph_frames' frames; and to itself over every partition into blocks and over 70 000 frames.
contours is held, bit for bit, to its composition (contours_ref) with the engine's kind call as the map function, to
contour for one track, and to the two-voice claims of tests/test_short_time_contours_cpu.py through the GPU's maps."""
import os

import numpy as np
import pytest

from contours_cases import contours_ref, guard_ref, pack_live, peel_ref, two_voice_signal
from follow_cases import F64, cases
from test_gpu_short_time_map import KERNEL, KINDS, bits, engine_map, launches, sqrt_hann

pytestmark = pytest.mark.gpu
CASES = cases()
N, HOP, L = 256, 64, 3000


@pytest.fixture(scope="module")
def engines():
    """(default engine, engine whose states always live in HBM); PH_HBM_WINDOW is read when the context is created and
    restored right after."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import PeriodEngine, default_engine

    old = os.environ.get("PH_HBM_WINDOW")
    os.environ["PH_HBM_WINDOW"] = "1"
    try:
        hbm = PeriodEngine(0)
    finally:
        if old is None:
            del os.environ["PH_HBM_WINDOW"]
        else:
            os.environ["PH_HBM_WINDOW"] = old
    yield {"lds": default_engine(), "hbm": hbm}
    hbm.close()


@pytest.fixture(scope="module")
def refs():
    """peel_ref of every case of the table and both trunc settings, computed once."""
    return {(c["name"], trunc): peel_ref(c["signal"], c["N"], c["hop"], 0, c["W"], c["window"], c["frame_dtype"], c["periods"],
                                         c["counts"], trunc) for c in CASES for trunc in (False, True)}


@pytest.fixture(scope="module")
def recording():
    """The first L samples of the two-voice signal, a (W, 3) table of tracks with silent entries, and its residual."""
    x = two_voice_signal()[0][:L].copy()
    W = 1 + -((N - L) // HOP)
    rng = np.random.default_rng(8)
    per = rng.integers(0, N + 1, (W, 3)).astype(np.int32)
    per[rng.random((W, 3)) < 0.3] = 0
    per[0], per[1], per[2] = (1, N, 2), (0, 0, 0), (N - 1, 63, 65)
    packed, counts = pack_live(per)
    win = sqrt_hann(N)
    return x, W, packed, counts, win, peel_ref(x, N, HOP, 0, W, win, F64, packed, counts, False)


def dev_of(eng):
    import torch

    return torch.device("cuda", eng.device)


def planted(c):
    """The case's periods with live-looking garbage behind counts[f] (never read), and the signal as the first L elements
    of a wider device buffer that holds NaN behind them (never read either)."""
    per = c["periods"].copy()
    pcap = per.shape[1]
    for f in range(c["W"]):
        per[f, min(max(int(c["counts"][f]), 0), pcap):] = 3
    wide = np.full(c["L"] + 2 * c["N"], np.nan, dtype=c["signal"].dtype)
    wide[: c["L"]] = c["signal"]
    return per, wide


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("placement", ["lds", "hbm"])
@pytest.mark.parametrize("trunc", [False, True], ids=["plain", "trunc"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_residual_kernel_against_the_restatement(engines, refs, case, trunc, placement):
    import torch

    from pyperiod_amd import _ffi

    eng, c = engines[placement], case
    assert eng.follow_plan(c["N"])[2] == (_ffi.PH_PLAN_LDS if placement == "lds" else _ffi.PH_PLAN_HBM)
    dev = dev_of(eng)
    per, wide = planted(c)
    x = torch.as_tensor(wide, device=dev)[: c["L"]]
    win = None if c["window"] is None else torch.as_tensor(c["window"], device=dev)
    args = (c["N"], c["hop"], 0, c["W"], torch.as_tensor(per, device=dev), torch.as_tensor(c["counts"], device=dev), win,
            c["frame_dtype"], trunc)
    got, names = launches(eng, lambda: eng.follow_residual(x, *args))
    assert names == ["k_follow_residual"]
    assert torch.is_tensor(got) and got.dtype == torch.float64 and tuple(got.shape) == (c["W"], c["N"])
    want = refs[c["name"], trunc]
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (c["name"], placement, trunc)
    # host arrays: the same bits
    host = eng.follow_residual(c["signal"], c["N"], c["hop"], 0, c["W"], per, c["counts"], c["window"], c["frame_dtype"], trunc)
    assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(want))


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_no_tracks_is_frames_and_the_tie_to_k_follow(engines, refs, placement):
    """Without tracks (None, no columns, zero counts) the rows are ph_frames' in the frame dtype, widened; with tracks
    they are those frames less the tiled segments k_follow writes for the same arguments, subtracted in order."""
    import torch

    eng = engines[placement]
    dev = dev_of(eng)
    for c in CASES:
        per, wide = planted(c)
        x = torch.as_tensor(wide, device=dev)[: c["L"]]
        win = None if c["window"] is None else torch.as_tensor(c["window"], device=dev)
        pd, cd = torch.as_tensor(c["periods"], device=dev), torch.as_tensor(c["counts"], device=dev)
        Nc, hop, W = c["N"], c["hop"], c["W"]
        frames = eng.frames(x, Nc, hop, W, win, c["frame_dtype"]).to(torch.float64).cpu().numpy()
        for p, n in ((None, None), (pd[:, :0], cd), (pd, torch.zeros_like(cd)), (pd, torch.full_like(cd, -3))):
            got = eng.follow_residual(x, Nc, hop, 0, W, p, n, win, c["frame_dtype"], True)
            assert np.array_equal(bits(got.cpu().numpy()), bits(frames)), c["name"]
        for trunc in (False, True):
            seg, _, done = (a.cpu().numpy() for a in eng.follow(x, Nc, hop, W, pd, cd, 3 * Nc, win, c["frame_dtype"], trunc))
            want = frames.copy()
            for f in range(W):
                off = 0
                for a in range(int(done[f])):
                    p = int(c["periods"][f, a])
                    want[f] = want[f] - np.tile(seg[f, off : off + p], Nc // p + 1)[:Nc]
                    off += p
            got = eng.follow_residual(x, Nc, hop, 0, W, torch.as_tensor(per, device=dev), cd, win, c["frame_dtype"], trunc)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (c["name"], trunc)
            assert np.array_equal(bits(want), bits(refs[c["name"], trunc]))


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_every_partition_into_blocks_gives_the_rows_of_the_whole_call(engines, recording, placement):
    import torch

    eng = engines[placement]
    dev = dev_of(eng)
    x, W, packed, counts, win, want = recording
    xd, pd, cd, wd = (torch.as_tensor(a, device=dev) for a in (x, packed, counts, win))
    whole = eng.follow_residual(xd, N, HOP, 0, W, pd, cd, wd)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))
    for B in (1, 7, W - 1, W):
        for f0 in range(0, W, B):
            Wb = min(B, W - f0)
            part = eng.follow_residual(xd, N, HOP, f0, Wb, pd[f0 : f0 + Wb], cd[f0 : f0 + Wb], wd)
            assert torch.equal(part.view(torch.int64), whole[f0 : f0 + Wb].view(torch.int64)), (B, f0)
    # a block from host arrays (the whole signal goes up, the block's periods and counts)
    part = eng.follow_residual(x, N, HOP, 5, 9, packed[5:14], counts[5:14], win)
    assert np.array_equal(bits(part), bits(want[5:14]))
    # device tensors on a side stream
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        part, names = launches(eng, lambda: eng.follow_residual(xd, N, HOP, 3, W - 3, pd[3:], cd[3:], wd))
    side.synchronize()
    assert names == ["k_follow_residual"] and np.array_equal(bits(part.cpu().numpy()), bits(want[3:]))


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_many_frames_repeat(engines, placement):
    """70 000 frames of 64 samples: every workgroup takes several trips of its frame loop and W * N passes 2^22.  The
    signal repeats every K hops and the periods every K frames, so frame f must give the bits of frame f mod K, whose
    restatement is computed once; a block that starts at a multiple of K gives the same rows."""
    import torch

    eng = engines[placement]
    dev = dev_of(eng)
    n, hop, W, K, pcap = 64, 3, 70000, 250, 2
    assert W > 8 * eng.num_cu * 4
    rng = np.random.default_rng(12)
    Ls = (W - 1) * hop + n
    x = np.resize(rng.standard_normal(hop * K), Ls)
    base = rng.integers(0, n + 2, (K, pcap)).astype(np.int32)  # (0 and n + 1: a stop)
    base[:4] = [[1, 64], [63, 2], [64, 1], [2, 63]]
    cnt = rng.integers(0, pcap + 2, K).astype(np.int32)
    cnt[:4] = pcap
    win = sqrt_hann(n)
    want = peel_ref(x, n, hop, 0, K, win, F64, base, cnt, False)
    xd, wd = torch.as_tensor(x, device=dev), torch.as_tensor(win, device=dev)
    pd, cd = torch.as_tensor(np.resize(base, (W, pcap)), device=dev), torch.as_tensor(np.resize(cnt, W), device=dev)
    wd64 = torch.as_tensor(bits(want).view(np.int64), device=dev)
    idx = torch.arange(W, device=dev) % K
    got = eng.follow_residual(xd, n, hop, 0, W, pd, cd, wd)
    assert torch.equal(got.view(torch.int64), wd64[idx])
    f0 = 3 * K
    got = eng.follow_residual(xd, n, hop, f0, W - f0, pd[f0:], cd[f0:], wd)
    assert torch.equal(got.view(torch.int64), wd64[idx[: W - f0]])


# ------------------------------------------------------------------ ShortTime.contours
def kind_map(eng, kind, lo, hi, trunc=False):
    """map_fn of contours_ref: the engine's kind call on the restatement's frames, uploaded as float64."""
    import torch

    return lambda frames: engine_map(eng, torch.as_tensor(frames, device=dev_of(eng)), kind, lo, hi, trunc).cpu().numpy()


def same_as_ref(res, ref, lo, hi, kind):
    per, sal, scores, maps = ref
    assert res.periods.dtype == np.int32 and np.array_equal(res.periods, per)
    assert np.array_equal(bits(res.salience), bits(sal)) and np.array_equal(bits(res.scores), bits(scores))
    assert len(res.maps) == len(maps)
    for k, m in enumerate(res.maps):
        assert m.kind == kind and np.array_equal(m.periods, np.arange(lo, hi + 1))
        assert np.array_equal(bits(m.values), bits(maps[k])), (kind, k)


@pytest.mark.parametrize("kind", KINDS)
def test_contours_is_its_composition(engines, recording, kind):
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    x = recording[0]
    win = sqrt_hann(N)
    st = ShortTime(N, HOP, window=win)
    W = st.frame_count(L)
    mid = float(np.median(st.contour(x, kind=kind, band=2, jump=0.01, min_length=5, max_length=60).salience))  # (an input)
    table = ((8, 0.0, 2, None, None, None, None), (2, 0.01, 5, 60, 7, mid, 1), (0, 0.0, 3, 30, W, None, 0),
             (64, 1e-3, 2, None, W - 1, mid, None))
    for band, jump, lo, hi, B, floor, guard in table:
        top = N // 3 if hi is None else hi
        res, names = launches(eng, lambda: st.contours(x, 3, kind=kind, band=band, jump=jump, min_length=lo, max_length=hi,
                                                        floor=floor, guard=guard, block_frames=B, return_maps=True))
        blocks = 1 if B is None else -(-W // B)
        assert names == (["k_follow_residual", KERNEL[kind]] * blocks + ["k_period_path"]) * 3, (kind, B)
        assert all(isinstance(m.values, np.ndarray) for m in res.maps)
        ref = contours_ref(x, N, HOP, W, win, F64, False, 3, kind_map(eng, kind, lo, top), lo, band, jump, floor, guard)
        same_as_ref(res, ref, lo, top, kind)
        if B == 7:  # (the floor is the median of this very path's salience: it silences some frames of track 0, not all)
            assert np.any(res.periods[:, 0] == 0) and np.any(res.periods[:, 0] != 0)
        if guard is not None:
            assert all(np.isneginf(m.values).any() for m in res.maps[1:]) and not np.isneginf(res.maps[0].values).any()
        # every block_frames gives the same result, maps included
        for B2 in (1, 7, W + 1):
            if B2 != B:
                other = st.contours(x, 3, kind=kind, band=band, jump=jump, min_length=lo, max_length=hi, floor=floor,
                                    guard=guard, block_frames=B2, return_maps=True)
                same_as_ref(other, ref, lo, top, kind)
        plain = st.contours(x, 3, kind=kind, band=band, jump=jump, min_length=lo, max_length=hi, floor=floor, guard=guard,
                            block_frames=B)
        assert plain.maps is None and np.array_equal(plain.periods, res.periods)


@pytest.mark.parametrize("kind", ["norm", "gamma"])
def test_contours_honours_trunc_and_float32_frames(engines, recording, kind):
    """trunc reaches the peel and the sweep; float32 frames are rounded once and every round runs the float64 kernel on
    them, widened."""
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    x = recording[0].astype(np.float32)
    st = ShortTime(N, HOP, pad_end=False, dtype=np.float32, trunc_to_integer_multiple=True)
    W = st.frame_count(L)
    res = st.contours(x, 2, kind=kind, band=4, jump=0.001, min_length=4, max_length=70, block_frames=9, return_maps=True)
    ref = contours_ref(x, N, HOP, W, None, np.float32, True, 2, kind_map(eng, kind, 4, 70, True), 4, 4, 0.001)
    same_as_ref(res, ref, 4, 70, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_one_track_is_contour_and_a_tensor_signal_gives_tensor_maps(engines, recording, kind):
    import torch

    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    x = recording[0]
    st = ShortTime(N, HOP, window=sqrt_hann(N))
    args = dict(kind=kind, band=2, jump=0.01, min_length=5, max_length=60)
    for B in (None, 7):
        c = st.contour(x, block_frames=B, return_map=True, **args)
        cs = st.contours(x, 1, block_frames=B, return_maps=True, **args)
        assert cs.periods.shape == (c.periods.size, 1) and np.array_equal(cs.periods[:, 0], c.periods)
        assert np.array_equal(bits(cs.salience[:, 0]), bits(c.salience)) and bits(cs.scores[0]) == bits(c.score)
        assert np.array_equal(bits(cs.maps[0].values), bits(c.map.values)) and np.array_equal(cs.maps[0].periods, c.map.periods)
    want = st.contours(x, 2, guard=1, return_maps=True, **args)
    got = st.contours(torch.as_tensor(x, device=dev_of(eng)), 2, guard=1, block_frames=5, return_maps=True, **args)
    assert isinstance(got.periods, np.ndarray) and np.array_equal(got.periods, want.periods)
    assert np.array_equal(bits(got.salience), bits(want.salience)) and np.array_equal(bits(got.scores), bits(want.scores))
    for a, b in zip(got.maps, want.maps):
        assert torch.is_tensor(a.values) and a.values.is_cuda and a.periods.is_cuda and a.periods.dtype == torch.int32
        assert isinstance(b.values, np.ndarray) and np.array_equal(bits(a.values.cpu().numpy()), bits(b.values))


def test_two_voices_through_the_gpu_maps(engines):
    """The claims of test_short_time_contours_cpu.py with the same three bounds: track 0 follows the glide, track 1 the
    second voice, and the second-best path through the unpeeled map does not."""
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    x, period_at, second = two_voice_signal()
    st = ShortTime(256, 64, pad_end=False)
    W = st.frame_count(x.size)
    truth = np.array([round(period_at(64 * f + 128)) for f in range(W)])
    res = st.contours(x, 2, kind="gamma", band=2, jump=0.002, min_length=8, max_length=85, return_maps=True)
    assert W == 61 and res.periods.shape == (W, 2)
    on_glide = float(np.mean(np.abs(res.periods[:, 0] - truth) <= 1))
    on_second = float(np.mean(res.periods[:, 1] == second))
    guarded = 0.0
    for g in (0, 2, 4):
        path = eng.period_path(guard_ref(res.maps[0].values, 8, res.periods[:, :1], g), 2, 0.002)[0]
        guarded = max(guarded, float(np.mean(8 + path == second)))
    print(f"two voices: track 0 on the glide {on_glide:.3f}, track 1 on 47 {on_second:.3f}, "
          f"guarded second path on 47 {guarded:.3f}")
    assert on_glide == 1.0
    assert on_second >= 0.90
    assert guarded <= 0.25
    # the tracks found are tracks of what follow extracts: both voices leave less than the first alone
    both = st.follow(x, res)
    cols = st.follow(x, [res.periods[:, 0], res.periods[:, 1]])
    for a, b in zip(both, cols):
        assert np.array_equal(a, b, equal_nan=True) and a.dtype == b.dtype
    one = st.follow(x, st.contour(x, kind="gamma", band=2, jump=0.002, min_length=8, max_length=85))
    e2, e1 = float(np.sum(both.residual**2)), float(np.sum(one.residual**2))
    print(f"two voices: residual energy after both tracks {e2:.2f}, after the first alone {e1:.2f}")
    assert e2 < e1


def test_contours_names_the_round_and_the_frame_without_a_path(engines, recording):
    from pyperiod_amd import ShortTime

    x = recording[0].copy()
    st = ShortTime(N, HOP, window=sqrt_hann(N))
    with pytest.raises(ValueError, match="round 1.*no finite value"):  # every column within the guard of track 0
        st.contours(x, 2, kind="gamma", guard=10**6)
    with pytest.raises(ValueError, match="round 1"):
        st.contours(x, 3, kind="orth", guard=N, block_frames=6)
    x[10 * HOP + 5] = np.nan  # in the frames 7 .. 10
    for B in (None, 4):
        with pytest.raises(ValueError, match="round 0.*frame 7 "):
            st.contours(x, 2, kind="gamma", block_frames=B)
