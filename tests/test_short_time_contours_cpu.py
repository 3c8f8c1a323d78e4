"""ph_follow_residual / ShortTime.contours without a GPU: the symbols, every refusal of the entry point, of the binding
and of ShortTime.contours, the numpy restatements (tests/contours_cases.py) against follow_ref and on a planted map, and
what peeling buys on the two-voice signal -- the second-best path through one map follows twice the glide, the best path
through the map of the residual follows the second voice."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from contours_cases import contours_ref, guard_ref, oracle_gamma_map, pack_live, peel_ref, two_voice_signal
from follow_cases import cases, follow_ref, frame_ref
from period_path_cases import period_path_ref


# ------------------------------------------------------------------ the C ABI without a GPU
def test_symbol_in_binding_header_and_package():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    assert "ph_follow_residual: the frames of a recording less the tracks named for them" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    m = re.search(r"\bint ph_follow_residual\s*\(([^;]*)\);", text)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 15 and len(_ffi.SIGNATURES["ph_follow_residual"]) == 15
    for arg, have in zip(args, _ffi.SIGNATURES["ph_follow_residual"]):
        if "*" in arg:
            assert have is ctypes.c_void_p, arg
        else:
            assert have is ctype[arg.rsplit(" ", 1)[0]], arg
    assert callable(_ffi.load().ph_follow_residual)  # exported
    import pyperiod_amd
    from pyperiod_amd import PeriodEngine, ShortTime, ShortTimeContours

    assert callable(PeriodEngine.follow_residual) and callable(ShortTime.contours)
    assert "ShortTimeContours" in pyperiod_amd.__all__
    assert ShortTimeContours._fields == ("periods", "salience", "scores", "maps")


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
    good = dict(ctx=ctx, signal=buf, in_dtype=_ffi.PH_F64, L=40, N=16, hop=8, f0=1, Wb=3, window=buf,
                frame_dtype=_ffi.PH_F32, periods=buf, counts=buf, pcap=3, flags=0, out=buf)
    order = list(good)

    def call(**change):
        a = dict(good, **change)
        return lib.ph_follow_residual(*[a[k] for k in order])

    def said(word):
        return word in lib.ph_last_error()

    for dev in (0, _ffi.PH_FLAG_DEVICE, _ffi.PH_FLAG_DEVICE | _ffi.PH_FLAG_TRUNC):
        assert call(ctx=None, flags=dev) == E and said(b"ctx")
        for name in ("signal", "out"):
            assert call(flags=dev, **{name: None}) == E and said(b"NULL"), name
        for change in (dict(periods=None), dict(counts=None), dict(periods=None, counts=None, pcap=1)):
            assert call(flags=dev, **change) == E and said(b"NULL") and said(b"pcap"), change
        for name in ("in_dtype", "frame_dtype"):
            for bad in (2, -1, 7):
                assert call(flags=dev, **{name: bad}) == E and said(b"dtype"), (name, bad)
        for name in ("L", "N", "hop", "Wb"):
            for bad in (0, -1):
                assert call(flags=dev, **{name: bad}) == E and said(b">= 1"), (name, bad)
        assert call(flags=dev, Wb=-2**63) == E and call(flags=dev, L=-2**63) == E
        for bad in (-1, -2**63):
            assert call(flags=dev, f0=bad) == E and said(b"f0"), bad
        # (f0 + Wb - 1) * hop >= L: 40 = L, at either end of f0's range, and with f0 + Wb beyond int64
        for change in (dict(f0=2, Wb=4), dict(f0=0, Wb=6), dict(f0=5, Wb=1), dict(f0=2**63 - 1), dict(f0=2**63 - 3, Wb=3)):
            assert call(flags=dev, **change) == E and said(b">= L"), change
        for pcap in (-1, 65, 2**31 - 1, -2**31):
            assert call(flags=dev, pcap=pcap) == E and said(b"pcap"), pcap
        big = 2**63 - 1
        assert call(flags=dev, L=big, Wb=1) == E and said(b"64 bits")  # L * 8
        assert call(flags=dev, L=2**60, Wb=1) == E and said(b"64 bits")
        assert call(flags=dev, L=2**59, hop=1, f0=0, Wb=2**57) == E and said(b"64 bits")  # Wb * N * 8 = 2^64
        assert call(flags=dev, L=2**58, N=1, hop=1, f0=0, Wb=2**57, pcap=64) == E and said(b"Wb * pcap")  # 2^65 bytes


def test_engine_follow_residual_argument_errors_without_gpu():
    import torch

    from test_short_time_cpu import cpu_engine

    eng, Reached = cpu_engine()
    x = torch.zeros(40, dtype=torch.float64)
    per, cnt = torch.ones((3, 2), dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="1-D"):
        eng.follow_residual(torch.zeros((2, 20)), 16, 8, 1, 3, per, cnt)
    with pytest.raises(ValueError, match="count"):
        eng.follow_residual(x, 16, 8, 1, -1, per, cnt)
    with pytest.raises(ValueError, match="together"):
        eng.follow_residual(x, 16, 8, 1, 3, per, None)
    with pytest.raises(ValueError, match="together"):
        eng.follow_residual(x, 16, 8, 1, 3, None, cnt)
    with pytest.raises(ValueError, match="periods"):
        eng.follow_residual(x, 16, 8, 1, 3, per[:2], cnt)
    with pytest.raises(ValueError, match="periods"):
        eng.follow_residual(x, 16, 8, 1, 3, per[:, 0], cnt)
    with pytest.raises(ValueError, match="counts"):
        eng.follow_residual(x, 16, 8, 1, 3, per, cnt[:2])
    with pytest.raises(TypeError, match="periods"):
        eng.follow_residual(x, 16, 8, 1, 3, per.numpy(), cnt)
    with pytest.raises(TypeError, match="counts"):
        eng.follow_residual(x, 16, 8, 1, 3, per, cnt.to(torch.int64))
    with pytest.raises(ValueError, match="window"):
        eng.follow_residual(x, 16, 8, 1, 3, per, cnt, window=torch.ones(15, dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        eng.follow_residual(x, 16, 8, 1, 3, per, cnt, frame_dtype=np.int32)
    for good in ((per, cnt), (None, None), (per[:, :0], cnt)):
        with pytest.raises(Reached):
            eng.follow_residual(x, 16, 8, 1, 3, *good, window=torch.ones(16, dtype=torch.float64), frame_dtype=torch.float32,
                                trunc=True)


def test_contours_validates_before_an_engine_exists(monkeypatch):
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
    # what contour refuses
    for bad, word in ((dict(kind="cepstrum"), "kind"), (dict(min_length=0), "min_length"), (dict(min_length=9, max_length=8), "max_length"),
                      (dict(kind="ramanujan", max_length=30030), "Ramanujan"), (dict(band=-1), "band"), (dict(band=65), "band"),
                      (dict(band=2.0), "band"), (dict(band=True), "band"), (dict(jump=-0.1), "jump"), (dict(jump=np.inf), "jump"),
                      (dict(jump=np.nan), "jump"), (dict(jump="1"), "jump"), (dict(min_length=1, max_length=8193), "periods"),
                      (dict(block_frames=0), "block_frames"), (dict(block_frames=2.0), "block_frames")):
        with pytest.raises(ValueError, match=word):
            st.contours(x, 2, **bad)
        with pytest.raises(ValueError, match=word):  # (and contour does refuse it)
            st.contour(x, **bad)
    for kind in ("orth", "ramanujan"):
        with pytest.raises(ValueError, match="trunc_to_integer_multiple"):
            ShortTime(96, 24, trunc_to_integer_multiple=True).contours(x, 2, kind=kind)
    # its own
    for bad in (0, -1, 65, 2.0, True, None, "2", 2**40):
        with pytest.raises(ValueError, match="count"):
            st.contours(x, bad)
    for bad in (-1, 1.0, True, "1", -2**40):
        with pytest.raises(ValueError, match="guard"):
            st.contours(x, 2, guard=bad)
    for bad in (np.nan, np.inf, -np.inf, "0.1", True, 1j, [0.1]):
        with pytest.raises(ValueError, match="floor"):
            st.contours(x, 2, floor=bad)
    for kind in ("norm", "gamma", "orth", "ramanujan"):
        for flags in (dict(orthogonalize=True), dict(orthogonalize=True, trunc_to_integer_multiple=True)):
            with pytest.raises(ValueError, match="orthogonalize"):
                ShortTime(96, 24, **flags).contours(x, 2, kind=kind)
    with pytest.raises(ValueError, match="1-D"):
        st.contours(np.zeros((2, 150)), 2)
    # what passes the checks reaches the engine
    for good in (dict(count=1), dict(count=64), dict(count=np.int64(3), guard=0, floor=0), dict(count=2, guard=np.int32(4), floor=-1.5),
                 dict(count=2, kind="orth", band=0, jump=0), dict(count=2, kind="ramanujan", block_frames=3, return_maps=True)):
        with pytest.raises(AssertionError, match="the GPU was touched"):
            st.contours(x, **good)
    with pytest.raises(AssertionError, match="the GPU was touched"):
        ShortTime(96, 24, trunc_to_integer_multiple=True, dtype=np.float32).contours(x.astype(np.float32), 2)


def test_follow_takes_contours_like_a_contour():
    from pyperiod_amd import ShortTime, ShortTimeContours

    st = ShortTime(96, 24)
    W = st.frame_count(300)
    per = np.stack([np.full(W, 20), np.where(np.arange(W) % 2, 0, 31)], 1).astype(np.int32)
    cs = ShortTimeContours(per, np.zeros((W, 2)), np.zeros(2))
    assert np.array_equal(st._follow_periods(cs, W), per)
    assert np.array_equal(st._follow_periods([cs, per[:, 0]], W), np.concatenate([per, per[:, :1]], 1))
    with pytest.raises(ValueError, match="rows"):
        st._follow_periods(cs, W + 1)


# ------------------------------------------------------------------ the restatement of the residual
CASES = cases()


@pytest.mark.parametrize("trunc", [False, True], ids=["plain", "trunc"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_peel_ref_is_frame_ref_less_the_tiled_segments_of_follow_ref(case, trunc):
    c = case
    N, hop, W = c["N"], c["hop"], c["W"]
    frames = np.stack([frame_ref(c["signal"], N, hop, f, c["window"], c["frame_dtype"]) for f in range(W)])
    # zero counts, no arrays, no columns: the frames themselves
    for per, cnt in ((c["periods"], np.zeros(W, dtype=np.int32)), (None, None), (c["periods"][:, :0], c["counts"])):
        got = peel_ref(c["signal"], N, hop, 0, W, c["window"], c["frame_dtype"], per, cnt, trunc)
        assert np.array_equal(got.view(np.uint64), frames.view(np.uint64))
    # no ccap in the residual: give follow_ref room for every block that the other two stop rules let through
    ccap = 3 * N
    seg, _, done = follow_ref(c["signal"], N, hop, W, c["window"], c["frame_dtype"], c["periods"], c["counts"], ccap, trunc)
    want = frames.copy()
    for f in range(W):
        off = 0
        for a in range(int(done[f])):
            p = int(c["periods"][f, a])
            want[f] = want[f] - np.tile(seg[f, off : off + p], N // p + 1)[:N]
            off += p
    got = peel_ref(c["signal"], N, hop, 0, W, c["window"], c["frame_dtype"], c["periods"], c["counts"], trunc)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if done.max() > 0:
        assert not np.array_equal(got, frames)
    # a block of the frames is those rows
    if W > 2:
        part = peel_ref(c["signal"], N, hop, 1, W - 2, c["window"], c["frame_dtype"], c["periods"][1:-1], c["counts"][1:-1], trunc)
        assert np.array_equal(part.view(np.uint64), got[1:-1].view(np.uint64))


# ------------------------------------------------------------------ floor and guard on a planted map
def planted(frames):
    """A map function that ignores the samples but for one thing: the energy of the frame scales column 2 (period 5),
    so a peeled frame loses it.  Columns are the periods 3 .. 9."""
    W = frames.shape[0]
    m = np.tile(np.array([0.1, 0.2, 0.0, 0.3, 0.35, 0.2, 0.4]), (W, 1))
    m[:, 2] = np.sqrt(np.mean(frames**2, axis=1))
    return m


def test_floor_silences_frames_and_silent_frames_are_not_peeled():
    N, hop, W = 20, 20, 6
    x = np.tile(np.array([4.0, 0, 0, 0, 0]), W * N // 5)  # rms 1.79 per frame, all of it at period 5
    x[2 * N : 3 * N] *= 0.25  # a frame whose rms, 0.447, still wins its row and lies under the floor
    per, sal, _, maps = contours_ref(x, N, hop, W, None, np.float64, False, 2, planted, 3, 8, 0.0, floor=0.5)
    quiet = np.arange(W) == 2
    assert np.array_equal(per[:, 0], np.where(quiet, 0, 5))  # column 2 wins everywhere, the floor silences frame 2
    assert np.all(sal[~quiet, 0] > 0.5) and sal[2, 0] == maps[0][2, 2] and 0.4 < sal[2, 0] <= 0.5  # salience keeps the value
    # round 1: the loud frames were peeled (period 5 removes all of them), the silent one was not
    frames1 = peel_ref(x, N, hop, 0, W, None, np.float64, *pack_live(per[:, :1]), False)
    assert np.all(frames1[~quiet] == 0.0) and np.array_equal(frames1[2], x[2 * N : 3 * N])
    assert np.all(maps[1][~quiet, 2] == 0.0) and maps[1][2, 2] == maps[0][2, 2]
    # ... so frame 2 finds period 5 again and the others period 9 at 0.4, all of it under the floor
    assert np.all(per[:, 1] == 0) and np.all(sal[~quiet, 1] == 0.4) and sal[2, 1] == sal[2, 0]
    # no floor: every frame is peeled, and the second track is period 9 everywhere
    per, sal, scores, maps = contours_ref(x, N, hop, W, None, np.float64, False, 2, planted, 3, 8, 0.0)
    assert np.all(per[:, 0] == 5) and np.all(maps[1][:, 2] == 0.0) and np.all(per[:, 1] == 9)
    assert scores[1] == period_path_ref(maps[1], 8, 0.0)[2] and scores[1] == np.sum(sal[:, 1])


def test_guard_cells_are_clipped_at_both_edges_and_a_dead_row_raises():
    m = np.arange(4 * 7, dtype=np.float64).reshape(4, 7)  # periods 3 .. 9
    earlier = np.array([[3, 0], [9, -4], [6, 4], [0, 0]], dtype=np.int32)
    assert np.array_equal(guard_ref(m, 3, earlier, None), m) and guard_ref(m, 3, earlier, None) is not m
    g0 = guard_ref(m, 3, earlier, 0)
    assert np.argwhere(np.isneginf(g0)).tolist() == [[0, 0], [1, 6], [2, 1], [2, 3]]
    g2 = guard_ref(m, 3, earlier, 2)
    dead = np.isneginf(g2)
    assert dead[0].tolist() == [True, True, True, False, False, False, False]  # 3 +- 2: 1 and 2 do not exist
    assert dead[1].tolist() == [False, False, False, False, True, True, True]  # 9 +- 2: 10 and 11 do not exist
    assert dead[2].tolist() == [True, True, True, True, True, True, False]  # 6 +- 2 and 4 +- 2 overlap
    assert not dead[3].any() and np.array_equal(g2[~dead], m[~dead])  # silent entries forbid nothing
    assert np.isneginf(guard_ref(m, 3, earlier, 10**9)[:3]).all()
    # through contours_ref: round 0 picks column 6 (period 9) everywhere; a guard of 6 forbids every column of round 1
    flat = lambda frames: np.tile(np.array([0.1, 0.2, 0.0, 0.3, 0.6, 0.2, 0.7]), (frames.shape[0], 1))  # noqa: E731
    x = np.ones(80)
    per, sal, _, maps = contours_ref(x, 20, 20, 4, None, np.float64, False, 2, flat, 3, 8, 0.0, guard=1)
    assert np.all(per[:, 0] == 9) and np.all(per[:, 1] == 7) and np.all(sal[:, 1] == 0.6)
    assert np.isneginf(maps[1][:, 5:]).all() and np.isfinite(maps[1][:, :5]).all() and np.isfinite(maps[0]).all()
    with pytest.raises(ValueError, match="round 1"):
        contours_ref(x, 20, 20, 4, None, np.float64, False, 2, flat, 3, 8, 0.0, guard=6)
    # a floor that silences round 0 leaves nothing to guard
    per, _, _, maps = contours_ref(x, 20, 20, 4, None, np.float64, False, 2, flat, 3, 8, 0.0, floor=0.9, guard=6)
    assert np.all(per == 0) and np.isfinite(maps[1]).all()


# ------------------------------------------------------------------ what peeling buys
def two_voice_shares(map_fn, maps_out=None):
    """The three shares of the two-voice claim for a map function over (W, 256) float64 frames, periods 8 .. 85:
    (frames where track 0 is within 1 of the glide, frames where track 1 is 47, frames where the guarded second path
    through the unpeeled map is 47 -- the largest over the guards 0, 2, 4)."""
    x, period_at, second = two_voice_signal()
    N, hop, lo, band, jump = 256, 64, 8, 2, 0.002
    W = 1 + (x.size - N) // hop  # pad_end=False
    assert W == 61
    truth = np.array([round(period_at(hop * f + N // 2)) for f in range(W)])
    per, _, _, maps = contours_ref(x, N, hop, W, None, np.float64, False, 2, map_fn, lo, band, jump)
    on_glide = float(np.mean(np.abs(per[:, 0] - truth) <= 1))
    on_second = float(np.mean(per[:, 1] == second))
    guarded = 0.0
    for g in (0, 2, 4):
        path = period_path_ref(guard_ref(maps[0], lo, per[:, :1], g), band, jump)[0]
        guarded = max(guarded, float(np.mean(lo + path == second)))
    return on_glide, on_second, guarded


def test_peeling_finds_the_second_voice_where_the_second_best_path_does_not():
    on_glide, on_second, guarded = two_voice_shares(oracle_gamma_map(8, 85))
    print(f"two voices: track 0 on the glide {on_glide:.3f}, track 1 on 47 {on_second:.3f}, "
          f"guarded second path on 47 {guarded:.3f}")
    assert on_glide == 1.0  # every frame
    assert on_second >= 0.90
    assert guarded <= 0.25
