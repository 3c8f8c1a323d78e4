"""ph_follow / ShortTime.follow without a GPU: the numpy restatement (tests/follow_cases.py) against the reference's own
Periods.project peeled T deep (tests/golden/follow.npz), its stop rules and unwritten elements, the packing helper, the
symbols, every refusal of the entry point and of ShortTime.follow, and what following a track buys on the glide signal."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from follow_cases import F32, F64, cases, follow_ref, glide_track, pack_ref
from period_path_cases import glide_signal


# ------------------------------------------------------------------ the restatement against the reference
def test_restatement_matches_reference_bit_for_bit(golden):
    g = golden("follow")
    assert int(g["count"]) == 16
    seen = set()
    for k in range(int(g["count"])):
        frame, periods, trunc = g[f"c{k}_frame"], g[f"c{k}_periods"], bool(g[f"c{k}_trunc"])
        N, T = frame.size, periods.size
        f32 = bool(np.array_equal(frame, frame.astype(np.float32).astype(np.float64)))
        seen.add((trunc, f32))
        seg, powers, done = follow_ref(frame, N, N, 1, None, F32 if f32 else F64, periods[None, :], [T], int(periods.sum()),
                                       trunc)
        assert done[0] == T
        assert np.array_equal(seg[0], g[f"c{k}_seg"]), k  # every element written, every bit the reference's
        norms = g[f"c{k}_norms"]
        assert np.array_equal(powers[0], (norms[:-1] - norms[1:]) / norms[0]), k
        # and the residual the walk leaves: one more block of period N projects it onto itself
        seg2, _, _ = follow_ref(frame, N, N, 1, None, F64, np.append(periods, N)[None, :], [T + 1], int(periods.sum()) + N,
                                trunc)
        assert np.array_equal(seg2[0, -N:], g[f"c{k}_residual"]), k
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_stop_rules_and_unwritten_elements():
    c = next(c for c in cases() if c["name"] == "stops")
    seg, powers, done = follow_ref(c["signal"], c["N"], c["hop"], c["W"], c["window"], c["frame_dtype"], c["periods"],
                                   c["counts"], c["ccap"], False)
    assert done.tolist() == [1, 0, 1, 1, 2, 0, 0]
    written = [5, 0, 5, 20, 30, 0, 0]
    for f, n in enumerate(written):
        assert np.all(np.isfinite(seg[f, :n])) and np.all(np.isnan(seg[f, n:])), f
        assert np.all(powers[f, done[f]:] == 0.0) and np.all(powers[f, : done[f]] > 0.0), f
    # counts are clipped to [0, pcap]; a silent frame writes nothing
    c = next(c for c in cases() if c["name"] == "n37")
    seg, powers, done = follow_ref(c["signal"], c["N"], c["hop"], c["W"], c["window"], c["frame_dtype"], c["periods"],
                                   c["counts"], c["ccap"], True)
    assert done.tolist() == [3, 3, 3, 0, 3, 0]
    assert np.all(np.isnan(seg[3])) and np.all(np.isnan(seg[5])) and np.all(np.isfinite(seg[2]))
    # an all-zero frame: powers exactly 0.0, the segments written as zeros
    seg, powers, done = follow_ref(np.zeros(40), 16, 8, 4, None, F64, np.full((4, 2), 5), [2] * 4, 10, False)
    assert np.all(seg == 0.0) and np.all(powers == 0.0) and done.tolist() == [2] * 4
    # a NaN sample propagates into its frames only
    x = np.ones(40)
    x[20] = np.nan
    seg, powers, done = follow_ref(x, 16, 8, 4, None, F64, np.full((4, 1), 4), [1] * 4, 4, False)
    assert done.tolist() == [1] * 4
    assert [bool(np.isnan(seg[f]).any()) for f in range(4)] == [False, True, True, False]
    assert [bool(np.isnan(powers[f, 0])) for f in range(4)] == [False, True, True, False]


def test_case_table_covers_what_it_says():
    cs = {c["name"]: c for c in cases()}
    assert {(c["N"], c["hop"]) for c in cs.values()} >= {(37, 5), (64, 64), (48, 61), (130, 33)}
    assert {c["periods"].shape[1] for c in cs.values()} == {1, 3}
    assert {1, 2, 63, 64, 65} <= set(np.concatenate([c["periods"].ravel() for c in cs.values()]).tolist())
    for c in cs.values():
        assert (c["W"] - 1) * c["hop"] < c["L"]
        assert {c["N"] - 1, c["N"]} & set(c["periods"].ravel().tolist()), c["name"]
    assert any(c["L"] < (c["W"] - 1) * c["hop"] + c["N"] for c in cs.values())  # a padded last frame
    assert {(c["signal"].dtype.type, c["frame_dtype"]) for c in cs.values()} == {(F64, F64), (F64, F32), (F32, F64),
                                                                                  (F32, F32)}


# ------------------------------------------------------------------ packing and masks
def test_pack_tracks_against_a_plain_loop():
    import torch

    from pyperiod_amd import ShortTime

    rng = np.random.default_rng(5)
    for W, T in ((1, 1), (7, 3), (5, 64), (40, 9)):
        per = rng.integers(-2, 6, (W, T)).astype(np.int32)
        per[0] = 3  # every column live in one frame (T = 64: bit 63 and the full row mask)
        if W > 1:
            per[1] = 0  # and a silent frame
        want = pack_ref(per)
        for arr in (per, torch.as_tensor(per)):
            packed, counts, masks, slot, live = ShortTime.pack_tracks(arr)
            got = [np.asarray(a) for a in (packed, counts, masks)]
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].shape == (T + 1, W)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(got[2].view(np.uint64), want[2])
            live, slot = np.asarray(live), np.asarray(slot)
            assert np.array_equal(live, per >= 1)
            f, t = np.nonzero(live)
            assert np.array_equal(got[0][f, slot[f, t]], per[f, t])


# ------------------------------------------------------------------ the C ABI without a GPU
def test_symbols_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    assert "ph_follow: extraction along a period track" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for name, n_args in (("ph_follow", 17), ("ph_follow_plan_info", 5)):
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args and len(_ffi.SIGNATURES[name]) == n_args
        for arg, have in zip(args, _ffi.SIGNATURES[name]):
            if "*" in arg:
                assert have in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), arg
            else:
                assert have is ctype[arg.rsplit(" ", 1)[0]], arg
    from pyperiod_amd import PeriodEngine, ShortTime, ShortTimeFollow

    assert callable(PeriodEngine.follow) and callable(PeriodEngine.follow_plan) and callable(ShortTime.follow)
    assert ShortTimeFollow._fields == ("periods", "powers", "tracks", "periodic", "residual")


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
    good = dict(ctx=ctx, signal=buf, in_dtype=_ffi.PH_F64, L=40, N=16, hop=8, W=4, window=buf, frame_dtype=_ffi.PH_F32,
                periods=buf, counts=buf, pcap=3, ccap=20, flags=0, seg=buf, powers=buf, done=buf)
    order = list(good)

    def call(**change):
        a = dict(good, **change)
        return lib.ph_follow(*[a[k] for k in order])

    def said(word):
        return word in lib.ph_last_error()

    for dev in (0, _ffi.PH_FLAG_DEVICE, _ffi.PH_FLAG_DEVICE | _ffi.PH_FLAG_TRUNC):
        assert call(ctx=None, flags=dev) == E and said(b"ctx")
        for name in ("signal", "periods", "counts", "seg", "powers", "done"):
            assert call(flags=dev, **{name: None}) == E and said(b"NULL"), name
        for name in ("in_dtype", "frame_dtype"):
            for bad in (2, -1, 7):
                assert call(flags=dev, **{name: bad}) == E and said(b"dtype"), (name, bad)
        for name in ("L", "N", "hop", "W"):
            for bad in (0, -1):
                assert call(flags=dev, **{name: bad}) == E and said(b">= 1"), (name, bad)
        assert call(flags=dev, W=-2**63) == E and call(flags=dev, L=-2**63) == E
        assert call(flags=dev, W=6) == E and said(b">= L")  # (W - 1) * hop = 40 >= L
        for pcap in (0, -1, 65, 2**31 - 1):
            assert call(flags=dev, pcap=pcap) == E and said(b"pcap"), pcap
        for ccap in (0, -1, 2**24 + 1, 2**31 - 1):
            assert call(flags=dev, ccap=ccap) == E and said(b"ccap"), ccap
        big = 2**63 - 1
        assert call(flags=dev, L=big, W=2**60, hop=1, ccap=2**24) == E and said(b"64 bits")
        assert call(flags=dev, L=big, W=1) == E and said(b"64 bits")
        assert call(flags=dev, L=2**50, W=2**40, hop=1, ccap=2**24) == E and said(b"64 bits")
        assert call(flags=dev, L=2**60 - 1, W=2**57, hop=2, pcap=64, ccap=1) == E and said(b"64 bits")
    n = ctypes.c_int(0)
    ref = ctypes.byref(n)
    assert lib.ph_follow_plan_info(None, 64, ref, ref, ref) == E
    assert lib.ph_follow_plan_info(ctx, 64, None, ref, ref) == E
    assert lib.ph_follow_plan_info(ctx, 64, ref, None, ref) == E
    assert lib.ph_follow_plan_info(ctx, 64, ref, ref, None) == E
    for N in (0, -5):
        assert lib.ph_follow_plan_info(ctx, N, ref, ref, ref) == E and said(b"N=")


def test_engine_follow_argument_errors_without_gpu():
    import torch

    from test_short_time_cpu import cpu_engine

    eng, Reached = cpu_engine()
    x = torch.zeros(40, dtype=torch.float64)
    per, cnt = torch.ones((4, 2), dtype=torch.int32), torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="1-D"):
        eng.follow(torch.zeros((2, 20)), 16, 8, 4, per, cnt, 8)
    with pytest.raises(ValueError, match="count"):
        eng.follow(x, 16, 8, -1, per, cnt, 8)
    with pytest.raises(ValueError, match="periods"):
        eng.follow(x, 16, 8, 4, per[:3], cnt, 8)
    with pytest.raises(ValueError, match="periods"):
        eng.follow(x, 16, 8, 4, per[:, 0], cnt, 8)
    with pytest.raises(ValueError, match="counts"):
        eng.follow(x, 16, 8, 4, per, cnt[:3], 8)
    with pytest.raises(TypeError, match="periods"):
        eng.follow(x, 16, 8, 4, per.numpy(), cnt, 8)
    with pytest.raises(TypeError, match="counts"):
        eng.follow(x, 16, 8, 4, per, cnt.to(torch.int64), 8)
    with pytest.raises(ValueError, match="window"):
        eng.follow(x, 16, 8, 4, per, cnt, 8, window=torch.ones(15, dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        eng.follow(x, 16, 8, 4, per, cnt, 8, frame_dtype=np.int32)
    with pytest.raises(TypeError, match="seg"):
        eng.follow(x, 16, 8, 4, per, cnt, 8, seg=np.zeros((4, 8)))
    with pytest.raises(ValueError, match="seg"):
        eng.follow(x, 16, 8, 4, per, cnt, 8, seg=torch.zeros((4, 9), dtype=torch.float64))
    with pytest.raises(Reached):
        eng.follow(x, 16, 8, 4, per, cnt, 8, window=torch.ones(16, dtype=torch.float64), frame_dtype=torch.float32,
                   trunc=True, seg=torch.zeros((4, 8), dtype=torch.float64))


def test_short_time_follow_validates_before_touching_the_gpu(monkeypatch):
    import sys

    import torch

    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime, ShortTimeContour

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)
    st = ShortTime(96, 24)
    x = np.zeros(300)
    W = st.frame_count(300)
    ok = np.full(W, 20, dtype=np.int32)
    for bad in (ok[:-1], np.full(W + 1, 20), np.full((W - 1, 2), 20), np.zeros((2, W), dtype=np.int64)):
        with pytest.raises(ValueError, match="rows"):
            st.follow(x, bad)
    with pytest.raises(ValueError, match="rows"):
        st.follow(x, [ok, ok[:-1]])
    with pytest.raises(ValueError, match="rows"):
        st.follow(x, np.zeros((W, 2, 2), dtype=np.int32))
    for bad in (np.zeros((W, 0), dtype=np.int32), np.full((W, 65), 3), [], [np.full((W, 40), 3), np.full((W, 25), 3)]):
        with pytest.raises(ValueError, match="tracks"):
            st.follow(x, bad)
    for bad in (np.full(W, 97), np.where(np.arange(W) == W - 1, 2**31 - 1, 5), [ok, np.full(W, 2**40)],
                torch.full((W,), 97, dtype=torch.int64)):
        with pytest.raises(ValueError, match="longer than a frame"):
            st.follow(x, bad)
    for bad in (ok.astype(np.float64), ok.astype(np.float32), ok > 0, torch.full((W,), 20.0), [ok, ok.astype(np.float64)]):
        with pytest.raises(ValueError, match="integers"):
            st.follow(x, bad)
    for flags in (dict(orthogonalize=True), dict(orthogonalize=True, trunc_to_integer_multiple=True)):
        with pytest.raises(ValueError, match="orthogonalize"):
            ShortTime(96, 24, **flags).follow(x, ok)
    with pytest.raises(ValueError, match="1-D"):
        st.follow(np.zeros((2, 150)), ok)
    # what passes the checks reaches the engine
    contour = ShortTimeContour(ok, np.zeros(W), 0.0)
    for good in (ok, ok.astype(np.int64), ok.astype(np.uint8), np.full((W, 64), 96), contour, [contour, ok - 30, np.zeros((W, 2), dtype=np.int16)],
                 np.full(W, -(2**40))):
        with pytest.raises(AssertionError, match="the GPU was touched"):
            st.follow(x, good)
    with pytest.raises(AssertionError, match="the GPU was touched"):
        ShortTime(96, 24, trunc_to_integer_multiple=True, dtype=np.float32).follow(x.astype(np.float32), ok)


# ------------------------------------------------------------------ what following a track buys
@pytest.mark.parametrize("windowed", [False, True], ids=["rectangular", "sqrt-hann"])
def test_glide_signal_residual_along_the_track_against_the_best_constant_period(windowed):
    """N = 128, hop = 32, the true track rounded, energy over the samples N .. L - N: following the track must leave at
    most 0.6 of what the best constant period in 18 .. 32 leaves (measured: 0.48 rectangular, 0.46 sqrt-Hann)."""
    from test_short_time_cpu import sqrt_hann
    from test_short_time_qo_cpu import ola_periodic_ref

    x, period_at = glide_signal()
    L, N, hop = x.size, 128, 32
    W = 1 + -((N - L) // hop)
    win = sqrt_hann(N) if windowed else None

    def residual_energy(track):
        per = np.asarray(track, dtype=np.int32).reshape(W, 1)
        counts = np.ones(W, dtype=np.int32)
        seg, _, done = follow_ref(x, N, hop, W, win, F64, per, counts, int(per.max()), False)
        assert np.all(done == 1)
        out = ola_periodic_ref(np.nan_to_num(seg), per, counts, np.ones((1, W), dtype=np.uint64), N, hop, L, win, win)[0]
        return float(np.sum((x - out[0])[N : L - N] ** 2))

    along = residual_energy(glide_track(N, hop, W, period_at))
    constant = min(residual_energy(np.full(W, p)) for p in range(18, 33))
    print(f"residual along the track {along:.1f}, best constant period {constant:.1f}, ratio {along / constant:.3f}")
    assert along <= 0.6 * constant
