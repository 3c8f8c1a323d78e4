"""k_follow (PeriodEngine.follow) and ShortTime.follow on the GPU, against the numpy restatement of ph_follow's
definition (tests/follow_cases.py): seg and done bit for bit, powers within 1e-10 * pn(r_a) / pn(x_f), on the default
engine (states in LDS) and on one created under PH_HBM_WINDOW=1 (states in a workspace of the context); the frame loop
over 70 000 frames; and the two-launch pipeline of ShortTime.follow against its host composition."""
import os

import numpy as np
import pytest

from follow_cases import F64, cases, follow_ref, pack_ref, power_bounds
from period_path_cases import glide_signal
from test_short_time_cpu import ola_bound, sqrt_hann
from test_short_time_qo_cpu import ola_periodic_ref

pytestmark = pytest.mark.gpu
CASES = cases()


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
    """follow_ref of every case of the table and both trunc settings, computed once."""
    out = {}
    for c in CASES:
        for trunc in (False, True):
            r = follow_ref(c["signal"], c["N"], c["hop"], c["W"], c["window"], c["frame_dtype"], c["periods"], c["counts"],
                           c["ccap"], trunc)
            out[c["name"], trunc] = r + (power_bounds(c["signal"], c["N"], c["hop"], c["W"], c["window"], c["frame_dtype"],
                                                      c["periods"], r[2], trunc),)
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def check(got, ref, what):
    """seg (NaN planted where nothing may be written: still that NaN) and done bit for bit, powers within the bound."""
    seg, powers, done = (np.asarray(a.cpu()) if hasattr(a, "cpu") else a for a in got)
    rseg, rpow, rdone, bound = ref
    assert np.array_equal(done, rdone), what
    assert np.array_equal(bits(seg), bits(rseg)), what  # (the restatement's NaN are the planted ones, bit for bit)
    err = np.abs(powers - rpow)
    print(f"{what}: max powers error over bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound), what
    for f in range(done.size):
        assert np.all(bits(powers[f, done[f]:]) == 0), what  # exactly +0.0 behind done


@pytest.mark.parametrize("placement", ["lds", "hbm"])
@pytest.mark.parametrize("trunc", [False, True], ids=["plain", "trunc"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_follow_kernel_against_the_restatement(engines, refs, case, trunc, placement):
    import torch

    from pyperiod_amd import _ffi

    eng, c = engines[placement], case
    block, lds, where = eng.follow_plan(c["N"])
    assert where == (_ffi.PH_PLAN_LDS if placement == "lds" else _ffi.PH_PLAN_HBM)
    assert 64 <= block <= 1024 and block % 64 == 0 and lds >= (2 * 8 * c["N"] if placement == "lds" else 0)
    dev = torch.device("cuda", eng.device)
    x = torch.as_tensor(c["signal"], device=dev)
    win = None if c["window"] is None else torch.as_tensor(c["window"], device=dev)
    per, cnt = torch.as_tensor(c["periods"], device=dev), torch.as_tensor(c["counts"], device=dev)
    seg = torch.full((c["W"], c["ccap"]), float("nan"), dtype=torch.float64, device=dev)
    got = eng.follow(x, c["N"], c["hop"], c["W"], per, cnt, c["ccap"], win, c["frame_dtype"], trunc, seg=seg)
    assert got[0] is seg
    check(got, refs[c["name"], trunc], f"{c['name']} {placement} trunc={trunc}")


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_host_arrays_and_a_signal_off_16_byte_alignment(engines, refs, placement):
    """The host-pointer form (seg travels both ways, so its planted NaN survive), and device signals whose first sample
    lies one element behind a 16-byte boundary."""
    import torch

    eng = engines[placement]
    for c in CASES[:3]:
        seg = np.full((c["W"], c["ccap"]), np.nan)
        got = eng.follow(c["signal"], c["N"], c["hop"], c["W"], c["periods"], c["counts"], c["ccap"], c["window"],
                         c["frame_dtype"], False, seg=seg)
        check(got, refs[c["name"], False], f"{c['name']} host arrays")
        dev = torch.device("cuda", eng.device)
        buf = torch.zeros(c["L"] + 1, dtype=torch.float64 if c["signal"].dtype == F64 else torch.float32, device=dev)
        buf[1:] = torch.as_tensor(c["signal"], device=dev)
        x = buf[1:]
        assert x.data_ptr() % 16 == x.element_size()
        win = None if c["window"] is None else torch.as_tensor(c["window"], device=dev)
        seg = torch.full((c["W"], c["ccap"]), float("nan"), dtype=torch.float64, device=dev)
        got = eng.follow(x, c["N"], c["hop"], c["W"], torch.as_tensor(c["periods"], device=dev),
                         torch.as_tensor(c["counts"], device=dev), c["ccap"], win, c["frame_dtype"], False, seg=seg)
        check(got, refs[c["name"], False], f"{c['name']} misaligned signal")


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_many_frames_repeat_and_alone(engines, placement):
    """70 000 frames of N = 16: every workgroup takes several trips of its frame loop.  The signal repeats every K hops
    and the periods every K frames, so frame f must give the bits of frame f mod K, whose restatement is computed once."""
    import torch

    eng = engines[placement]
    N, hop, W, K, pcap = 16, 3, 70000, 250, 2
    assert W > 8 * eng.num_cu * 4
    rng = np.random.default_rng(11)
    L = (W - 1) * hop + N
    x = np.resize(rng.standard_normal(hop * K), L)
    base = rng.integers(0, N + 1, (K, pcap)).astype(np.int32)  # (0: a stop)
    per = np.resize(base, (W, pcap))
    cnt = np.resize(rng.integers(0, pcap + 2, K).astype(np.int32), W)
    ccap = 2 * N
    win = sqrt_hann(N)
    rseg, rpow, rdone = follow_ref(x, N, hop, K, win, F64, base, cnt[:K], ccap, False)
    bound = power_bounds(x, N, hop, K, win, F64, base, rdone, False)
    dev = torch.device("cuda", eng.device)
    args = (torch.as_tensor(x, device=dev), N, hop, W, torch.as_tensor(per, device=dev), torch.as_tensor(cnt, device=dev), ccap,
            torch.as_tensor(win, device=dev), None, False)
    runs = []
    for _ in range(2):
        seg = torch.full((W, ccap), float("nan"), dtype=torch.float64, device=dev)
        runs.append([a.cpu().numpy() for a in eng.follow(*args, seg=seg)])
    for a, b in zip(*runs):  # a repeated call gives the same bits
        assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                              b.view(np.uint64 if b.dtype == np.float64 else b.dtype))
    seg, powers, done = runs[0]
    idx = np.arange(W) % K
    assert np.array_equal(done, rdone[idx])
    assert np.array_equal(bits(seg), bits(rseg)[idx])
    assert np.array_equal(bits(powers), bits(powers[:K])[idx])  # the reduction has one order, whichever workgroup runs it
    assert np.all(np.abs(powers[:K] - rpow) <= bound)
    # five frames together and each alone
    f0 = 40
    xs = torch.as_tensor(x[f0 * hop : (f0 + 4) * hop + N], device=dev)
    together = [a.cpu().numpy() for a in eng.follow(xs, N, hop, 5, args[4][f0 : f0 + 5], args[5][f0 : f0 + 5], ccap, args[7],
                                                    seg=torch.full((5, ccap), float("nan"), dtype=torch.float64, device=dev))]
    for k in range(5):
        alone = [a.cpu().numpy() for a in eng.follow(xs[k * hop : k * hop + N], N, hop, 1, args[4][f0 + k : f0 + k + 1],
                                                     args[5][f0 + k : f0 + k + 1], ccap, args[7],
                                                     seg=torch.full((1, ccap), float("nan"), dtype=torch.float64, device=dev))]
        assert np.array_equal(bits(alone[0][0]), bits(together[0][k])) and np.array_equal(bits(alone[1][0]), bits(together[1][k]))
        assert alone[2][0] == together[2][k]
        assert np.array_equal(bits(together[0][k]), bits(seg[f0 + k]))


# ------------------------------------------------------------------ ShortTime.follow
def launches(eng, call):
    eng.profile(True)
    try:
        res = call()
        return res, [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)


def host_composition(st, x, per):
    """ShortTime.frames, then follow_ref on those frames, then ola_periodic_ref: -> (rows (T + 1, L), bound, seg, packed,
    counts, masks, powers (W, T), their bound (W, T))."""
    N, hop, L = st.frame_length, st.hop, x.shape[0]
    frames = np.asarray(st.frames(x), dtype=np.float64)
    W, T = per.shape
    packed, counts, masks = pack_ref(per)
    ccap = max(1, int(packed.sum(1).max()))
    seg, pw, done = follow_ref(frames.ravel(), N, N, W, None, F64, packed, counts, ccap, st._trunc_to_integer_multiple)
    assert np.array_equal(done, counts)
    seg = np.nan_to_num(seg)
    out, mag, den, K = ola_periodic_ref(seg, packed, counts, masks, N, hop, L, st.window, st.window)
    pb = power_bounds(frames.ravel(), N, N, W, None, F64, packed, done, st._trunc_to_integer_multiple)
    powers, pbound = np.zeros((W, T)), np.zeros((W, T))
    for f in range(W):
        powers[f, per[f] >= 1] = pw[f, : counts[f]]
        pbound[f, per[f] >= 1] = pb[f, : counts[f]]
    return out, ola_bound(mag, den, K, N, hop), seg, packed, counts, masks, powers, pbound


def check_follow(eng, st, x, per, res):
    out, bound, seg, packed, counts, masks, powers, pbound = host_composition(st, np.asarray(x.cpu()) if hasattr(x, "cpu") else x, per)
    T, L = per.shape[1], out.shape[1]
    got = [np.asarray(a.cpu()) if hasattr(a, "cpu") else a for a in res]
    assert np.array_equal(got[0], per) and got[0].dtype == np.int32
    rows = np.vstack([got[2], got[3][None, :]])
    assert rows.shape == (T + 1, L)
    assert np.all(np.abs(rows - out) <= bound)
    again = eng.overlap_add_periodic(seg, packed, counts, masks, st.frame_length, st.hop, L, st.window, st.window)
    assert np.array_equal(bits(rows), bits(again))  # the restatement's segments give these very bits
    assert np.all(np.abs(got[1] - powers) <= pbound) and np.all(got[1][per < 1] == 0.0)
    xs = np.asarray(x.cpu()) if hasattr(x, "cpu") else x
    assert np.array_equal(bits(got[4]), bits(xs.astype(np.float64) - got[3]))
    return rows


def test_follow_a_contour_of_the_glide_signal(engines):
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    x, _ = glide_signal()
    st = ShortTime(128, 32, window=sqrt_hann(128))
    c = st.contour(x, kind="gamma", band=2, jump=0.002, min_length=8, max_length=42)
    res, names = launches(eng, lambda: st.follow(x, c))
    assert names == ["k_follow", "k_overlap_add_periodic"]
    assert all(isinstance(a, np.ndarray) for a in res) and res.tracks.shape == (1, x.size)
    rows = check_follow(eng, st, x, c.periods.reshape(-1, 1), res)
    assert np.array_equal(bits(rows[0]), bits(rows[1]))  # one track: it is the periodic part


@pytest.mark.parametrize("dtype,trunc", [(np.float64, False), (np.float32, True)])
def test_follow_two_tracks_with_silent_frames(engines, dtype, trunc):
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    rng = np.random.default_rng(3)
    n = np.arange(1500)
    x = (np.sin(2 * np.pi * n / 9.0) + np.sign(np.sin(2 * np.pi * n / 14.0)) + 0.2 * rng.standard_normal(n.size)).astype(dtype)
    st = ShortTime(96, 40, window=sqrt_hann(96), dtype=dtype, trunc_to_integer_multiple=trunc)
    W = st.frame_count(x.size)
    a = np.where(np.arange(W) % 4 == 1, 0, 9).astype(np.int32)
    b = np.where(np.arange(W) % 5 == 2, -1, 14).astype(np.int64)
    b[3], a[3] = 0, 0  # a frame in which both are silent
    res, names = launches(eng, lambda: st.follow(x, [a, b]))
    assert names == ["k_follow", "k_overlap_add_periodic"]
    per = np.stack([a, b.astype(np.int32)], 1)
    check_follow(eng, st, x, per, res)
    assert res.tracks.shape == (2, x.size) and np.any(res.tracks[0] != 0) and np.any(res.tracks[1] != 0)


def test_follow_a_tensor_signal_on_a_side_stream(engines):
    import torch

    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    dev = torch.device("cuda", eng.device)
    x, _ = glide_signal(2000)
    st = ShortTime(64, 16)
    W = st.frame_count(x.size)
    per = np.stack([np.full(W, 25), np.where(np.arange(W) % 3 == 0, 0, 13)], 1).astype(np.int32)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        xd = torch.as_tensor(x, device=dev)
        res, names = launches(eng, lambda: st.follow(xd, torch.as_tensor(per, device=dev)))
    side.synchronize()
    assert names == ["k_follow", "k_overlap_add_periodic"]
    assert all(torch.is_tensor(a) and a.device == dev for a in res)
    assert res.periods.dtype == torch.int32 and res.tracks.shape == (2, x.size)
    check_follow(eng, st, x, per, res)
    host = st.follow(x, per)  # numpy in, numpy out, the same bits
    for a, b in zip(res, host):
        assert isinstance(b, np.ndarray) and np.array_equal(a.cpu().numpy(), b, equal_nan=True)


def test_bad_arguments_launch_nothing(engines):
    from pyperiod_amd import ShortTime

    eng = engines["lds"]
    st = ShortTime(64, 16)
    x = np.zeros(500)
    W = st.frame_count(500)
    for bad in (np.full(W - 1, 5), np.full(W, 65), np.full(W, 5.0), np.zeros((W, 65), dtype=np.int32)):
        eng.profile(True)
        try:
            with pytest.raises(ValueError):
                st.follow(x, bad)
            assert eng.profile_read() == []
        finally:
            eng.profile(False)
    eng.profile(True)
    try:
        with pytest.raises(ValueError):
            ShortTime(64, 16, orthogonalize=True).follow(x, np.full(W, 5))
        with pytest.raises(ValueError):  # the library's own refusal: a frame that starts behind the signal
            eng.follow(x, 64, 16, W + 40, np.ones((W + 40, 1), dtype=np.int32), np.ones(W + 40, dtype=np.int32), 8)
        assert eng.profile_read() == []
    finally:
        eng.profile(False)
