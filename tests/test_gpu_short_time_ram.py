"""ShortTime.decompose_ramanujan on the MI355X.

Kernel: k_ram_select_ref (PeriodEngine.ramanujan_select) bit for bit against the numpy restatement of its rule
(test_short_time_ram_cpu.select_ref) on the planted norm tables of that file -- no transform runs --, against
k_ram_select through ramanujan_fit where no row is over the cap, and against itself: numpy and tensor input, a side
stream, a repeated call, every row alone.

Pipeline: decompose_ramanujan on the recording of test_short_time_ram_cpu against the host route a user would write
from the public classes: numpy frames -> RamanujanPeriods.find_periods (batched) -> the rule -> the 1-D
find_periods_with_weights with each frame's list as test function -> QOPeriods.get_periods -> np.add.at.

Bars.  Lists, counts, `over`, frame_status and track_periods: equal.  Norms: 1e-10 B_q per entry against
po.ramanujan_norm_projector_q in longdouble (tests/test_gpu_ramanujan_census.py; float32 frames against the rounded
samples).  tracks / other / periodic: 1e-8 of the largest periodic sample (float32 frames: 1e-4), the bars of
tests/test_gpu_ram_fit.py and tests/test_gpu_short_time_qo.py for fitted weights, on every sample that no frame above
the condition cut covers -- cond(A A^T) <= 1e7 (float32: 1e5) of the ORACLE's dictionary; a frame above it may be
fitted on either side (status 0, 1 or 3) and is held to its list alone.  Powers are squares of the waveforms: twice
the bar.  Samples that only frames without a block cover are exactly 0.0.  The census of test_short_time_ram_cpu.py
holds, without a GPU, that at most 1 frame in 4 lies above the cut and that no norm is within 1e-6 of its threshold."""

import contextlib
import warnings

import numpy as np
import pytest

from test_short_time_cpu import frames_ref, sqrt_hann
from test_short_time_ram_cpu import (COND_CUT, PCAPS, Q_HIS, R_HOP, R_L, R_N, R_QHI, THRESH, host_route, planted, recording,
                                     reference_level, select_ref_batch)

pytestmark = pytest.mark.gpu

COND_CUT_F32 = 1e5  # tests/test_gpu_ram_fit.py


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


# ------------------------------------------------------------------ the kernel
def _same(got, want, what):
    for g, w, name in zip(got, want, ("periods", "counts", "over")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("q_hi", Q_HIS)
def test_kernel_against_the_rule(eng, torch_dev, q_hi):
    torch, dev = torch_dev
    side = torch.cuda.Stream(device=dev)
    for pcap in PCAPS:
        for with_ref in (False, True):
            norms, ref, labels = planted(q_hi, pcap, with_ref)
            want = select_ref_batch(norms, THRESH, ref, pcap)
            what = (q_hi, pcap, with_ref)
            _same(eng.ramanujan_select(norms, THRESH, ref, pcap), want, what + ("numpy",))
            _same(eng.ramanujan_select(norms, THRESH, ref, pcap), want, what + ("numpy again",))
            nd = torch.as_tensor(norms, device=dev)
            rd = None if ref is None else torch.as_tensor(ref, device=dev)
            got = eng.ramanujan_select(nd, THRESH, rd, pcap)
            assert all(g.is_cuda for g in got)
            _same(got, want, what + ("tensor",))
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                got = eng.ramanujan_select(nd, THRESH, rd, pcap)
                side.synchronize()
            _same(got, want, what + ("side stream",))
            for w, label in enumerate(labels):  # each row alone equals the row in the batch
                alone = eng.ramanujan_select(norms[w : w + 1], THRESH, None if ref is None else ref[w : w + 1], pcap)
                _same(alone, [a[w : w + 1] for a in want], what + (label,))


def test_kernel_on_a_long_row(eng):
    """Rows of many strides (q_hi = 1365, frame_length 4096 // 3), every row over the cap, ties in every stride."""
    rng = np.random.default_rng(3)
    norms = rng.integers(1, 40, (8, 1366)).astype(np.float64)  # few distinct values: ties at every cut
    norms[3, 100] = np.nan
    for pcap, ref in ((64, None), (16, np.full(8, 10.0)), (1, np.full(8, 1.0))):
        want = select_ref_batch(norms, 0.3, ref, pcap)
        assert (want[2] > pcap).sum() >= 7
        _same(eng.ramanujan_select(norms, 0.3, ref, pcap), want, ("long", pcap))


def test_lists_of_ramanujan_fit_where_no_row_is_over_the_cap(eng):
    """ref=None and over <= pcap: the lists k_ram_select writes inside ramanujan_fit, from the same norms."""
    from pyperiod_amd.synth import multi_sinusoid_window

    rng = np.random.default_rng(11)
    x = np.stack([multi_sinusoid_window(s, 192) for s in range(4)] + [rng.standard_normal(192) for _ in range(3)]
                 + [np.zeros(192)])
    for thresh in (0.2, 0.05):
        norms, per, counts = eng.ramanujan_fit(x, 2, 64, thresh, 64, 512)[:3]
        assert counts.max() <= 64 and counts.max() >= 3 and counts.min() == 0
        got = eng.ramanujan_select(norms, thresh, None, 64)
        _same(got, (per, counts, counts), ("fit", thresh))
        # the list survives a smaller capacity as long as it fits
        cap = int(counts.max())
        got = eng.ramanujan_select(norms, thresh, None, cap)
        _same(got, (per[:, :cap], counts, counts), ("fit at the cap", thresh))


def test_binding_refuses_before_launching(eng):
    eng.profile(True)
    try:
        for bad in (dict(thresh=0.0), dict(thresh=float("nan")), dict(pcap=0), dict(pcap=(1 << 20) + 1)):
            kw = dict(dict(thresh=0.2, pcap=4), **bad)
            with pytest.raises(Exception):
                eng.ramanujan_select(np.ones((3, 9)), kw["thresh"], None, kw["pcap"])
        with pytest.raises(Exception):
            eng.ramanujan_select(np.ones((3, 1)), 0.2)  # q_hi = 0
        with pytest.raises(ValueError):
            eng.ramanujan_select(np.ones((3, 9)), 0.2, np.ones(4))
        assert eng.profile_read() == []
        eng.ramanujan_select(np.ones((3, 9)), 0.2)
        assert [n for n, _ in eng.profile_read()] == ["k_ram_select_ref"]
    finally:
        eng.profile(False)


# ------------------------------------------------------------------ the pipeline: the host route from the public classes
def _class_norms(frames, q_lo, q_hi):
    from pyperiod_amd import RamanujanPeriods

    return RamanujanPeriods().find_periods(frames, q_lo, q_hi)


def _class_fit(frame, periods):
    from pyperiod_amd import RamanujanPeriods

    try:
        out, _ = RamanujanPeriods().find_periods_with_weights(frame, 2, R_QHI, test_function=lambda _norms: periods)
    except np.linalg.LinAlgError:
        return None
    d = out["basis_dictionary"]
    return [int(q) for q in d], [int(r) for r in d.values()], np.asarray(out["weights"], dtype=np.float64)


def _class_waves(keys, rows, weights):
    from pyperiod_amd import QOPeriods

    return np.concatenate(QOPeriods().get_periods(weights, {str(q): r for q, r in zip(keys, rows)}))


_WINDOWS = {"hann": sqrt_hann(R_N), "rect": None}
_HOST = {}


def _host(wname, dtype, thresh=0.2, reference="recording", max_periods=16):
    """The host route of one setting, computed once and shared; read only."""
    key = (wname, np.dtype(dtype).name, thresh, reference, max_periods)
    if key not in _HOST:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _HOST[key] = host_route(recording(), _WINDOWS[wname], thresh, reference, max_periods, dtype, _class_norms,
                                    _class_fit, _class_waves)
    return _HOST[key]


@contextlib.contextmanager
def _nan_planted(eng, torch):
    """While decompose_ramanujan runs: NaN in every weight behind the rows of a fitted dictionary (in every weight of a
    frame the fit did not finish), in the residual of the fit and in every segment element behind a frame's blocks --
    what the pipeline must not read."""
    fit, getp = eng.qo_fit, eng.qo_get_periods

    def qo_fit(x, periods, n_periods=None, kcap=512, max_period=None, window=None):
        keeps, wts, resid, st = fit(x, periods, n_periods, kcap, max_period, window)
        used = torch.where(st == 0, keeps.sum(dim=1), torch.zeros_like(st))[:, None]
        col = torch.arange(wts.shape[1], device=wts.device)[None, :]
        return keeps, torch.where(col < used, wts, wts.new_full((), np.nan)), torch.full_like(resid, np.nan), st

    def qo_get_periods(periods, rows, counts, weights, max_period=None, ccap=None):
        seg, st = getp(periods, rows, counts, weights, max_period, ccap)
        slot = torch.arange(periods.shape[1], device=seg.device)[None, :]
        total = (periods.clamp(min=0) * (slot < counts[:, None])).sum(dim=1, keepdim=True)
        col = torch.arange(seg.shape[1], device=seg.device)[None, :]
        return torch.where(col < total, seg, seg.new_full((), np.nan)), st

    eng.qo_fit, eng.qo_get_periods = qo_fit, qo_get_periods
    try:
        yield
    finally:
        del eng.qo_fit, eng.qo_get_periods


def _run(eng, torch, wname, dtype, signal=None, **kw):
    """-> (result, warnings, kernel names) of one decompose_ramanujan call with NaN planted around what it may read."""
    from pyperiod_amd import ShortTime

    st = ShortTime(R_N, R_HOP, window=_WINDOWS[wname], dtype=dtype)
    x = recording() if signal is None else signal
    eng.profile(True)
    try:
        with warnings.catch_warnings(record=True) as caught, _nan_planted(eng, torch):
            warnings.simplefilter("always")
            res = st.decompose_ramanujan(x, **kw)
        names = [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)
    return res, [str(c.message) for c in caught if "decompose_ramanujan" in str(c.message)], names


def _norm_units(frames):
    from oracle import period_oracle as po

    W = frames.shape[0]
    want = np.zeros((W, R_QHI + 1), dtype=np.longdouble)
    unit = np.zeros_like(want)
    for f in range(W):
        if frames[f].any():
            for q in range(2, R_QHI + 1):
                want[f, q], unit[f, q] = po.ramanujan_norm_projector_q(frames[f].astype(np.float64), q)
    return want, unit


_UNITS = {}


def _against_host(res, host, wname, dtype, fitted_on_host=False):
    from pyperiod_amd import ShortTimeRamanujan

    f32 = np.dtype(dtype) == np.float32
    cut, bar = (COND_CUT_F32, 1e-4) if f32 else (COND_CUT, 1e-8)
    x = recording()
    W = host["counts"].size
    assert isinstance(res, ShortTimeRamanujan)
    # ---- norms, entry by entry
    key = (wname, np.dtype(dtype).name)
    if key not in _UNITS:
        _UNITS[key] = _norm_units(frames_ref(x, R_N, R_HOP, W, _WINDOWS[wname], dtype))
    want, unit = _UNITS[key]
    assert res.norms.dtype == np.float64 and res.norms.shape == (W, R_QHI + 1)
    err = np.abs(res.norms.astype(np.longdouble) - want)
    print("norms: worst error in B_q", float(np.max(err[unit > 0] / unit[unit > 0])))
    assert np.all(err <= 1e-10 * unit)
    # ---- the lists: every frame
    assert res.over.dtype == np.int32 and np.array_equal(res.over, host["over"])
    assert res.frame_status.dtype == np.int8 and res.frame_status.shape == (W,)
    hard = (host["cond"] > cut) | (host["frame_status"] == 3)
    assert 4 * hard.sum() <= W
    good = ~hard
    fitted = good & (host["frame_status"] == 0)
    assert np.array_equal(res.frame_status[good], np.where(fitted & fitted_on_host, 1, host["frame_status"])[good])
    assert np.all(np.isin(res.frame_status[hard], (0, 1, 3)))
    assert res.counts.dtype == np.int32 and np.array_equal(res.counts[good], host["counts"][good])
    assert res.periods.shape == host["periods"].shape and np.array_equal(res.periods[good], host["periods"][good])
    listed = np.where(np.isin(res.frame_status, (0, 1)), host["list_counts"], 0)
    assert np.array_equal(res.counts, listed)  # a fitted frame keeps its whole list, any other frame nothing
    for f in np.flatnonzero(res.counts):
        assert res.periods[f, : res.counts[f]].tolist() == host["lists"][f, : res.counts[f]].tolist()
        assert not res.periods[f, res.counts[f] :].any() and not res.powers[f, res.counts[f] :].any()
    # ---- powers: squares of the waveforms
    scale = host["powers"].max()
    perr = np.abs(res.powers - host["powers"])[good]
    print("powers: worst error / largest power", float(perr.max() / scale))
    assert np.all(perr <= 2 * bar * scale)
    if not hard.any():
        assert res.track_periods == host["track_periods"]
    # ---- the waveforms on the time axis, where no frame above the cut is heard
    covered = np.zeros((W, R_L), bool)
    for f in range(W):
        covered[f, f * R_HOP : f * R_HOP + R_N] = True
    held = ~covered[hard].any(axis=0)
    blockless = ~covered[res.counts > 0].any(axis=0)
    assert held.sum() >= R_L // 2
    T = len(res.track_periods)
    got = np.concatenate([res.tracks, res.other[None, :], res.periodic[None, :]])
    assert got.dtype == np.float64 and got.shape == (T + 2, R_L)
    assert np.all(got[:, blockless] == 0.0)
    assert np.all(np.isfinite(got[:, held]))
    if res.track_periods == host["track_periods"]:
        ref = np.concatenate([host["tracks"], host["other"][None, :], host["periodic"][None, :]])
    else:  # (a frame above the cut moved a rank: the periodic part alone)
        got, ref = got[-1:], host["periodic"][None, :]
    scale = np.abs(host["periodic"][held]).max()
    terr = np.abs(got - ref)[:, held].max()
    print(f"tracks / other / periodic: worst error {terr:.2e} of {scale:.2e}, bar {bar:.0e}")
    assert terr <= bar * scale
    assert np.array_equal(res.residual, x - res.periodic)
    # ---- activity: the powers of the track's blocks, ascending block order
    act = np.zeros((T, W))
    for a in range(res.periods.shape[1]):
        for t, g in enumerate(res.track_periods):
            act[t] += np.where((a < res.counts) & np.isin(res.periods[:, a], g), res.powers[:, a], 0.0)
    assert np.array_equal(res.activity, act)


@pytest.mark.parametrize("wname", ["hann", "rect"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_decompose_ramanujan_against_host_route(eng, torch_dev, wname, dtype):
    torch, dev = torch_dev
    host = _host(wname, dtype)
    res, said, names = _run(eng, torch, wname, dtype)
    print(names, res.counts.tolist(), res.over.tolist(), res.frame_status.tolist(), res.track_periods)
    assert not said
    _against_host(res, host, wname, dtype)
    assert (7,) in res.track_periods and (12,) in res.track_periods
    unheard = np.ones(R_L, bool)  # the samples no frame with a list covers: the zero and quiet stretch
    for f in np.flatnonzero(host["list_counts"]):
        unheard[f * R_HOP : f * R_HOP + R_N] = False
    assert unheard.sum() >= 2 * R_HOP and not res.periodic[unheard].any() and res.periodic[~unheard].any()
    # the kernels of one call: the old selection kernel is not among them
    assert names.count("k_frames") == 1 and names.count("k_ramanujan") == 1
    assert names.count("k_ram_select") == 0 and names.count("k_ram_select_ref") == 1
    assert names.count("k_qo_fit") == 1 and names.count("k_qo_extract") == 1
    assert names.count("k_overlap_add_periodic") == 1 and names[-1] == "k_overlap_add_periodic"
    if wname == "hann" and dtype == np.float64:
        # a 1-D device tensor gives the same result
        res_d = _run(eng, torch, wname, dtype, signal=torch.as_tensor(recording(), device=dev))[0]
        for a, b in zip(res, res_d):
            assert a == b if isinstance(a, list) else np.array_equal(a, b)
        # explicit tracks: a group of two periods, a period that never occurs, the rest in `other`
        explicit = [(7, 12), 31]
        res_e = _run(eng, torch, wname, dtype, tracks=explicit)[0]
        assert res_e.track_periods == [(7, 12), (31,)]
        assert np.array_equal(res_e.periodic, res.periodic) and np.array_equal(res_e.periods, res.periods)
        assert np.all(res_e.tracks[1] == 0.0) and np.all(res_e.activity[1] == 0.0)
        host_e = host_route(recording(), _WINDOWS[wname], 0.2, "recording", 16, dtype, lambda *a: host["norms"],
                            lambda fr, lst: _fit_of(host, fr, lst), lambda k, r, w: w, tracks=[(7, 12), (31,)])
        _against_host(res_e, host_e, wname, dtype)


def _fit_of(host, frame, lst):
    """The fit the shared host route already made for this frame, as (keys, rows, waveforms): the explicit-track route
    reuses it (its `waves_fn` hands the waveforms through)."""
    for f in np.flatnonzero(host["counts"]):
        if np.array_equal(host["frames"][f], frame):
            assert host["periods"][f, : host["counts"][f]].tolist() == lst.tolist()
            return lst.tolist(), lst.tolist(), host["seg"][f, : int(lst.sum())]
    raise AssertionError(lst)


@pytest.mark.parametrize("wname", ["hann", "rect"])
def test_reference_modes(eng, torch_dev, wname):
    torch, _ = torch_dev
    host = _host(wname, np.float64)
    W = host["counts"].size
    zero = [f for f in range(W) if not host["frames"][f].any()]
    quiet = [f for f in range(W) if host["frames"][f].any() and np.abs(host["frames"][f]).max() < 0.01]
    assert zero and quiet
    rec = _run(eng, torch, wname, np.float64, reference="recording")[0]
    assert np.all(rec.frame_status[zero] == 2) and np.all(rec.frame_status[quiet] == 2)
    assert not rec.counts[zero].any() and not rec.counts[quiet].any()
    # measured against itself a quiet frame selects like a loud one; a zero frame never does
    fr, said, _ = _run(eng, torch, wname, np.float64, reference="frame")
    print("frame:", fr.counts.tolist(), fr.frame_status.tolist(), said)
    assert np.all(fr.over[quiet] > 0) and np.all(np.isin(fr.frame_status[quiet], (0, 1))) and np.all(fr.counts[quiet] > 0)
    assert np.all(fr.frame_status[zero] == 2) and not fr.over[zero].any()
    assert np.array_equal(fr.norms, rec.norms)
    _against_host(fr, _host(wname, np.float64, reference="frame"), wname, np.float64)
    # an absolute level equal to the recording's maximum is the "recording" mode, bit for bit
    level = float(reference_level(rec.norms, "recording")[0])
    assert level == rec.norms.max()
    ab = _run(eng, torch, wname, np.float64, reference=level)[0]
    for a, b in zip(rec, ab):
        assert a == b if isinstance(a, list) else np.array_equal(a, b)
    # a level far above every norm: nothing is selected, nothing is periodic
    none = _run(eng, torch, wname, np.float64, reference=1e3 * level)[0]
    assert np.all(none.frame_status == 2) and not none.over.any() and not none.periodic.any()
    assert none.track_periods == [] and none.tracks.shape == (0, R_L)


@pytest.mark.parametrize("wname", ["hann", "rect"])
def test_capped_lists(eng, torch_dev, wname):
    """thresh = 0.01 with max_periods = 4: frames over the cap keep their four strongest candidates."""
    torch, _ = torch_dev
    res, said, names = _run(eng, torch, wname, np.float64, thresh=0.01, max_periods=4)
    print(res.counts.tolist(), res.over.tolist(), res.frame_status.tolist())
    assert (res.over > res.counts).sum() >= 3 and res.counts.max() == 4 and res.periods.shape[1] == 4
    assert names.count("k_ram_select") == 0 and names.count("k_ram_select_ref") == 1
    ref = reference_level(res.norms, "recording")
    lists, counts, over = select_ref_batch(res.norms, 0.01, ref, 4)  # the rule on the device's own norms
    assert np.array_equal(res.over, over)
    fitted = np.isin(res.frame_status, (0, 1))
    assert np.array_equal(res.counts[fitted], counts[fitted]) and np.array_equal(res.periods[fitted], lists[fitted])
    _against_host(res, _host(wname, np.float64, 0.01, "recording", 4), wname, np.float64)


def test_capacity_step_and_host_fallback(eng, torch_dev):
    torch, _ = torch_dev
    host = _host("hann", np.float64)
    plain = _run(eng, torch, "hann", np.float64)[0]
    # max_rows = 50: capacities 32 and 50 -- the frames with more than 32 dictionary rows run a second time
    step, said, names = _run(eng, torch, "hann", np.float64, max_rows=50)
    print(names)
    assert not said and names.count("k_qo_fit") == 2 and names.count("k_overlap_add_periodic") == 1
    assert np.array_equal(step.frame_status, plain.frame_status) and np.array_equal(step.periods, plain.periods)
    _against_host(step, host, "hann", np.float64)
    # max_rows = 1: no dictionary fits; every frame with a list runs on the host and is named
    back, said, names = _run(eng, torch, "hann", np.float64, max_rows=1)
    assert len(said) == 1 and names.count("k_overlap_add_periodic") == 1
    named = [int(v) for v in said[0].split("[")[1].split("]")[0].split(",")]
    assert named == np.flatnonzero(host["list_counts"]).tolist() and len(named) >= 6
    assert np.array_equal(back.frame_status[named], np.ones(len(named), np.int8))
    assert np.array_equal(back.periods, plain.periods) and np.array_equal(back.counts, plain.counts)
    _against_host(back, host, "hann", np.float64, fitted_on_host=True)
