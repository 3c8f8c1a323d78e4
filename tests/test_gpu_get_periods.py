"""QOPeriods.get_periods on the MI355X: k_qo_extract (ph_qo_get_periods) against the repaired reference's results
(tests/golden/qo_get_periods.npz), in both placements of its work arrays, as one mixed batch, from device tensors, by its
status words and at the placement switch; and the class surface after a batched find_periods.

Bars: 1e-10 (the project's fp64 bar) against the fixture and against the numpy restatement of the closed form
(tests/test_get_periods_cpu.py), relative to max(1, max |result|); equal bits between the two placements, between a batch
and its rows and between host arrays and device tensors (one fixed summation order); 1e-12 for the three properties,
which compare two runs of the same arithmetic on inputs that differ by rounding.  The class after find_periods is held
to 1e-8 against the fixture: its weights come from the device solve, which tests/test_gpu_qo_batch.py holds to that bar
against the reference's weights, and the extraction is a projection (it does not amplify them)."""

import os
import warnings

import numpy as np
import pytest

from pyperiod_amd.synth import multi_sinusoid_window
from test_get_periods_cpu import cases, closed_form

pytestmark = pytest.mark.gpu
TOL_REF, TOL_SAME, TOL_SOLVE = 1e-10, 1e-12, 1e-8


@pytest.fixture(scope="module")
def engines():
    """(default engine, engine whose work arrays always live in HBM); PH_HBM_WINDOW is read when the context is created
    and restored right after."""
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
    yield default_engine(), hbm
    hbm.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("qo_get_periods")


def _pack(dicts):
    """[(keys, vals, weights)] -> periods, rows (W, pcap) int32, counts (W) int32, weights (W, kcap) float64."""
    W, pcap = len(dicts), max(len(k) for k, _, _ in dicts)
    kcap = max(1, max(len(w) for _, _, w in dicts))
    per, rws = np.zeros((W, pcap), dtype=np.int32), np.zeros((W, pcap), dtype=np.int32)
    cnt, wts = np.zeros(W, dtype=np.int32), np.zeros((W, kcap))
    for i, (k, v, w) in enumerate(dicts):
        per[i, : len(k)], rws[i, : len(k)], cnt[i], wts[i, : len(w)] = k, v, len(k), w
    return per, rws, cnt, wts


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _rel(got, want):
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


@pytest.fixture(scope="module")
def per_case(engines, fixture):
    """Every fixture case through both engines, one call each: {k: (lds result, hbm result)} (computed once)."""
    from pyperiod_amd import _ffi

    out = {}
    for k, keys, vals, wts in cases(fixture):
        res = []
        for eng in engines:
            o, st = eng.qo_get_periods(*_pack([(keys, vals, wts)]))
            assert st.tolist() == [_ffi.PH_ST_OK], (k, st)
            assert o.shape == (1, sum(keys)) and o.dtype == np.float64
            res.append(o[0])
        out[k] = tuple(res)
    return out


def test_plan_places_the_engines(engines):
    from pyperiod_amd import _ffi

    lds, hbm = (e.plan_info("qo_get_periods", 600, (300, 100))[0] for e in engines)
    assert (lds.window, lds.second, lds.block) == (_ffi.PH_PLAN_LDS, _ffi.PH_PLAN_LDS, 256)
    assert (hbm.window, hbm.second, hbm.block) == (_ffi.PH_PLAN_HBM, _ffi.PH_PLAN_HBM, 256)
    assert hbm.lds_bytes < lds.lds_bytes


def test_every_fixture_case_in_both_placements(fixture, per_case):
    worst = 0.0
    for k, keys, vals, wts in cases(fixture):
        lds, hbm = per_case[k]
        assert _same_bits(lds, hbm), (k, keys)
        for t in ("rr", "lu", "qr", "lstsq"):
            want = fixture.get(f"c{k}_{t}", fixture[f"c{k}_lstsq"])  # raised / singular: the projector's result
            err = _rel(lds, want)
            worst = max(worst, err)
            assert err <= TOL_REF, (k, keys, t, err)
    print("k_qo_extract vs reference fixture: worst", worst)


def test_mixed_batch_equals_the_rows(engines, fixture, per_case):
    from pyperiod_amd import _ffi

    all_cases = list(cases(fixture))
    assert {len(keys) for _, keys, _, _ in all_cases} == {1, 2, 3, 4, 5}
    for which, eng in enumerate(engines):
        out, st = eng.qo_get_periods(*_pack([(keys, vals, wts) for _, keys, vals, wts in all_cases]))
        assert st.tolist() == [_ffi.PH_ST_OK] * len(all_cases)
        assert out.shape == (len(all_cases), max(sum(keys) for _, keys, _, _ in all_cases))
        for (k, keys, _, _), row in zip(all_cases, out):
            assert _same_bits(row[: sum(keys)], per_case[k][which]), (k, keys)
            assert not row[sum(keys):].any()  # zero behind the last segment


def _property_cases(fixture):
    return [(k, keys, vals, wts) for k, keys, vals, wts in cases(fixture) if fixture[f"c{k}_n"] == 600 or keys == [36, 24, 16]]


def test_reconstruction_is_kept(engines, fixture, per_case):
    eng = engines[0]
    sel = _property_cases(fixture)
    assert len(sel) == 7
    for k, keys, vals, wts in sel:
        n = int(fixture[f"c{k}_n"]) or int(np.lcm.reduce(keys))
        before = eng.tile_sum(wts[None, :], n, keys, vals)[0]
        after = eng.tile_sum(per_case[k][0][None, :], n, keys, keys)[0]
        assert _rel(after, before) <= TOL_SAME, (k, keys)


def test_idempotent(engines, fixture, per_case):
    for k, keys, vals, wts in _property_cases(fixture):
        once = per_case[k][0]
        twice, st = engines[0].qo_get_periods(*_pack([(keys, keys, once)]))
        assert st[0] == 0 and _rel(twice[0], once) <= TOL_SAME, (k, keys)


def test_permuting_the_dictionary_permutes_the_output(engines, fixture, per_case):
    for k, keys, vals, wts in _property_cases(fixture):
        order = list(np.random.default_rng(k).permutation(len(keys)))
        if order == sorted(order):
            order = order[::-1]
        blocks = np.split(wts, np.cumsum(vals)[:-1])
        segs = np.split(per_case[k][0], np.cumsum(keys)[:-1])
        got, st = engines[0].qo_get_periods(*_pack([([keys[a] for a in order], [vals[a] for a in order],
                                                      np.concatenate([blocks[a] for a in order]))]))
        assert st[0] == 0 and _rel(got[0], np.concatenate([segs[a] for a in order])) <= TOL_SAME, (k, keys, order)


def test_status_words(engines):
    from pyperiod_amd import _ffi

    rng = np.random.default_rng(5)
    good = ([12, 18], [12, 12], rng.standard_normal(24))
    want_good = closed_form(*good)
    for eng in engines:
        per, rws, cnt, wts = _pack([good, good, good, good, good, good])
        cnt[1] = 0  # K = 0
        per[2] = [12, 12]  # a repeated period
        rws[3] = [13, 12]  # rows > period
        per[4] = [0, 18]  # a period of 0
        rws[4] = [0, 12]
        out, st = eng.qo_get_periods(per, rws, cnt, wts, max_period=18, ccap=30)
        assert st.tolist() == [_ffi.PH_ST_OK, _ffi.PH_ST_NO_PERIOD, _ffi.PH_ST_ITER_CAP, _ffi.PH_ST_ITER_CAP, _ffi.PH_ST_ITER_CAP,
                               _ffi.PH_ST_OK]
        assert not out[1:5].any()
        for w in (0, 5):  # the rows around them are untouched
            assert _rel(out[w], want_good) <= TOL_REF
        per, rws, cnt, wts = _pack([good, ([5, 7], [5, 6], rng.standard_normal(11))])
        out, st = eng.qo_get_periods(per, rws, cnt, wts, max_period=18, ccap=29)  # one short of sum(p) = 30
        assert st.tolist() == [_ffi.PH_ST_CAP, _ffi.PH_ST_OK] and not out[0].any() and out[1, :12].any()
        out, st = eng.qo_get_periods(per, rws, cnt, np.ascontiguousarray(wts[:, :23]), max_period=18, ccap=30)  # sum(rows) = 24
        assert st.tolist() == [_ffi.PH_ST_CAP, _ffi.PH_ST_OK] and not out[0].any() and out[1, :12].any()
        per[1, 0] = 19  # beyond max_period
        out, st = eng.qo_get_periods(per, rws, cnt, wts, max_period=18, ccap=30)
        assert st.tolist() == [_ffi.PH_ST_OK, _ffi.PH_ST_ITER_CAP] and not out[1].any()


def test_placement_switch(engines):
    """Dictionaries {2m: 2m, 3m: 2m} (gcd m): the largest m whose work arrays fit the LDS, found by bisection on the plan,
    and the next one."""
    from pyperiod_amd import _ffi

    eng = engines[0]

    def in_lds(m):
        return eng.plan_info("qo_get_periods", 5 * m, (5 * m, 3 * m))[0].window == _ffi.PH_PLAN_LDS

    lo, hi = 1, 1 << 16
    assert in_lds(lo) and not in_lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_lds(mid) else (lo, mid)
    assert eng.plan_info("qo_get_periods", 5 * lo, (5 * lo, 3 * lo))[0].lds_bytes <= eng.lds_bytes
    print("placement switch: sum(p) =", 5 * lo, "in LDS,", 5 * hi, "in HBM")
    for m in (lo, hi):
        keys, vals = [2 * m, 3 * m], [2 * m, 2 * m]
        wts = np.random.default_rng(m).standard_normal(sum(vals))
        got, st = eng.qo_get_periods(*_pack([(keys, vals, wts)]))
        assert st[0] == 0 and got.shape == (1, 5 * m)
        assert _rel(got[0], closed_form(keys, vals, wts)) <= TOL_REF, m


def test_device_tensors_give_the_host_bits(engines, fixture):
    torch = pytest.importorskip("torch")
    packed = _pack([(keys, vals, wts) for _, keys, vals, wts in cases(fixture)])
    for eng in engines:
        host, hst = eng.qo_get_periods(*packed)
        dev, dst = eng.qo_get_periods(*(torch.as_tensor(a, device="cuda") for a in packed))
        torch.cuda.synchronize()
        assert dev.is_cuda and dst.is_cuda and dev.dtype == torch.float64 and dst.dtype == torch.int32
        assert _same_bits(dev.cpu().numpy(), host) and np.array_equal(dst.cpu().numpy(), hst)
        # capacities given: no word is read back
        dev2, _ = eng.qo_get_periods(*(torch.as_tensor(a, device="cuda") for a in packed), max_period=100, ccap=host.shape[1])
        torch.cuda.synchronize()
        assert _same_bits(dev2.cpu().numpy(), host)


def _names(eng):
    return [name for name, _ in eng.profile_read()]


def test_class_after_batched_find_periods(engines, fixture):
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    ks = [k for k, *_ in cases(fixture) if fixture[f"c{k}_n"] == 600]
    assert [int(fixture[f"c{k}_seed"]) for k in ks] == list(range(6))
    x = np.stack([multi_sinusoid_window(s, 600) for s in range(6)])
    qo = QOPeriods()
    qo.find_periods(x, num=4, thresh=0.01, min_length=2, max_length=100)
    wlist = [b["weights"] for b in qo.output_bases]
    dlist = [b["basis_dictionary"] for b in qo.output_bases]
    eng.profile(True)
    try:
        got = qo.get_periods(wlist, dlist)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_extract"]
    assert isinstance(got, list) and len(got) == 6
    for w, k in enumerate(ks):
        keys = [int(q) for q in dlist[w]]
        assert keys == fixture[f"c{k}_keys"].tolist() and list(dlist[w].values()) == fixture[f"c{k}_vals"].tolist(), (w, dlist[w])
        assert isinstance(got[w], tuple) and [len(a) for a in got[w]] == keys
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in got[w])
        one = qo.get_periods(wlist[w], dlist[w])
        assert isinstance(one, tuple) and all(_same_bits(a, b) for a, b in zip(one, got[w]))
        flat = np.concatenate(got[w])
        assert _rel(flat, closed_form(keys, list(dlist[w].values()), wlist[w])) <= TOL_REF
        err = _rel(flat, fixture[f"c{k}_lstsq"])
        print(f"row {w}: class vs fixture {err:.2e}")
        assert err <= TOL_SOLVE, (w, err)


def test_class_after_ramanujan_fit(engines):
    from pyperiod_amd import RamanujanPeriods

    eng = engines[0]
    ram = RamanujanPeriods()
    out, _ = ram.find_periods_with_weights(multi_sinusoid_window(2, 240), 2, 40)
    d, wts = out["basis_dictionary"], out["weights"]
    assert len(d) >= 1
    eng.profile(True)
    try:
        got = ram.get_periods([wts], [d])
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_extract"] and isinstance(got, list) and len(got) == 1
    one = ram.get_periods(wts, d)
    keys = [int(q) for q in d]
    assert isinstance(one, tuple) and [len(a) for a in one] == keys and all(a.dtype == np.float64 for a in one)
    assert all(_same_bits(a, b) for a, b in zip(one, got[0]))
    assert _rel(np.concatenate(one), closed_form(keys, list(d.values()), wts)) <= TOL_REF
