"""The windowed QOPeriods.find_periods batches on the MI355X: the fixed-weight loop under an analysis window in one
launch per batch (ph_qo_greedy_win, k_qo_greedy_win) and orthogonal selection with weights re-solved under a window
(k_qo_orth_select + k_qo_fit_win per round), against the reference fixture tests/golden/qo_window_keep.npz, the numpy
restatement of tests/test_qo_window_keep_cpu.py and the 1-D calls.  Engines: the default one and one created under
PH_HBM_WINDOW=1 (the residual in the HBM workspace).

Bars: lists, keeps, counts and statuses exact; 1e-10 on norms, weights and residual of the fixed-weight loop against the
fixture, the restatement and the 1-D calls (the bar of tests/test_gpu_qo_batch.py); 1e-8 on weights and residual of the
re-solved O groups (the solver bar of tests/test_gpu_qo_window.py); 1e-12 between two runs of the same arithmetic in
another order; 1e-4 for float32 input."""

import ctypes
import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window
from test_qo_batch_cpu import keep_quirk_rows
from test_qo_window_keep_cpu import K_GROUPS, ROWS, k_group_kw, np_find_periods_keep_win, o_group_kw

pytestmark = pytest.mark.gpu
TOL, TOL_SOLVE, TOL32, TOL_SAME = 1e-10, 1e-8, 1e-4, 1e-12


@pytest.fixture(scope="module")
def engines():
    """(default engine, engine whose residual always lives in HBM); PH_HBM_WINDOW is read when the context is created
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


def _greedy(eng, x, win, kw, trunc=False, kcap=None):
    kcap = kw["num"] * kw["max_length"] if kcap is None else kcap
    return eng.qo_find_periods(x, kw["num"], kw["thresh"], kw["min_length"], kw["max_length"], kcap, trunc=trunc,
                               update_weights=False, window=win)


def _blocks(got, w):
    per, _, keeps, counts = got[:4]
    return [(int(per[w, b]), int(keeps[w, b])) for b in range(int(counts[w, 1]))]


def _check_row(got, w, want, want_res, tol, what):
    """Row w of an engine result against dict(periods, norms, weights, blocks) and a residual."""
    per, nrm, keeps, counts, wts, resid, st = got
    n_report, blocks = int(counts[w, 0]), _blocks(got, w)
    rows = sum(k if k else p for p, k in blocks)
    en, ew, er = rel_err(nrm[w, :n_report], want["norms"]), rel_err(wts[w, :rows], want["weights"]), rel_err(resid[w], want_res)
    print(f"{what} row {w}: status {st[w]} blocks {blocks} norms {en:.2e} weights {ew:.2e} residual {er:.2e}")
    assert st[w] == 0, (what, w)
    assert blocks == [tuple(b) for b in want["blocks"]], (what, w)
    assert list(per[w, :n_report]) == list(want["periods"]) and n_report == len(want["periods"]), (what, w)
    assert not per[w, len(blocks):].any() and not keeps[w, len(blocks):].any() and not nrm[w, len(blocks):].any(), (what, w)
    assert rows == np.asarray(want["weights"]).size and not wts[w, rows:].any(), (what, w)
    assert en <= tol and ew <= tol and er <= tol, (what, w)


_RESTATED = {}


def _restated(x, win, kw, trunc):
    """np_find_periods_keep_win of one row, computed once for both engines."""
    key = (x.tobytes(), win.tobytes(), tuple(sorted(kw.items())), trunc)
    if key not in _RESTATED:
        _RESTATED[key] = np_find_periods_keep_win(x, win, trunc=trunc, **kw)
    return _RESTATED[key]


def _check_restatement(got, x, win, kw, trunc, tol, what):
    for w in range(x.shape[0]):
        want, res = _restated(x[w], win, kw, trunc)
        _check_row(got, w, want, res, tol, what)


def _same(a, b, tol):
    """Two engine results: lists exact, values within tol."""
    for k in (0, 2, 3, 6):
        assert np.array_equal(a[k], b[k]), k
    for k in (1, 4, 5):
        assert rel_err(a[k], b[k]) <= tol, (k, rel_err(a[k], b[k]))


# ---------------------------------------------------------------------------- 1. the reference fixture
@pytest.mark.parametrize("tag", K_GROUPS)
def test_engine_against_reference_fixture(engines, golden, tag):
    g = golden("qo_window_keep")
    n, win, kw, trunc = k_group_kw(g, tag)
    x = np.stack([multi_sinusoid_window(int(g[f"{tag}{w}_seed"]), n) for w in range(ROWS)])
    for name, eng in zip(("lds", "hbm"), engines):
        got = _greedy(eng, x, win, kw, trunc)
        assert not got[6].any()  # no row is handed back
        for w in range(ROWS):
            want = {k: g[f"{tag}{w}_{k}"] for k in ("periods", "norms", "weights")}
            want["blocks"] = g[f"{tag}{w}_blocks"].tolist()
            _check_row(got, w, want, g[f"{tag}{w}_residual"], TOL, f"{tag} residual in {name}")


# ---------------------------------------------------------------------------- 2. ones window, 3. scaled window
@pytest.mark.parametrize("n", [600, 1024])
def test_ones_window_is_the_unwindowed_loop(engines, n):
    kw = dict(num=4, thresh=0.05, min_length=2, max_length=n // 6)
    x = np.stack([multi_sinusoid_window(40 + w, n) for w in range(5)])
    for trunc in (False, True):
        plain = engines[0].qo_find_periods(x, 4, 0.05, 2, n // 6, 4 * (n // 6), trunc=trunc, update_weights=False)
        assert not plain[6].any()
        for eng in engines:
            _same(_greedy(eng, x, np.ones(n), kw, trunc), plain, TOL_SAME)


def test_scaled_window_gives_the_same_fit(engines):
    n, kw = 600, dict(num=4, thresh=0.05, min_length=2, max_length=100)
    x = np.stack([multi_sinusoid_window(50 + w, n) for w in range(4)])
    for eng in engines:
        one = _greedy(eng, x, np.hanning(n), kw)
        assert not one[6].any()
        _same(_greedy(eng, x, 3.0 * np.hanning(n), kw), one, TOL_SAME)


# ---------------------------------------------------------------------------- 4. fold paths, 5. quirk rows
def _rows_p23(n):
    """Periods 2 and 3 over a little noise: with max_length = 3 every class holds >= 256 samples at n = 1024."""
    out = []
    for s in range(3):
        r = np.random.default_rng(20 + s)
        out.append(np.tile(r.standard_normal(2), n // 2 + 1)[:n] + 0.7 * np.tile(r.standard_normal(3), n // 3 + 1)[:n]
                   + 0.05 * r.standard_normal(n))
    return np.stack(out)


@pytest.mark.parametrize("trunc", [False, True])
def test_fold_paths(engines, trunc):
    """N = 1024, periods 2 .. 3: one wavefront per residue (>= 4 * 64 samples per class; the third round repeats a
    period, keep == 0).  N = 1023, periods up to 341: one thread per residue, a short last row, p does not divide N."""
    for n, x, hi in ((1024, _rows_p23(1024), 3), (1023, np.stack([multi_sinusoid_window(s, 1023) for s in range(3)]), 341)):
        kw = dict(num=3, thresh=0.05, min_length=2, max_length=hi)
        win = np.hanning(n)
        for name, eng in zip(("lds", "hbm"), engines):
            _check_restatement(_greedy(eng, x, win, kw, trunc), x, win, kw, trunc, TOL, f"N={n} trunc={trunc} {name}")


def test_keep_quirk_rows_under_a_window(engines):
    x = keep_quirk_rows(900)
    kw = dict(num=5, thresh=0.1, min_length=2, max_length=300)
    win = np.hanning(900)
    for name, eng in zip(("lds", "hbm"), engines):
        got = _greedy(eng, x, win, kw)
        _check_restatement(got, x, win, kw, False, TOL, f"quirk rows {name}")
        a, b = _blocks(got, 0), _blocks(got, 1)
        assert a[:4] == [(30, 30), (12, 6), (2, 0), (12, 0)]  # keep == 0: all 2, all 12 rows are fitted
        assert b == [(40, 40), (37, 36), (37, 36)] and int(got[3][1, 0]) == 1  # stopped: 37's block re-fitted, appended
        assert np.count_nonzero(got[4][0]) >= 30 + 6 + 2 + 12


# ---------------------------------------------------------------------------- 6. status
def _periodic_rows():
    """(7-periodic row, 7- plus 14-periodic row) of 70 samples; the second picks 7 and then 14, whose block keeps 7 of
    its 14 rows (the 14-periodic part changes sign after 7 samples and has equal even and odd sums)."""
    base = np.tile(np.array([3.0, -1.0, 2.0, 0.5, -2.5, 1.0, 4.0]), 10)
    x7 = base + 0.01 * np.random.default_rng(5).standard_normal(70)
    v = np.array([2.0, 1, -1, -2, 1, 1, -2])
    x14 = base + 0.5 * np.tile(np.concatenate([v, -v]), 5) + 0.01 * np.random.default_rng(6).standard_normal(70)
    return x7, x14


def test_status_codes(engines):
    from pyperiod_amd import _ffi

    x7, x14 = _periodic_rows()
    ok_win = np.hanning(70) + 0.1
    kw = dict(num=2, thresh=0.05, min_length=2, max_length=20)
    x = np.stack([x7, x14])
    for eng in engines:
        got = _greedy(eng, x, ok_win, kw)
        assert not got[6].any() and _blocks(got, 0)[0] == (7, 7) and _blocks(got, 1) == [(7, 7), (14, 7)]
        # zero on a whole class of the first period: no fit, nothing reported
        win = ok_win.copy()
        win[3::7] = 0.0
        per, nrm, keeps, counts, wts, resid, st = _greedy(eng, x, win, kw)
        assert np.all(st == _ffi.PH_ST_ITER_CAP) and not wts.any() and not counts.any() and not per.any()
        # zero on a fitted class of the second block only (class 3 of period 14; class 3 of period 7 keeps n = 10, 24, ...)
        win = ok_win.copy()
        win[3::14] = 0.0
        got = _greedy(eng, x, win, kw)
        assert got[6][1] == _ffi.PH_ST_ITER_CAP and _blocks(got, 1) == [(7, 7)] and not got[4][1, 7:].any()
        # zero on a class at or beyond `rows` of the keep < p block: that class is not fitted
        win = ok_win.copy()
        win[10::14] = 0.0
        got = _greedy(eng, x, win, kw)
        assert not got[6].any() and _blocks(got, 1) == [(7, 7), (14, 7)]
        _check_restatement(got, x, win, kw, False, TOL, "zero beyond rows")
        # capacity: 7 + 7 rows
        assert not _greedy(eng, x[1:], ok_win, kw, kcap=14)[6].any()
        per, nrm, keeps, counts, wts, resid, st = _greedy(eng, x[1:], ok_win, kw, kcap=13)
        assert st[0] == _ffi.PH_ST_CAP and list(per[0]) == [7, 0] and not wts[0, 7:].any()
        with pytest.raises(ValueError):
            _greedy(eng, x, np.ones(69), kw)
        with pytest.raises(ValueError):
            eng.qo_find_periods(x, 2, 0.05, 2, 20, 64, window=ok_win)  # re-solved weights: the host-stepped loop
        # PH_FLAG_ORTH is refused by the entry point itself
        out = [np.zeros(s, dtype=t) for s, t in (((2, 2), np.uint32), ((2, 2), np.float64), ((2, 2), np.int32), ((2, 2), np.int32),
                                                 ((2, 64), np.float64), ((2, 70), np.float64), ((2,), np.int32))]
        rc = eng._lib.ph_qo_greedy_win(eng._ctx, x.ctypes.data, _ffi.PH_F64, 2, 70, ok_win.ctypes.data, 2, 0.05, 2, 20, 64,
                                       _ffi.PH_FLAG_ORTH, *(ctypes.c_void_p(a.ctypes.data) for a in out))
        assert rc == _ffi.PH_E_UNSUPPORTED


# ---------------------------------------------------------------------------- 7. placements
def test_placements(engines):
    from pyperiod_amd import _ffi

    eng, hbm = engines
    n, kw = 600, dict(num=4, thresh=0.05, min_length=2, max_length=100)
    x = np.stack([multi_sinusoid_window(60 + w, n) for w in range(4)])
    assert eng.qo_plan_info(n, update_weights=False)[0] == _ffi.PH_QO_LDS_BEHIND
    assert hbm.qo_plan_info(n, update_weights=False)[0] == _ffi.PH_QO_HBM
    a, b = _greedy(eng, x, np.hanning(n), kw), _greedy(hbm, x, np.hanning(n), kw)
    assert not a[6].any()
    _same(a, b, TOL_SAME)

    def in_lds(m):
        return eng.qo_plan_info(m, update_weights=False, max_length=40)[0] == _ffi.PH_QO_LDS_BEHIND

    lo, hi = 1, 1 << 20
    assert in_lds(lo) and not in_lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_lds(mid) else (lo, mid)
    kw = dict(num=2, thresh=0.05, min_length=2, max_length=40)
    for m in (lo, lo + 1):
        assert in_lds(m) == (m == lo)
        x = np.stack([multi_sinusoid_window(70 + w, m) for w in range(2)])
        win = np.hanning(m)
        got = _greedy(eng, x, win, kw)
        _check_restatement(got, x, win, kw, False, TOL, f"N={m} ({'LDS' if m == lo else 'HBM'})")
        _same(got, _greedy(hbm, x, win, kw), TOL_SAME)


# ---------------------------------------------------------------------------- 8. float32, device tensors
def test_float32_against_the_upcast_rows(engines, golden):
    g = golden("qo_window_keep")
    n, win, kw, trunc = k_group_kw(g, "KB")
    x32 = np.stack([multi_sinusoid_window(int(g[f"KB{w}_seed"]), n) for w in range(ROWS)]).astype(np.float32)
    for eng in engines:
        a = _greedy(eng, x32, win, kw)
        b = _greedy(eng, x32.astype(np.float64), win, kw)
        assert a[5].dtype == np.float32 and not a[6].any()
        _same(a, b, TOL32)


def test_device_tensors_give_the_same_bits(engines):
    import torch

    n, kw = 600, dict(num=4, thresh=0.05, min_length=2, max_length=100)
    x = np.stack([multi_sinusoid_window(80 + w, n) for w in range(4)])
    win = np.hanning(n)
    for eng in engines:
        for dt in (np.float64, np.float32):
            host = _greedy(eng, x.astype(dt), win, kw)
            dev = _greedy(eng, torch.as_tensor(x.astype(dt), device="cuda"), torch.as_tensor(win, device="cuda"), kw)
            torch.cuda.synchronize()
            assert all(d.is_cuda for d in dev)
            dev = [d.cpu().numpy() for d in dev]
            assert np.array_equal(dev[0].view(np.uint32), host[0])
            for k in range(1, 7):
                assert np.array_equal(dev[k], host[k]), k


# ---------------------------------------------------------------------------- 9. the class, fixed weights
def _names(eng):
    return [name for name, _ in eng.profile_read()]


def _same_result(got, want, tol):
    (gb, gr), (wb, wr) = got, want
    assert set(gb.keys()) == set(wb.keys())
    assert np.array_equal(gb["periods"], wb["periods"]) and np.asarray(gb["periods"]).dtype == np.asarray(wb["periods"]).dtype
    assert gb["basis_dictionary"] == wb["basis_dictionary"]
    assert rel_err(gb["norms"], wb["norms"]) <= tol
    assert np.shape(gb["weights"]) == np.shape(wb["weights"]) and rel_err(gb["weights"], wb["weights"]) <= tol
    assert gr.dtype == np.float64 and gr.shape == wr.shape and rel_err(gr, wr) <= tol
    assert np.array_equal(gb["subspaces"], wb["subspaces"])  # built on read


def test_class_fixed_weights_under_a_window(engines, golden):
    """find_periods(x(W, N), update_weights=False) with ``window`` set: one k_qo_greedy_win launch, row by row what the
    1-D call returns.

    The 16-row batch (14 signals, an all-zero row, the 7-periodic row of test_status_codes tiled to N = 600) runs under
    np.hanning(600) set to zero on n = 3 (mod 7): np.hanning(600) itself is positive on 1 .. 598, so under it no
    residue class of a period <= 100 has a zero sum and no row could come back PH_ST_ITER_CAP.  The 14 signals are
    seeds whose runs pick no multiple of 7 (a class of such a period can lie inside the zeroed samples)."""
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    g = golden("qo_window_keep")
    n = 600
    kw = dict(num=4, thresh=0.05, min_length=2, max_length=100)
    qo = QOPeriods()
    qo.window = np.hanning(n)
    # rows that all stay on the device: exactly one launch
    seeds = [int(g[f"KB{w}_seed"]) for w in range(ROWS)]
    x = np.stack([multi_sinusoid_window(s, n) for s in seeds])
    eng.profile(True)
    try:
        batch = qo.find_periods(x, update_weights=False, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_greedy_win"], names
    assert len(batch) == ROWS and qo.output_bases == [b for b, _ in batch]
    for w in range(ROWS):
        assert dict.__getitem__(batch[w][0], "subspaces") is None  # a device row: built on read
        _same_result(batch[w], qo.find_periods(x[w], update_weights=False, **kw), TOL)
        want = {k: g[f"KB{w}_{k}"] for k in ("periods", "norms", "weights", "residual")}
        assert np.array_equal(batch[w][0]["periods"], want["periods"])
        assert rel_err(batch[w][0]["norms"], want["norms"]) <= TOL and rel_err(batch[w][0]["weights"], want["weights"]) <= TOL
        assert rel_err(batch[w][1], want["residual"]) <= TOL
    # KE: rows the test function stops report one period fewer and keep the re-fitted block's weights
    _, _, kwe, _ = k_group_kw(g, "KE")
    xe = np.stack([multi_sinusoid_window(int(g[f"KE{w}_seed"]), n) for w in range(ROWS)])
    batch = qo.find_periods(xe, update_weights=False, **kwe)
    stopped = 0
    for w in range(ROWS):
        blocks = g[f"KE{w}_blocks"].tolist()
        bases, res = batch[w]
        _same_result(batch[w], qo.find_periods(xe[w], update_weights=False, **kwe), TOL)
        assert rel_err(bases["weights"], g[f"KE{w}_weights"]) <= TOL and rel_err(res, g[f"KE{w}_residual"]) <= TOL
        assert bases["weights"].size == sum(k if k else p for p, k in blocks)
        if len(bases["periods"]) < len(blocks):
            stopped += 1
            assert len(bases["periods"]) == len(blocks) - 2 and blocks[-1] == blocks[-2]
            assert np.count_nonzero(bases["weights"][-(blocks[-1][1] or blocks[-1][0]):]) > 0
    assert 0 < stopped < ROWS
    # the mixed batch: the device hands back exactly the all-zero row and the row with a class of zero window sum
    win = np.hanning(n)
    win[3::7] = 0.0
    qo.window = win
    signals = [multi_sinusoid_window(s, n) for s in (2, 3, 4, 5, 8, 11, 13, 14, 15, 16, 17, 18, 19, 21)]
    x7 = np.tile(np.array([3.0, -1.0, 2.0, 0.5, -2.5, 1.0, 4.0]), n // 7 + 1)[:n] + 0.01 * np.random.default_rng(5).standard_normal(n)
    x = np.stack(signals + [np.zeros(n), x7])
    dev = qo._find_periods_device_batch(eng, x, kw["num"], kw["thresh"], kw["min_length"], kw["max_length"], False, window=win)
    assert [r is None for r in dev] == [False] * 14 + [True, True]
    batch = qo.find_periods(x, update_weights=False, **kw)
    for w in range(16):
        one = qo.find_periods(x[w], update_weights=False, **kw)
        if w < 14:
            _same_result(batch[w], one, TOL)
        else:  # the 1-D call itself ran on the row
            assert list(batch[w][0]["periods"]) == list(one[0]["periods"]) and batch[w][0]["basis_dictionary"] == one[0]["basis_dictionary"]
            assert np.array_equal(batch[w][1], one[1])
    assert list(batch[14][0]["periods"]) == [1] and not batch[14][1].any()  # all zero: the reference's fixed answer
    assert len(batch[15][0]["periods"]) == 0 and np.array_equal(batch[15][1], x[15])  # singular first fit: nothing found
    # a window the device refuses (wrong length) keeps the row-by-row path
    qo.window = np.hanning(n - 1)
    eng.profile(True)
    try:
        with pytest.raises(ValueError):
            qo.find_periods(x[:2], update_weights=False, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert "k_qo_greedy_win" not in names


# ---------------------------------------------------------------------------- 10. the class, orthogonal selection
@pytest.mark.parametrize("tag", ["OB", "OC", "OE"])
def test_class_orthogonal_selection_under_a_window(engines, golden, tag):
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    g = golden("qo_window_keep")
    n, win, num, thresh, max_length, trunc = o_group_kw(g, tag)
    kw = dict(num=num, thresh=thresh, min_length=2, max_length=max_length)
    x = np.stack([multi_sinusoid_window(int(g[f"{tag}{w}_seed"]), n) for w in range(ROWS)])
    qo = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True)
    qo.window = win
    eng.profile(True)
    try:
        batch = qo.find_periods(x, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_orth_select", "k_qo_fit_win"] * 4, names
    assert len(batch) == ROWS and qo.output_bases == [b for b, _ in batch]
    for w in range(ROWS):
        bases, res = batch[w]
        want = {k: g[f"{tag}{w}_{k}"] for k in ("periods", "norms", "weights", "dict_keys", "dict_vals", "residual")}
        assert np.array_equal(bases["periods"], want["periods"]) and len(bases["periods"]) == want["periods"].size
        assert [int(q) for q in bases["basis_dictionary"]] == list(want["dict_keys"])
        assert list(bases["basis_dictionary"].values()) == list(want["dict_vals"])
        assert np.array_equal(bases["subspaces"], po.qo_get_subspaces(list(want["dict_keys"]), n)[0])
        ew, er, en = rel_err(bases["weights"], want["weights"]), rel_err(res, want["residual"]), rel_err(bases["norms"], want["norms"])
        print(f"{tag}{w}: periods {list(bases['periods'])} weights {ew:.2e} residual {er:.2e} norms {en:.2e}")
        assert en <= TOL and ew <= TOL_SOLVE and er <= TOL_SOLVE
        gb, gr = batch[w]
        wb, wr = qo.find_periods(x[w], **kw)
        assert set(gb.keys()) == set(wb.keys())
        assert np.array_equal(gb["periods"], wb["periods"]) and gb["basis_dictionary"] == wb["basis_dictionary"], w
        assert np.asarray(gb["periods"]).dtype == np.asarray(wb["periods"]).dtype
        assert rel_err(gb["norms"], wb["norms"]) <= TOL_SAME, w
        assert rel_err(gb["weights"], wb["weights"]) <= TOL_SOLVE and rel_err(gr, wr) <= TOL_SOLVE, w
        assert gr.dtype == np.float64 and np.array_equal(gb["subspaces"], wb["subspaces"])
    if tag == "OE":  # the mixed-fate batch
        short = [len(b["periods"]) < len(b["basis_dictionary"]) for b, _ in batch]
        assert any(short) and not all(short)
    if tag == "OB":  # without a window the launches are what they were (group B of qo_orth.npz: four rounds, no row back)
        go = golden("qo_orth")
        xb = np.stack([multi_sinusoid_window(int(go[f"B{w}_seed"]), n) for w in range(8)])
        qo.window = False
        eng.profile(True)
        try:
            qo.find_periods(xb, **kw)
            names = _names(eng)
        finally:
            eng.profile(False)
        assert names == ["k_qo_orth_select", "k_qo_fit"] * 4, names
