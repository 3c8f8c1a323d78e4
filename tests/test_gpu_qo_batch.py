"""QOPeriods.find_periods over a (W, N) batch on the MI355X: the default, fixed-weight (update_weights=False) and
trunc variants in one launch per batch (k_qo_find / k_qo_greedy), against the 1-D calls, the host-driven loop, the
reference's trunc fixture and the numpy restatement of tests/test_qo_batch_cpu.py."""

import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch
from test_qo_batch_cpu import keep_quirk_rows, np_find_periods

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _rows_900():
    """multi_sinusoid_batch(70, 6, 900) plus an all-zero row and a white-noise row that stops after its first period."""
    x = multi_sinusoid_batch(70, 6, 900)
    noise = 0.5 * np.random.default_rng(3).standard_normal(900)
    return np.vstack([x, np.zeros((1, 900)), noise[None, :]])


def _host(trunc, x, **kw):
    """The 1-D class call: for trunc / update_weights=False that is the host-driven loop."""
    from pyperiod_amd import QOPeriods

    return QOPeriods(trunc_to_integer_multiple=trunc).find_periods(x, **kw)


def _same_result(got, want, tol, exact_norms=False):
    (gb, gr), (wb, wr) = got, want
    assert set(gb.keys()) == set(wb.keys())
    assert np.array_equal(gb["periods"], wb["periods"]) and gb["periods"].dtype == wb["periods"].dtype
    assert gb["basis_dictionary"] == wb["basis_dictionary"]
    if exact_norms:
        assert np.array_equal(gb["norms"], wb["norms"])
    else:
        assert rel_err(gb["norms"], wb["norms"]) <= tol
    assert gb["weights"].shape == wb["weights"].shape and rel_err(gb["weights"], wb["weights"]) <= tol
    assert gr.dtype == np.float64 and gr.shape == wr.shape and rel_err(gr, wr) <= tol
    assert np.array_equal(gb["subspaces"], wb["subspaces"])  # built on read


def test_batch_equals_rows_fp64(eng):
    from pyperiod_amd import QOPeriods

    x = _rows_900()
    kw = dict(num=5, thresh=0.2, min_length=2, max_length=300)
    qo = QOPeriods()
    out = qo.find_periods(x, **kw)
    assert isinstance(out, list) and len(out) == x.shape[0]
    assert qo.output_bases == [b for b, _ in out]
    for w in range(x.shape[0]):
        _same_result(out[w], QOPeriods().find_periods(x[w], **kw), 1e-12, exact_norms=True)
    assert list(out[6][0]["periods"]) == [1]  # the all-zero row: the reference's fixed answer
    assert len(out[7][0]["periods"]) == 0 and len(out[7][0]["basis_dictionary"]) == 1  # stopped after one period
    # a dictionary beyond the device's capacity (the 16384-sample three-period signal): the row falls back
    t = np.arange(16384, dtype=np.float64)
    sig = np.sin(2 * np.pi * t / 299.0) + 0.8 * np.sin(2 * np.pi * t / 293.0 + 1.0) + 0.6 * np.sin(2 * np.pi * t / 283.0 + 2.0)
    sig = sig + 0.01 * np.random.default_rng(5).standard_normal(t.size)
    xb = np.vstack([sig, multi_sinusoid_batch(71, 1, 16384)[0]])
    kw = dict(num=3, thresh=0.01, min_length=200, max_length=300)
    out = QOPeriods().find_periods(xb, **kw)
    assert sum(out[0][0]["basis_dictionary"].values()) > 512
    for w in range(2):
        _same_result(out[w], QOPeriods().find_periods(xb[w], **kw), 1e-12, exact_norms=True)


def test_subspaces_are_built_on_read(eng):
    from pyperiod_amd import QOPeriods

    x = multi_sinusoid_batch(72, 2, 700)
    out = QOPeriods().find_periods(x, num=3, thresh=0.1)
    b = out[0][0]
    assert dict.__getitem__(b, "subspaces") is None  # not materialised by the call
    one = QOPeriods().find_periods(x[0], num=3, thresh=0.1)[0]
    assert np.array_equal(dict(b)["subspaces"], one["subspaces"]) and np.array_equal(b["subspaces"], one["subspaces"])


@pytest.mark.parametrize("trunc", [False, True])
def test_fixed_weights_batch(eng, trunc):
    """update_weights=False on rows built for the keep == 0 quirk (keep_quirk_rows: a period dividing an earlier one,
    a repeated period, a row stopped by the test whose last block is re-fitted) and on multi-sinusoid rows, against the
    host-driven loop and the numpy restatement."""
    x = np.vstack([keep_quirk_rows(900), multi_sinusoid_batch(70, 6, 900)])
    kw = dict(num=5, thresh=0.1, min_length=2, max_length=300, update_weights=False)
    out = _host(trunc, x, **kw)
    per, nrm, keeps, counts, wts, resid, st = eng.qo_find_periods(x, 5, 0.1, 2, 300, 1600, trunc=trunc, update_weights=False)
    assert not st.any()
    blocks_of = []
    for w in range(x.shape[0]):
        host = _host(trunc, x[w], **kw)
        want, wres = np_find_periods(x[w], 5, 0.1, 2, 300, trunc=trunc, update_weights=False)
        nb = int(counts[w, 1])
        blocks = [(int(per[w, b]), int(keeps[w, b])) for b in range(nb)]
        blocks_of.append(blocks)
        assert blocks == want["blocks"], w
        assert int(counts[w, 0]) == len(want["periods"])
        for ref, rres in ((host[0], host[1]), (want, wres)):
            got = out[w][0]
            assert np.array_equal(got["periods"], ref["periods"]) and got["basis_dictionary"] == ref["basis_dictionary"]
            assert rel_err(got["norms"], ref["norms"]) <= 1e-10
            assert rel_err(got["weights"], ref["weights"]) <= 1e-10 and rel_err(out[w][1], rres) <= 1e-10
            assert got["subspaces"].shape == ref["subspaces"].shape == (sum(k if k else q for q, k in blocks), 900)
            assert np.array_equal(got["subspaces"], ref["subspaces"])
    # the rows cover what they were built for
    a, b = blocks_of[0], blocks_of[1]
    assert (2, 0) in a and 30 in [q for q, _ in a[:2]]  # 2 divides the earlier 30: keep 0, both rows fitted
    assert a[:4] == [(30, 30), (12, 6), (2, 0), (12, 0)]  # 12 repeats: keep 0, all 12 rows fitted
    assert b == [(40, 40), (37, 36), (37, 36)] and int(counts[1, 0]) == 1  # stopped: 37's block re-fitted, appended


def test_trunc_batch_against_reference_fixture(eng, golden):
    from pyperiod_amd import QOPeriods

    g = golden("qoperiods_trunc")
    for tag in ("w5", "w9"):
        num, thresh, lo, hi = g[f"{tag}_kw"]
        x = g[f"{tag}_x"]
        kw = dict(num=int(num), thresh=thresh, min_length=int(lo), max_length=int(hi))
        (b, res), = QOPeriods(trunc_to_integer_multiple=True).find_periods(x[None, :], **kw)
        assert np.array_equal(b["periods"], g[f"{tag}_periods"]), tag
        assert [int(k) for k in b["basis_dictionary"]] == list(g[f"{tag}_dict_keys"])
        assert list(b["basis_dictionary"].values()) == list(g[f"{tag}_dict_vals"])
        assert rel_err(b["norms"], g[f"{tag}_norms"]) <= 1e-10
        assert rel_err(b["weights"], g[f"{tag}_weights"]) <= 1e-8 and rel_err(res, g[f"{tag}_residual"]) <= 1e-8
        _same_result((b, res), _host(True, x, **kw), 1e-8)


def test_trunc_sweep_agrees_with_ph_sweep(eng):
    """The selection of the trunc kernels: its first pick equals the argmax of ph_sweep(GAMMA, TRUNC), and the norm
    agrees to 1e-12."""
    from pyperiod_amd import _ffi

    x = multi_sinusoid_batch(73, 4, 1000)
    per, nrm, keeps, counts, wts, resid, st = eng.qo_find_periods(x, 1, 0.0, 2, 333, 512, trunc=True)
    pg, ng, kg, cg, wg, rg, sg = eng.qo_find_periods(x, 1, 0.0, 2, 333, 512, trunc=True, update_weights=False)
    sw = eng.sweep(x, 2, 333, _ffi.PH_SWEEP_NORM_GAMMA, True)
    for w in range(4):
        k = int(np.argmax(sw[w]))
        assert per[w, 0] == pg[w, 0] == 2 + k
        assert abs(nrm[w, 0] - sw[w, k]) <= 1e-12 * sw[w, k] and abs(ng[w, 0] - sw[w, k]) <= 1e-12 * sw[w, k]


@pytest.mark.parametrize("variant", ["keep", "trunc", "keep_trunc"])
def test_long_windows_hbm(eng, variant):
    """N = 32768 fp64: the windows do not fit the LDS (HBM-window instantiations)."""
    trunc = "trunc" in variant
    uw = "keep" not in variant
    x = multi_sinusoid_batch(74, 2, 32768)
    kw = dict(num=3, thresh=0.05, min_length=8, max_length=400, update_weights=uw)
    out = _host(trunc, x, **kw)
    for w in range(2):
        host = _host(trunc, x[w], **kw)
        got = out[w]
        assert np.array_equal(got[0]["periods"], host[0]["periods"]) and got[0]["basis_dictionary"] == host[0]["basis_dictionary"]
        assert rel_err(got[0]["norms"], host[0]["norms"]) <= 1e-10
        tol = 1e-8 if uw else 1e-10
        assert rel_err(got[0]["weights"], host[0]["weights"]) <= tol and rel_err(got[1], host[1]) <= tol


def test_config5_class_batch_fp32(eng):
    from pyperiod_amd import QOPeriods

    n, W = 16384, 1024
    xb = multi_sinusoid_batch(0, W, n, dtype=np.float32)
    out = QOPeriods().find_periods(xb, num=3, thresh=0.1, min_length=8, max_length=300)
    per, nrm, keeps, counts, wts, resid, st = eng.qo_find_periods(xb, 3, 0.1, 8, 300, 960)
    assert not st.any()
    for w in range(W):
        b, res = out[w]
        nrep, nb = counts[w]
        assert np.array_equal(b["periods"], per[w, :nrep])
        assert list(b["basis_dictionary"].values()) == list(keeps[w, :nb]) and len(b["basis_dictionary"]) == nb
        assert res.dtype == np.float64
    for w in (0, 1, 511, 1023):
        assert np.array_equal(out[w][1], resid[w].astype(np.float64))
        ref, rres = po.qo_find_periods(xb[w].astype(np.float64), 3, 0.1, 8, 300)
        b, res = out[w]
        assert np.array_equal(b["periods"], ref["periods"])
        assert rel_err(b["norms"], ref["norms"]) < 1e-4 and rel_err(b["weights"], ref["weights"]) < 1e-4
        assert rel_err(res, rres) < 1e-4


@pytest.mark.parametrize("trunc,uw", [(False, True), (True, True), (False, False), (True, False)])
def test_one_launch_per_batch(eng, trunc, uw):
    from pyperiod_amd import QOPeriods

    x = multi_sinusoid_batch(75, 16, 1200)
    eng.profile(True)
    try:
        QOPeriods(trunc_to_integer_multiple=trunc).find_periods(x, num=4, thresh=0.1, max_length=200, update_weights=uw)
        names = [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)
    assert [n for n in names if n.startswith("k_qo_")] == (["k_qo_find"] if uw else ["k_qo_greedy"])
    assert not [n for n in names if n in ("k_sweep", "k_fold_sums", "k_tile_sum") or n.startswith("k_sweep")]


def test_orth_flag_is_refused(eng):
    """PH_FLAG_ORTH: no device loop for the orthogonal selection -- PH_E_UNSUPPORTED from a real call."""
    import ctypes

    from pyperiod_amd import _ffi

    x = multi_sinusoid_batch(76, 1, 600)
    per, cnt = np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.int32)
    nrm, kp, wts = np.zeros((1, 2)), np.zeros((1, 2), np.int32), np.zeros((1, 512))
    res, st = np.zeros((1, 600)), np.zeros(1, np.int32)
    for extra in (0, _ffi.PH_FLAG_TRUNC, _ffi.PH_FLAG_KEEP_WEIGHTS):
        rc = eng._lib.ph_qo_find_periods(eng._ctx, x.ctypes.data, _ffi.PH_F64, 1, 600, 2, 0.1, 2, 200, 512,
                                         _ffi.PH_FLAG_ORTH | extra, per.ctypes.data, nrm.ctypes.data, kp.ctypes.data,
                                         cnt.ctypes.data, wts.ctypes.data, res.ctypes.data, st.ctypes.data)
        assert rc == _ffi.PH_E_UNSUPPORTED
    ctypes.c_int(0)  # (the context stays usable)
    assert eng.qo_find_periods(x, 2, 0.1, 2, 200, 512, update_weights=False)[6][0] == 0


def test_fixed_weights_large_max_length(eng):
    """The fixed-weight kernel keeps only the window in LDS: N = 65536 with the default max_length = N / 3 = 21845
    (a divisor bitset and block weights that would not fit the LDS) runs on the device, and every row equals its
    1-D call (the host-driven loop)."""
    from pyperiod_amd import QOPeriods

    n = 65536
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(77)
    x = np.vstack([np.sin(2 * np.pi * t / p1 + ph) + 0.7 * np.sin(2 * np.pi * t / p2) + 0.05 * rng.standard_normal(n)
                   for p1, p2, ph in ((37.0, 101.0, 0.3), (64.0, 45.0, 1.1))])
    assert eng.qo_feasible(n, np.float64, 1 << 16, None, update_weights=False)
    per, nrm, keeps, counts, wts, resid, st = eng.qo_find_periods(x, 2, 0.1, 2, None, 4096, update_weights=False)
    assert not st.any() and counts[:, 1].min() >= 1 and per.max() < 1000
    out = QOPeriods().find_periods(x, num=2, thresh=0.1, update_weights=False)
    for w in range(2):
        b, r = out[w]
        assert np.array_equal(b["periods"], per[w, : counts[w, 0]])
        hb, hr = QOPeriods().find_periods(x[w], num=2, thresh=0.1, update_weights=False)
        assert np.array_equal(b["periods"], hb["periods"]) and b["basis_dictionary"] == hb["basis_dictionary"]
        assert rel_err(b["norms"], hb["norms"]) <= 1e-10
        assert rel_err(b["weights"], hb["weights"]) <= 1e-10 and rel_err(r, hr) <= 1e-10
