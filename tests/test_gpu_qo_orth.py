"""QOPeriods.find_periods over a (W, N) batch under orthogonal (Muresan-Parks) selection on the MI355X: the selection
kernel k_qo_orth_select (ph_qo_orth_select) against the three calls it replaces (ph_orth_powers, ph_project_batch with
PH_FLAG_ORTH, ph_periodic_norm), both placements of its window, float32 input and device tensors; and the class surface
against the reference fixture tests/golden/qo_orth.npz, against the 1-D calls, and by the kernels it launches.

Bars: powers bit-equal to ph_orth_powers in the same placement (shared device function); 1e-12 between two runs of the
same arithmetic in another order (the norm's reduction, the two placements); against the reference fixture 1e-10 on powers
and norms and 1e-8 on weights and residual (the bar tests/test_gpu_qo_window.py holds the same solver to on its fixture);
batch against 1-D calls 1e-12 on norms and 1e-8 on weights and residual (device solve against host solve,
tests/test_gpu_qo_batch.py)."""

import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

pytestmark = pytest.mark.gpu
TOL_REF, TOL_SOLVE, TOL_SAME = 1e-10, 1e-8, 1e-12
GROUPS = "ABCDE"


@pytest.fixture(scope="module")
def engines():
    """(default engine, engine whose windows and work arrays always live in HBM); PH_HBM_WINDOW is read when the context
    is created and restored right after."""
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


def _rows(n):
    """0, 1: sinusoids of period 12 and 30 (composite winners: non-empty orth lists); 2, 3: zero-mean patterns of period 7
    and 13 (prime winners); 4: DC only (winner 1); 5: all zero (winner 1, norm 0); 6: a three-sinusoid window; 7: a NaN
    sample (its powers clip to zero, its norm is NaN: handed back)."""
    rng = np.random.default_rng(7)
    t = np.arange(n)
    out = [np.sin(2 * np.pi * t / 12 + 0.3) + 0.01 * rng.standard_normal(n),
           0.7 * np.sin(2 * np.pi * t / 30 + 1.1) + 0.01 * rng.standard_normal(n)]
    for p in (7, 13):
        pat = rng.standard_normal(p)
        pat -= pat.mean()
        out.append(np.tile(pat, n // p + 1)[:n] + 0.01 * rng.standard_normal(n))
    out += [np.full(n, 2.5), np.zeros(n), multi_sinusoid_window(3, n), multi_sinusoid_window(4, n)]
    out[7][5] = np.nan
    return np.stack(out)


def _rule(pows):
    best = int(np.argmax(pows))
    return best if best > 0 else 1  # (QOPeriods.py:1227-1232)


def _three_calls(eng, x, max_p, trunc):
    """(powers, periods, norms) of the finite rows of x by ph_orth_powers, ph_project_batch and ph_periodic_norm."""
    pows = eng.orth_powers(x, max_p, True)
    per = np.array([_rule(r) for r in pows])
    nrm = np.zeros(x.shape[0])
    for w, p in enumerate(per):
        base = eng.project_batch(x[w:w + 1], [int(p)], trunc, True)[0, 0]
        nrm[w] = eng.periodic_norm(base[None, :], int(p))[0]
    return pows, per, nrm


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------- 1. select against the three calls
@pytest.mark.parametrize("trunc", [False, True])
@pytest.mark.parametrize("n", [36, 97, 600, 1024])
def test_select_against_the_three_calls(engines, n, trunc):
    from pyperiod_amd import _ffi

    eng = engines[0]
    x = _rows(n)
    fin = np.arange(7)
    for max_p in sorted({max(2, min(mp, n // 3)) for mp in (2, 12, 100)}):
        assert eng.plan_info("qo_orth_select", n, (max_p,))[0].window == eng.plan_info("orth_powers", n, (max_p,))[0].window
        per, nrm, st, pows = eng.qo_orth_select(x, max_p, trunc, want_powers=True)
        want_pows, want_per, want_nrm = _three_calls(eng, x[fin], max_p, trunc)
        assert _same_bits(pows[fin], want_pows), (n, max_p)
        assert np.array_equal(pows[7], eng.orth_powers(x[7:], max_p, True)[0], equal_nan=True)
        assert list(st) == [_ffi.PH_ST_OK] * 7 + [_ffi.PH_ST_NO_PERIOD] and per[7] == 0 and nrm[7] == 0
        assert np.array_equal(per[fin], want_per), (n, max_p, per, want_per)
        err = np.abs(nrm[fin] - want_nrm) / np.maximum(want_nrm, 1e-300)
        print(f"N={n} max_p={max_p} trunc={trunc}: periods {per.tolist()} norm err {err.max():.2e}")
        assert np.all(err <= TOL_SAME), (n, max_p, err)
        assert per[4] == 1 and per[5] == 1 and nrm[5] == 0.0 and not pows[5].any()
        if max_p > 30:
            assert list(per[:4]) == [12, 30, 7, 13]
        per2, nrm2, st2 = eng.qo_orth_select(x, max_p, trunc)  # powers = NULL
        assert np.array_equal(per2, per) and np.array_equal(nrm2, nrm) and np.array_equal(st2, st)


def test_round0_powers_of_the_fixture(engines, golden):
    g = golden("qo_orth")
    for tag in "ABD":
        n, _, _, max_length, _ = g[f"{tag}_kw"]
        x = np.stack([multi_sinusoid_window(int(g[f"{tag}{w}_seed"]), int(n)) for w in range(8)])
        for eng in engines:
            per, nrm, st, pows = eng.qo_orth_select(x, int(max_length), False, want_powers=True)
            assert not st.any()
            for w in range(8):
                assert rel_err(pows[w], g[f"{tag}{w}_pows0"]) <= TOL_REF, (tag, w)
                assert per[w] == _rule(g[f"{tag}{w}_pows0"])
                if g[f"{tag}{w}_periods"].size:
                    assert per[w] == g[f"{tag}{w}_periods"][0] and abs(nrm[w] - g[f"{tag}{w}_norms"][0]) <= TOL_REF * nrm[w]


def test_argument_checks(engines):
    eng = engines[0]
    x = np.zeros((2, 600))
    with pytest.raises(ValueError):
        eng.qo_orth_select(x, 1)
    with pytest.raises(ValueError):
        eng.plan_info("qo_orth_select", 600, (1,))
    from pyperiod_amd import _factors, _ffi

    off, q = _factors.orth_tables(10)  # covers p <= 10, max_p = 12 needs 11
    out = [np.zeros(2, np.int32), np.zeros(2), np.zeros(2, np.int32)]
    rc = eng._lib.ph_qo_orth_select(eng._ctx, x.ctypes.data, _ffi.PH_F64, 2, 600, 12, off.ctypes.data, q.ctypes.data, 10, 0,
                                    out[0].ctypes.data, out[1].ctypes.data, None, out[2].ctypes.data)
    assert rc == _ffi.PH_E_ARG
    assert eng.plan_info("qo_orth_select", 600)[0].lds_bytes == eng.plan_info("qo_orth_select", 600, (200,))[0].lds_bytes


# ---------------------------------------------------------------------------- 2. placements
def test_both_placements(engines):
    from pyperiod_amd import _ffi

    eng, hbm = engines
    for n, max_p in ((97, 32), (600, 100), (1024, 128)):
        assert hbm.plan_info("qo_orth_select", n, (max_p,))[0].window == _ffi.PH_PLAN_HBM
        assert eng.plan_info("qo_orth_select", n, (max_p,))[0].window == _ffi.PH_PLAN_LDS
        x = _rows(n)
        for trunc in (False, True):
            a = eng.qo_orth_select(x, max_p, trunc, want_powers=True)
            b = hbm.qo_orth_select(x, max_p, trunc, want_powers=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            assert np.all(np.abs(a[1] - b[1]) <= TOL_SAME * np.abs(a[1]))
            assert _same_bits(b[3][:7], hbm.orth_powers(x[:7], max_p, True))  # the same placement: the same bits


def test_placement_switch(engines):
    from pyperiod_amd import _ffi

    eng, hbm = engines
    max_p = 64

    def where(e, n):
        (k,) = e.plan_info("qo_orth_select", n, (max_p,))
        assert k.block == 512 and k.window == k.second
        return k

    lo, hi = 1, 1 << 20
    assert where(eng, lo).window == _ffi.PH_PLAN_LDS and where(eng, hi).window == _ffi.PH_PLAN_HBM
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if where(eng, mid).window == _ffi.PH_PLAN_LDS else (lo, mid)
    n_star = lo
    assert where(eng, n_star).lds_bytes <= eng.lds_bytes < where(eng, n_star).lds_bytes + 32
    assert where(eng, n_star + 1).lds_bytes == where(hbm, 64).lds_bytes < 1024
    # no more LDS than k_orth_powers beyond the reduction slots
    assert where(eng, n_star).lds_bytes - eng.plan_info("orth_powers", n_star, (max_p,))[0].lds_bytes == where(hbm, 64).lds_bytes
    for n in (n_star - 1, n_star, n_star + 1):
        x = np.stack([multi_sinusoid_window(20 + w, n) for w in range(2)])
        a = eng.qo_orth_select(x, max_p)
        b = hbm.qo_orth_select(x, max_p)
        print(f"N={n}: window {where(eng, n).window} periods {a[0].tolist()} norms {a[1].tolist()}")
        assert not a[2].any() and not b[2].any() and np.array_equal(a[0], b[0])
        assert np.all(np.abs(a[1] - b[1]) <= TOL_SAME * np.abs(a[1]))


# ---------------------------------------------------------------------------- 3. float32, 4. device tensors
def test_float32_rows_equal_the_upcast_rows(engines):
    for eng in engines:
        for n, max_p in ((97, 32), (600, 100)):
            x32 = _rows(n).astype(np.float32)
            for trunc in (False, True):
                a = eng.qo_orth_select(x32, max_p, trunc, want_powers=True)
                b = eng.qo_orth_select(x32.astype(np.float64), max_p, trunc, want_powers=True)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
                assert _same_bits(a[1], b[1]) and _same_bits(a[3][:7], b[3][:7])


def test_device_tensors_give_the_numpy_result(engines):
    import torch

    for eng in engines:
        x = _rows(600)
        for dt in (np.float64, np.float32):
            host = eng.qo_orth_select(x.astype(dt), 100, True, want_powers=True)
            dev = eng.qo_orth_select(torch.as_tensor(x.astype(dt), device="cuda"), 100, True, want_powers=True)
            torch.cuda.synchronize()
            dev = [d.cpu().numpy() for d in dev]
            assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[2], host[2])
            assert _same_bits(dev[1], host[1]) and _same_bits(dev[3][:7], host[3][:7])


# ---------------------------------------------------------------------------- 5. find_periods on the fixture
def _names(eng):
    return [name for name, _ in eng.profile_read()]


def _group(g, tag):
    n, num, thresh, max_length, trunc = g[f"{tag}_kw"]
    kw = dict(num=int(num), thresh=float(thresh), min_length=2, max_length=int(max_length))
    x = np.stack([multi_sinusoid_window(int(g[f"{tag}{w}_seed"]), int(n)) for w in range(8)])
    return x, kw, bool(trunc)


@pytest.mark.parametrize("tag", list(GROUPS))
def test_find_periods_batch_against_reference_fixture(engines, golden, tag):
    from pyperiod_amd import QOPeriods

    g = golden("qo_orth")
    x, kw, trunc = _group(g, tag)
    n = x.shape[1]
    qo = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True)
    batch = qo.find_periods(x, **kw)
    assert len(batch) == 8 and qo.output_bases == [b for b, _ in batch]
    for w in range(8):
        bases, res = batch[w]
        want = {k: g[f"{tag}{w}_{k}"] for k in ("periods", "norms", "weights", "dict_keys", "dict_vals", "residual")}
        assert np.array_equal(bases["periods"], want["periods"]) and len(bases["periods"]) == want["periods"].size
        assert [int(q) for q in bases["basis_dictionary"]] == list(want["dict_keys"])
        assert list(bases["basis_dictionary"].values()) == list(want["dict_vals"])
        assert np.array_equal(bases["subspaces"], po.qo_get_subspaces(list(want["dict_keys"]), n)[0])
        ew, er, en = rel_err(bases["weights"], want["weights"]), rel_err(res, want["residual"]), rel_err(bases["norms"], want["norms"])
        print(f"{tag}{w}: periods {list(bases['periods'])} weights {ew:.2e} residual {er:.2e} norms {en:.2e}")
        assert en <= TOL_REF and ew <= TOL_SOLVE and er <= TOL_SOLVE
    if tag == "E":  # the mixed-fate batch
        short = [len(b["periods"]) < len(b["basis_dictionary"]) for b, _ in batch]
        assert any(short) and not all(short)


# ---------------------------------------------------------------------------- 6. batch equals rows
def test_batch_equals_rows(engines):
    """Sixteen rows, an all-zero and a constant one among them, against the sixteen 1-D calls.  The constant row picks
    period 1 in round one, is fitted exactly, and picks period 1 again on its zero residual: ph_qo_fit hands the list
    [1, 1] back (a block without rows) and the row goes to the 1-D call, whose answer for it is a ValueError
    (get_subspaces gives the repeated period no rows and ph_fold_sums refuses a dictionary without rows) -- before this
    path existed and now.  So the batch with that row raises what the row raises, the device loop itself hands the row
    back without raising, and the other fifteen rows are compared value by value."""
    from pyperiod_amd import QOPeriods

    n, kw = 600, dict(num=4, thresh=0.05, min_length=2, max_length=100)
    rows = [multi_sinusoid_window(30 + w, n) for w in range(14)] + [np.zeros(n), np.full(n, 1.5)]
    x = np.stack(rows)
    for trunc in (False, True):
        qo = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True)
        with pytest.raises(ValueError, match="keep"):
            QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True).find_periods(x[15], **kw)
        with pytest.raises(ValueError, match="keep"):
            qo.find_periods(x, **kw)
        stepped = qo._find_periods_stepped(engines[0], x, qo._select_orthogonal(engines[0], kw["max_length"]), kw["num"],
                                           kw["thresh"], kw["max_length"])
        assert stepped[14] is None and stepped[15] is None and all(r is not None for r in stepped[:14])
        batch = qo.find_periods(x[:15], **kw)
        for w in range(15):
            gb, gr = batch[w]
            wb, wr = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True).find_periods(x[w], **kw)
            assert set(gb.keys()) == set(wb.keys())
            assert np.array_equal(gb["periods"], wb["periods"]) and gb["basis_dictionary"] == wb["basis_dictionary"], w
            assert np.asarray(gb["periods"]).dtype == np.asarray(wb["periods"]).dtype
            assert rel_err(gb["norms"], wb["norms"]) <= TOL_SAME, w
            assert rel_err(gb["weights"], wb["weights"]) <= TOL_SOLVE and rel_err(gr, wr) <= TOL_SOLVE, w
            assert gr.dtype == np.float64 and np.array_equal(gb["subspaces"], wb["subspaces"])
        assert list(batch[14][0]["periods"]) == [1] and not batch[14][1].any()  # all zero: the reference's fixed answer


# ---------------------------------------------------------------------------- 7. launches
def test_two_launches_per_round(engines, golden):
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    x, kw, trunc = _group(golden("qo_orth"), "B")  # eight rows, four rounds each, nothing handed back
    qo = QOPeriods(orthogonalize=True)
    eng.profile(True)
    try:
        qo.find_periods(x, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_orth_select", "k_qo_fit"] * 4, names
    # the mixed-fate batch: rows leave after the first fit, the rounds stay two launches
    x, kw, trunc = _group(golden("qo_orth"), "E")
    eng.profile(True)
    try:
        qo.find_periods(x, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names == ["k_qo_orth_select", "k_qo_fit"] * 4, names
    for gone in ("k_orth_powers", "k_project_batch", "k_periodic_norm", "k_fold_sums", "k_tile_sum"):
        assert gone not in names
    # what stays on the 1-D path: update_weights=False under orthogonal selection, a window
    eng.profile(True)
    try:
        qo.find_periods(x[:2], update_weights=False, **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert "k_qo_orth_select" not in names and "k_orth_powers" in names
