"""CPU-only checks for the batched QOPeriods.find_periods under orthogonal selection: the fixture
tests/golden/qo_orth.npz holds data only, the oracle's pieces reproduce every row of it in the loop the reference's
commented-out lines intend (QOPeriods.py:435-448), and the new C ABI rejects bad arguments without a GPU."""

import ctypes
import os
import re
import zipfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

GROUPS = "ABCDE"
ROWS = 8
KEYS = {"seed", "periods", "norms", "dict_keys", "dict_vals", "weights", "residual", "gaps", "cond", "pows0"}


def rms(v):
    return np.sqrt(np.sum(np.power(v, 2)) / len(v))  # (Periods.py:16-30)


def group_kw(g, tag):
    n, num, thresh, max_length, trunc = g[f"{tag}_kw"]
    return int(n), int(num), float(thresh), int(max_length), bool(trunc)


def oracle_orth_find_periods(x, num, thresh, max_length, trunc):
    """_find_periods_host + _strongest_period under orthogonalize=True, update_weights=True, default test function, from
    the oracle's pieces.  -> (periods reported, norms reported, dims, weights, residual, round-0 powers)."""
    n = x.size
    res = x.copy()
    periods, norms = [], []
    pows0 = recon = dims = w = None
    n_report = None
    for i in range(num):
        if i > 0 and not (rms(recon) > rms(x) * thresh):
            n_report = len(periods) - 1
            break
        if i == 0:
            pows0 = po.orth_powers(res, max_length, True)
        p = po.best_period_orthogonal(res, max_length, True)
        base = po.project(res, p, trunc, True)
        norms.append(po.periodic_norm(base, p))
        periods.append(p)
        a, dims = po.qo_get_subspaces(periods, n)
        w, recon = po.qo_solve_quadratic(x, a)
        res = x - recon
    n_report = len(periods) if n_report is None else n_report
    return periods[:n_report], norms[:n_report], dims, w, res, pows0


def test_fixture_holds_data_only():
    path = os.path.join(GOLDEN, "qo_orth.npz")
    assert os.path.getsize(path) < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                                       if f.endswith(".npz") and f != "qo_orth.npz")
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
    assert all(nm.endswith(".npy") for nm in names)
    g = np.load(path, allow_pickle=False)  # (object arrays -- anything pickled -- would raise on access)
    want = {f"{t}{w}_{k}" for t in GROUPS for w in range(ROWS) for k in KEYS} | {f"{t}_kw" for t in GROUPS}
    assert set(g.files) == want
    for k in g.files:
        assert g[k].dtype.kind in "fi", k


def test_fixture_conditions(golden):
    """What make_golden_qo_orth.py asserted when it wrote the file still holds for the file that is committed."""
    g = golden("qo_orth")
    assert [group_kw(g, t) for t in GROUPS] == [(36, 4, 0.05, 12, False), (600, 4, 0.05, 100, False), (600, 4, 0.05, 100, True),
                                                (1024, 4, 0.05, 128, False), (600, 4, 0.6, 100, False)]
    for t in GROUPS:
        for w in range(ROWS):
            assert g[f"{t}{w}_gaps"].min() >= 1e-6 and g[f"{t}{w}_cond"] <= 1e7 and g[f"{t}{w}_dict_vals"].min() > 0
    full = [g[f"E{w}_periods"].size == g[f"E{w}_dict_keys"].size for w in range(ROWS)]
    assert any(full) and not all(full)  # the mixed-fate batch
    for w in range(ROWS):  # trunc changes norms, not periods
        assert g[f"B{w}_seed"] == g[f"C{w}_seed"] and np.array_equal(g[f"B{w}_periods"], g[f"C{w}_periods"])
    assert any(not np.array_equal(g[f"B{w}_norms"], g[f"C{w}_norms"]) for w in range(ROWS))


@pytest.mark.parametrize("tag", list(GROUPS))
def test_oracle_pieces_reproduce_the_fixture(golden, tag):
    g = golden("qo_orth")
    n, num, thresh, max_length, trunc = group_kw(g, tag)
    for w in range(ROWS):
        key = f"{tag}{w}"
        x = multi_sinusoid_window(int(g[f"{key}_seed"]), n)
        periods, norms, dims, wts, res, pows0 = oracle_orth_find_periods(x, num, thresh, max_length, trunc)
        assert periods == list(g[f"{key}_periods"]), key
        assert [int(q) for q in dims] == list(g[f"{key}_dict_keys"]) and list(dims.values()) == list(g[f"{key}_dict_vals"]), key
        assert rel_err(norms, g[f"{key}_norms"]) <= 1e-10, key
        assert rel_err(pows0, g[f"{key}_pows0"]) <= 1e-10, key
        assert rel_err(wts, g[f"{key}_weights"]) <= 1e-8 and rel_err(res, g[f"{key}_residual"]) <= 1e-8, key


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    return _ffi.load()


def test_new_symbol_and_plan_op_reject_bad_arguments_without_gpu(lib):
    from pyperiod_amd import _ffi

    rc = lib.ph_qo_orth_select(None, None, _ffi.PH_F64, 1, 16, 5, None, None, 0, 0, None, None, None, None)
    assert rc == _ffi.PH_E_ARG and b"ctx" in lib.ph_last_error()
    rec = (ctypes.c_int32 * _ffi.PH_PLAN_LEN)()
    for max_p in (1, 0):
        prm = (ctypes.c_int32 * 1)(max_p)
        rc = lib.ph_plan_info(None, _ffi.PH_OP_QO_ORTH_SELECT, _ffi.PH_F64, 600, ctypes.addressof(prm), 1, 0, ctypes.addressof(rec))
        assert rc == _ffi.PH_E_ARG
    with pytest.raises(ValueError):
        _ffi.check(rc)


def test_header_binding_and_engine_agree():
    from pyperiod_amd import _ffi
    from pyperiod_amd.engine import PeriodEngine

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    m = re.search(r"#define PH_OP_QO_ORTH_SELECT (\d+)", text)
    assert m and int(m.group(1)) == _ffi.PH_OP_QO_ORTH_SELECT == 11
    assert PeriodEngine._PLAN_OPS["qo_orth_select"] == 11
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\bint ph_qo_orth_select\((.*?)\);", flat, flags=re.S).group(1)
    assert len(args.split(",")) == len(_ffi.SIGNATURES["ph_qo_orth_select"]) == 14
