"""CPU-only checks for the batched RamanujanPeriods.find_periods_with_weights: the oracle against the reference's
fixture (tests/golden/ramanujan_fit.npz), k_ram_select's selection rule restated in numpy against the reference's
expression, and the new C ABI's argument checks without a GPU."""

import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT, rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

COND_CUT = 1e7  # rows above it are not compared value by value: the reference's own weights are LAPACK noise there


def _cases(g):
    for tag in ("A", "B"):
        n, lo, hi, thresh = g[f"{tag}_kw"]
        kw = dict(min_length=int(lo), max_length=int(hi), thresh=float(thresh))
        for w, seed in enumerate(g[f"{tag}_seeds"]):
            yield tag, w, multi_sinusoid_window(int(seed), int(n)), kw


def test_fixture_conditions(golden):
    """What make_golden_ram_fit.py asserted when it wrote the file still holds for the file that is committed."""
    g = golden("ramanujan_fit")
    assert list(g["A_seeds"]) == list(range(32)) and list(g["B_seeds"]) == list(range(8))
    assert g["A_margin"].min() >= 1e-3 and g["B_margin"].min() >= 1e-3
    assert int(np.sum((g["A_cond"] <= COND_CUT) & (g["A_rows"] <= 2048))) >= 28
    assert int(np.sum(g["B_cond"] <= COND_CUT)) >= 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ramanujan_fit.npz")) < 772 * 1024


def test_oracle_matches_reference_rows(golden):
    g = golden("ramanujan_fit")
    compared = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (numpy.linalg.solve warns on the numerically singular rows)
        for tag, w, sig, kw in _cases(g):
            out, res = po.ramanujan_find_periods_with_weights(sig, **kw)
            key = f"{tag}{w}"
            assert np.array_equal(out["periods"], g[f"{key}_periods"]), key
            assert [int(k) for k in out["basis_dictionary"]] == list(g[f"{key}_dict_keys"]), key
            assert list(out["basis_dictionary"].values()) == list(g[f"{key}_dict_vals"]), key
            assert rel_err(out["norms"], g[f"{key}_norms"][g[f"{key}_periods"]]) < 1e-5, key
            if g[f"{tag}_cond"][w] <= COND_CUT:
                compared += 1
                assert rel_err(out["weights"], g[f"{key}_weights"]) < 1e-8, key
                assert rel_err(res, g[f"{key}_residual"]) < 1e-8, key
    assert compared >= 33


def ram_select_rule(norms, thresh, pcap):
    """k_ram_select restated: m = |max| over the whole row, a NaN anywhere makes it NaN (numpy.max); the ascending q with
    norms[q] / m > thresh (IEEE division, strict); the true count and the first pcap periods, zeros behind them."""
    norms = np.asarray(norms, dtype=np.float64)
    m = np.nan if np.isnan(norms).any() else np.max(norms)
    m = np.abs(m)
    with np.errstate(all="ignore"):
        sel = np.flatnonzero(norms / m > thresh)
    per = np.zeros(pcap, dtype=np.int32)
    per[: min(sel.size, pcap)] = sel[:pcap]
    return sel.size, per


def test_select_rule_matches_reference_expression():
    rng = np.random.default_rng(5)
    rows = [rng.uniform(0, 1, 130) for _ in range(20)]
    rows[1][7] = np.nan  # a NaN anywhere: numpy.max is NaN, nothing is selected
    rows[2][:] = 0.0  # all-zero: 0 / 0 is NaN, nothing is selected
    rows[3][:] = np.nan
    rows[4] = -rows[4]  # all negative: |max| is positive, every ratio negative
    rows[5][:] = 0.0
    rows[5][[10, 20, 30]] = [5.0, 1.0, 1.0 + 2**-50]  # a tie at the threshold: 1 / 5 > 0.2 is false, the next double true
    rows[6][0] = 0.0
    rows[7][[0, 1]] = 0.0  # entries below q_lo are zero and take part in the maximum
    rows[8] = np.full(130, 3.0)  # everything selected, more than pcap
    for i, r in enumerate(rows):
        for thresh in (0.2, 0.1, 0.5, 1.0):
            with np.errstate(all="ignore"):
                want = np.argwhere(r / np.abs(np.max(r)) > thresh).flatten()  # RamanujanPeriods.py:97-99
            count, per = ram_select_rule(r, thresh, 64)
            assert count == want.size, (i, thresh)
            assert list(per[: min(count, 64)]) == list(want[:64]) and not per[min(count, 64):].any(), (i, thresh)
    assert ram_select_rule(rows[5], 0.2, 64)[0] == 2 and list(ram_select_rule(rows[5], 0.2, 64)[1][:2]) == [10, 30]
    assert ram_select_rule(rows[8], 0.2, 64)[0] == 130
    for k in (1, 2, 3, 4):
        assert ram_select_rule(rows[k], 0.2, 64)[0] == 0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    return _ffi.load()


def test_new_symbols_reject_bad_arguments_without_gpu(lib):
    from pyperiod_amd import _ffi

    rc = lib.ph_qo_fit(None, None, _ffi.PH_F64, 1, 16, None, None, 4, 0, 16, 64, 0, None, None, None, None)
    assert rc == _ffi.PH_E_ARG and b"ctx" in lib.ph_last_error()
    rc = lib.ph_ramanujan_fit(None, None, _ffi.PH_F64, 1, 16, 2, 5, 0.2, 4, 64, 0, None, None, None, None, None, None, None)
    assert rc == _ffi.PH_E_ARG and b"ctx" in lib.ph_last_error()
    for bad in (0.0, -0.5, float("nan")):
        rc = lib.ph_ramanujan_fit(None, None, _ffi.PH_F64, 1, 16, 2, 5, bad, 4, 64, 0, None, None, None, None, None, None, None)
        assert rc == _ffi.PH_E_ARG and b"thresh" in lib.ph_last_error(), bad
    rec = (ctypes.c_int32 * _ffi.PH_PLAN_LEN)()
    prm = (ctypes.c_int32 * 2)(512, 128)
    assert lib.ph_plan_info(None, _ffi.PH_OP_QO_FIT, _ffi.PH_F64, 1024, ctypes.addressof(prm), 2, 0, ctypes.addressof(rec)) == _ffi.PH_E_ARG
    with pytest.raises(ValueError):
        _ffi.check(rc)


def test_header_constants_match_binding():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    m = re.search(r"#define PH_OP_QO_FIT (\d+)", text)
    assert m and int(m.group(1)) == _ffi.PH_OP_QO_FIT == 9
    assert re.search(r"#define PH_VERSION 100\b", text)
    for name in ("ph_qo_fit", "ph_ramanujan_fit"):
        assert name in _ffi.SIGNATURES and re.search(rf"\bint {name}\(", text)
    # the argument counts of the declarations and of the binding agree
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ph_qo_fit", "ph_ramanujan_fit"):
        args = re.search(rf"\bint {name}\((.*?)\);", flat, flags=re.S).group(1)
        assert len(args.split(",")) == len(_ffi.SIGNATURES[name]), name
