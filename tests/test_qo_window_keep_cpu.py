"""CPU checks of the two windowed QOPeriods.find_periods batches that run on the device: the fixed-weight loop under an
analysis window (ph_qo_greedy_win) and orthogonal selection with weights re-solved under one.  The fixture
tests/golden/qo_window_keep.npz (the reference's own runs) holds data only and is reproduced by two dense numpy
restatements -- ``np_find_periods_keep_win`` also serves tests/test_gpu_qo_window_keep.py for inputs the fixture does not
hold --, the new C ABI rejects bad arguments without a GPU, and a (W, N) batch reaches the engine calls the routes name."""

import os
import re
import sys
import zipfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window
from test_qo_batch_cpu import _factors, _phi, np_pp, np_strongest
from test_qo_orth_cpu import rms
from test_qo_window_cpu import WINDOWS, windowed_solve

K_GROUPS = ("KA", "KB", "KC", "KD", "KE", "KF")
O_GROUPS = ("OB", "OC", "OE")
ROWS = 6
K_KEYS = {"seed", "periods", "norms", "dict_keys", "dict_vals", "weights", "residual", "blocks", "gaps", "minden"}
O_KEYS = {"seed", "periods", "norms", "dict_keys", "dict_vals", "weights", "residual", "gaps", "cond", "pows0"}


def k_group_kw(g, tag):
    """-> (N, window, dict(num, thresh, min_length, max_length), trunc) of a K group."""
    n, num, thresh, lo, hi, trunc, code = g[f"{tag}_kw"]
    return int(n), WINDOWS[int(code)](int(n)), dict(num=int(num), thresh=float(thresh), min_length=int(lo), max_length=int(hi)), bool(trunc)


def o_group_kw(g, tag):
    """-> (N, window, num, thresh, max_length, trunc) of an O group."""
    n, num, thresh, hi, trunc, code = g[f"{tag}_kw"]
    return int(n), WINDOWS[int(code)](int(n)), int(num), float(thresh), int(hi), bool(trunc)


# ---------------------------------------------------------------------------- numpy restatements
def np_find_periods_keep_win(x, win, num, thresh, min_length, max_length, trunc=False):
    """QOPeriods.find_periods(update_weights=False) with ``window`` set (QOPeriods.py:373-596 with _dont_update_weights,
    :645-714, whose solve_quadratic gets the window, :779-796), in dense numpy.  The selection, the stop test and the
    residual update are not windowed; only the block's weights are.  -> (dict(periods, norms, weights,
    basis_dictionary, blocks), residual) with `blocks` the (period, keep) of every block in the order fitted
    (duplicates and the re-fitted last block included), or (None, residual) when the first solve is singular."""
    data = np.asarray(x, dtype=np.float64)
    n = data.size
    res = data.copy()
    periods, norms, blocks, wts, dims = [], [], [], np.array([]), {}
    recon, result = None, None

    def fit(p):
        keep = p - sum(_phi(f) for f in set().union(*[_factors(q) for q in periods[:-1]], set()) & _factors(p))
        w, rec = windowed_solve(res, win, np_pp(p, n, keep))  # (a zero window sum on a fitted class: LinAlgError)
        return keep, w, rec

    def report(count):
        return {"periods": np.array(periods[:count], dtype=np.uint32), "norms": np.array(norms[:count]), "weights": wts,
                "basis_dictionary": dict(dims), "blocks": list(blocks)}

    for i in range(num):
        if i > 0 and not rms(recon) > rms(data) * thresh:  # the last block once more, the residual as it is
            keep, w, _ = fit(periods[-1])
            dims[str(periods[-1])] = keep
            blocks.append((periods[-1], keep))
            wts = np.concatenate((wts, w))
            return report(len(periods) - 1), res
        p, g = np_strongest(res, min_length, max_length, trunc)
        assert p > 0
        periods.append(p)
        norms.append(g)
        try:
            keep, w, recon = fit(p)
        except np.linalg.LinAlgError:  # QOPeriods.py:552-559
            periods.pop()
            norms.pop()
            break
        dims[str(p)] = keep
        blocks.append((p, keep))
        wts = np.concatenate((wts, w))
        res = res - recon
        result = report(len(periods))
    return result, res


def np_orth_find_periods_win(x, win, num, thresh, max_length, trunc):
    """test_qo_orth_cpu.oracle_orth_find_periods with every solve under the analysis window (only the fit sees it).
    -> (periods reported, norms reported, dims, weights, residual, round-0 powers)."""
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
        w, recon = windowed_solve(x, win, a)
        res = x - recon
    n_report = len(periods) if n_report is None else n_report
    return periods[:n_report], norms[:n_report], dims, w, res, pows0


# ---------------------------------------------------------------------------- the fixture
def test_fixture_holds_data_only():
    path = os.path.join(GOLDEN, "qo_window_keep.npz")
    assert os.path.getsize(path) < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                                       if f.endswith(".npz") and f != "qo_window_keep.npz")
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
    assert all(nm.endswith(".npy") for nm in names)
    g = np.load(path, allow_pickle=False)  # (object arrays -- anything pickled -- would raise on access)
    want = {f"{t}{w}_{k}" for t in K_GROUPS for w in range(ROWS) for k in K_KEYS} | {f"{t}_kw" for t in K_GROUPS + O_GROUPS}
    want |= {f"{t}{w}_{k}" for t in O_GROUPS for w in range(ROWS) for k in O_KEYS}
    assert set(g.files) == want
    for k in g.files:
        assert g[k].dtype.kind in "fi", k


def test_fixture_conditions(golden):
    """What make_golden_qo_window_keep.py asserted when it wrote the file still holds for the file that is committed."""
    g = golden("qo_window_keep")
    want = {"KA": (36, 12, 0.05, 0, False), "KB": (600, 100, 0.05, 0, False), "KC": (600, 100, 0.05, 0, True),
            "KD": (1024, 128, 0.05, 1, False), "KE": (600, 100, 0.3, 0, False), "KF": (600, 100, 0.05, 2, False)}
    for t, (n, hi, thresh, code, trunc) in want.items():
        assert list(g[f"{t}_kw"]) == [n, 4, thresh, 2, hi, int(trunc), code], t
        for w in range(ROWS):
            assert g[f"{t}{w}_gaps"].min() >= 1e-6 and g[f"{t}{w}_minden"] >= 1e-3, (t, w)
    assert (np.hanning(600) - 0.2).min() < 0  # KF's window is negative at the ends
    for w in range(ROWS):
        assert g[f"KB{w}_seed"] == g[f"KC{w}_seed"]
    stopped = [g[f"KE{w}_periods"].size < g[f"KE{w}_blocks"].shape[0] for w in range(ROWS)]
    assert any(stopped) and not all(stopped)  # the mixed-fate batch
    assert sum(int((g[f"{t}{w}_blocks"][:, 1] == 0).any()) for t in K_GROUPS for w in range(ROWS)) >= 4  # the keep == 0 quirk
    for t in O_GROUPS:
        n, _, num, thresh, hi, trunc = o_group_kw(g, t)
        assert (n, num, hi, trunc) == (600, 4, 100, t == "OC") and thresh == (0.05 if t != "OE" else g["OE_kw"][2])
        for w in range(ROWS):
            assert g[f"{t}{w}_gaps"].min() >= 1e-6 and g[f"{t}{w}_cond"] <= 1e7 and g[f"{t}{w}_dict_vals"].min() > 0
    assert g["OE_kw"][2] in (0.3, 0.45, 0.6, 0.75)
    full = [g[f"OE{w}_periods"].size == g[f"OE{w}_dict_keys"].size for w in range(ROWS)]
    assert any(full) and not all(full)
    for w in range(ROWS):
        assert g[f"OB{w}_seed"] == g[f"OC{w}_seed"]


@pytest.mark.parametrize("tag", K_GROUPS)
def test_keep_restatement_reproduces_the_fixture(golden, tag):
    g = golden("qo_window_keep")
    n, win, kw, trunc = k_group_kw(g, tag)
    for w in range(ROWS):
        key = f"{tag}{w}"
        x = multi_sinusoid_window(int(g[f"{key}_seed"]), n)
        out, res = np_find_periods_keep_win(x, win, trunc=trunc, **kw)
        assert np.array_equal(out["periods"], g[f"{key}_periods"]), key
        assert out["blocks"] == [tuple(b) for b in g[f"{key}_blocks"].tolist()], key
        assert [int(q) for q in out["basis_dictionary"]] == list(g[f"{key}_dict_keys"]), key
        assert list(out["basis_dictionary"].values()) == list(g[f"{key}_dict_vals"]), key
        assert out["weights"].size == g[f"{key}_weights"].size == sum(k if k else p for p, k in out["blocks"]), key
        assert rel_err(out["norms"], g[f"{key}_norms"]) <= 1e-10, key
        assert rel_err(out["weights"], g[f"{key}_weights"]) <= 1e-10 and rel_err(res, g[f"{key}_residual"]) <= 1e-10, key


def test_keep_restatement_singular_window():
    """A window that is zero on a whole fitted residue class: the reference's matrix is singular, its loop ends on
    LinAlgError with the result so far (none in the first round).  Zero only on a class the block does not fit: solved."""
    n = 70
    x = np.tile(np.array([3.0, -1.0, 2.0, 0.5, -2.5, 1.0, 4.0]), 10) + 0.01 * np.random.default_rng(5).standard_normal(n)
    win = np.hanning(n) + 0.1
    win[3::7] = 0.0
    out, res = np_find_periods_keep_win(x, win, 3, 0.05, 2, 12)
    assert out is None and np.array_equal(res, x)
    out, _ = np_find_periods_keep_win(x, np.hanning(n) + 0.1, 3, 0.05, 2, 12)
    assert out["blocks"][0] == (7, 7)


@pytest.mark.parametrize("tag", O_GROUPS)
def test_orth_restatement_reproduces_the_fixture(golden, tag):
    g = golden("qo_window_keep")
    n, win, num, thresh, max_length, trunc = o_group_kw(g, tag)
    for w in range(ROWS):
        key = f"{tag}{w}"
        x = multi_sinusoid_window(int(g[f"{key}_seed"]), n)
        periods, norms, dims, wts, res, pows0 = np_orth_find_periods_win(x, win, num, thresh, max_length, trunc)
        assert periods == list(g[f"{key}_periods"]), key
        assert [int(q) for q in dims] == list(g[f"{key}_dict_keys"]) and list(dims.values()) == list(g[f"{key}_dict_vals"]), key
        assert rel_err(norms, g[f"{key}_norms"]) <= 1e-10, key
        assert rel_err(pows0, g[f"{key}_pows0"]) <= 1e-10, key
        assert rel_err(wts, g[f"{key}_weights"]) <= 1e-8 and rel_err(res, g[f"{key}_residual"]) <= 1e-8, key


# ---------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    return _ffi.load()


def test_greedy_win_rejects_null_context_and_window_without_gpu(lib):
    from pyperiod_amd import _ffi

    x = np.ones(64)
    for flags in (0, _ffi.PH_FLAG_TRUNC, _ffi.PH_FLAG_KEEP_WEIGHTS, _ffi.PH_FLAG_KEEP_WEIGHTS | _ffi.PH_FLAG_TRUNC):
        rc = lib.ph_qo_greedy_win(None, x.ctypes.data, _ffi.PH_F64, 1, 64, x.ctypes.data, 2, 0.1, 2, 20, 64, flags,
                                  None, None, None, None, None, None, None)
        assert rc == _ffi.PH_E_ARG and b"ctx" in lib.ph_last_error()
    rc = lib.ph_qo_greedy_win(None, x.ctypes.data, _ffi.PH_F64, 1, 64, None, 2, 0.1, 2, 20, 64, 0,
                              None, None, None, None, None, None, None)
    assert rc == _ffi.PH_E_ARG
    with pytest.raises(ValueError):
        _ffi.check(rc)


def test_header_and_binding_agree():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\bint ph_qo_greedy_win\((.*?)\);", flat, flags=re.S).group(1)
    assert len(args.split(",")) == len(_ffi.SIGNATURES["ph_qo_greedy_win"]) == 19
    # ph_qo_find_periods plus the window behind N
    old = re.search(r"\bint ph_qo_find_periods\((.*?)\);", flat, flags=re.S).group(1)
    assert len(old.split(",")) == len(_ffi.SIGNATURES["ph_qo_find_periods"]) == 18
    assert "const double* window" in args.split(",")[5]


# ---------------------------------------------------------------------------- routing
class _FakeEngine:
    """Records the engine calls of a batch and answers them with well-formed arrays; nothing touches a GPU.  It has no
    sweep / fold_sums / orth_powers: a row that falls to the 1-D call raises AttributeError."""

    def __init__(self):
        self.calls = []

    def qo_find_periods(self, x, num, thresh, min_length=2, max_length=None, kcap=512, trunc=False, update_weights=True,
                        window=None):
        self.calls.append(("qo_find_periods", dict(update_weights=update_weights, window=window, trunc=trunc, shape=x.shape)))
        W, N = x.shape
        per = np.zeros((W, num), dtype=np.uint32)
        per[:, 0] = 7
        keeps = np.zeros((W, num), dtype=np.int32)
        keeps[:, 0] = 7
        nrm = np.zeros((W, num))
        nrm[:, 0] = 1.0
        return (per, nrm, keeps, np.tile(np.array([[1, 1]], dtype=np.int32), (W, 1)), np.zeros((W, kcap)), x.copy(),
                np.zeros(W, dtype=np.int32))

    def qo_orth_select(self, x, max_p, trunc=False, want_powers=False):
        self.calls.append(("qo_orth_select", dict(shape=x.shape, max_p=max_p, trunc=trunc)))
        W = x.shape[0]
        p = 5 if sum(1 for c in self.calls if c[0] == "qo_orth_select") == 1 else 7
        return np.full(W, p, dtype=np.int32), np.ones(W), np.zeros(W, dtype=np.int32)

    def qo_fit_feasible(self, kcap, max_period, n=None, window=False):
        return kcap <= 512

    def qo_fit(self, x, periods, n_periods=None, kcap=512, max_period=None, window=None):
        self.calls.append(("qo_fit", dict(window=window, shape=x.shape, counts=list(n_periods))))
        W, N = x.shape
        keeps = np.zeros(periods.shape, dtype=np.int32)
        for w in range(W):
            keeps[w, : n_periods[w]] = [5, 6][: n_periods[w]]
        return keeps, np.zeros((W, kcap)), 0.5 * x, np.zeros(W, dtype=np.int32)


def test_windowed_batches_are_routed_to_the_device_calls(monkeypatch):
    """A (W, N) batch with ``window`` set and update_weights=False reaches qo_find_periods once, with the window; with
    orthogonalize=True (re-solved weights) it reaches qo_orth_select and qo_fit(..., window=...) once per round.  No
    row runs the 1-D call (the fake engine could not serve it)."""
    from pyperiod_amd import QOPeriods

    mod = sys.modules[QOPeriods.__module__]
    x = np.stack([multi_sinusoid_window(s, 96) for s in range(3)])
    win = np.hanning(96)

    fake = _FakeEngine()
    monkeypatch.setattr(mod, "default_engine", lambda: fake)
    qo = QOPeriods()
    qo.window = win
    out = qo.find_periods(x, num=2, thresh=0.1, max_length=20, update_weights=False)
    assert [c[0] for c in fake.calls] == ["qo_find_periods"]
    call = fake.calls[0][1]
    assert call["update_weights"] is False and call["shape"] == (3, 96) and np.array_equal(call["window"], win)
    assert call["window"].dtype == np.float64 and not call["trunc"]
    assert len(out) == 3 and all(list(b["periods"]) == [7] and b["basis_dictionary"] == {"7": 7} for b, _ in out)

    fake = _FakeEngine()
    monkeypatch.setattr(mod, "default_engine", lambda: fake)
    qo = QOPeriods(trunc_to_integer_multiple=True, orthogonalize=True)
    qo.window = list(win)  # (anything numpy turns into N finite doubles)
    out = qo.find_periods(x, num=2, thresh=0.1, max_length=20)
    assert [c[0] for c in fake.calls] == ["qo_orth_select", "qo_fit", "qo_orth_select", "qo_fit"]
    for name, call in fake.calls:
        if name == "qo_fit":
            assert np.array_equal(call["window"], win) and call["shape"] == (3, 96)
        else:
            assert call["trunc"] and call["max_p"] == 20
    assert fake.calls[1][1]["counts"] == [1, 1, 1] and fake.calls[3][1]["counts"] == [2, 2, 2]
    assert len(out) == 3 and all(list(b["periods"]) == [5, 7] and b["basis_dictionary"] == {"5": 5, "7": 6} for b, _ in out)

    # without a window the orthogonal batch fits without one, as before
    fake = _FakeEngine()
    monkeypatch.setattr(mod, "default_engine", lambda: fake)
    QOPeriods(orthogonalize=True).find_periods(x, num=1, thresh=0.1, max_length=20)
    assert [c[0] for c in fake.calls] == ["qo_orth_select", "qo_fit"] and fake.calls[1][1]["window"] is None


def test_engine_refuses_a_window_with_resolved_weights():
    """qo_find_periods(window=..., update_weights=True) is a ValueError before anything is launched (that loop is
    stepped from the host); checked on the method itself, without a context."""
    from pyperiod_amd.engine import PeriodEngine

    eng = object.__new__(PeriodEngine)
    eng._ctx = None
    with pytest.raises(ValueError):
        eng.qo_find_periods(np.ones((2, 64)), 2, 0.1, window=np.ones(64))
    with pytest.raises(ValueError):
        eng.qo_find_periods(np.ones((2, 64)), 2, 0.1, update_weights=False, window=np.ones(63))
