"""CPU checks of batched / trunc / fixed-weight QOPeriods.find_periods: the C ABI of the new flag, and the
reference's trunc fixture against a numpy restatement of the greedy loop.  The restatement (``np_find_periods``)
also serves the GPU tests of tests/test_gpu_qo_batch.py: it restates QOPeriods.py:373-596 with the plain
(update_weights=True, :598-643) and the fixed-weight (update_weights=False, :645-714) solves, in dense numpy."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rel_err


# ---------------------------------------------------------------------------- numpy restatement
def np_project(x, p, trunc):
    """Periods.project (Periods.py:171-198), plain or trunc."""
    n = x.size
    rows = -(-n // p)
    short = rows * p - n
    cp = np.pad(x, (0, short)).reshape(rows, p)
    if trunc:
        mean = cp.mean(0) if short == 0 else cp[:-1].mean(0)
    else:
        mean = cp.sum(0) / np.where(np.arange(p) < p - short, rows, rows - 1)
    return np.tile(mean, n // p + 1)[:n]


def np_strongest(res, lo, hi, trunc):
    """First maximum of the gamma norms periodic_norm(project(res, p), p) (QOPeriods.py:470-478)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = np.array([np.linalg.norm(np_project(res, p, trunc)) / np.sqrt(res.size) / np.sqrt(p) for p in range(lo, hi + 1)])
    order = np.where(np.isnan(vals), -np.inf, vals)
    k = int(np.argmax(order))
    return (lo + k, vals[k]) if order[k] > 0 else (0, 0.0)


def _factors(n):
    return {d for d in range(1, n + 1) if n % d == 0}


def _phi(n):
    return sum(1 for k in range(1, n + 1) if math.gcd(n, k) == 1)


def np_pp(p, n, keep):
    m = (np.arange(n)[None, :] % p == np.arange(p)[:, None]).astype(np.float64)
    return m[:keep] if keep else m  # QOPeriods.py:970-974


def _solve(x, a):
    w = np.linalg.solve(a @ a.T, a @ x)  # QOPeriods.py:779-796
    return w, a.T @ w


def np_find_periods(x, num, thresh, min_length, max_length, trunc=False, update_weights=True):
    """-> (dict(periods, norms, subspaces, weights, basis_dictionary, blocks), residual); `blocks` lists
    (period, keep) of every block in the order fitted (duplicates and the re-fitted last block included)."""
    data = np.asarray(x, dtype=np.float64)
    n = data.size
    rms = lambda v: np.sqrt(np.sum(np.power(v, 2)) / len(v))  # noqa: E731
    st = {"A": np.empty((0, n)), "dims": {}, "w": np.array([]), "recon": None, "blocks": []}
    res = data.copy()
    periods, norms, result = [], [], None

    def resolve(active):
        if update_weights:  # get_subspaces (QOPeriods.py:830-840) + solve against the data
            seen, old, dims = set(), 0, {}
            for q in active:
                seen |= _factors(q)
                s = sum(_phi(r) for r in seen)
                dims[str(q)] = s - old
                old = s
            a = np.vstack([np_pp(int(q), n, k) for q, k in dims.items()])
            w, rec = _solve(data, a)
            st.update(A=a, dims=dims, w=w, recon=rec, blocks=[(int(q), k) for q, k in dims.items()])
        else:  # _dont_update_weights: the newest period's rows fitted to the residual
            last = active[-1]
            keep = last
            existing = set()
            for q in active[:-1]:
                existing |= _factors(q)
            for f in sorted(existing & _factors(last)):
                keep -= _phi(f)
            b = np_pp(last, n, keep)
            w, rec = _solve(res, b)
            st["dims"][str(last)] = keep
            st.update(A=np.vstack((st["A"], b)), w=np.concatenate((st["w"], w)), recon=rec,
                      blocks=st["blocks"] + [(last, keep)])

    def report(count):
        return {"periods": np.array(periods[:count], dtype=np.uint32), "norms": np.array(norms[:count]),
                "subspaces": st["A"], "weights": st["w"], "basis_dictionary": dict(st["dims"]), "blocks": list(st["blocks"])}

    for i in range(num):
        if i > 0 and not rms(st["recon"]) > rms(data) * thresh:
            resolve(periods)
            return report(len(periods) - 1), res
        p, g = np_strongest(res, min_length, max_length, trunc)
        assert p > 0
        periods.append(p)
        norms.append(g)
        try:
            resolve(periods)
        except np.linalg.LinAlgError:
            periods.pop()
            norms.pop()
            break
        res = (data - st["recon"]) if update_weights else (res - st["recon"])
        result = report(len(periods))
    return result, res


# ---------------------------------------------------------------------------- tests
def test_trunc_fixture_matches_numpy_restatement(golden):
    """tests/golden/qoperiods_trunc.npz (the reference's plain branch with trunc_to_integer_multiple=True) is what the
    restatement computes: the fixture and the restatement check each other."""
    g = golden("qoperiods_trunc")
    for tag in ("w5", "w9"):
        num, thresh, lo, hi = g[f"{tag}_kw"]
        out, res = np_find_periods(g[f"{tag}_x"], int(num), thresh, int(lo), int(hi), trunc=True)
        assert np.array_equal(out["periods"], g[f"{tag}_periods"]), tag
        assert [int(k) for k in out["basis_dictionary"]] == list(g[f"{tag}_dict_keys"])
        assert list(out["basis_dictionary"].values()) == list(g[f"{tag}_dict_vals"])
        assert rel_err(out["norms"], g[f"{tag}_norms"]) < 1e-12
        assert rel_err(out["weights"], g[f"{tag}_weights"]) < 1e-9 and rel_err(res, g[f"{tag}_residual"]) < 1e-9
    # trunc changes the selection's norms on these windows (N is not a multiple of the periods)
    plain, _ = np_find_periods(g["w5_x"], 4, 0.2, 4, 200, trunc=False)
    assert rel_err(plain["norms"], g["w5_norms"]) > 1e-6


def keep_quirk_rows(n=900):
    """Rows whose fixed-weight loop meets the `matrix[:keep] if keep else matrix` quirk (QOPeriods.py:970-974):
    A = periods 30 and 12: after 30 and 12 (6 new rows) come 2, which divides 30, and 12 again, both with
    keep == 0; B = tiled random periods 40 and 10: after 40 the next block (37) reconstructs so little that the test
    stops the loop, so 37's block is fitted once more and appended.  A little noise keeps the residuals above
    rounding level, so that they can be compared at a relative bar."""
    t = np.arange(float(n))
    rng = np.random.default_rng(1)
    a = np.sin(2 * np.pi * t / 30.0) + 0.3 * np.sin(2 * np.pi * t / 12.0 + 0.4)
    b = np.tile(rng.standard_normal(40), n // 40 + 1)[:n] + 0.5 * np.tile(rng.standard_normal(10), n // 10 + 1)[:n]
    a = a + 0.02 * np.random.default_rng(2).standard_normal(n)
    b = b + 0.02 * np.random.default_rng(4).standard_normal(n)
    return np.vstack([a, b])


def test_fixed_weight_restatement_keep_quirk():
    """update_weights=False in the restatement: a period that divides an earlier one or repeats keeps no new row,
    and its block is then fitted with ALL p rows; a stopped loop appends the re-fitted last block."""
    a, b = keep_quirk_rows(900)
    out, res = np_find_periods(a, 4, 1e-3, 2, 300, update_weights=False)
    assert out["blocks"] == [(30, 30), (12, 6), (2, 0), (12, 0)]
    assert out["basis_dictionary"] == {"30": 30, "12": 0, "2": 0}  # the repeat overwrites 12's entry
    assert out["subspaces"].shape == (30 + 6 + 2 + 12, 900) and out["weights"].size == 50
    assert np.array_equal(out["subspaces"][36:38], np_pp(2, 900, None))  # (2, 0): both rows of period 2
    assert np.array_equal(out["subspaces"][38:50], np_pp(12, 900, None))  # (12, 0): all 12 rows
    out, res = np_find_periods(b, 5, 0.1, 2, 300, update_weights=False)
    assert out["blocks"] == [(40, 40), (37, 36), (37, 36)] and list(out["periods"]) == [40]
    assert out["subspaces"].shape == (40 + 36 + 36, 900) and out["basis_dictionary"] == {"40": 40, "37": 36}


def test_restatement_matches_edge_fixture(golden):
    """np_find_periods against the reference's edge cases (tests/golden/qoperiods_edges.npz; the three cases with
    dictionaries of 1700+ rows are left to the generator's oracle check)."""
    g = golden("qoperiods_edges")
    for tag in (str(t) for t in g["tags"]):
        if tag in ("blocks40", "blocks40_t", "blocks70"):
            continue
        num, thresh, lo, hi, trunc, uw = g[f"{tag}_kw"]
        x = g[f"{tag}_x"]
        hi = x.size // 3 if hi < 0 else int(hi)
        out, res = np_find_periods(x, int(num), thresh, int(lo), hi, trunc=bool(trunc), update_weights=bool(uw))
        tol = 1e-4 if x.dtype == np.float32 else 1e-8
        assert np.array_equal(out["periods"], g[f"{tag}_periods"]), tag
        assert list(out["basis_dictionary"].values()) == list(g[f"{tag}_dict_vals"]), tag
        assert out["weights"].size == int(g[f"{tag}_rows"]), tag
        assert rel_err(out["weights"], g[f"{tag}_weights"]) < tol and rel_err(res, g[f"{tag}_residual"]) < tol, tag


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    return _ffi.load()


def test_keep_weights_flag_matches_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    m = re.search(r"#define PH_FLAG_KEEP_WEIGHTS (\d+)u", text)
    assert m and int(m.group(1)) == _ffi.PH_FLAG_KEEP_WEIGHTS == 32
    # a flag bit of its own
    others = (_ffi.PH_FLAG_TRUNC, _ffi.PH_FLAG_ORTH, _ffi.PH_FLAG_SINGLE, _ffi.PH_FLAG_DEVICE, _ffi.PH_FLAG_NOSYNC)
    assert all(_ffi.PH_FLAG_KEEP_WEIGHTS & f == 0 for f in others)


def test_qo_find_periods_null_context_with_new_flags(lib):
    from pyperiod_amd import _ffi

    assert lib.ph_version() == 100
    for flags in (_ffi.PH_FLAG_TRUNC, _ffi.PH_FLAG_KEEP_WEIGHTS, _ffi.PH_FLAG_KEEP_WEIGHTS | _ffi.PH_FLAG_TRUNC):
        rc = lib.ph_qo_find_periods(None, None, _ffi.PH_F64, 1, 64, 2, 0.1, 2, 20, 64, flags,
                                    None, None, None, None, None, None, None)
        assert rc == _ffi.PH_E_ARG


def test_batch_input_is_routed_not_rejected(monkeypatch):
    """A (W, N) ndarray goes to the batch path (the 1-D path raises ValueError for 2-D input).  With a custom test
    function every row runs the 1-D call, and an all-zero row gets the reference's fixed answer there without
    touching the GPU."""
    from pyperiod_amd import QOPeriods

    x = np.zeros((3, 96))
    out = QOPeriods().find_periods(x, num=2, thresh=0.1, test_function=lambda self, a, b: True)
    assert isinstance(out, list) and len(out) == 3
    for bases, res in out:
        assert list(bases["periods"]) == [1] and bases["basis_dictionary"] == {"1": 96}
        assert np.array_equal(res, np.zeros(96)) and bases["subspaces"].shape == (1, 96)
