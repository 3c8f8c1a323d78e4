"""tests/golden/qo_window.npz (the reference's QOPeriods under an analysis window) checked on the CPU: every stored set
of weights is the numpy solve of (A diag(win)) A^T w = (A diag(win)) x on the oracle's dictionary rows, and the file
holds data only."""

import numpy as np

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

WINDOWS = (np.hanning, np.hamming, lambda n: np.hanning(n) - 0.2)  # fit<k>_case[2]


def fit_case(g, k):
    """-> (x, window, period list, None or dict(weights, recon, dict_keys, dict_vals, cond)) of fit case k."""
    n, seed, code = (int(v) for v in g[f"fit{k}_case"])
    want = None
    if not int(g[f"fit{k}_none"]):
        want = {name: g[f"fit{k}_{name}"] for name in ("weights", "recon", "dict_keys", "dict_vals", "cond")}
    return multi_sinusoid_window(seed, n), WINDOWS[code](n), [int(p) for p in g[f"fit{k}_periods"]], want


def windowed_solve(x, win, rows):
    w = np.linalg.solve((rows * win) @ rows.T, (rows * win) @ x)
    return w, rows.T @ w


def test_fit_weights_are_the_windowed_solve(golden):
    g = golden("qo_window")
    count = int(g["fit_count"])
    assert count == 26
    singular = 0
    for k in range(count):
        x, win, lst, want = fit_case(g, k)
        rows, dims = po.qo_get_subspaces(lst, x.size)
        if want is None:
            singular += 1
            assert 0 in dims.values()  # a block without rows: the reference's Pp hands back all p rows
            continue
        assert [int(q) for q in dims] == list(want["dict_keys"]) and list(dims.values()) == list(want["dict_vals"])
        assert float(want["cond"]) <= 1e7
        w, recon = windowed_solve(x, win, rows)
        scale = np.max(np.abs(want["weights"]))
        assert np.max(np.abs(w - want["weights"])) <= 1e-10 * scale, k
        assert np.max(np.abs(recon - want["recon"])) <= 1e-10 * np.max(np.abs(want["recon"])), k
    assert singular == 1


def test_find_periods_weights_are_the_windowed_solve(golden):
    g = golden("qo_window")
    n, num, thresh, lo, hi = g["fp_kw"]
    n = int(n)
    win = np.hanning(n)
    for w in range(8):
        x = multi_sinusoid_window(int(g[f"fp{w}_seed"]), n)
        keys, vals = g[f"fp{w}_dict_keys"], g[f"fp{w}_dict_vals"]
        rows, dims = po.qo_get_subspaces([int(q) for q in keys], n)
        assert list(dims.values()) == list(vals) and 0 not in vals
        wts, recon = windowed_solve(x, win, rows)
        assert np.max(np.abs(wts - g[f"fp{w}_weights"])) <= 1e-10 * np.max(np.abs(g[f"fp{w}_weights"])), w
        assert np.max(np.abs((x - recon) - g[f"fp{w}_residual"])) <= 1e-10 * np.max(np.abs(x)), w
        assert g[f"fp{w}_gaps"].min() >= 1e-6 and float(g[f"fp{w}_cond"]) <= 1e7
        periods = g[f"fp{w}_periods"]
        assert periods.size <= int(num) and np.all((periods >= lo) & (periods <= hi))
        assert list(periods) == list(keys[: periods.size])


def test_fixture_holds_data_only(golden):
    g = golden("qo_window")
    fit = {"case", "periods", "none", "weights", "recon", "dict_keys", "dict_vals", "cond"}
    fp = {"periods", "norms", "weights", "dict_keys", "dict_vals", "residual", "gaps", "cond", "seed"}
    for key, arr in g.items():
        assert arr.dtype.kind in "fi", key  # numbers: no strings, objects or pickles
        if key in ("fit_count", "fp_kw"):
            continue
        head, _, name = key.partition("_")
        if head.startswith("fit"):
            assert head[3:].isdigit() and int(head[3:]) < 26 and name in fit, key
        else:
            assert head.startswith("fp") and head[2:].isdigit() and int(head[2:]) < 8 and name in fp, key
