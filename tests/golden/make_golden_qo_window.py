#!/usr/bin/env python3
"""Generate tests/golden/qo_window.npz: the *reference* QOPeriods under an analysis window -- compute_reconstruction(x,
periods, type="solve", window=win) and find_periods with ``_window`` set (solve_quadratic's windowed branch,
QOPeriods.py:779-796).  Same reference setup as make_golden.py (``load_reference``, ``make_qo``); build container only:
the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qo_window.py

  fit cases ("fit<k>_*"): x = multi_sinusoid_window(seed, N); per case N, seed, the window, the period list and the
    reference's weights, reconstruction, dictionary keys / values and cond of its windowed Gram matrix
      N = 36, 600, 1024 x np.hanning(N), np.hamming(N) x the lists of LISTS[N]
      N = 600 x np.hanning(N) - 0.2 (negative at the ends; the reference still solves it) x LISTS[600]
      N = 1024, np.hanning(N), [128, 64]: the second block has no rows, the reference returns None ("fit<k>_none" = 1)
  find_periods ("fp<k>_*"): N = 600, _window = np.hanning(600), 8 seeds, num=4, thresh=0.05, min_length=2,
    max_length=100; per row the seed, periods, norms, dictionary, weights, residual, cond of the last windowed Gram
    matrix and the relative gap between the best and second-best gamma norm of every round.  A seed whose smallest gap
    is below 1e-6, or whose run meets a block without rows, is replaced by the next seed.

Every stored non-singular case has cond <= 1e7 (asserted).  Subspaces are stored as the dictionary (keys, values): the
rows are rebuilt from it.  Only data (inputs + the reference's outputs) is stored; no reference source.
"""

import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference, make_qo  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import period_oracle as po  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

LISTS = {
    36: ([2, 3], [4, 6], [5, 7, 12]),
    600: ([7, 12], [5, 6, 10, 30], [64, 96], [3, 9, 27], [13, 17, 19, 23]),
    1024: ([4, 6, 9, 100], [96, 64, 100, 81]),
}
WINDOWS = {"hanning": np.hanning, "hamming": np.hamming, "hanning_m02": lambda n: np.hanning(n) - 0.2}
WINDOW_CODES = {"hanning": 0, "hamming": 1, "hanning_m02": 2}
FP_KW = dict(num=4, thresh=0.05, min_length=2, max_length=100)
FP_N, FP_ROWS = 600, 8
GAP = 1e-6
COND_CUT = 1e7


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    out = {}
    cases = [(n, name, lst) for n in (36, 600, 1024) for name in ("hanning", "hamming") for lst in LISTS[n]]
    cases += [(600, "hanning_m02", lst) for lst in LISTS[600]]
    cases += [(1024, "hanning", [128, 64])]
    for k, (n, name, lst) in enumerate(cases):
        seed = k
        x = multi_sinusoid_window(seed, n)
        win = WINDOWS[name](n)
        with contextlib.redirect_stdout(io.StringIO()):
            got = qo.compute_reconstruction(x, lst, type="solve", window=win)
        out[f"fit{k}_case"] = np.array([n, seed, WINDOW_CODES[name]], dtype=np.int64)
        out[f"fit{k}_periods"] = np.array(lst, dtype=np.int64)
        out[f"fit{k}_none"] = np.int64(got is None)
        if got is None:
            print(f"fit{k}: N={n} {name} {lst}: the reference returns None")
            continue
        recon, bases = got
        a = np.asarray(bases["subspaces"], dtype=np.float64)
        dims = bases["basis_dictionary"]
        rows, odims = po.qo_get_subspaces(lst, n)
        assert np.array_equal(rows, a) and {str(q): v for q, v in odims.items()} == {str(q): v for q, v in dims.items()}, k
        cond = float(np.linalg.cond((a * win) @ a.T))
        assert cond <= COND_CUT, (k, cond)
        out[f"fit{k}_weights"] = np.asarray(bases["weights"], dtype=np.float64)
        out[f"fit{k}_recon"] = np.asarray(recon, dtype=np.float64)
        out[f"fit{k}_dict_keys"] = np.array([int(q) for q in dims.keys()])
        out[f"fit{k}_dict_vals"] = np.array([int(v) for v in dims.values()])
        out[f"fit{k}_cond"] = np.float64(cond)
        print(f"fit{k}: N={n} {name} {lst}: rows {a.shape[0]} cond {cond:.3g}", flush=True)
    out["fit_count"] = np.int64(len(cases))

    # ---- find_periods under the window: the gamma norms of every round are taken off periodic_norm as the reference
    #      calls it (one call per candidate period and round, QOPeriods.py:470-478)
    win = np.hanning(FP_N)
    qo._window = win
    seen = []
    norm = qo.periodic_norm
    zero_rows = []
    subspaces = qo.get_subspaces

    def norm_and_keep(*a, **k):
        seen.append(float(norm(*a, **k)))
        return seen[-1]

    def subspaces_and_check(*a, **k):
        got = subspaces(*a, **k)
        zero_rows.append(any(int(v) == 0 for v in got[1].values()))
        return got

    qo.periodic_norm = norm_and_keep
    qo.get_subspaces = subspaces_and_check
    n_cand = FP_KW["max_length"] - FP_KW["min_length"] + 1
    seed, w = 0, 0
    while w < FP_ROWS:
        x = multi_sinusoid_window(seed, FP_N)
        del seen[:], zero_rows[:]
        with contextlib.redirect_stdout(io.StringIO()):
            bases, res = qo.find_periods(x, **FP_KW)
        seed += 1
        assert len(seen) % n_cand == 0
        rounds = np.array(seen).reshape(-1, n_cand)
        top = np.sort(rounds, axis=1)[:, ::-1]
        gaps = (top[:, 0] - top[:, 1]) / top[:, 0]
        if any(zero_rows):
            print(f"fp: seed {seed - 1} skipped, a block without rows")
            continue
        if gaps.min() < GAP:
            print(f"fp: seed {seed - 1} skipped, smallest gap {gaps.min():.2e}")
            continue
        a = np.asarray(bases["subspaces"], dtype=np.float64)
        cond = float(np.linalg.cond((a * win) @ a.T))
        assert cond <= COND_CUT, (seed - 1, cond)
        dims = bases["basis_dictionary"]
        out[f"fp{w}_periods"] = np.asarray(bases["periods"], dtype=np.int64)
        out[f"fp{w}_norms"] = np.asarray(bases["norms"], dtype=np.float64)
        out[f"fp{w}_weights"] = np.asarray(bases["weights"], dtype=np.float64)
        out[f"fp{w}_dict_keys"] = np.array([int(q) for q in dims.keys()])
        out[f"fp{w}_dict_vals"] = np.array([int(v) for v in dims.values()])
        out[f"fp{w}_residual"] = np.asarray(res, dtype=np.float64)
        out[f"fp{w}_gaps"] = gaps
        out[f"fp{w}_cond"] = np.float64(cond)
        out[f"fp{w}_seed"] = np.int64(seed - 1)
        print(f"fp{w}: seed {seed - 1} periods {out[f'fp{w}_periods']} dict {dict(dims)} cond {cond:.3g} min gap {gaps.min():.2e}", flush=True)
        w += 1
    out["fp_kw"] = np.array([FP_N, FP_KW["num"], FP_KW["thresh"], FP_KW["min_length"], FP_KW["max_length"]], dtype=np.float64)
    path = os.path.join(HERE, "qo_window.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "qo_window.npz")
    assert os.path.getsize(path) < largest


if __name__ == "__main__":
    main()
