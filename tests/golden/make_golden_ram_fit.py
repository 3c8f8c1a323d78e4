#!/usr/bin/env python3
"""Generate tests/golden/ramanujan_fit.npz: the *reference* RamanujanPeriods.find_periods_with_weights
(RamanujanPeriods.py:88-122) on two seeded batches, row by row.  Same reference setup as make_golden.py with its
shims 1 (``builtins.Any``), 4a (``_k = 0``) and 4b (``solve_quadratic``'s pair in the order :109 expects); build
container only: the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ram_fit.py

  batch A: multi_sinusoid_window(seed, 1024), 32 windows, min_length=2, max_length=128, thresh=0.2
  batch B: multi_sinusoid_window(seed, 600),   8 windows, min_length=3, max_length=150, thresh=0.1

Per window: the seed, the reference's full norms row, periods, dictionary keys / values, weights, residual, and two
numbers the tests use as CONDITIONS: cond(A A^T) of the reference's dictionary and the selection margin
min_q |norms[q] / max - thresh| / thresh.  A window whose margin is below 1e-3 is replaced by the next unused seed (the
reference accumulates its norms in float32, about 1e-5 relative away from the fp64 folded form: with that margin the
selection cannot flip).  Subspaces are not stored (the file stays below the largest fixture committed).
Only data (inputs + the reference's outputs) is stored; no reference source.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import period_oracle as po  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

BATCHES = (
    ("A", 32, 1024, dict(min_length=2, max_length=128, thresh=0.2)),
    ("B", 8, 600, dict(min_length=3, max_length=150, thresh=0.1)),
)
MARGIN = 1e-3
COND_CUT = 1e7


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    QOP = qo_mod.QOPeriods
    ram = ram_mod.RamanujanPeriods()
    ram._k = 0  # shim 4a
    ram._window = False
    ram.solve_quadratic = lambda x, a: QOP.solve_quadratic(x, a)[::-1]  # shim 4b: order expected at :109
    seen = {}
    find = ram.find_periods

    def find_and_keep(*a, **k):  # the full norms row (the output dict only keeps norms[periods])
        seen["norms"] = find(*a, **k)
        return seen["norms"]

    ram.find_periods = find_and_keep
    out = {}
    for tag, count, n, kw in BATCHES:
        seeds, margins, conds, rows = [], [], [], []
        seed = 0
        while len(seeds) < count:
            sig = multi_sinusoid_window(seed, n)
            res_out, res = ram.find_periods_with_weights(sig, **kw)
            norms = np.asarray(seen["norms"], dtype=np.float64)
            ratio = norms / np.abs(np.max(norms))
            margin = float(np.min(np.abs(ratio - kw["thresh"])) / kw["thresh"])
            seed += 1
            if margin < MARGIN:
                print(f"{tag}: seed {seed - 1} skipped, selection margin {margin:.2e}")
                continue
            w = len(seeds)
            periods = np.asarray(res_out["periods"])
            # the oracle's fp64 folded norms select the same periods
            o_out, _ = po.ramanujan_find_periods_with_weights(sig, **kw)
            assert np.array_equal(o_out["periods"], periods), (tag, seed - 1, periods, o_out["periods"])
            a = np.asarray(res_out["subspaces"])
            cond = float(np.linalg.cond(a @ a.T))
            out[f"{tag}{w}_norms"] = norms
            out[f"{tag}{w}_periods"] = periods
            out[f"{tag}{w}_dict_keys"] = np.array([int(k) for k in res_out["basis_dictionary"].keys()])
            out[f"{tag}{w}_dict_vals"] = np.array([int(v) for v in res_out["basis_dictionary"].values()])
            out[f"{tag}{w}_weights"] = np.asarray(res_out["weights"])
            out[f"{tag}{w}_residual"] = np.asarray(res)
            seeds.append(seed - 1)
            margins.append(margin)
            conds.append(cond)
            rows.append(a.shape[0])
            print(f"{tag}{w}: seed {seed - 1} periods {periods.size} rows {a.shape[0]} cond {cond:.2e} margin {margin:.2e}", flush=True)
        out[f"{tag}_seeds"] = np.array(seeds)
        out[f"{tag}_margin"] = np.array(margins)
        out[f"{tag}_cond"] = np.array(conds)
        out[f"{tag}_rows"] = np.array(rows)
        out[f"{tag}_kw"] = np.array([n, kw["min_length"], kw["max_length"], kw["thresh"]], dtype=np.float64)
        good = int(np.sum((np.array(conds) <= COND_CUT) & (np.array(rows) <= 2048)))
        print(f"{tag}: min margin {min(margins):.2e}, {good} of {count} windows with cond <= {COND_CUT:g} and <= 2048 rows")
        assert min(margins) >= MARGIN
        assert good >= (28 if tag == "A" else 5), (tag, good)
    path = os.path.join(HERE, "ramanujan_fit.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 772 * 1024


if __name__ == "__main__":
    main()
