#!/usr/bin/env python3
"""Generate tests/golden/qoperiods_trunc.npz: the *reference* QOPeriods.find_periods (plain branch,
update_weights=True) with trunc_to_integer_multiple=True, on seeded inputs.  Same reference setup and
shims as make_golden.py (build container only; the .npz travels, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trunc.py

Only data (inputs + the reference's outputs) is stored; no reference source.
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

from make_golden import load_reference, make_qo  # noqa: E402

from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

# (tag, window seed, N, find_periods keywords): N is not a multiple of most candidate periods, so the
# trunc means (complete rows only, Periods.py:178-184) differ from the plain ones
CASES = (
    ("w5", 5, 1537, dict(num=4, thresh=0.2, min_length=4, max_length=200)),
    ("w9", 9, 1000, dict(num=3, thresh=0.05, min_length=2, max_length=120)),
)


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    qo._trunc_to_integer_multiple = True
    out = {}
    for tag, seed, n, kw in CASES:
        sig = multi_sinusoid_window(seed, n)
        with contextlib.redirect_stdout(io.StringIO()):  # QOPeriods.py:488 prints unconditionally
            res_out, res = qo.find_periods(sig, **kw)
        out[f"{tag}_x"] = sig
        out[f"{tag}_kw"] = np.array([kw["num"], kw["thresh"], kw["min_length"], kw["max_length"]], dtype=np.float64)
        out[f"{tag}_periods"] = np.asarray(res_out["periods"])
        out[f"{tag}_norms"] = np.asarray(res_out["norms"])
        out[f"{tag}_weights"] = np.asarray(res_out["weights"])
        out[f"{tag}_dict_keys"] = np.array([int(k) for k in res_out["basis_dictionary"].keys()])
        out[f"{tag}_dict_vals"] = np.array([int(v) for v in res_out["basis_dictionary"].values()])
        out[f"{tag}_residual"] = res
        print(tag, out[f"{tag}_periods"], out[f"{tag}_dict_vals"])
    np.savez_compressed(os.path.join(HERE, "qoperiods_trunc.npz"), **out)


if __name__ == "__main__":
    main()
