#!/usr/bin/env python3
"""Generate tests/golden/qo_get_periods.npz: the *reference* QOPeriods.get_periods (QOPeriods.py:719-741) with its one
broken call repaired.  Same reference setup as make_golden.py (``load_reference``, ``make_qo``) plus one shim: v1 passes
``self._k`` positionally into solve_quadratic's ``type`` (TypeError); the shim drops that stray positional argument and
changes nothing else.  Build container only: the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_get_periods.py

  find_periods cases: the dictionary and weights the reference's own find_periods(num, thresh=0.01, min_length=2,
    max_length) returns on multi_sinusoid_window(seed, N), seeds 0 .. 5:  N = 36 (max_length 12, num 4), N = 240 (40, 5),
    N = 600 (100, 4)
  hand-made cases: the dictionaries of HAND with default_rng(k).standard_normal weights

Per case "c<k>_*": keys, vals (the dictionary in order), weights, n (N, or 0 for a hand-made case), seed, the stacked
matrix of stack_pairwise_gcd_subspaces when sum(p) <= 100, and for each decomp_type t (rr, lu, qr, lstsq) one of
"c<k>_<t>" (the concatenated result), "c<k>_<t>_raised" (the exception's class name) or "c<k>_<t>_singular" (see below).

What the repaired reference does, asserted here:
  - 'lstsq' always returns;
  - 'row reduction' raises LinAlgError exactly on rank-1 matrices (one period, two coprime periods); otherwise it returns
    and agrees with 'lstsq' to 1e-12 (relative to max(1, max |result|));
  - 'lu' and 'qr' hand numpy.linalg.solve the factor of ALL stacked rows.  With one or two periods the rows are
    independent: both return and agree with 'lstsq' to 1e-12.  With three or more periods the rows are always dependent
    and the solve is singular: depending on rounding in LAPACK it raises LinAlgError ('lu' mostly), returns the
    projector's result all the same (the null-space part of the coefficients drops out of the reconstruction; 'qr'
    mostly), or returns a result that is off by up to O(1).  The last kind is not stored as a result: "c<k>_<t>_singular"
    holds its distance from 'lstsq' instead.  Every stored result agrees with 'lstsq' to 1e-12.
Only data is stored.
"""

import contextlib
import io
import os
import sys
import warnings
from math import gcd

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference, make_qo  # noqa: E402

sys.path.insert(0, ROOT)
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

FP = ((36, 12, 4), (240, 40, 5), (600, 100, 4))  # N, max_length, num
SEEDS = range(6)
HAND = ({12: 12}, {6: 6, 35: 34}, {12: 12, 18: 12}, {10: 10, 5: 1}, {12: 12, 18: 12, 8: 4}, {36: 36, 24: 12, 16: 8},
        {1: 1, 7: 6, 14: 7})
TYPES = ("row reduction", "lu", "qr", "lstsq")
NAMES = {"row reduction": "rr", "lu": "lu", "qr": "qr", "lstsq": "lstsq"}


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    solve = qo_mod.QOPeriods.solve_quadratic

    def solve_without_stray_k(x, A, *args, **kw):
        if args and not isinstance(args[0], str):  # the positional self._k
            args = args[1:]
        return solve(x, A, *args, **kw)

    qo.solve_quadratic = solve_without_stray_k
    cases = []
    for n, max_length, num in FP:
        for seed in SEEDS:
            x = multi_sinusoid_window(seed, n)
            with contextlib.redirect_stdout(io.StringIO()):
                bases, _ = qo.find_periods(x, num=num, thresh=0.01, min_length=2, max_length=max_length)
            d = {int(q): int(v) for q, v in bases["basis_dictionary"].items()}
            cases.append((n, seed, d, np.asarray(bases["weights"], dtype=np.float64)))
    for k, d in enumerate(HAND):
        cases.append((0, k, dict(d), np.random.default_rng(k).standard_normal(sum(d.values()))))
    out = {}
    for k, (n, seed, d, wts) in enumerate(cases):
        keys, vals = list(d.keys()), list(d.values())
        dictionary = {str(q): v for q, v in d.items()}
        out[f"c{k}_keys"] = np.array(keys, dtype=np.int64)
        out[f"c{k}_vals"] = np.array(vals, dtype=np.int64)
        out[f"c{k}_weights"] = wts
        out[f"c{k}_n"] = np.int64(n)
        out[f"c{k}_seed"] = np.int64(seed)
        if sum(keys) <= 100:
            out[f"c{k}_matrix"] = np.asarray(qo.stack_pairwise_gcd_subspaces(np.array(keys)), dtype=np.float64)
        got, raised, off = {}, {}, {}
        for t in TYPES:
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    res = qo.get_periods(wts, dictionary, decomp_type=t)
                assert [len(r) for r in res] == keys
                got[t] = np.concatenate([np.asarray(r, dtype=np.float64) for r in res])
            except Exception as exc:  # noqa: BLE001 -- the class name is the datum
                raised[t] = type(exc).__name__
        assert "lstsq" in got, k
        scale = max(1.0, float(np.max(np.abs(got["lstsq"]))))
        for t in list(got):
            dev = float(np.max(np.abs(got[t] - got["lstsq"]))) / scale
            if dev > 1e-12:
                off[t] = dev
                del got[t]
        rank1 = len(keys) == 1 or (len(keys) == 2 and gcd(*keys) == 1)
        dependent = len(keys) >= 3  # the stacked rows are then always linearly dependent
        assert ("row reduction" in raised) == rank1 and "row reduction" not in off, (k, keys)
        assert all(v == "LinAlgError" for v in raised.values()), (k, raised)
        for t in ("lu", "qr"):  # a singular solve when the rows are dependent, a regular one otherwise
            assert t in got or dependent, (k, t)
        for t in TYPES:
            if t in got:
                out[f"c{k}_{NAMES[t]}"] = got[t]
            elif t in raised:
                out[f"c{k}_{NAMES[t]}_raised"] = np.array(raised[t])
            else:
                out[f"c{k}_{NAMES[t]}_singular"] = np.float64(off[t])
        print(f"c{k}: N={n} seed {seed} dict {d}: " + ", ".join(t if t in got else f"{t} RAISED" if t in raised else f"{t} OFF BY {off[t]:.2g}" for t in TYPES), flush=True)
    out["count"] = np.int64(len(cases))
    path = os.path.join(HERE, "qo_get_periods.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "qo_get_periods.npz")
    assert os.path.getsize(path) < largest


if __name__ == "__main__":
    main()
