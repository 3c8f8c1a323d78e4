#!/usr/bin/env python3
"""Generate tests/golden/follow.npz: the *reference* Periods.project(..., return_single_period=True) peeled T deep on a
handful of frames, the way ph_follow peels it.  Same reference setup as make_golden.py (``load_reference``).  Build
container only: the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_follow.py

Per case "c<k>_*": frame (N,) float64 -- already rounded through float32 for the float32 cases --, periods (T,), trunc,
seg (sum p,) the concatenated single periods, residual (N,) what is left after the last subtraction, and norms (T + 1,)
the reference's periodic_norm of the residual before every block and after the last.  Only data is stored."""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from follow_cases import _signal, _window  # noqa: E402

# N, periods, float32-rounded frame
CASES = ((37, (5, 9, 37), False), (37, (36, 2, 1), True), (64, (64, 16, 3), False), (130, (63, 64, 65), False),
         (130, (65, 13, 10), True), (48, (47, 16, 3), True), (200, (23, 100, 199), False), (128, (24, 25, 7, 50), False))


def main():
    warnings.simplefilter("ignore")
    per_mod, _, _ = load_reference()
    P = per_mod.Periods
    out = {}
    k = 0
    for N, periods, f32 in CASES:
        frame = _signal(N, N, np.float64) * _window(N)
        if f32:
            frame = frame.astype(np.float32).astype(np.float64)
        for trunc in (False, True):
            r = frame.copy()
            segs, norms = [], [P.periodic_norm(r)]
            for p in periods:
                s = P.project(r, p, trunc, False, return_single_period=True)
                base = P.project(r, p, trunc, False)
                assert np.array_equal(base, np.tile(s, N // p + 1)[:N])
                r = r - base  # Periods.py:277
                segs.append(np.asarray(s, dtype=np.float64))
                norms.append(P.periodic_norm(r))
            out[f"c{k}_frame"] = frame
            out[f"c{k}_periods"] = np.array(periods, dtype=np.int32)
            out[f"c{k}_trunc"] = np.bool_(trunc)
            out[f"c{k}_seg"] = np.concatenate(segs)
            out[f"c{k}_residual"] = r
            out[f"c{k}_norms"] = np.array(norms, dtype=np.float64)
            k += 1
    out["count"] = np.int64(k)
    path = os.path.join(HERE, "follow.npz")
    np.savez_compressed(path, **out)
    print(k, "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
