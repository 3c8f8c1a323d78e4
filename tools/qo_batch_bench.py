#!/usr/bin/env python3
"""Batched QOPeriods.find_periods on one GPU: the class batch call against a loop of 1-D calls for the default,
update_weights=False and trunc variants (256 x 4096 fp64, num=4), and the class call at config 5 (1024 x 16384
fp32, num=3, thresh=0.1, min_length=8, max_length=300) against the bare eng.qo_find_periods call on the same
numpy array.  Wall-clock seconds (best of --reps after one warm-up call); prints one JSON line.

    python tools/qo_batch_bench.py [--reps 3] [--loop-rows 32]

The 1-D loops are slow (the host-driven loop for trunc / update_weights=False): they time --loop-rows rows and
the per-row time is scaled to the 256 rows of the batch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from pyperiod_amd import QOPeriods, default_engine  # noqa: E402
from pyperiod_amd.QOPeriods import _to_f64  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_batch  # noqa: E402


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-rows", type=int, default=32)
    a = ap.parse_args()
    eng = default_engine()
    out = {}
    x = multi_sinusoid_batch(0, 256, 4096)
    kw = dict(num=4, thresh=0.1)
    for name, trunc, uw in (("default", False, True), ("update_weights_false", False, False), ("trunc", True, True),
                            ("trunc_update_weights_false", True, False)):
        qo = QOPeriods(trunc_to_integer_multiple=trunc)
        t_batch = best(lambda: qo.find_periods(x, update_weights=uw, **kw), a.reps)
        rows = x[: a.loop_rows]
        t_loop = best(lambda: [qo.find_periods(r, update_weights=uw, **kw) for r in rows], 1) * x.shape[0] / rows.shape[0]
        out[name] = {"batch_s": round(t_batch, 5), "loop_s": round(t_loop, 4), "speedup": round(t_loop / t_batch, 1)}
    xb = multi_sinusoid_batch(0, 1024, 16384, dtype=np.float32)
    qo = QOPeriods()
    t_class = best(lambda: qo.find_periods(xb, num=3, thresh=0.1, min_length=8, max_length=300), a.reps)
    t_bare = best(lambda: eng.qo_find_periods(xb, 3, 0.1, 8, 300, 960), a.reps)
    # what the class adds to the bare call: the float64 copy of the float32 residuals and the per-row results
    resid32 = eng.qo_find_periods(xb, 3, 0.1, 8, 300, 960)[5]
    t_conv = best(lambda: _to_f64(resid32), a.reps)
    eng.profile(True)
    eng.qo_find_periods(xb, 3, 0.1, 8, 300, 960)
    kern = [ms for n, ms in eng.profile_read() if n == "k_qo_find"]
    eng.profile(False)
    out["config5"] = {"class_s": round(t_class, 5), "bare_s": round(t_bare, 5), "ratio": round(t_class / t_bare, 3),
                      "residual_to_f64_s": round(t_conv, 5), "rest_of_class_s": round(t_class - t_bare - t_conv, 5),
                      "kernel_ms": round(kern[0], 3) if kern else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
