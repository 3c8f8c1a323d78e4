#!/usr/bin/env python3
"""Batched QOPeriods.compute_reconstruction under an analysis window (one ph_qo_fit_win launch) against the loop of
1-D calls it replaces (dense dictionary, rocBLAS products, host solve per row), in one process on one GPU, and the
HIP-event time of k_qo_fit_win -- for both placements of its staging vector u: the default engine (u in LDS while it
fits) and an engine created under PH_HBM_WINDOW=1 (u in an HBM workspace).

    python tools/qo_window_bench.py [reps]

Shapes: multi_sinusoid_batch(0, W, N) under np.hanning(N)
    W = 256, N = 1024,  periods [4, 6, 9, 100]      (110 dictionary rows)
    W = 256, N = 4096,  periods [96, 64, 100, 81]   (302 rows)
    W = 64,  N = 16384, periods [7, 12, 100]        (114 rows; past the N at which u leaves the LDS at kcap 512)
Every measurement warms up with untimed calls; times are wall-clock (batch, loop) or HIP events (kernel), median of the
repetitions with their spread.  Only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pyperiod_amd import PeriodEngine, QOPeriods, _ffi, default_engine  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_batch  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = ((256, 1024, [4, 6, 9, 100]), (256, 4096, [96, 64, 100, 81]), (64, 16384, [7, 12, 100]))


def spread(v):
    v = sorted(v)
    return "median %.3f min %.3f max %.3f (n=%d)" % (v[len(v) // 2], v[0], v[-1], len(v))


def hbm_engine():
    old = os.environ.get("PH_HBM_WINDOW")
    os.environ["PH_HBM_WINDOW"] = "1"
    try:
        return PeriodEngine(0)
    finally:
        if old is None:
            del os.environ["PH_HBM_WINDOW"]
        else:
            os.environ["PH_HBM_WINDOW"] = old


engines = (("default", default_engine()), ("PH_HBM_WINDOW=1", hbm_engine()))
module = sys.modules["pyperiod_amd.QOPeriods"]
place = {_ffi.PH_PLAN_LDS: "LDS", _ffi.PH_PLAN_HBM: "HBM"}
qo = QOPeriods()
for W, N, periods in SHAPES:
    x = multi_sinusoid_batch(0, W, N)
    win = np.hanning(N)
    # the loop of 1-D calls: what a batch with a window ran before the batched path existed
    for w in range(min(W, 4)):
        qo.compute_reconstruction(x[w], periods, "solve", win)
    loop = []
    for _ in range(max(1, REPS // 2)):
        t0 = time.perf_counter()
        ref = [qo.compute_reconstruction(x[w], periods, "solve", win) for w in range(W)]
        loop.append(1e3 * (time.perf_counter() - t0))
    rows = ref[0][1]["weights"].size
    print(f"QOWIN W={W} N={N} periods {periods} ({rows} rows): loop of 1-D calls ms {spread(loop)}", flush=True)
    for name, eng in engines:
        module.default_engine = lambda eng=eng: eng
        try:
            plan = eng.plan_info("qo_fit_win", N, (512, max(periods)))[0]
            qo.compute_reconstruction(x, periods, "solve", win)
            batch, kernel = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                got = qo.compute_reconstruction(x, periods, "solve", win)
                batch.append(1e3 * (time.perf_counter() - t0))
            for _ in range(REPS):
                eng.profile(True)
                eng.qo_fit(x, periods, kcap=512, window=win)
                kernel += [ms for k, ms in eng.profile_read() if k == "k_qo_fit_win"]
                eng.profile(False)
        finally:
            module.default_engine = default_engine
        err = max(float(np.max(np.abs(got[w][0] - ref[w][0]))) for w in range(W)) / float(np.max(np.abs(x)))
        med = sorted(batch)[len(batch) // 2]
        print(f"QOWIN   engine {name}: u in {place[plan.second]}, block {plan.block}, LDS {plan.lds_bytes} B; batch call ms {spread(batch)}; "
              f"k_qo_fit_win ms {spread(kernel)}; loop / batch = {sorted(loop)[len(loop) // 2] / med:.1f}; "
              f"largest reconstruction difference to the loop {err:.1e}", flush=True)
for _, eng in engines[1:]:
    eng.close()
