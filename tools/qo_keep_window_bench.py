#!/usr/bin/env python3
"""Batched QOPeriods.find_periods(update_weights=False) under an analysis window (one ph_qo_greedy_win launch per batch)
against the loop of 1-D calls on the same rows -- what such a (W, N) batch ran before the batched path existed: per row
and round one ph_sweep, two ph_fold_sums (one of them on the dense block times the window), a host solve and one
ph_tile_sum -- in one process on one GPU, and the HIP-event time of k_qo_greedy_win by placement of its residual: the
default engine (residual in LDS while it fits) and an engine created under PH_HBM_WINDOW=1 (residual in the HBM
workspace).  The analysis window itself is read through L2 in both.

    python tools/qo_keep_window_bench.py [reps [loop_rows]]        defaults 5, 16

Shapes, rows multi_sinusoid_batch(0, W, N) under np.hanning(N):
    W = 1024, N = 16384, float32, num=3, thresh=0.1, periods 8 .. 300     (bench.py's config-5 batch)
    W = 64,   N = 4096,  float64, num=4, thresh=0.05, periods 2 .. 1365
The loop is timed on the first `loop_rows` rows and compared per row.  Every measurement warms up with an untimed call
(the first batch call also brings the clock up); times are wall-clock (batch, loop) or HIP events (kernel), median of the
repetitions with their spread.  Only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pyperiod_amd import PeriodEngine, QOPeriods, _ffi, default_engine  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_batch  # noqa: E402

ARGS = [int(a) for a in sys.argv[1:]]
REPS, LOOP_ROWS = (ARGS + [5, 16][len(ARGS):])[:2]
SHAPES = (
    (1024, 16384, np.float32, dict(num=3, thresh=0.1, min_length=8, max_length=300)),
    (64, 4096, np.float64, dict(num=4, thresh=0.05, min_length=2, max_length=1365)),
)


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
place = {_ffi.PH_QO_LDS_OVERLAY: "LDS", _ffi.PH_QO_LDS_BEHIND: "LDS", _ffi.PH_QO_HBM: "HBM"}
for W, N, dtype, kw in SHAPES:
    x = multi_sinusoid_batch(0, W, N, dtype=dtype)
    qo = QOPeriods()
    qo.window = np.hanning(N)
    rows = min(W, LOOP_ROWS)
    kcap = min(4096, -(-kw["num"] * kw["max_length"] // 64) * 64)
    # the loop of 1-D calls: what a batch with these settings ran before the batched path existed
    qo.find_periods(x[0], update_weights=False, **kw)
    loop = []
    for _ in range(max(1, REPS // 2)):
        t0 = time.perf_counter()
        ref = [qo.find_periods(x[w], update_weights=False, **kw) for w in range(rows)]
        loop.append(1e3 * (time.perf_counter() - t0))
    loop_row = sorted(loop)[len(loop) // 2] / rows
    print(f"QOKEEPWIN W={W} N={N} {np.dtype(dtype).name} {kw}: loop of 1-D calls on {rows} rows ms {spread(loop)} = {loop_row:.3f} per row",
          flush=True)
    for name, eng in engines:
        module.default_engine = lambda eng=eng: eng
        try:
            where, lds = eng.qo_plan_info(N, dtype, kcap, kw["max_length"], update_weights=False)
            qo.find_periods(x, update_weights=False, **kw)
            batch, kernel = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                got = qo.find_periods(x, update_weights=False, **kw)
                batch.append(1e3 * (time.perf_counter() - t0))
            for _ in range(REPS):
                eng.profile(True)
                st = eng.qo_find_periods(x, kw["num"], kw["thresh"], kw["min_length"], kw["max_length"], kcap,
                                         update_weights=False, window=qo.window)[6]
                kernel += [ms for k, ms in eng.profile_read() if k == "k_qo_greedy_win"]
                eng.profile(False)
        finally:
            module.default_engine = default_engine
        same = all(np.array_equal(got[w][0]["periods"], ref[w][0]["periods"]) for w in range(rows))
        err = max(float(np.max(np.abs(got[w][1] - ref[w][1]))) for w in range(rows)) / float(np.max(np.abs(x)))
        med = sorted(batch)[len(batch) // 2]
        print(f"QOKEEPWIN   engine {name}: residual in {place[where]}, LDS {lds} B; batch call ms {spread(batch)} = {med / W:.3f} per row; "
              f"loop / batch per row = {loop_row / (med / W):.1f}; k_qo_greedy_win ({W} rows) ms {spread(kernel)}; rows handed back "
              f"{int(np.count_nonzero(st))}; periods equal to the loop's: {same}; largest residual difference {err:.1e}", flush=True)
for _, eng in engines[1:]:
    eng.close()
