#!/usr/bin/env python3
"""Batched QOPeriods.find_periods under orthogonal selection (one ph_qo_orth_select and one ph_qo_fit launch per round)
against the loop of 1-D calls on the same rows -- what a (W, N) batch with orthogonalize=True ran before the batched
path existed: per row and round three launches, a dense dictionary, its upload and a host solve -- in one process on
one GPU, and the HIP-event time of k_qo_orth_select for both placements of its window: the default engine (window and
work arrays in LDS while they fit) and an engine created under PH_HBM_WINDOW=1 (window read from HBM / L2, work arrays
in an HBM workspace).

    python tools/qo_orth_bench.py [reps [W [N [loop_rows]]]]        defaults 5, 256, 4096, W

Rows: multi_sinusoid_batch(0, W, N); find_periods(num=4, thresh=0.05), default max_length (N / 3).  The loop is timed on
the first `loop_rows` rows (it costs seconds per row at N = 4096) and compared per row.  Every measurement warms up with
an untimed call; times are wall-clock (batch, loop) or HIP events (kernel), median of the repetitions with their spread.
Only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pyperiod_amd import PeriodEngine, QOPeriods, _ffi, default_engine  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_batch  # noqa: E402

ARGS = [int(a) for a in sys.argv[1:]]
REPS, W, N = (ARGS + [5, 256, 4096][len(ARGS):])[:3]
LOOP_ROWS = min(W, ARGS[3]) if len(ARGS) > 3 else W
KW = dict(num=4, thresh=0.05)


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
qo = QOPeriods(orthogonalize=True)
x = multi_sinusoid_batch(0, W, N)
max_p = N // 3

qo.find_periods(x[0], **KW)
loop = []
for _ in range(max(1, REPS // 2)):
    t0 = time.perf_counter()
    ref = [qo.find_periods(x[w], **KW) for w in range(LOOP_ROWS)]
    loop.append(1e3 * (time.perf_counter() - t0))
loop_row = sorted(loop)[len(loop) // 2] / LOOP_ROWS
print(f"QOORTH W={W} N={N} max_length {max_p}: loop of 1-D calls on {LOOP_ROWS} rows ms {spread(loop)} = {loop_row:.3f} per row", flush=True)
for name, eng in engines:
    module.default_engine = lambda eng=eng: eng
    try:
        plan = eng.plan_info("qo_orth_select", N, (max_p,))[0]
        qo.find_periods(x, **KW)
        batch, kernel, fit = [], [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            got = qo.find_periods(x, **KW)
            batch.append(1e3 * (time.perf_counter() - t0))
        eng.profile(True)
        qo.find_periods(x, **KW)
        names = eng.profile_read()
        eng.profile(False)
        for _ in range(REPS):
            eng.profile(True)
            eng.qo_orth_select(x, max_p)
            kernel += [ms for k, ms in eng.profile_read() if k == "k_qo_orth_select"]
            eng.profile(False)
    finally:
        module.default_engine = default_engine
    same = all(np.array_equal(got[w][0]["periods"], ref[w][0]["periods"]) for w in range(LOOP_ROWS))
    err = max(float(np.max(np.abs(got[w][1] - ref[w][1]))) for w in range(LOOP_ROWS)) / float(np.max(np.abs(x)))
    med = sorted(batch)[len(batch) // 2]
    per_kernel = {}
    for k, ms in names:
        per_kernel.setdefault(k, []).append(ms)
    launches = ", ".join(f"{k} x{len(v)} {sum(v):.3f} ms" for k, v in per_kernel.items())
    print(f"QOORTH   engine {name}: window in {place[plan.window]}, block {plan.block}, LDS {plan.lds_bytes} B; batch call ms {spread(batch)} "
          f"= {med / W:.3f} per row; loop / batch per row = {loop_row / (med / W):.1f}; k_qo_orth_select (first round, {W} rows) ms "
          f"{spread(kernel)}; launches of one call: {launches}; periods equal to the loop's: {same}; largest residual difference {err:.1e}",
          flush=True)
for _, eng in engines[1:]:
    eng.close()
