#!/usr/bin/env python3
"""Time QOPeriods.get_periods as a batch on the device (PeriodEngine.qo_get_periods, kernel k_qo_extract) against the
dense route of the reference: one numpy least-squares solve per row on ``stack_pairwise_gcd_subspaces``.

    python tools/qo_get_periods_bench.py [--rows 1024] [--budget 3.0]

Two batches: config-5 like (`--rows` windows of N = 16384, dictionaries from find_periods(num=3, update_weights=False)
with periods up to N / 3 = 5461) and small (N = 600, num=4, max_length=100).  Per batch: kernel time (HIP events around the launch, best of 5) in the default placement and
with the work arrays forced into HBM (PH_HBM_WINDOW=1), and the dense loop on as many rows as finish within `--budget`
seconds, extrapolated to the batch.  Prints one JSON line per batch."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engines():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import PeriodEngine

    lds = PeriodEngine(0)
    old = os.environ.get("PH_HBM_WINDOW")
    os.environ["PH_HBM_WINDOW"] = "1"
    try:
        hbm = PeriodEngine(0)
    finally:
        if old is None:
            del os.environ["PH_HBM_WINDOW"]
        else:
            os.environ["PH_HBM_WINDOW"] = old
    return lds, hbm


def dictionaries(eng, n, rows, num, max_length, update_weights):
    """(periods, rows, counts, weights) of a batched find_periods on `rows` synthetic windows, as the engine returns them.
    update_weights=False (the fixed-weight loop, the only one whose dictionary fits at max_length = N / 3): a keeps
    entry of 0 stands for `period` rows, and rows whose loop picked a period twice are left out."""
    from pyperiod_amd.synth import multi_sinusoid_window

    x = np.stack([multi_sinusoid_window(s, n) for s in range(rows)])
    per, _, keeps, counts, wts, _, st = eng.qo_find_periods(x, num, 0.01, 2, max_length, kcap=num * max_length,
                                                            update_weights=update_weights)
    per, cnt = per.astype(np.int32), np.ascontiguousarray(counts[:, 1])
    keeps = np.where(keeps == 0, per, keeps).astype(np.int32)
    ok = np.array([st[w] == 0 and cnt[w] > 0 and len(set(per[w, : cnt[w]])) == cnt[w] for w in range(rows)])
    return per[ok], keeps[ok], cnt[ok], wts[ok]


def kernel_ms(eng, args, reps=5):
    from pyperiod_amd import _ffi

    best, place = float("inf"), None
    for _ in range(reps):
        eng.profile(True)
        out, st = eng.qo_get_periods(*args)
        prof = eng.profile_read()
        eng.profile(False)
        assert [n for n, _ in prof] == ["k_qo_extract"] and not st.any()
        best = min(best, prof[0][1])
    plan = eng.plan_info("qo_get_periods", out.shape[1], (out.shape[1], int(args[0].max())))[0]
    place = "lds" if plan.window == _ffi.PH_PLAN_LDS else "hbm"
    return best, place, out


def dense_loop(args, out, budget):
    from pyperiod_amd import QOPeriods

    per, rws, cnt, wts = args
    t0, done, worst = time.perf_counter(), 0, 0.0
    for w in range(per.shape[0]):
        keys, vals = per[w, : cnt[w]], rws[w, : cnt[w]]
        c = QOPeriods.concatenate_periods(wts[w], {str(int(q)): int(r) for q, r in zip(keys, vals)})
        a = QOPeriods.stack_pairwise_gcd_subspaces(keys)
        ref = c - a.T @ np.linalg.lstsq(a @ a.T, a @ c, rcond=None)[0]
        worst = max(worst, float(np.max(np.abs(ref - out[w, : c.size]))) / max(1.0, float(np.max(np.abs(ref)))))
        done += 1
        if time.perf_counter() - t0 > budget:
            break
    return (time.perf_counter() - t0) / done, done, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--budget", type=float, default=3.0)
    a = ap.parse_args()
    lds, hbm = engines()
    for name, n, num, max_length, upd in (("config5", 16384, 3, 16384 // 3, False), ("small", 600, 4, 100, True)):
        args = dictionaries(lds, n, a.rows, num, max_length, upd)
        ms_d, place_d, out = kernel_ms(lds, args)
        ms_h, place_h, out_h = kernel_ms(hbm, args)
        assert np.array_equal(out, out_h)
        t0 = time.perf_counter()
        lds.qo_get_periods(*args)
        wall = time.perf_counter() - t0
        per_row, done, worst = dense_loop(args, out, a.budget)
        print(json.dumps({
            "batch": name, "N": n, "rows": int(args[0].shape[0]), "sum_p_max": int(out.shape[1]),
            "kernel_ms": {place_d: round(ms_d, 4), place_h + "_forced": round(ms_h, 4)},
            "host_call_ms": round(1e3 * wall, 3),
            "dense_ms_per_row": round(1e3 * per_row, 3), "dense_rows_timed": done,
            "dense_ms_batch_extrapolated": round(1e3 * per_row * args[0].shape[0], 1),
            "max_rel_diff_vs_dense": worst,
        }), flush=True)


if __name__ == "__main__":
    main()
