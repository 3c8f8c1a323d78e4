#!/usr/bin/env python3
"""A/B of the shared-load pass of m_best step 1 in one process on one box: the window-pair screen with one pass per
period (PH_PAIR_DUO=0) against the plan that folds p and p + 64 from one set of LDS reads (default).  Config 2 batch,
alternating rounds, plain m_best and m_best_gamma, both variants' outputs compared, kernel times from the library's HIP
events.  The gain counts only if the difference of the means exceeds three times the largest spread (max - min of the
round means) of either variant."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import __graft_entry__ as ge

ge.build()
from pyperiod_amd import PeriodEngine
from pyperiod_amd.synth import multi_sinusoid_batch

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
REPS, ROUNDS = 10, 5
x = torch.from_numpy(multi_sinusoid_batch(0, W, N)).cuda()
eng = {}
for name, env in (("single", "0"), ("duo", "1")):
    os.environ["PH_PAIR_DUO"] = env
    eng[name] = PeriodEngine(0)
    for gamma in (False, True):
        print(name, f"gamma={gamma}: plan entries, periods screened, LDS elements per sweep:", eng[name].m_best_screen_info(N, 10, gamma=gamma))
del os.environ["PH_PAIR_DUO"]
res, k1s, k2s = {}, {}, {}
for rnd in range(ROUNDS):
    for name in ("single", "duo"):
        e = eng[name]
        for gamma in (False, True):
            out = e.m_best(x, 10, None, 2, gamma, want_sweeps=True)
            torch.cuda.synchronize()
            e.profile(True)
            t0 = time.perf_counter()
            for _ in range(REPS):
                out = e.m_best(x, 10, None, 2, gamma, want_sweeps=True)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / REPS * 1e3
            prof = e.profile_read()
            e.profile(False)
            k1 = [ms for nm, ms in prof if nm == "k_mbest_step1"]
            k2 = [ms for nm, ms in prof if nm == "k_mbest_step2"]
            res[(name, gamma)] = [o.cpu().numpy() for o in out]
            k1s.setdefault((name, gamma), []).append(float(np.mean(k1)))
            k2s.setdefault((name, gamma), []).append(float(np.mean(k2)))
            print(f"round {rnd} {name:6s} gamma={gamma!s:5s} step1 {np.mean(k1):.4f} ms (min {np.min(k1):.4f})  step2 {np.mean(k2):.4f} ms  "
                  f"wall {wall:.3f} ms  sweeps {res[(name, gamma)][4].sum()}", flush=True)
for gamma in (False, True):
    a, b = res[("single", gamma)], res[("duo", gamma)]
    bad = np.nonzero((a[0] != b[0]).any(axis=1))[0]
    dpow = np.max(np.abs(a[1] - b[1]) / np.maximum(np.abs(a[1]), 1e-300))
    print(f"gamma={gamma}: periods equal {np.array_equal(a[0], b[0])} (windows differing: {bad[:10].tolist()}), powers rel {dpow:.2e}, "
          f"bases identical {np.array_equal(a[2], b[2])}, status {np.array_equal(a[3], b[3])}, sweeps equal {np.array_equal(a[4], b[4])}")
    s, d = np.array(k1s[("single", gamma)]), np.array(k1s[("duo", gamma)])
    spread = max(s.max() - s.min(), d.max() - d.min())
    diff = s.mean() - d.mean()
    print(f"gamma={gamma}: step 1 single {s.mean():.4f} ms (spread {s.max() - s.min():.4f}), duo {d.mean():.4f} ms (spread {d.max() - d.min():.4f}): "
          f"{s.mean() / d.mean():.3f} x, difference {diff:.4f} ms = {diff / spread if spread > 0 else float('inf'):.1f} spreads "
          f"({'counts' if diff > 3 * spread else 'inside the noise'}); step 2 {np.mean(k2s[('single', gamma)]):.4f} / {np.mean(k2s[('duo', gamma)]):.4f} ms")
for e in eng.values():
    e.close()
