#!/usr/bin/env python3
"""A/B of the fold-once path of m_best step 1 in one process on one box: the window-pair kernel with the phases behind
its screen as they were (PH_PAIR_FOLD_ONCE=0) against the kernel that folds the residual once at the surviving top
period (default).  Config 2 batch, alternating rounds, both variants' outputs compared bit for bit, kernel times from the
library's HIP events; m_best_gamma alongside (its single listed period takes the path too when it is long).
The spreads printed here are over the rounds of ONE process with warm engines: they show that the switch moves the time,
and do not compare with the 3-spread bar of tools/ab_builds.py, which is set on rounds of fresh processes."""
import os
import sys

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
REPS, ROUNDS = 10, 3
x = torch.from_numpy(multi_sinusoid_batch(0, W, N)).cuda()
eng = {}
for name, env in (("staged", "0"), ("fold", "1")):
    os.environ["PH_PAIR_FOLD_ONCE"] = env
    eng[name] = PeriodEngine(0)
del os.environ["PH_PAIR_FOLD_ONCE"]
res, times = {}, {}
for rnd in range(ROUNDS):
    for name in ("staged", "fold"):
        e = eng[name]
        for gamma in (False, True):
            out = e.m_best(x, 10, None, 2, gamma, want_sweeps=True)
            torch.cuda.synchronize()
            e.profile(True)
            for _ in range(REPS):
                out = e.m_best(x, 10, None, 2, gamma, want_sweeps=True)
            torch.cuda.synchronize()
            prof = e.profile_read()
            e.profile(False)
            k1 = [ms for nm, ms in prof if nm == "k_mbest_step1"]
            k2 = [ms for nm, ms in prof if nm == "k_mbest_step2"]
            res[(name, gamma)] = [o.cpu().numpy() for o in out]
            times.setdefault((name, gamma), []).append(float(np.mean(k1)))
            print(f"round {rnd} {name:6s} gamma={gamma!s:5s} step1 {np.mean(k1):.4f} ms (min {np.min(k1):.4f})  step2 {np.mean(k2):.4f} ms  "
                  f"sweeps {res[(name, gamma)][4].sum()}", flush=True)
for gamma in (False, True):
    a, b = res[("staged", gamma)], res[("fold", gamma)]
    ok = a[3] == 0
    print(f"gamma={gamma}: periods equal {np.array_equal(a[0], b[0])}, powers identical {np.array_equal(a[1][ok], b[1][ok])}, "
          f"bases identical {np.array_equal(a[2][ok], b[2][ok])}, status {np.array_equal(a[3], b[3])}, sweeps equal {np.array_equal(a[4], b[4])}")
    s, d = np.array(times[("staged", gamma)]), np.array(times[("fold", gamma)])
    spread = max(s.max() - s.min(), d.max() - d.min())
    print(f"gamma={gamma}: step 1 staged {s.mean():.4f} ms, fold {d.mean():.4f} ms: {s.mean() / d.mean():.3f} x, "
          f"difference {(s.mean() - d.mean()) / spread if spread > 0 else float('inf'):.1f} spreads")
for e in eng.values():
    e.close()
