#!/usr/bin/env python3
"""A/B of the cover rule of m_best step 1 in one process on one box: the window-pair screen over every period
(PH_PAIR_COVER=0) against the screen of the top half with the divisor list (default).  Config 2 batch, alternating
rounds, both variants' outputs compared, kernel times from the library's HIP events; m_best_gamma (which the
switch must not touch) alongside."""
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
REPS, ROUNDS = 10, 3
x = torch.from_numpy(multi_sinusoid_batch(0, W, N)).cuda()
eng = {}
for name, env in (("full", "0"), ("cover", "1")):
    os.environ["PH_PAIR_COVER"] = env
    eng[name] = PeriodEngine(0)
    print(name, "passes per sweep, periods:", eng[name].m_best_plan_info(N, 10))
del os.environ["PH_PAIR_COVER"]
res = {}
for rnd in range(ROUNDS):
    for name in ("full", "cover"):
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
            print(f"round {rnd} {name:6s} gamma={gamma!s:5s} step1 {np.mean(k1):.3f} ms (min {np.min(k1):.3f})  step2 {np.mean(k2):.3f} ms  "
                  f"wall {wall:.3f} ms  sweeps {res[(name, gamma)][4].sum()}", flush=True)
for gamma in (False, True):
    a, b = res[("full", gamma)], res[("cover", gamma)]
    bad = np.nonzero((a[0] != b[0]).any(axis=1))[0]
    dpow = np.max(np.abs(a[1] - b[1]) / np.maximum(np.abs(a[1]), 1e-300))
    print(f"gamma={gamma}: periods equal {np.array_equal(a[0], b[0])} (windows differing: {bad[:10].tolist()}), powers rel {dpow:.2e}, "
          f"bases identical {np.array_equal(a[2], b[2])}, status {np.array_equal(a[3], b[3])}, sweeps equal {np.array_equal(a[4], b[4])}")
for e in eng.values():
    e.close()
