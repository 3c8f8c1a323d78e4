#!/usr/bin/env python3
"""k_period_path by the engine's HIP-event timers, next to what feeds it and what it replaces.

    python tools/period_path_bench.py kernel [reps]   k_period_path on device tensors of random costs at (W, P, band) =
                                                      (4096, 1365, 8), (65536, 1365, 8), (4096, 8192, 64) and a batch
                                                      of 256 maps of (1024, 1365, 8); the launch shape of each P
    python tools/period_path_bench.py sweep [reps]    the k_sweep launch that produces a (4096, 1365) gamma map: 4096
                                                      float64 frames of 4096 samples, periods 1 .. 1365
    python tools/period_path_bench.py host            the numpy restatement of the path (tests/period_path_cases.py) on
                                                      the host at (1024, 1365, 8) and (4096, 1365, 8), wall clock, once

PH_PATH_TILE_ROWS=1 in the environment (read when the context is made) caps the backtrace tile at one row: the same
forward pass with one HBM round trip per frame of the walk back -- what the tiling buys is `kernel` with and without it.
Every mode warms the clock with untimed calls; only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SHAPES = ((1, 4096, 1365, 8), (1, 65536, 1365, 8), (1, 4096, 8192, 64), (256, 1024, 1365, 8))
tag = "tile cap " + os.environ.get("PH_PATH_TILE_ROWS", "none")


def spread(v):
    v = sorted(v)
    return "median %.4f min %.4f max %.4f (n=%d)" % (v[len(v) // 2], v[0], v[-1], len(v))


def timed(eng, torch, call, name):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        eng.profile(True)
        call()
        torch.cuda.synchronize()
        ms += [t for n, t in eng.profile_read() if n == name]
        eng.profile(False)
    return ms


if mode == "host":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from period_path_cases import period_path_ref

    for W, P, band in ((1024, 1365, 8), (4096, 1365, 8)):
        cost = np.random.default_rng(0).standard_normal((W, P))
        t0 = time.perf_counter()
        period_path_ref(cost, band, 1e-3)
        print(f"PATH host W={W} P={P} band={band}: {1e3 * (time.perf_counter() - t0):.1f} ms (numpy restatement, one run)", flush=True)
elif mode in ("kernel", "sweep"):
    import torch

    from pyperiod_amd import _ffi, default_engine

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    gen = torch.Generator(device=dev).manual_seed(0)
    if mode == "kernel":
        for R, W, P, band in SHAPES:
            cost = torch.randn((R, W, P) if R > 1 else (W, P), dtype=torch.float64, device=dev, generator=gen)
            block, lds, tile = eng.period_path_plan(P)
            ms = timed(eng, torch, lambda: eng.period_path(cost, band, 1e-3), "k_period_path")
            med = sorted(ms)[len(ms) // 2]
            print(f"PATH kernel [{tag}] R={R} W={W} P={P} band={band}: block {block}, LDS {lds} B, tile {tile} rows; ms {spread(ms)}; "
                  f"{1e3 * med / W:.3f} us per frame", flush=True)
            del cost
    else:
        fr = torch.randn((4096, 4096), dtype=torch.float64, device=dev, generator=gen)
        ms = timed(eng, torch, lambda: eng.sweep(fr, 1, 1365, _ffi.PH_SWEEP_NORM_GAMMA), "k_sweep")
        print(f"PATH sweep: k_sweep gamma, 4096 frames of 4096 float64 samples, periods 1 .. 1365: ms {spread(ms)}", flush=True)
else:
    sys.exit("mode must be kernel, sweep or host")
