#!/usr/bin/env python3
"""ShortTime.follow next to the route the library offered before it, and k_follow by the engine's HIP-event timers.

    python tools/short_time_follow_bench.py [reps] [seconds]

The recording is `seconds` (default 60) at 48 kHz from a seed: T gliding pulse trains in noise.  Shapes: frames of 4096
with hop 512 and frames of 1024 with hop 256, T = 1 and T = 4 tracks whose periods glide slowly between 96 and 480
samples.  Per shape, in one process, alternating after two untimed rounds:

  follow   ShortTime.follow on the device tensor (k_follow + k_overlap_add_periodic), wall clock around a synchronize,
           and both kernels by the engine's event timers
  parent   ShortTime.frames, then per track and per distinct period engine.project_batch on the frames that carry it and
           the subtraction, the bases gathered into (W, T, N), then overlap_add_tracks -- the same result to rounding

and the bytes the algorithm has to move (the signal once, periods and counts, the segments, powers and done) over the
k_follow time against the HBM peak of 8 TB/s.  Only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
RATE, HBM_PEAK = 48000, 8.0e12
SHAPES = ((4096, 512), (1024, 256))


def spread(v):
    v = sorted(v)
    return "median %.3f min %.3f max %.3f (n=%d)" % (v[len(v) // 2], v[0], v[-1], len(v))


def recording(L, T, seed=0):
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal(L)
    n = np.arange(L)
    for t in range(T):
        period = 288.0 + 150.0 * np.sin(2 * np.pi * (n / L) * (t + 1) + t)  # samples, gliding
        phase = np.cumsum(1.0 / period)
        x += (np.diff(np.floor(phase), prepend=0.0) > 0).astype(np.float64)
    return x - x.mean()


def tracks(W, N, hop, L, T):
    f = np.arange(W) * hop + N / 2.0
    return np.stack([np.clip(np.rint(288.0 + 150.0 * np.sin(2 * np.pi * (f / L) * (t + 1) + t)), 96, min(480, N)).astype(np.int32)
                     for t in range(T)], 1)


def main():
    import torch

    from pyperiod_amd import ShortTime, default_engine

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    L = int(SECONDS * RATE)
    for N, hop in SHAPES:
        for T in (1, 4):
            st = ShortTime(N, hop, window=np.sqrt(np.hanning(N + 1)[:N]))
            W = st.frame_count(L)
            per = tracks(W, N, hop, L, T)
            xd = torch.as_tensor(recording(L, T), device=dev)
            perd = torch.as_tensor(per, device=dev)
            win = torch.as_tensor(st.window, device=dev)
            cols = [[(int(p), torch.as_tensor(np.flatnonzero(per[:, t] == p), device=dev)) for p in np.unique(per[:, t])]
                    for t in range(T)]
            masks = torch.as_tensor((np.uint64(1) << np.arange(T, dtype=np.uint64))[:, None].repeat(W, 1).view(np.int64), device=dev)
            masks = torch.cat([masks, masks.sum(0, keepdim=True)], 0)

            def follow():
                return st.follow(xd, perd)

            def parent():
                res = st.frames(xd)
                y = torch.empty((W, T, N), dtype=torch.float64, device=dev)
                for t in range(T):
                    for p, idx in cols[t]:
                        base = eng.project_batch(res[idx], [p])[:, 0]
                        y[idx, t] = base
                        res[idx] -= base
                return eng.overlap_add_tracks(y, masks, hop, L, None, win, win, True)

            got, want = follow(), parent()
            err = float((torch.vstack([got.tracks, got.periodic[None]]) - want).abs().max())
            for _ in range(2):
                follow(), parent()
            torch.cuda.synchronize()
            wall = {"follow": [], "parent": []}
            kern = {"k_follow": [], "k_overlap_add_periodic": []}
            for _ in range(REPS):
                for name, call in (("follow", follow), ("parent", parent)):
                    if name == "follow":
                        eng.profile(True)
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                    if name == "follow":
                        for n, ms in eng.profile_read():
                            kern[n].append(ms)
                        eng.profile(False)
            block, lds, where = eng.follow_plan(N)
            seg_doubles = int(per.sum())
            need = 8 * L + 4 * W * (T + 1) + 8 * seg_doubles + 8 * W * T + 4 * W
            kmed = sorted(kern["k_follow"])[len(kern["k_follow"]) // 2]
            fmed, pmed = (sorted(wall[k])[len(wall[k]) // 2] for k in ("follow", "parent"))
            print(f"FOLLOW N={N} hop={hop} T={T} W={W} L={L}: block {block}, LDS {lds} B, placement {where}; "
                  f"distinct periods per track {[len(c) for c in cols]}; max |follow - parent| {err:.3g}", flush=True)
            print(f"  k_follow ms {spread(kern['k_follow'])}; {1e3 * kmed / W:.3f} us per frame; needs {need / 1e6:.1f} MB -> "
                  f"{need / (1e-3 * kmed) / 1e9:.1f} GB/s = {100 * need / (1e-3 * kmed) / HBM_PEAK:.2f} % of the HBM peak", flush=True)
            print(f"  k_overlap_add_periodic ms {spread(kern['k_overlap_add_periodic'])}", flush=True)
            print(f"  ShortTime.follow wall ms {spread(wall['follow'])}", flush=True)
            print(f"  parent route wall ms {spread(wall['parent'])}; follow is {pmed / fmed:.2f} x the parent route's speed", flush=True)
            del xd, want, got


if __name__ == "__main__":
    main()
