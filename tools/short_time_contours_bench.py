#!/usr/bin/env python3
"""ShortTime.contours and k_follow_residual by the engine's HIP-event timers, next to the torch route of the same residual.

    python tools/short_time_contours_bench.py [reps] [seconds]

The recording is `seconds` (default 60) at 48 kHz from a seed: four gliding pulse trains in noise (the recording of
tools/short_time_follow_bench.py).  Frames of 4096 with hop 512, sqrt-Hann window, kind gamma over the periods
2 .. 1365, band 8, jump 0.002, four tracks.  In one process, alternating after two untimed rounds:

  residual   k_follow_residual without tracks next to k_frames writing float64 (the same bytes written: what round 0
             cost before), and k_follow_residual with 1, 2 and 3 of the true tracks
  rounds     the kernels of one contours call by name, and each one's share of the call's kernel time
  contours   ShortTime.contours on the device tensor next to the torch route of the same rounds -- frames, then per
             track one (W, N) int64 index array, a scatter-add for the column sums and one gather and subtraction;
             the same sweep and path launches -- by wall clock around a synchronize and by torch's peak allocation

Only numbers taken in one session on one device compare."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from short_time_follow_bench import recording, spread, tracks  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
RATE, N, HOP, K, KIND, BAND, JUMP = 48000, 4096, 512, 4, "gamma", 8, 0.002


def main():
    import torch

    from pyperiod_amd import ShortTime, _ffi, default_engine

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    L = int(SECONDS * RATE)
    st = ShortTime(N, HOP, window=np.sqrt(np.hanning(N + 1)[:N]))
    W, lo, hi = st.frame_count(L), 2, N // 3
    xd = torch.as_tensor(recording(L, K), device=dev)
    win = torch.as_tensor(st.window, device=dev)
    true = torch.as_tensor(tracks(W, N, HOP, L, K), device=dev)
    print(f"CONTOURS N={N} hop={HOP} W={W} L={L} kind={KIND} periods {lo}..{hi} band={BAND} jump={JUMP} count={K}; "
          f"follow plan (block, LDS bytes, placement) {eng.follow_plan(N)}", flush=True)

    def timed(call):
        eng.profile(True)
        try:
            call()
            return eng.profile_read()
        finally:
            eng.profile(False)

    # ---- k_follow_residual next to k_frames, and with tracks
    calls = {"k_frames float64": lambda: eng.frames(xd, N, HOP, W, win, np.float64),
             "k_follow_residual, no tracks": lambda: eng.follow_residual(xd, N, HOP, 0, W, None, None, win)}
    for t in (1, 2, 3):
        packed, counts = st.pack_tracks(true[:, :t])[:2]
        calls[f"k_follow_residual, {t} tracks"] = (lambda p, c: lambda: eng.follow_residual(xd, N, HOP, 0, W, p, c, win))(packed, counts)
    ms = {name: [] for name in calls}
    for rep in range(REPS + 2):
        for name, call in calls.items():
            got = timed(call)
            if rep >= 2:
                ms[name].append(got[0][1])
    for name, v in ms.items():
        print(f"  {name}: ms {spread(v)}", flush=True)

    # ---- the rounds of one contours call
    def contours():
        return st.contours(xd, K, kind=KIND, band=BAND, jump=JUMP)

    def torch_route():
        """The same rounds with the residual made by torch ops on a (W, N) array."""
        fr = eng.frames(xd, N, HOP, W, win, np.float64)
        periods = torch.zeros((W, K), dtype=torch.int32, device=dev)
        ar = torch.arange(N, device=dev)
        for k in range(K):
            if k:
                p = periods[:, k - 1].to(torch.int64).clamp(min=1)
                idx = ar[None, :] % p[:, None]
                sums = torch.zeros((W, N), dtype=torch.float64, device=dev).scatter_add_(1, idx, fr)
                cnt = torch.zeros((W, N), dtype=torch.float64, device=dev).scatter_add_(1, idx, torch.ones_like(fr))
                fr = fr - (sums / cnt.clamp(min=1)).gather(1, idx)
            values = eng.sweep(fr, lo, hi, _ffi.PH_SWEEP_NORM_GAMMA, False, False)
            path, _, _, status = eng.period_path(values, BAND, JUMP)
            assert int(status.item()) == 0
            periods[:, k] = path + lo
        return periods.cpu().numpy()

    res = contours()
    same = float(np.mean(res.periods == torch_route()))
    hit = [float(np.mean(np.abs(res.periods[:, k : k + 1] - true.cpu().numpy()).min(1) <= 1)) for k in range(K)]
    print(f"  frames where track k is within 1 of one of the true tracks: {['%.3f' % h for h in hit]}; "
          f"entries equal to the torch route's {same:.4f}", flush=True)
    by_name, wall, peak = {}, {"contours": [], "torch route": []}, {}
    for rep in range(REPS + 2):
        for name, call in (("contours", contours), ("torch route", torch_route)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            prof = name == "contours" and rep >= 2
            if prof:
                eng.profile(True)
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            if prof:
                got = eng.profile_read()
                eng.profile(False)
                total = {}
                for n, t in got:
                    total[n] = total.get(n, 0.0) + t
                for n, t in total.items():
                    by_name.setdefault(n, []).append(t)
            if rep >= 2:
                wall[name].append(dt)
                peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 2**20
    all_ms = sum(sorted(v)[len(v) // 2] for v in by_name.values())
    for n, v in by_name.items():
        print(f"  {n}: ms per call ({K} rounds) {spread(v)}; {100 * sorted(v)[len(v) // 2] / all_ms:.1f} % of the kernel time", flush=True)
    for name in wall:
        print(f"  {name}: wall ms {spread(wall[name])}; peak allocation above the signal {peak[name]:.0f} MiB", flush=True)
    cm, tm = (sorted(wall[k])[len(wall[k]) // 2] for k in ("contours", "torch route"))
    print(f"  contours is {tm / cm:.2f} x the torch route's speed", flush=True)


if __name__ == "__main__":
    main()
