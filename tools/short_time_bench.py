#!/usr/bin/env python3
"""Time the short-time route (ShortTime.analyze: frame on the device, analyse, overlap-add on the device) against the host
route, and its two kernels against their yardsticks.

    python tools/short_time_bench.py [--frames 1024] [--n 4096] [--num 10] [--reps 20] [--e2e-reps 5]

Kernels (HIP events around the one launch, `--reps` repeats after 3 warm-up calls, alternating with the yardstick; median,
min and max reported), float64, W = `--frames`, N = `--n`, K = `--num`, L = (W - 1) hop + N:
  k_frames       against torch.Tensor.clone() of its output -- it writes W N elements and reads at most as many
  k_overlap_add  against y.sum(dim=1) in torch on the same (W, K, N) tensor -- the same bytes read, W N written instead of L
for hop in {512, 1024, 4096}, and k_overlap_add alone for smaller hops (64 .. 256), where the walk of K N / hop terms per
sample grows.
End to end (host clock around calls that end in a download, `--e2e-reps` repeats after one warm-up, alternating):
  ShortTime.analyze("m_best", num=K) against frames built in numpy, Periods().m_best(batch, num=K) and a numpy
  overlap-add, for the same three hops; the two periodic parts are compared.
Prints one JSON line per measurement.

    python tools/short_time_bench.py --blocks [--frames 1024] [--n 4096] [--hop 512] [--num 10] [--block-frames 16,64,256]

The blocked mode, everything in one process:
  kernels     k_overlap_add_block per block + one k_overlap_add_finish against the one k_overlap_add launch on the same
              (W, K, N) bases, between the engine's event timers (ph_timer_begin / ph_timer_end around the whole
              sequence of launches), alternating; the two results are compared bit for bit.  Next to the times stands
              what is known without a run: per block 2 * 8 * (Wb hop + N) bytes of the running sum moved against
              8 * Wb K N bytes of bases read.
  end to end  ShortTime.analyze("m_best", num=K) without blocks and at every `--block-frames`: wall time (host clock, the
              call ends in a download) and torch.cuda.max_memory_allocated over the call, less what was allocated before
              it; the results are compared field for field."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def torch_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def kernel_ms(eng, name, fn):
    eng.profile(True)
    out = fn()
    prof = eng.profile_read()
    eng.profile(False)
    del out
    assert [n for n, _ in prof] == [name], prof
    return prof[0][1]


def alternate(ours, yard, reps):
    for _ in range(3):
        ours(), yard()
    a, b = [], []
    for _ in range(reps):
        a.append(ours())
        b.append(yard())
    return a, b


def host_route(x, n, hop, w_count, win, num):
    """What a user does today: the (W, N) batch built on the host, the (W, K, N) bases brought back, overlap-add in numpy."""
    from pyperiod_amd import Periods

    pad = np.zeros((w_count - 1) * hop + n)
    pad[: x.size] = x
    batch = np.lib.stride_tricks.sliding_window_view(pad, n)[::hop][:w_count] * win
    per, pw, bases = Periods().m_best(batch, num=num)
    part = bases.sum(axis=1) * win
    num_, den = np.zeros(pad.size), np.zeros(pad.size)
    for f in range(w_count):
        num_[f * hop : f * hop + n] += part[f]
        den[f * hop : f * hop + n] += win * win
    out = np.zeros(x.size)
    pos = den[: x.size] > 0
    out[pos] = num_[: x.size][pos] / den[: x.size][pos]
    return per, pw, out


def timed_ms(eng, fn):
    """Milliseconds between the engine's two event timers around fn() (all of fn's launches, on the engine's stream)."""
    eng.timer_begin()
    out = fn()
    ms = eng.timer_end()
    return ms, out


def blocks_mode(a):
    import __graft_entry__ as ge

    ge.build()
    import torch

    from pyperiod_amd import ShortTime, default_engine
    from pyperiod_amd.synth import multi_sinusoid_window

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    W, N, K, hop = a.frames, a.n, a.num, a.hop
    L = (W - 1) * hop + N
    sizes = [int(b) for b in a.block_frames.split(",")]
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    win_d = torch.as_tensor(win, device=dev)
    y = torch.randn((W, K, N), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def one_launch():
        return eng.overlap_add(y, hop, L, None, win_d, win_d, True)

    def blocked(B):
        acc = torch.zeros(L, dtype=torch.float64, device=dev)
        for f0 in range(0, W, B):
            eng.overlap_add_block(y[f0 : f0 + B], hop, L, f0, acc, None, None, win_d)
        return eng.overlap_add_finish(acc, N, hop, W, win_d, win_d, out=acc)

    # the engine's timers record on the stream the engine is bound to: bind it to torch's with one call first
    want = one_launch()
    for B in sizes:
        same = bool(torch.equal(blocked(B).view(torch.int64), want.view(torch.int64)))
        ours, yard = alternate(lambda: timed_ms(eng, lambda: blocked(B))[0], lambda: timed_ms(eng, one_launch)[0], a.reps)
        so, sy = stats(ours), stats(yard)
        nb = -(-W // B)
        acc_bytes = sum(2 * 8 * (min(L, (min(f0 + B, W) - 1) * hop + N) - f0 * hop) for f0 in range(0, W, B))
        print(json.dumps({"kernels": "k_overlap_add_block x blocks + k_overlap_add_finish", "W": W, "K": K, "N": N, "hop": hop,
                          "L": L, "block_frames": B, "blocks": nb, "bytes_read": W * K * N * 8, "acc_bytes_moved": acc_bytes,
                          "acc_over_read": round(acc_bytes / (W * K * N * 8), 4), "ms": so, "one_launch_ms": sy,
                          "ratio_to_one_launch": round(so["median"] / sy["median"], 3), "bit_equal": same}), flush=True)
    del y, want
    stream.synchronize()
    torch.cuda.empty_cache()

    x = np.concatenate([multi_sinusoid_window(s, N) for s in range(-(-L // N))])[:L]
    st = ShortTime(N, hop, window=win)
    assert st.frame_count(L) == W

    def run(B):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        res = st.analyze(x, method="m_best", num=K, block_frames=B)
        ms = 1e3 * (time.perf_counter() - t0)
        return res, ms, torch.cuda.max_memory_allocated(dev) - base

    ref = run(None)[0]  # warm-up
    for B in sizes:
        run(B)
    times, peaks, same = {B: [] for B in [None] + sizes}, {}, {}
    for _ in range(a.e2e_reps):
        for B in [None] + sizes:
            res, ms, peak = run(B)
            times[B].append(ms)
            peaks[B] = peak
            same[B] = all(np.array_equal(g, w) for g, w in zip(res[:4], ref[:4]))
    base_ms = stats(times[None])["median"]
    for B in [None] + sizes:
        sb = stats(times[B])
        print(json.dumps({"end_to_end": "m_best", "num": K, "W": W, "N": N, "hop": hop, "L": L, "block_frames": B,
                          "analyze_ms": sb, "ratio_to_unblocked": round(sb["median"] / base_ms, 3),
                          "peak_torch_bytes": peaks[B], "peak_over_unblocked": round(peaks[B] / peaks[None], 4),
                          "bases_bytes": W * K * N * 8, "equal_to_unblocked": same[B]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", action="store_true", help="the blocked mode (analyze with block_frames, the block kernels)")
    ap.add_argument("--hop", type=int, default=512, help="--blocks only")
    ap.add_argument("--block-frames", default="16,64,256", help="--blocks only: comma-separated block sizes")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--num", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=5)
    a = ap.parse_args()
    if a.blocks:
        return blocks_mode(a)
    import __graft_entry__ as ge

    ge.build()
    import torch

    from pyperiod_amd import ShortTime, default_engine
    from pyperiod_amd.synth import multi_sinusoid_window

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    W, N, K = a.frames, a.n, a.num
    y = torch.randn((W, K, N), dtype=torch.float64, device=dev)
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    win_d = torch.as_tensor(win, device=dev)
    sum_ms = None
    for hop in (4096, 1024, 512, 256, 128, 64):
        L = (W - 1) * hop + N
        x = torch.randn(L, dtype=torch.float64, device=dev)
        if hop >= 512:
            fr = eng.frames(x, N, hop, W, win_d)
            ours, yard = alternate(lambda: kernel_ms(eng, "k_frames", lambda: eng.frames(x, N, hop, W, win_d)),
                                   lambda: torch_ms(torch, fr.clone), a.reps)
            so, sy = stats(ours), stats(yard)
            print(json.dumps({"kernel": "k_frames", "W": W, "N": N, "hop": hop, "L": L, "bytes_written": W * N * 8,
                              "ms": so, "clone_ms": sy, "ratio_to_clone": round(so["median"] / sy["median"], 3)}), flush=True)
            del fr
        ours, yard = alternate(lambda: kernel_ms(eng, "k_overlap_add",
                                                 lambda: eng.overlap_add(y, hop, L, None, win_d, win_d, True)),
                               lambda: torch_ms(torch, lambda: y.sum(dim=1)), a.reps)
        so, sy = stats(ours), stats(yard)
        print(json.dumps({"kernel": "k_overlap_add", "W": W, "K": K, "N": N, "hop": hop, "L": L,
                          "terms_per_sample": K * -(-N // hop), "bytes_read": W * K * N * 8, "ms": so, "sum_dim1_ms": sy,
                          "ratio_to_sum": round(so["median"] / sy["median"], 3),
                          "read_TBps": round(W * K * N * 8 / so["median"] / 1e9, 3)}), flush=True)
        del x
    del y
    torch.cuda.empty_cache()
    for hop in (4096, 1024, 512):
        L = (W - 1) * hop + N
        reps_n = -(-L // N)
        x = np.concatenate([multi_sinusoid_window(s, N) for s in range(reps_n)])[:L]
        st = ShortTime(N, hop, window=win)
        assert st.frame_count(L) == W
        res = st.analyze(x, method="m_best", num=K)  # warm-up of both routes
        per, pw, ref = host_route(x, N, hop, W, win, K)
        same = bool(np.array_equal(res.periods, per) and np.array_equal(res.powers, pw))
        diff = float(np.max(np.abs(res.periodic - ref)))
        t_dev, t_host = [], []
        for _ in range(a.e2e_reps):
            t0 = time.perf_counter()
            st.analyze(x, method="m_best", num=K)
            t_dev.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            host_route(x, N, hop, W, win, K)
            t_host.append(1e3 * (time.perf_counter() - t0))
        sd, sh = stats(t_dev), stats(t_host)
        print(json.dumps({"end_to_end": "m_best", "num": K, "W": W, "N": N, "hop": hop, "L": L, "analyze_ms": sd,
                          "host_route_ms": sh, "speedup": round(sh["median"] / sd["median"], 2),
                          "periods_powers_equal": same, "periodic_max_abs_diff": diff}), flush=True)


if __name__ == "__main__":
    main()
