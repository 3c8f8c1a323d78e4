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
Prints one JSON line per measurement."""

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--num", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=5)
    a = ap.parse_args()
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
