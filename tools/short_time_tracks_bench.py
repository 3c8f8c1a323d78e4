#!/usr/bin/env python3
"""Time the routed overlap-add (k_overlap_add_tracks) against k_overlap_add on the same bases, and ShortTime.decompose
against the host route it replaces.

    python tools/short_time_tracks_bench.py [--frames 1024] [--n 4096] [--hop 512] [--num 10] [--tracks 8]
                                            [--reps 20] [--e2e-reps 3]

Kernel (the engine's HIP-event timers around the one launch, `--reps` repeats after 3 warm-up calls, alternating between
the two kernels in one process; median, min and max reported): float64 y (W, K, N) with W = `--frames`, N = `--n`,
K = `--num`, L = (W - 1) hop + N, under a sqrt-Hann window, and `--tracks` + 1 masks that partition the rows at random.
Both kernels read the same W K N elements once; the routed one writes (T + 1) L doubles instead of L, so the ratio that
traffic alone explains is (W K N + (T + 1) L) / (W K N + L).
End to end (host clock around calls that end in a download, `--e2e-reps` repeats after one warm-up, alternating):
  ShortTime.decompose("m_best", num=K, max_tracks=T)  against  Periods().m_best on the frames (the (W, K, N) bases brought
  back to the host) followed by one np.add.at per basis row into its track; the tracks of the two routes are compared.
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


def kernel_ms(eng, name, fn):
    eng.profile(True)
    out = fn()
    prof = eng.profile_read()
    eng.profile(False)
    del out
    assert [n for n, _ in prof] == [name], prof
    return prof[0][1]


def host_route(st, x, num, max_tracks):
    """What a user does without decompose: frames on the device, Periods().m_best with the bases brought back, then on the
    host the ranking, and per track one np.add.at per basis row."""
    from pyperiod_amd import Periods, ShortTime

    n, hop, win = st.frame_length, st.hop, st.window
    frames = st.frames(x)
    per, pw, bases = Periods().m_best(frames, num=num)
    groups = [(p,) for p in ShortTime.rank_periods(per, pw, None, max_tracks)]
    w_count = frames.shape[0]
    idx = np.arange(w_count)[:, None] * hop + np.arange(n)[None, :]
    ok = idx < x.size
    den = np.zeros(x.size)
    np.add.at(den, idx[ok], np.broadcast_to(win * win, idx.shape)[ok])
    pos = den > 0
    tracks = np.zeros((len(groups) + 1, x.size))
    label = np.full(per.shape, len(groups))
    for t, g in enumerate(groups):
        label[np.isin(per, g)] = t
    for k in range(per.shape[1]):
        term = bases[:, k] * win
        for t in range(len(groups) + 1):
            use = ok & (label[:, k] == t)[:, None]
            np.add.at(tracks[t], idx[use], term[use])
    tracks[:, pos] /= den[pos]
    tracks[:, ~pos] = 0.0
    return groups, tracks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--num", type=int, default=10)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    import torch

    from pyperiod_amd import ShortTime, default_engine
    from pyperiod_amd.synth import multi_sinusoid_window

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    W, N, hop, K, T = a.frames, a.n, a.hop, a.num, a.tracks
    L = (W - 1) * hop + N
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    win_d = torch.as_tensor(win, device=dev)
    y = torch.randn((W, K, N), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    label = rng.integers(0, T + 1, (W, K))
    masks = np.zeros((T + 1, W), np.uint64)
    for k in range(K):
        for t in range(T + 1):
            masks[t, label[:, k] == t] |= np.uint64(1) << np.uint64(k)
    masks_d = torch.as_tensor(masks.view(np.int64), device=dev)

    def routed():
        return kernel_ms(eng, "k_overlap_add_tracks",
                         lambda: eng.overlap_add_tracks(y, masks_d, hop, L, None, win_d, win_d, True))

    def plain():
        return kernel_ms(eng, "k_overlap_add", lambda: eng.overlap_add(y, hop, L, None, win_d, win_d, True))

    for _ in range(3):
        routed(), plain()
    r, p = [], []
    for _ in range(a.reps):
        r.append(routed())
        p.append(plain())
    sr, sp = stats(r), stats(p)
    ratios = stats([u / v for u, v in zip(r, p)])
    read, wr_r, wr_p = W * K * N * 8, (T + 1) * L * 8, L * 8
    print(json.dumps({"kernel": "k_overlap_add_tracks", "W": W, "K": K, "N": N, "hop": hop, "L": L, "masks": T + 1,
                      "bytes_read": read, "bytes_written": wr_r, "ms": sr, "k_overlap_add_ms": sp,
                      "ratio": round(sr["median"] / sp["median"], 3), "ratio_per_rep": ratios,
                      "ratio_from_traffic": round((read + wr_r) / (read + wr_p), 3),
                      "TBps": round((read + wr_r) / sr["median"] / 1e9, 3)}), flush=True)
    del y, masks_d
    torch.cuda.empty_cache()

    x = np.concatenate([multi_sinusoid_window(s, N) for s in range(-(-L // N))])[:L]
    st = ShortTime(N, hop, window=win)
    assert st.frame_count(L) == W
    res = st.decompose(x, method="m_best", num=K, max_tracks=T)  # warm-up of both routes
    groups, ref = host_route(st, x, K, T)
    same = res.track_periods == groups
    diff = float(np.max(np.abs(np.concatenate([res.tracks, res.other[None, :]]) - ref))) if same else None
    t_dev, t_host = [], []
    for _ in range(a.e2e_reps):
        t0 = time.perf_counter()
        st.decompose(x, method="m_best", num=K, max_tracks=T)
        t_dev.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        host_route(st, x, K, T)
        t_host.append(1e3 * (time.perf_counter() - t0))
    sd, sh = stats(t_dev), stats(t_host)
    print(json.dumps({"end_to_end": "m_best", "num": K, "max_tracks": T, "W": W, "N": N, "hop": hop, "L": L,
                      "decompose_ms": sd, "host_route_ms": sh, "speedup": round(sh["median"] / sd["median"], 2),
                      "track_periods_equal": same, "tracks_max_abs_diff": diff}), flush=True)


if __name__ == "__main__":
    main()
