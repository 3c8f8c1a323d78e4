#!/usr/bin/env python3
"""Time the routed overlap-add of periodic segments (k_overlap_add_periodic) against the dense route on the same
segments, and ShortTime.decompose_qo against the host route it replaces.

    python tools/short_time_qo_bench.py [--frames 2048] [--n 4096] [--hop 512] [--blocks 8] [--tracks 8] [--reps 10]
                                        [--e2e-frames 256] [--e2e-n 1024] [--e2e-hop 256] [--e2e-num 4] [--e2e-reps 3]

Kernel (`--reps` rounds after 3 warm-up rounds; every round runs each variant once, one after the other, in one process;
median, min and max reported).  W = `--frames` frames of N = `--n` samples, K = `--blocks` blocks per frame with periods
spread over 2 .. N / 3 (every frame draws its own), float64 segments (W, sum p), L = (W - 1) hop + N under a sqrt-Hann
window, `--tracks` masks that partition the blocks at random:
  periodic   k_overlap_add_periodic on the segments (the engine's HIP-event timer around the one launch)
  dense      what the parent offers: the segments tiled to (W, K, N) with torch (torch events around the gather), then
             k_overlap_add_tracks (the engine's timer); the two times are reported apart and added
  probes     the same launch of k_overlap_add_periodic with every period = 2 (all gathers of a frame fall into 16 bytes:
             what is left is the remainder, the per-frame words, the window and the stores) and with every period = N
             (i mod p = i: the gathers are the coalesced reads of the dense kernel)
End to end (host clock around calls that end in a download, `--e2e-reps` rounds after one warm-up, alternating):
  ShortTime.decompose_qo(num, thresh)  against  ShortTime.frames -> QOPeriods().find_periods(batch) -> get_periods ->
  numpy tiling and one np.add.at per block; the periodic parts of the two routes are compared.
Prints one JSON line per measurement."""

import argparse
import json
import os
import sys
import time
import warnings

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


def host_route(st, x, num, thresh):
    """What a user does without decompose_qo: frames, the batched find_periods and get_periods (numpy in, numpy out),
    every waveform tiled to the frame and overlap-added with np.add.at.  -> the periodic part."""
    from pyperiod_amd import QOPeriods

    n, hop, win = st.frame_length, st.hop, st.window
    frames = st.frames(x)
    qo = QOPeriods()
    fits = qo.find_periods(frames, num, thresh)
    live = [f for f in range(frames.shape[0]) if np.abs(frames[f]).sum() > 1e-16]
    waves = qo.get_periods([fits[f][0]["weights"] for f in live], [fits[f][0]["basis_dictionary"] for f in live])
    num_, den = np.zeros(x.size), np.zeros(x.size)
    i = np.arange(n)
    for f in range(frames.shape[0]):
        m = min(n, x.size - f * hop)
        den[f * hop : f * hop + m] += (win * win)[:m]
    for f, ws in zip(live, waves):
        m = min(n, x.size - f * hop)
        for v in ws:
            np.add.at(num_, f * hop + i[:m], (win * v[i % v.size])[:m])
    pos = den > 0
    out = np.zeros(x.size)
    out[pos] = num_[pos] / den[pos]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-frames", type=int, default=256)
    ap.add_argument("--e2e-n", type=int, default=1024)
    ap.add_argument("--e2e-hop", type=int, default=256)
    ap.add_argument("--e2e-num", type=int, default=4)
    ap.add_argument("--e2e-reps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    import torch

    from pyperiod_amd import ShortTime, default_engine

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    W, N, hop, K, T = a.frames, a.n, a.hop, a.blocks, a.tracks
    L = (W - 1) * hop + N
    win_d = torch.as_tensor(np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)), device=dev)
    rng = np.random.default_rng(0)
    # one period per block out of its own slice of 2 .. N / 3, so every frame has short and long ones
    edges = np.linspace(2, N // 3, K + 1).astype(np.int64)
    periods = np.stack([rng.integers(edges[k], edges[k + 1] + 1, W) for k in range(K)], axis=1).astype(np.int32)
    counts = np.full(W, K, np.int32)
    label = rng.integers(0, T, (W, K))
    masks = np.zeros((T, W), np.uint64)
    for k in range(K):
        for t in range(T):
            masks[t, label[:, k] == t] |= np.uint64(1) << np.uint64(k)
    masks_d = torch.as_tensor(masks.view(np.int64), device=dev)
    cnt_d = torch.as_tensor(counts, device=dev)

    def case(per):
        ccap = int(per.astype(np.int64).sum(axis=1).max())
        return torch.randn((W, ccap), dtype=torch.float64, device=dev), torch.as_tensor(per, device=dev), ccap

    seg_d, per_d, ccap = case(periods)
    seg2_d, per2_d, _ = case(np.full((W, K), 2, np.int32))
    segn_d, pern_d, _ = case(np.full((W, K), N, np.int32))

    def periodic(s=seg_d, p=per_d):
        return kernel_ms(eng, "k_overlap_add_periodic",
                         lambda: eng.overlap_add_periodic(s, p, cnt_d, masks_d, N, hop, L, win_d, win_d, True))

    off = torch.cumsum(per_d.to(torch.int64), dim=1) - per_d
    ar = torch.arange(N, device=dev)[None, None, :]

    def tile():
        idx = off[:, :, None] + ar % per_d[:, :, None]
        return torch.gather(seg_d[:, None, :].expand(W, K, ccap), 2, idx)

    def dense():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = tile()
        e1.record()
        ms = kernel_ms(eng, "k_overlap_add_tracks", lambda: eng.overlap_add_tracks(y, masks_d, hop, L, cnt_d, win_d, win_d, True))
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), ms

    got = eng.overlap_add_periodic(seg_d, per_d, cnt_d, masks_d, N, hop, L, win_d, win_d, True)
    ref = eng.overlap_add_tracks(tile(), masks_d, hop, L, cnt_d, win_d, win_d, True)
    max_diff = float((got - ref).abs().max().item())
    same_bits = bool(torch.equal(got, ref))
    del got, ref
    for _ in range(3):
        periodic(), dense(), periodic(seg2_d, per2_d), periodic(segn_d, pern_d)
    p, ti, tr, p2, pn = [], [], [], [], []
    for _ in range(a.reps):
        p.append(periodic())
        t_tile, t_tracks = dense()
        ti.append(t_tile)
        tr.append(t_tracks)
        p2.append(periodic(seg2_d, per2_d))
        pn.append(periodic(segn_d, pern_d))
    sp, sd = stats(p), stats([u + v for u, v in zip(ti, tr)])
    print(json.dumps({"kernel": "k_overlap_add_periodic", "W": W, "K": K, "N": N, "hop": hop, "L": L, "tracks": T,
                      "ccap": ccap, "seg_bytes": int(periods.astype(np.int64).sum()) * 8, "dense_bytes": W * K * N * 8,
                      "bytes_written": T * L * 8, "ms": sp, "dense_route_ms": sd, "tile_ms": stats(ti),
                      "k_overlap_add_tracks_ms": stats(tr), "speedup_over_dense": round(sd["median"] / sp["median"], 2),
                      "speedup_per_round": stats([(u + v) / w for u, v, w in zip(ti, tr, p)]),
                      "speedup_over_k_overlap_add_tracks_alone": round(stats(tr)["median"] / sp["median"], 2),
                      "all_periods_2_ms": stats(p2), "all_periods_N_ms": stats(pn),
                      "max_abs_diff_to_dense": max_diff, "same_bits_as_dense": same_bits}), flush=True)
    del seg_d, seg2_d, segn_d
    torch.cuda.empty_cache()

    # ---- end to end
    W, N, hop, num, thresh = a.e2e_frames, a.e2e_n, a.e2e_hop, a.e2e_num, 0.1
    L = (W - 1) * hop + N
    x = 0.02 * rng.standard_normal(L)
    for k, q in enumerate((41, 97, 233)):  # three periodic components that switch on and off
        wave = rng.standard_normal(q)
        on = (np.arange(L) // (7 * hop) + k) % 3 != 0
        x += np.where(on, np.tile(wave - wave.mean(), L // q + 1)[:L], 0.0)
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    st = ShortTime(N, hop, window=win)
    assert st.frame_count(L) == W
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = st.decompose_qo(x, num, thresh)  # warm-up of both routes
        ref = host_route(st, x, num, thresh)
        diff = float(np.max(np.abs(res.periodic - ref)))
        t_dev, t_host = [], []
        for _ in range(a.e2e_reps):
            t0 = time.perf_counter()
            st.decompose_qo(x, num, thresh)
            t_dev.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            host_route(st, x, num, thresh)
            t_host.append(1e3 * (time.perf_counter() - t0))
    sd, sh = stats(t_dev), stats(t_host)
    print(json.dumps({"end_to_end": "decompose_qo", "num": num, "thresh": thresh, "W": W, "N": N, "hop": hop, "L": L,
                      "tracks": len(res.track_periods), "blocks_per_frame_max": int(res.counts.max()),
                      "decompose_qo_ms": sd, "host_route_ms": sh, "speedup": round(sh["median"] / sd["median"], 2),
                      "periodic_max_abs_diff": diff, "residual_rms_over_signal_rms":
                      round(float(np.sqrt(np.mean(res.residual**2) / np.mean(x**2))), 4)}), flush=True)


if __name__ == "__main__":
    main()
