#!/usr/bin/env python3
"""Time ShortTime.decompose_ramanujan against the host route it replaces, and the capped selection kernel
(k_ram_select_ref) against k_ram_select on the same norms.

    python tools/short_time_ram_bench.py [--frames 2048] [--n 4096] [--reps 10]
                                         [--e2e-frames 256] [--e2e-n 1024] [--e2e-hop 256] [--e2e-reps 3]

Kernel (`--reps` rounds after 3 warm-up rounds; every round runs each variant once, one after the other, in one process;
median, min and max of the engine's HIP-event time around the one launch).  W = `--frames` windows of N = `--n` samples
of white noise, norms of the periods 2 .. N / 3 from one ramanujan_fit call:
  k_ram_select          inside ramanujan_fit (thresh 0.2, pcap 64), as it runs today
  k_ram_select_ref      on those norms with thresh 0.2 and pcap 64, with and without reference levels: no row is over
                        the cap, the bisection never runs (the report says how many rows were over)
  k_ram_select_ref      with thresh 0.001 and pcap 16: every row is over the cap and runs the 64 bisection passes
End to end (host clock around calls that end in a download, `--e2e-reps` rounds after one warm-up, alternating):
  ShortTime.decompose_ramanujan(thresh 0.2, reference="frame", max_periods=64)  against  ShortTime.frames (numpy) ->
  RamanujanPeriods().find_periods_with_weights(batch) -> QOPeriods.get_periods -> numpy tiling and one np.add.at per
  block; the periodic parts of the two routes are compared.  Frames whose dictionary the device fit hands back run the
  same 1-D call in both routes.  Then decompose_ramanujan(thresh 0.2, reference="recording", max_periods=8) alone.
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
    """The time of the one launch of `name` among the launches of fn()."""
    eng.profile(True)
    out = fn()
    prof = eng.profile_read()
    eng.profile(False)
    ms = [t for n, t in prof if n == name]
    assert len(ms) == 1, prof
    return ms[0], out


def host_route(st, x, thresh):
    """What a user does without decompose_ramanujan: frames, the batched find_periods_with_weights and get_periods
    (numpy in, numpy out), every waveform tiled to the frame and overlap-added with np.add.at.  -> the periodic part."""
    from pyperiod_amd import QOPeriods, RamanujanPeriods

    n, hop, win = st.frame_length, st.hop, st.window
    frames = st.frames(x)
    fits = RamanujanPeriods().find_periods_with_weights(frames, 2, n // 3, thresh)
    live = [f for f in range(frames.shape[0]) if len(fits[f][0]["basis_dictionary"])]
    waves = QOPeriods().get_periods([fits[f][0]["weights"] for f in live], [fits[f][0]["basis_dictionary"] for f in live])
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-frames", type=int, default=256)
    ap.add_argument("--e2e-n", type=int, default=1024)
    ap.add_argument("--e2e-hop", type=int, default=256)
    ap.add_argument("--e2e-reps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    import torch

    from pyperiod_amd import ShortTime, default_engine

    eng = default_engine()
    dev = torch.device("cuda", eng.device)
    W, N = a.frames, a.n
    q_hi = N // 3
    x_d = torch.randn((W, N), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def old():
        return kernel_ms(eng, "k_ram_select", lambda: eng.ramanujan_fit(x_d, 2, q_hi, 0.2, 64, 512))

    norms = old()[1][0]
    level = norms.max(dim=1).values.contiguous()

    def new(thresh, ref, pcap):
        return kernel_ms(eng, "k_ram_select_ref", lambda: eng.ramanujan_select(norms, thresh, ref, pcap))

    over_lo = int((new(0.2, None, 64)[1][2] > 64).sum().item())
    over_hi = int((new(0.001, None, 16)[1][2] > 16).sum().item())
    for _ in range(3):
        old(), new(0.2, None, 64), new(0.2, level, 64), new(0.001, None, 16)
    t_old, t_new, t_ref, t_cap = [], [], [], []
    for _ in range(a.reps):
        t_old.append(old()[0])
        t_new.append(new(0.2, None, 64)[0])
        t_ref.append(new(0.2, level, 64)[0])
        t_cap.append(new(0.001, None, 16)[0])
    so, sn = stats(t_old), stats(t_new)
    print(json.dumps({"kernel": "k_ram_select_ref", "W": W, "N": N, "q_hi": q_hi, "norm_bytes": W * (q_hi + 1) * 8,
                      "k_ram_select_ms": so, "no_row_over_ms": sn, "no_row_over_with_levels_ms": stats(t_ref),
                      "rows_over_at_thresh_0.2_pcap_64": over_lo, "every_row_over_ms": stats(t_cap),
                      "rows_over_at_thresh_0.001_pcap_16": over_hi,
                      "ratio_to_k_ram_select": round(sn["median"] / so["median"], 2),
                      "ratio_every_row_over": round(stats(t_cap)["median"] / so["median"], 2)}), flush=True)
    del x_d, norms
    torch.cuda.empty_cache()

    # ---- end to end
    rng = np.random.default_rng(0)
    W, N, hop, thresh = a.e2e_frames, a.e2e_n, a.e2e_hop, 0.2
    L = (W - 1) * hop + N
    x = 0.02 * rng.standard_normal(L)
    for k, q in enumerate((41, 97, 233)):  # three periodic components that switch on and off
        wave = rng.standard_normal(q)
        on = (np.arange(L) // (7 * hop) + k) % 3 != 0
        x += np.where(on, np.tile(wave - wave.mean(), L // q + 1)[:L], 0.0)
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    st = ShortTime(N, hop, window=win)
    assert st.frame_count(L) == W
    kw = dict(thresh=thresh, reference="frame", max_periods=64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = st.decompose_ramanujan(x, **kw)  # warm-up of both routes
        ref = host_route(st, x, thresh)
        diff = float(np.max(np.abs(res.periodic - ref)))
        t_dev, t_host = [], []
        for _ in range(a.e2e_reps):
            t0 = time.perf_counter()
            st.decompose_ramanujan(x, **kw)
            t_dev.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            host_route(st, x, thresh)
            t_host.append(1e3 * (time.perf_counter() - t0))
        # the recording-level settings, which the host route has no counterpart for: the device pipeline alone
        kw_rec = dict(thresh=thresh, reference="recording", max_periods=8)
        rec = st.decompose_ramanujan(x, **kw_rec)
        t_rec = []
        for _ in range(a.e2e_reps):
            t0 = time.perf_counter()
            st.decompose_ramanujan(x, **kw_rec)
            t_rec.append(1e3 * (time.perf_counter() - t0))
    sd, sh = stats(t_dev), stats(t_host)
    print(json.dumps({"end_to_end": "decompose_ramanujan", "thresh": thresh, "reference": "recording", "max_periods": 8,
                      "W": W, "N": N, "hop": hop, "L": L, "blocks_per_frame_max": int(rec.counts.max()),
                      "frames_by_status": np.bincount(rec.frame_status, minlength=4).tolist(),
                      "frames_over_the_cap": int((rec.over > rec.counts).sum()), "decompose_ramanujan_ms": stats(t_rec),
                      "residual_rms_over_signal_rms": round(float(np.sqrt(np.mean(rec.residual**2) / np.mean(x**2))), 4)}),
          flush=True)
    print(json.dumps({"end_to_end": "decompose_ramanujan", "thresh": thresh, "reference": "frame", "W": W, "N": N, "hop": hop,
                      "L": L, "tracks": len(res.track_periods), "blocks_per_frame_max": int(res.counts.max()),
                      "frames_by_status": np.bincount(res.frame_status, minlength=4).tolist(),
                      "frames_over_the_cap": int((res.over > res.counts).sum()),
                      "decompose_ramanujan_ms": sd, "host_route_ms": sh, "speedup": round(sh["median"] / sd["median"], 2),
                      "periodic_max_abs_diff": diff,
                      "residual_rms_over_signal_rms": round(float(np.sqrt(np.mean(res.residual**2) / np.mean(x**2))), 4)}),
          flush=True)


if __name__ == "__main__":
    main()
