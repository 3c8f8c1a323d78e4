"""The numpy restatement of ph_follow_residual's definition (include/periodhip.h) and of ShortTime.contours, and the
two-voice signal, shared by tests/test_short_time_contours_cpu.py and tests/test_gpu_short_time_contours.py.

peel_ref is the definition line by line on oracle.period_oracle.project: the frame as ph_frames rounds it, then one
projection and one rounded subtraction per live entry.  contours_ref is the four steps of a round -- residual frames,
map, guard, path -- on numpy arrays, with the map function handed in: the oracle's sweep on the CPU, the engine's kind
call on the GPU."""

import numpy as np

from follow_cases import frame_ref
from oracle import period_oracle as po
from period_path_cases import PH_ST_OK, glide_signal, period_path_ref


def two_voice_signal():
    """The glide signal (a pulse train whose period glides from 20 to 30 samples, 5 % noise) plus a pulse train of
    constant period 47, amplitude 0.8, first pulse at sample 3: -> (signal, true period of the glide at sample n, 47)."""
    x, period_at = glide_signal()
    y = x.copy()
    y[3::47] += 0.8
    return y, period_at, 47


def peel_ref(signal, N, hop, f0, Wb, window, frame_dtype, periods, counts, trunc):
    """-> (Wb, N) float64: row i is frame f0 + i less the projections onto periods[i, 0], periods[i, 1], ... peeled in
    order; the walk of a row ends at counts[i] entries (clipped to 0 .. pcap) or at the first period < 1 or > N.
    `periods` None: no entries."""
    signal = np.asarray(signal)
    out = np.empty((Wb, N))
    pcap = 0 if periods is None else np.asarray(periods).shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(Wb):
            r = frame_ref(signal, N, hop, f0 + i, window, frame_dtype)
            for a in range(min(max(int(counts[i]), 0), pcap) if pcap else 0):
                p = int(periods[i, a])
                if p < 1 or p > N:
                    break
                s = po.project(r, p, trunc, False, True)
                r = r - np.tile(s, N // p + 1)[:N]
            out[i] = r
    return out


def pack_live(periods):
    """Each row's entries >= 1 packed to the front in column order: -> (packed (W, T) int32, counts (W,) int32)."""
    periods = np.asarray(periods)
    W, T = periods.shape
    packed = np.zeros((W, T), dtype=np.int32)
    counts = np.zeros(W, dtype=np.int32)
    for f in range(W):
        live = periods[f][periods[f] >= 1]
        packed[f, : live.size] = live
        counts[f] = live.size
    return packed, counts


def guard_ref(values, lo, earlier, guard):
    """A copy of the map (W, P), column j period lo + j, with -inf in every cell within `guard` columns of a live
    (>= 1) period of `earlier` (W, k) in that frame; cells outside the period range do not exist.  None: a plain copy."""
    out = np.array(values, dtype=np.float64)
    if guard is None:
        return out
    W, P = out.shape
    for f in range(W):
        for p in np.asarray(earlier)[f]:
            if p >= 1:
                a, b = max(int(p) - guard - lo, 0), min(int(p) + guard - lo, P - 1)
                if a <= b:
                    out[f, a : b + 1] = -np.inf
    return out


def contours_ref(signal, N, hop, W, window, frame_dtype, trunc, count, map_fn, lo, band, jump, floor=None, guard=None):
    """ShortTime.contours on numpy arrays: map_fn(frames (W, N) float64) -> (W, P) float64, column j period lo + j.
    -> (periods (W, count) int32, salience (W, count), scores (count,), maps: the `count` maps as each round's path saw
    them).  ValueError naming the round when a round has no path."""
    periods = np.zeros((W, count), dtype=np.int32)
    salience = np.zeros((W, count))
    scores = np.zeros(count)
    maps = []
    for k in range(count):
        packed, counts = pack_live(periods[:, :k])
        frames = peel_ref(signal, N, hop, 0, W, window, frame_dtype, packed if k else None, counts, trunc)
        m = guard_ref(map_fn(frames), lo, periods[:, :k], guard)
        path, values, score, status = period_path_ref(m, band, jump)
        if status != PH_ST_OK:
            raise ValueError(f"contours: round {k}: no path exists")
        col = (lo + path).astype(np.int32)
        if floor is not None:
            col = np.where(values > floor, col, 0).astype(np.int32)
        periods[:, k], salience[:, k], scores[k] = col, values, score
        maps.append(m)
    return periods, salience, scores, maps


def oracle_gamma_map(lo, hi, trunc=False):
    """map_fn of contours_ref: the oracle's gamma sweep of every frame, periods lo .. hi."""
    return lambda frames: np.stack([po.sweep_norms(fr, lo, hi, gamma=True, trunc=trunc) for fr in frames])
