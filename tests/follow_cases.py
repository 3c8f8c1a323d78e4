"""The numpy restatement of ph_follow's definition (include/periodhip.h) and the case table that
tests/test_short_time_follow_cpu.py and tests/test_gpu_short_time_follow.py share.

The restatement is the definition line by line on oracle.period_oracle.project: the frame as ph_frames rounds it, the
per-frame walk with its three stop rules, one rounded subtraction per sample, the powers from periodic_norm.
seg comes back with NaN left in every element that must not be written; powers behind done is 0.0, which is written,
and so is every element of done."""

import numpy as np

from oracle import period_oracle as po

F64, F32 = np.float64, np.float32


def frame_ref(signal, N, hop, f, window, frame_dtype):
    """Frame f as ph_frames writes it, widened to float64."""
    L = signal.shape[0]
    x = np.zeros(N, dtype=np.float64)
    n = max(0, min(N, L - f * hop))
    x[:n] = signal[f * hop : f * hop + n].astype(np.float64)
    if window is not None:
        x[:n] = x[:n] * np.asarray(window, dtype=np.float64)[:n]
    return x.astype(frame_dtype).astype(np.float64)


def follow_ref(signal, N, hop, W, window, frame_dtype, periods, counts, ccap, trunc):
    """-> (seg (W, ccap), powers (W, pcap), done (W,)): NaN in every element of seg that is not written."""
    signal = np.asarray(signal)
    periods = np.asarray(periods)
    pcap = periods.shape[1]
    seg = np.full((W, ccap), np.nan)
    powers = np.zeros((W, pcap))
    done = np.zeros(W, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for f in range(W):
            x = frame_ref(signal, N, hop, f, window, frame_dtype)
            pn0 = po.periodic_norm(x)
            r, off = x, 0
            for a in range(min(max(int(counts[f]), 0), pcap)):
                p = int(periods[f, a])
                if p < 1 or p > N or off + p > ccap:
                    break
                s = po.project(r, p, trunc, False, True)
                seg[f, off : off + p] = s
                nxt = r - np.tile(s, N // p + 1)[:N]
                powers[f, a] = 0.0 if pn0 == 0 else (po.periodic_norm(r) - po.periodic_norm(nxt)) / pn0
                r, off = nxt, off + p
                done[f] = a + 1
    return seg, powers, done


def power_bounds(signal, N, hop, W, window, frame_dtype, periods, done, trunc):
    """1e-10 * pn(r_a) / pn(x_f) for every written block (the bar of the small_to_large census), 0 elsewhere."""
    bound = np.zeros(np.asarray(periods).shape)
    for f in range(W):
        x = frame_ref(np.asarray(signal), N, hop, f, window, frame_dtype)
        pn0 = po.periodic_norm(x)
        r = x
        for a in range(int(done[f])):
            p = int(periods[f, a])
            bound[f, a] = 1e-10 * po.periodic_norm(r) / pn0 if pn0 > 0 else 0.0
            r = r - np.tile(po.project(r, p, trunc, False, True), N // p + 1)[:N]
    return bound


def pack_ref(periods):
    """ShortTime.pack_tracks as a plain loop: -> (packed, counts, masks (T + 1, W) uint64)."""
    periods = np.asarray(periods)
    W, T = periods.shape
    packed = np.zeros((W, T), dtype=np.int32)
    counts = np.zeros(W, dtype=np.int32)
    masks = np.zeros((T + 1, W), dtype=np.uint64)
    for f in range(W):
        a = 0
        for t in range(T):
            if periods[f, t] >= 1:
                packed[f, a] = periods[f, t]
                masks[t, f] = np.uint64(1 << a)
                masks[T, f] |= np.uint64(1 << a)
                a += 1
        counts[f] = a
    return packed, counts, masks


# ------------------------------------------------------------------ the case table
def _signal(seed, L, dtype):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    x = np.sin(2 * np.pi * n / 7.0) + 0.5 * np.sign(np.sin(2 * np.pi * n / 12.0)) + 0.3 * rng.standard_normal(L)
    return x.astype(dtype)


def _window(N):
    return np.sqrt(np.hanning(N + 2)[1:-1]) if N > 1 else np.ones(1)


def make_case(name, N, hop, W, periods, counts, ccap, sig_dtype=F64, frame_dtype=F64, windowed=True, pad=True, seed=0):
    """One case: a signal whose last frame is zero-padded (`pad`) and the arrays of one ph_follow call."""
    L = (W - 1) * hop + (max(1, N - N // 3) if pad else N)
    periods = np.asarray(periods, dtype=np.int32).reshape(W, -1)
    return dict(name=name, N=N, hop=hop, W=W, L=L, signal=_signal(seed + N, L, sig_dtype),
                window=_window(N) if windowed else None, frame_dtype=frame_dtype, periods=periods,
                counts=np.asarray(counts, dtype=np.int32), ccap=int(ccap))


def cases():
    """Periods 1, 2, 63, 64, 65, N - 1, N, divisors and non-divisors of N; pcap 1 and 3; counts 0 and silent frames;
    every stop rule; both signal and frame dtypes; (N, hop) = (37, 5), (64, 64), (48, 61) and N = 130."""
    out = []
    # (37, 5): pcap 3, non-divisors, N - 1 and N, a frame of count 0, a count above pcap and one below 0
    out.append(make_case("n37", 37, 5, 6,
                         [[1, 2, 36], [37, 5, 7], [36, 37, 1], [12, 3, 2], [7, 7, 7], [2, 1, 37]],
                         [3, 3, 3, 0, 9, -2], 37 + 36 + 1))
    # (64, 64): pcap 1, divisors, 63 / 64
    out.append(make_case("n64", 64, 64, 5, [[64], [63], [2], [1], [16]], [1, 1, 1, 1, 0], 64, windowed=False, pad=False))
    # (48, 61): gaps between the frames, float32 signal and frames
    out.append(make_case("n48", 48, 61, 4, [[12, 5, 48], [47, 16, 3], [1, 48, 7], [24, 9, 2]], [3, 2, 3, 3], 70,
                         sig_dtype=F32, frame_dtype=F32))
    # N = 130: periods 63, 64, 65 on either side of a wavefront, more threads than one wavefront
    out.append(make_case("n130", 130, 33, 4, [[63, 64, 65], [65, 13, 10], [129, 130, 1], [64, 2, 63]], [3, 3, 3, 3], 260))
    # float64 signal rounded to float32 frames, and float32 signal widened to float64 frames
    out.append(make_case("n37_f32frames", 37, 5, 3, [[5, 9, 37], [36, 2, 1], [11, 4, 6]], [3, 3, 3], 80, frame_dtype=F32))
    out.append(make_case("n37_f32signal", 37, 5, 3, [[5, 9, 37], [36, 2, 1], [11, 4, 6]], [3, 3, 3], 80, sig_dtype=F32))
    # the stop rules: p < 1 (0 and negative), p > N, off + p > ccap (exactly ccap still fits), each with live blocks behind
    out.append(make_case("stops", 37, 5, 7,
                         [[5, 0, 7], [-3, 5, 7], [5, 38, 7], [20, 20, 7], [21, 9, 7], [37, 1, 1], [2**31 - 1, 2, 3]],
                         [3, 3, 3, 3, 3, 3, 3], 30))
    # a long frame: several samples per thread in every pass, rows in the dozens
    out.append(make_case("n700", 700, 180, 3, [[23, 350, 699], [700, 64, 1], [128, 27, 2]], [3, 3, 3], 1100))
    return out


def glide_track(N, hop, W, true_period):
    """The true period at the centre of every frame, rounded."""
    return np.array([int(round(true_period(f * hop + N / 2.0))) for f in range(W)], dtype=np.int32)
