"""The numpy restatement of ph_period_path's definition (include/periodhip.h) and the cost tables that
tests/test_period_path_cpu.py and tests/test_gpu_period_path.py share.

The restatement is the definition line by line: pen[o] = jump * o from a table, every difference and sum one float64
operation, offsets tried in the order 0, -1, +1, -2, +2, ... with a strict comparison, the first maximum of the last
row, the walk back.  numpy's element-wise float64 arithmetic rounds once per operation, so the kernel is held to this
bit for bit, not to a tolerance."""

import itertools

import numpy as np

PH_ST_OK, PH_ST_NO_PERIOD = 0, 1


def period_path_ref(cost, band, jump):
    """-> (path (W,) int32, values (W,) float64, score float64, status) for cost (W, P)."""
    c = np.asarray(cost, dtype=np.float64)
    W, P = c.shape
    band = int(band)
    cs = np.where(np.isfinite(c), c, -np.inf)
    pen = np.array([np.float64(jump) * np.float64(o) for o in range(band + 1)], dtype=np.float64)
    H = band
    D = np.full(P + 2 * H, -np.inf)  # the row with `band` forbidden cells on either side
    D[H : H + P] = cs[0]
    bp = np.zeros((W, P), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for f in range(1, W):
            best = D[H : H + P] - pen[0]
            off = np.zeros(P, dtype=np.int64)
            # (an offset of P or more leaves the row from every state: -inf, never strictly greater, not tried)
            for o in range(1, min(band, P - 1) + 1):
                for sgn in (-1, 1):
                    cand = D[H + sgn * o : H + sgn * o + P] - pen[o]
                    take = cand > best
                    best = np.where(take, cand, best)
                    off[take] = sgn * o
            D[H : H + P] = cs[f] + best
            bp[f] = off
    last = D[H : H + P]
    end = int(np.argmax(last))  # the first maximum
    score = np.float64(last[end])
    if score == -np.inf:
        return np.full(W, -1, np.int32), np.zeros(W), score, PH_ST_NO_PERIOD
    path = np.empty(W, dtype=np.int32)
    path[W - 1] = end
    for f in range(W - 1, 0, -1):
        path[f - 1] = path[f] + bp[f, path[f]]
    return path, c[np.arange(W), path], score, PH_ST_OK


def brute_force(cost, band, jump):
    """Exhaustive search over all paths of a small integer-valued table with a dyadic jump (every sum exact):
    -> (best score or -inf, the list of all paths that reach it)."""
    c = np.asarray(cost, dtype=np.float64)
    W, P = c.shape
    best, paths = -np.inf, []
    for p in itertools.product(range(P), repeat=W):
        if any(abs(p[f] - p[f - 1]) > band for f in range(1, W)):
            continue
        if not all(np.isfinite(c[f, p[f]]) for f in range(W)):
            continue
        s = sum(c[f, p[f]] for f in range(W)) - sum(jump * abs(p[f] - p[f - 1]) for f in range(1, W))
        if s > best:
            best, paths = s, [p]
        elif s == best:
            paths.append(p)
    return best, paths


# ------------------------------------------------------------------ cost tables
def random_cost(seed, W, P):
    return np.random.default_rng(seed).standard_normal((W, P))


def tie_cost(seed, W, P, levels=3):
    """Integer costs from a few levels: ties everywhere, so the order of the offsets and the lowest end state decide."""
    return np.random.default_rng(seed).integers(0, levels, (W, P)).astype(np.float64)


def ridge_cost(W, P, step, start=None, height=100.0):
    """Zeros with one cell of `height` per frame that moves by +step, -step, +step, ... (reflected inside the table)."""
    c = np.zeros((W, P))
    j = P // 2 if start is None else start
    for f in range(W):
        c[f, j] = height
        d = step if f % 2 == 0 else -step
        if not 0 <= j + d < P:
            d = -d
        if 0 <= j + d < P:
            j += d
    return c


def pinned_cost(W, P, column):
    """The best path is `column` in every frame: the states whose neighbourhood reaches into a halo."""
    c = np.random.default_rng(P + column).standard_normal((W, P))
    c[:, column] += 50.0
    return c


def with_forbidden(cost, seed, frac=0.2):
    """NaN, +inf and -inf sprinkled over a copy of the table."""
    rng = np.random.default_rng(seed)
    c = np.array(cost, dtype=np.float64)
    kind = rng.random(c.shape)
    c[kind < frac / 3] = np.nan
    c[(kind >= frac / 3) & (kind < 2 * frac / 3)] = np.inf
    c[(kind >= 2 * frac / 3) & (kind < frac)] = -np.inf
    return c


def with_dead_frame(cost, frame):
    """A copy whose row `frame` holds no finite value (a mix of NaN and both infinities)."""
    c = np.array(cost, dtype=np.float64)
    c[frame] = np.resize([np.nan, np.inf, -np.inf], c.shape[1])
    return c


def glide_signal(L=4096):
    """A pulse train whose period glides from 20 to 30 samples over L samples, 5 % noise, mean removed, and the true
    period at sample n."""
    x = np.zeros(L)
    t = 0.0
    while t < L:
        x[int(t)] = 1.0
        t += 20.0 + 10.0 * t / L
    x += 0.05 * np.random.default_rng(0).standard_normal(L)
    return x - x.mean(), lambda n: 20.0 + 10.0 * n / L
