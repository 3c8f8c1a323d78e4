"""Case table of the Ramanujan census (test_ramanujan_census_cpu.py, test_gpu_ramanujan_census.py): the (N, q_lo, q_hi)
calls, their windows, the oracle's answers, and a restatement in Python integers of what the host derives from a call
(ram_prepare in period_hip.hip) and of the branch each derived number selects in k_ramanujan (ph_ram.h).  `classify`
turns a case into the set of CLASSES labels it reaches; the CPU census asserts that the table as a whole reaches every
label, so the GPU test can say which fold shapes and factor sets it ran.

Every case has four windows, seeded by (N, q_hi) alone:
  (a) white noise;  (b) noise + 1e3;  (c) a unit impulse at n = N - 1;  (d) a period-12 pattern + 0.1 noise.
A case with a third entry below four runs only its first windows (the one wide range that pays for k >= 9 children).
"""

import functools

import numpy as np

from oracle import period_oracle as po

SEED = 20261
TOL = 1e-10  # the suite's fp64 tolerance; here in units of B_q (po.ramanujan_norm_projector_q)
KINDS = "abcd"
WAVES = 16  # kRamMaxWaves

# group -> ((N, q_lo, q_hi[, windows]), ...).  Single roots q_lo == q_hi == Q sweep N = rows Q - s: U = 1 .. 8 at k = 1,
# the batch splits (k, U, rem), the chunk tails and the masks of the partial last row; then the ranges.
GROUPS = {
    # one root of 64 or more: rows 1 .. 8 (k = 1, U = rows), tails 1, 2, 3, 0, nfull == Q, nfull == 1, Q % 64 != 0
    "root_rows": (
        (64, 64, 64), (127, 64, 64), (3 * 100 - 99, 100, 100), (4 * 130 - 7, 130, 130), (5 * 192, 192, 192),
        (6 * 200 - 150, 200, 200), (7 * 256 - 255, 256, 256), (8 * 70 - 3, 70, 70)),
    # k >= 2: rows 9 (k 2, U 4, rem 1), 10 (U 5, rem 0), 11 (U 5, rem 1), 14 (U 7, rem 0), 15 (U 7, rem 1), 17 (k 3,
    # U 5, rem 2), 24 (k 3, U 8), ...  U = 4 with rem == 0 exists at k = 1 only: 4 k rows make ceil(k / 2) batches
    "root_batches": (
        (9 * 66 - 5, 66, 66), (10 * 64, 64, 64), (11 * 129 - 128, 129, 129), (14 * 65 - 1, 65, 65), (15 * 64 - 63, 64, 64),
        (17 * 72 - 9, 72, 72), (24 * 64 - 1, 64, 64), (25 * 80 - 79, 80, 80), (33 * 64 - 20, 64, 64), (19 * 96, 96, 96),
        (20 * 67 - 66, 67, 67), (21 * 64 - 3, 64, 64), (39 * 64 - 1, 64, 64)),
    # nfull <= 64 under a root of 5 and more chunks: whole groups of chunks without a last row
    "root_masks": ((3 * 320 - 319, 320, 320), (2 * 321 - 300, 321, 321), (4 * 520 - 470, 520, 520), (12 * 300 - 299, 300, 300)),
    "small_roots": (
        (200, 1, 1), (200, 1, 2), (200, 1, 3), (200, 2, 3), (97, 61, 61), (300, 32, 32), (301, 33, 64), (500, 17, 32),
        (250, 20, 63), (90, 1, 127), (64, 1, 32)),
    # Q >= N, N >= 64 and N < 64
    "long_periods": (
        (100, 99, 99), (100, 100, 100), (100, 101, 101), (100, 200, 200), (100, 60, 200), (100, 1, 101),
        (40, 39, 39), (40, 40, 40), (40, 41, 41), (40, 80, 80), (40, 1, 80), (33, 20, 34), (70, 69, 71), (64, 63, 65)),
    # children: q < 64 and q = 1, k = 2 .. 8 at q >= 64
    "children": ((700, 1, 128), (1000, 1, 256), (900, 64, 512), (1111, 64, 576), (777, 2, 130)),
    # children with k >= 9, odd and even: the one wide range, two windows
    "wide": ((1300, 64, 768, 2),),
    # projector steps: primes of 256 and more (d == 1), d >= 64 with r = 2, 3, 5, 7 and other primes, d < 64 in every
    # row-group count, LAST and not; up to five steps
    "steps": (
        (600, 251, 263), (1500, 120, 130), (997, 30, 66), (2000, 440, 450), (1700, 536, 540), (2200, 700, 720),
        (1800, 380, 390), (1500, 640, 650), (2100, 1001, 1001), (3000, 1150, 1160)),
    "five_primes": ((4700, 2304, 2312), (5000, 2726, 2732)),
    "edges": ((300, 5, 4), (300, 100, 99), (300, 51, 100), (300, 50, 100), (300, 65, 128), (300, 64, 128)),
}
CASES = tuple(c for g in GROUPS.values() for c in g)

CLASSES = tuple(
    [f"root fold: k = 1, U = {u}" for u in range(1, 9)]
    + [f"root fold: k >= 2, U = {u}, rem == 0" for u in (5, 7, 8)]
    + [f"root fold: k >= 2, U = {u}, rem > 0" for u in (4, 5, 7)]
    + ["root fold: k >= 3"]
    + [f"root fold: chunk tail {t}" for t in range(4)]
    + ["root fold: nfull == Q", "root fold: nfull == 1", "root fold: nfull <= 64 under 5+ chunks",
       "root fold: Q % 64 != 0", "root fold: 2+ groups of 4 chunks"]
    + ["root < 64", "root < 64: prime", "root < 64: power of two", "root < 64: several row groups"]
    + [f"Q = {name}, N {side} 64" for name in ("N - 1", "N", "N + 1", "2 N") for side in (">=", "<")]
    + ["child of a root >= N", "child: q < 64", "child: q == 1"]
    + [f"child: q >= 64, k = {k}" for k in range(2, 9)]
    + ["child: q >= 64, k >= 9 odd", "child: q >= 64, k >= 9 even"]
    + [f"step: d < 64, G = {g}, LAST" for g in (1, 2, 3, 4, 8, 16, 32, 64)]
    + [f"step: d < 64, G = {g}, not LAST" for g in (1, 2, 3, 4)]
    + ["step: d == 1, q >= 256 (four loads per trip + remainder)"]
    + [f"step: d >= 64, r = {r}, {w}" for r in (2, 3, 5, 7) for w in ("LAST", "not LAST")]
    + ["step: d >= 64, other prime r, LAST", "step: d >= 64, other prime r, not LAST"]
    + [f"steps: {n}" for n in range(6)]
    + ["range: q_lo == q_hi", "range: q_lo > q_hi", "range: no child", "range: one child", "range: q_hi == 1",
       "range: q_hi == 2", "range: q_hi == 3", "range: roots >= 4 x 16 wavefronts", "range: roots == 16 wavefronts"]
)


# --------------------------------------------------------------------------------------------- the host, restated
@functools.lru_cache(maxsize=None)
def primes_of(q):
    """Distinct primes of q, ascending (ram_prepare's sieve order)."""
    out, m, d = [], q, 2
    while d * d <= m:
        if m % d == 0:
            out.append(d)
            while m % d == 0:
                m //= d
        d += 1
    if m > 1:
        out.append(m)
    return tuple(out)


def steps(q):
    """The factors (I - P_d) of E_q as the record lists them: (r, d = q / r) for each prime r | q, ascending r."""
    return tuple((r, q // r) for r in primes_of(q))


def geometry(n, q):
    """rows = ceil(N / q), nfull = N - (rows - 1) q: residues below nfull own `rows` samples, the others rows - 1."""
    rows = -(-n // q)
    return rows, n - (rows - 1) * q


def batches(rows):
    """ram_root_fold: k = ceil(rows / 8) batches of U or U + 1 rows, rem of them with U + 1."""
    k = (rows + 7) >> 3
    u = 1
    while (u + 1) * k <= rows:
        u += 1
    return k, u, rows - u * k


def assign(n, q_lo, q_hi):
    """ram_prepare's root plan: -> {root Q: [children in the order they were handed out]} for the roots that are
    launched (Q >= q_lo, or with a child), in launch order (decreasing load, stable)."""
    if q_lo > q_hi:
        return {}
    half = q_hi // 2
    kids = {Q: [] for Q in range(half + 1, q_hi + 1)}
    load = {Q: n + Q for Q in kids}
    for q in range(min(half, q_hi), q_lo - 1, -1):
        best = 0
        for Q in range((half // q + 1) * q, q_hi + 1, q):
            if not best or load[Q] < load[best]:
                best = Q
        kids[best].append(q)
        load[best] += 2 * best + 4 * q
    order = [Q for Q in kids if Q >= q_lo or kids[Q]]
    order.sort(key=lambda Q: -load[Q])  # (stable)
    return {Q: kids[Q] for Q in order}


def _step_labels(q):
    out = {f"steps: {len(steps(q))}"}
    st = steps(q)
    for i, (r, d) in enumerate(st):
        last = "LAST" if i == len(st) - 1 else "not LAST"
        if d < 64:
            out.add(f"step: d < 64, G = {64 // d}, {last}")
            if d == 1 and q >= 256:
                out.add("step: d == 1, q >= 256 (four loads per trip + remainder)")
        elif r in (2, 3, 5, 7):
            out.add(f"step: d >= 64, r = {r}, {last}")
        else:
            out.add(f"step: d >= 64, other prime r, {last}")
    return out


def classify(case):
    """The CLASSES labels (and others of the same families, e.g. further G) that the call reaches."""
    n, q_lo, q_hi = case[:3]
    out = set()
    plan = assign(n, q_lo, q_hi)
    if q_lo > q_hi:
        return {"range: q_lo > q_hi"}
    if q_lo == q_hi:
        out.add("range: q_lo == q_hi")
    n_child = sum(len(v) for v in plan.values())
    if q_lo == q_hi // 2 + 1:
        assert n_child == 0
        out.add("range: no child")
    if q_lo == q_hi // 2 and q_lo >= 1:
        assert n_child == 1
        out.add("range: one child")
    if q_hi <= 3:
        out.add(f"range: q_hi == {q_hi}")
    if len(plan) >= 4 * WAVES:
        out.add("range: roots >= 4 x 16 wavefronts")
    if len(plan) == WAVES:
        out.add("range: roots == 16 wavefronts")
    for Q, kids in plan.items():
        rows, nfull = geometry(n, Q)
        if Q < 64:
            out.add("root < 64")
            if primes_of(Q) == (Q,):
                out.add("root < 64: prime")
            if Q & (Q - 1) == 0:
                out.add("root < 64: power of two")
            if 64 // Q >= 2 and n >= 2 * (64 // Q) * Q:
                out.add("root < 64: several row groups")
        else:
            k, u, rem = batches(rows)
            chunks = (Q + 63) >> 6
            if k == 1:
                out.add(f"root fold: k = 1, U = {u}")
            else:
                out.add(f"root fold: k >= 2, U = {u}, rem {'== 0' if rem == 0 else '> 0'}")
            if k >= 3:
                out.add("root fold: k >= 3")
            out.add(f"root fold: chunk tail {chunks & 3}")
            if chunks >= 8:
                out.add("root fold: 2+ groups of 4 chunks")
            if nfull == Q:
                out.add("root fold: nfull == Q")
            if nfull == 1:
                out.add("root fold: nfull == 1")
            if nfull <= 64 and chunks >= 5:
                out.add("root fold: nfull <= 64 under 5+ chunks")
            if Q % 64:
                out.add("root fold: Q % 64 != 0")
        side = ">=" if n >= 64 else "<"
        for name, val in (("N - 1", n - 1), ("N", n), ("N + 1", n + 1), ("2 N", 2 * n)):
            if Q == val and Q >= q_lo:
                out.add(f"Q = {name}, N {side} 64")
        if Q >= q_lo:
            out |= _step_labels(Q)
        for q in kids:
            assert Q % q == 0 and q_lo <= q <= q_hi // 2
            if Q >= n:
                out.add("child of a root >= N")
            if q < 64:
                out.add("child: q < 64")
                if q == 1:
                    out.add("child: q == 1")
            elif Q // q <= 8:
                out.add(f"child: q >= 64, k = {Q // q}")
            else:
                out.add(f"child: q >= 64, k >= 9 {'odd' if (Q // q) & 1 else 'even'}")
            out |= _step_labels(q)
    emitted = sorted([Q for Q in plan if Q >= q_lo] + [q for v in plan.values() for q in v])
    assert emitted == list(range(q_lo, q_hi + 1)), case  # every period of the range exactly once
    return out


def n_windows(case):
    return case[3] if len(case) > 3 else len(KINDS)


# --------------------------------------------------------------------------------------------- windows and the oracle
_WIN = {}
_REF = {}


def windows(case, dtype=np.float64):
    """(n_windows, N) windows (a)-(d) of a case; float32: the float64 windows rounded."""
    n, _, q_hi = case[:3]
    key = (n, q_hi, n_windows(case), np.dtype(dtype).name)
    if key not in _WIN:
        rng = np.random.default_rng([SEED, n, q_hi])
        t = np.arange(n)
        a = rng.standard_normal(n)
        b = rng.standard_normal(n) + 1e3
        c = np.zeros(n)
        c[n - 1] = 1.0
        d = rng.standard_normal(12)[t % 12] + 0.1 * rng.standard_normal(n)
        x = np.stack([a, b, c, d])[: n_windows(case)].astype(dtype)
        x.setflags(write=False)
        _WIN[key] = x
    return _WIN[key]


def ref(case, dtype=np.float64):
    """The oracle's (norms, B) for a case, both (n_windows, q_hi + 1) longdouble with zeros outside [q_lo, q_hi]; for
    float32 on the float32-rounded samples cast to float64.  Computed once and shared; read only."""
    key = (case, np.dtype(dtype).name)
    if key not in _REF:
        n, q_lo, q_hi = case[:3]
        x = windows(case, dtype).astype(np.float64)
        want = np.zeros((x.shape[0], q_hi + 1), dtype=np.longdouble)
        unit = np.zeros_like(want)
        for w in range(x.shape[0]):
            for q in range(q_lo, q_hi + 1):
                want[w, q], unit[w, q] = po.ramanujan_norm_projector_q(x[w], q)
        want.setflags(write=False)
        unit.setflags(write=False)
        _REF[key] = (want, unit)
    return _REF[key]
