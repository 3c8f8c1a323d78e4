"""m_best step 2 (k_mbest_step2, Periods.py:540-598) on the CPU: the oracle's step-2 trace tied to the reference's own
fixtures, a restatement of the kernel's path predicates, and the case table of tests/test_gpu_m_best_step2.py with the
census that keeps it honest.

The kernel has a compact row form folded from a count-scaled p-vector (`short_row`), a tiled row form, a staging area
into which the next composite row is prefetched, splits as slot permutations, a general (trunc / orth) path and an HBM
window.  Which of these a call takes is decided by N, the periods step 1 picked and what the loop does to them, so the
table below is stated as signals -- sums of zero-mean random periodic components with integer periods plus noise, see
`signal` -- and `walk` replays the oracle's trace through the kernel's predicates to say which paths each case takes.
`CHECKLIST` names every path the GPU tests are meant to pin; the census asserts that the table as a whole contains each
of them, and that every decision of every case is far enough from a tie for a summation-order difference not to flip it
(step-1 gaps, step-2 leads and the three acceptance margins >= 1e-6 in fp64, >= 1e-2 on float32 input: four and two
decades above the 1e-10 / 1e-4 bars the kernels are held to).
"""

import functools

import numpy as np
import pytest

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

BLOCK = 512  # k_mbest_step2's workgroup in plain mode (the general path runs 256 and stages nothing)
KPAD = 256
PRE = 3  # kStep2Pre: a staged row has at most 3 elements per thread
GAP64, GAP32 = 1e-6, 1e-2


# ------------------------------------------------------------------------------------------ generator
def signal(n, comps, seed, noise=0.05, dtype=np.float64):
    """Sum of zero-mean random periodic components ((period, rms amplitude), ...) plus white noise of rms `noise`."""
    rng = np.random.default_rng(seed)
    x = noise * rng.standard_normal(n)
    for p, amp in comps:
        v = rng.standard_normal(p)
        v -= v.mean()
        v *= amp / np.sqrt(np.mean(v * v))
        x = x + np.tile(v, n // p + 1)[:n]
    return x.astype(dtype)


# ------------------------------------------------------------------------------------------ the kernel's predicates
def row_stride(max_length):
    return (max_length + 127) & ~127


def n_divisors(p):
    return len(po.factor_set(p, True)) if p > 1 else 0


def short_row(n, per, plain64=True):
    """Factor norms folded from the count-scaled p-vector and its phantom extra row: fp64, plain projection only."""
    return plain64 and per + per // 2 + 256 <= n + KPAD


def pieces(pn):
    return -(-pn // 128)


def staged(n, per, pn, max_length, plain64=True, lds_window=True, block=BLOCK):
    """Whether the iteration on a row of period `per` prefetches the next composite row (period `pn`) into the upper
    part of the row buffer.  The last two terms keep the DMA inside the compact row and the staged divisor list."""
    zend = per + per // 2 + 256
    so = (zend + 1) & ~1
    return (lds_window and short_row(n, per, plain64) and pn <= PRE * block and pn + pn // 2 + 256 <= n + KPAD
            and so + 128 * pieces(pn) <= n and 128 * pieces(pn) <= row_stride(max_length) and n_divisors(pn) <= 64)


def walk(n, max_length, trace, plain64=True, lds_window=True):
    """The kernel's loop over the oracle's step-2 trace: it visits composite rows only, knows the next composite row one
    iteration ahead, and forgets what it staged when it splits.  -> one dict per kernel iteration."""
    out = []
    stage_row, prev_split, first = -1, False, True
    for rec in trace["step2"]:
        if not rec["divisors"]:
            continue  # next_row(): a prime (or an unfilled row) is not even read
        i, per, periods = rec["i"], rec["period"], rec["periods"]
        nxt = [k for k in range(i + 1, len(periods)) if n_divisors(int(periods[k]))]
        pn = int(periods[nxt[0]]) if nxt else 0
        it = dict(rec, short=short_row(n, per, plain64), from_stage=stage_row == i, first=first, after_split=prev_split,
                  pn=pn, stages=bool(nxt) and staged(n, per, pn, max_length, plain64, lds_window))
        it["pieces"] = pieces(pn) if it["stages"] else 0
        out.append(it)
        stage_row = nxt[0] if it["stages"] else -1
        prev_split = rec["outcome"] == "split"
        if prev_split:
            stage_row = -1
        first = False
    return out


# ------------------------------------------------------------------------------------------ the case table
def case(name, n=None, comps=(), seed=0, num=5, max_length=None, min_length=2, gamma=False, trunc=False, orth=False, dtype=np.float64,
         noise=0.05, items=""):
    return dict(name=name, n=n, comps=tuple(comps), seed=seed, noise=noise, num=num, min_length=min_length,
                max_length=max_length, gamma=gamma, trunc=trunc, orth=orth, dtype=dtype, items=items)


F32 = np.float32
# one shape per mixed launch: every window of a call shares N, num and max_length
MIXED_PLAIN = dict(n=700, num=5, max_length=48)
MIXED_GAMMA = dict(n=700, num=5, max_length=24, gamma=True)
_TRUNC = dict(n=402, comps=((2, 1.74), (4, 1.56), (5, 0.88), (9, 1.12), (16, 1.67)), seed=0, num=6, max_length=48)

CASES = [
    # ---- fp64, plain projection, N <= 1000
    case("cascade_present", 1000, ((3, 1.64), (7, 2.07), (9, 0.7), (13, 0.55), (16, 2.83)), 996, 6, 36, items="abcdej"),
    case("two_cascades", 402, ((4, 2.75), (8, 1.55), (11, 1.31)), 771, 6, 100, noise=0.2, items="abcd"),
    case("n_small_at_floor", 1000, ((6, 0.5), (14, 2.14), (20, 0.62), (30, 0.25)), 892, 6, 30, items="abe"),
    case("one_row", 402, ((4, 1.0), (9, 1.0)), 1, 1, 40, items="j"),
    case("mix_cascade", comps=((3, 2.35), (4, 1.72), (7, 0.33), (8, 0.69), (16, 0.44)), seed=142, noise=0.5, items="bc", **MIXED_PLAIN),
    case("mix_primes", comps=((29, 2.0), (31, 1.4), (37, 1.0), (41, 0.7), (43, 0.5)), seed=1, items="", **MIXED_PLAIN),
    case("mix_present", comps=((5, 1.92), (7, 1.45), (11, 0.42), (13, 0.88), (16, 0.34)), seed=718, noise=0.2, items="abd", **MIXED_PLAIN),
    case("mix_last", comps=((7, 0.32), (11, 0.42)), seed=547, noise=0.5, items="ab", **MIXED_PLAIN),
    # ---- fp64, plain projection, the larger shapes
    case("two_pieces", 2000, ((16, 1.0), (45, 0.8), (701, 0.5), (709, 0.3)), 0, 5, 720, items="abcdf"),
    case("tiled_split", 1000, ((16, 1.0), (45, 0.8), (701, 0.5)), 1, 4, 720, items="bcg"),
    case("long_short_row", 4000, ((16, 1.0), (105, 0.8), (1601, 0.5), (1607, 0.3)), 17, 4, 1700, min_length=1600, noise=0.2, items="bcfi"),
    case("many_divisors_short", 15200, ((32, 1.0), (315, 0.8), (10007, 0.6)), 0, 3, 10080, min_length=10000, noise=0.2, items="bh"),
    case("many_divisors_tiled", 12000, ((32, 1.0), (315, 0.8), (10007, 0.6)), 0, 4, 10080, min_length=10000, noise=0.2, items="bh"),
    # ---- gamma mode: the stale `p` of Periods.py:559,572 divides every factor norm
    case("gamma_n240", 240, ((5, 2.02), (16, 0.86)), 222, 3, 24, gamma=True, items="bdk"),
    case("gamma_n402", 402, ((13, 0.42), (16, 0.82)), 391, 6, 24, gamma=True, items="bdk"),
    case("gamma_n1000", 1000, ((4, 0.79), (15, 1.13), (16, 0.46)), 407, 4, 24, gamma=True, noise=0.2, items="adek"),
    case("gmix_cascade", comps=((7, 1.07), (16, 1.1)), seed=591, noise=0.2, items="bdk", **MIXED_GAMMA),
    case("gmix_primes", comps=((5, 2.0), (7, 1.4), (11, 1.0), (13, 0.7), (17, 0.5)), seed=1, items="", **MIXED_GAMMA),
    case("gmix_present", comps=((8, 1.67), (10, 1.98), (12, 0.35), (16, 1.95)), seed=738, items="adek", **MIXED_GAMMA),
    case("gmix_last", comps=((2, 1.21), (14, 0.71), (16, 0.75)), seed=885, noise=0.2, items="abdk", **MIXED_GAMMA),
    # ---- float32 input: every row is tiled
    case("f32_cascade", 700, ((3, 0.47), (4, 0.47), (7, 2.74), (8, 0.69), (16, 2.75)), 302, 4, 64, noise=0.5, dtype=F32, items="bc"),
    case("f32_present", 402, ((2, 0.4), (8, 1.93), (13, 1.0), (16, 2.28)), 552, 4, 24, noise=0.5, dtype=F32, items="bd"),
    # ---- trunc / orth: the general path (block_sweep_value, workgroups of 256)
    case("trunc_cascade", trunc=True, items="bcd", **_TRUNC),
    case("orth_rows", orth=True, items="", **_TRUNC),
    case("trunc_orth_rows", trunc=True, orth=True, items="", **_TRUNC),
]


def case_signal(c):
    return signal(c["n"], c["comps"], c["seed"], c["noise"], c["dtype"])


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = BY_NAME[name]
    x = case_signal(c).astype(np.float64)  # float32 cases: the oracle on the float32-rounded input
    tr = {}
    per, pw, bs = po.m_best(x, c["num"], c["max_length"], c["min_length"], c["gamma"], c["trunc"], c["orth"], trace=tr)
    for a in (per, pw, bs):
        a.setflags(write=False)
    return per, pw, bs, tr


BY_NAME = {c["name"]: c for c in CASES}


def oracle_of(c):
    """(periods, powers, bases, trace) of a case: computed once, shared, read-only."""
    return _oracle(c["name"])


def walk_of(c):
    plain64 = c["dtype"] == np.float64 and not (c["trunc"] or c["orth"])
    return walk(c["n"], c["max_length"], oracle_of(c)[3], plain64)


def split_chains(its):
    """Runs of consecutive splits at one position: [(position, [period, factor, factor, ...]), ...]."""
    chains = []
    for k, it in enumerate(its):
        if it["outcome"] != "split":
            continue
        if chains and chains[-1][2] == k - 1 and chains[-1][0] == it["i"]:
            chains[-1][1].append(it["top_f"])
            chains[-1][2] = k
        else:
            chains.append([it["i"], [it["period"], it["top_f"]], k])
    return [(i, ch) for i, ch, _ in chains]


def _alone(it, k):
    return it["outcome"] == "nosplit" and [not h for h in it["holds"]] == [j == k for j in range(3)]


def _present_after_split(c, its):
    step1 = set(int(p) for p in oracle_of(c)[3]["step1_periods"])
    return any(it["outcome"] == "present" and it["top_f"] not in step1 for it in its)


def _plain64(c):
    return c["dtype"] == np.float64 and not (c["trunc"] or c["orth"])


# The three inequalities of the acceptance test (Periods.py:573-575) as `nosplit` reasons.  n_big is the largest factor
# norm and n_small one of them, so `n_big <= floor` never fails alone.  `n_small <= floor` alone needs n_big > norms[i]
# (else the sum inequality gives n_small > norms[num - 1] >= floor): only the remainder row of an earlier split has that,
# because the reference files it under the norm of the last factor's projection, not under its own.
CHECKLIST = {
    "a: split of a row that arrived through the staging area": lambda c, its: any(
        it["from_stage"] and it["outcome"] == "split" for it in its),
    "b: split of the first composite row (never staged)": lambda c, its: any(
        it["first"] and not it["from_stage"] and it["outcome"] == "split" for it in its),
    "b: split of a row visited right after a split (never staged)": lambda c, its: any(
        it["after_split"] and not it["from_stage"] and it["outcome"] == "split" for it in its),
    "c: three or more consecutive splits at one position": lambda c, its: any(
        len(ch) >= 4 for _, ch in split_chains(its)),
    "d: top factor already present after an earlier split put it there": _present_after_split,
    "e: nosplit by the sum inequality alone": lambda c, its: any(_alone(it, 0) for it in its),
    "e: nosplit by n_small <= floor alone": lambda c, its: any(_alone(it, 1) for it in its),
    "f: staged row of two or more 128-element pieces": lambda c, its: any(it["pieces"] >= 2 for it in its),
    "f: next row beyond 1536 elements, not staged behind a short row": lambda c, its: any(
        it["short"] and it["pn"] > PRE * BLOCK and not it["stages"] for it in its),
    "g: fp64 plain split on the tiled path (period > 2N/3)": lambda c, its: _plain64(c) and any(
        it["outcome"] == "split" and not it["short"] and 3 * it["period"] > 2 * c["n"] for it in its),
    "h: more than 64 proper divisors, short row": lambda c, its: _plain64(c) and any(
        len(it["divisors"]) > 64 and it["short"] and it["outcome"] == "split" for it in its),
    "h: more than 64 proper divisors, tiled row": lambda c, its: _plain64(c) and any(
        len(it["divisors"]) > 64 and not it["short"] and it["outcome"] == "split" for it in its),
    "i: split of a short row longer than 1536 elements": lambda c, its: any(
        it["short"] and it["period"] > PRE * BLOCK and 3 * it["period"] < 2 * c["n"] and it["outcome"] == "split"
        for it in its),
    "j: num larger than the number of composite rows": lambda c, its: c["num"] > 1 and 0 < sum(
        n_divisors(int(p)) > 0 for p in oracle_of(c)[3]["step1_periods"]) < c["num"],
    "j: num = 1 (no split is possible)": lambda c, its: c["num"] == 1 and len(its) == 1 and its[0]["outcome"] == "nosplit",
    "k: gamma-mode split (stale p)": lambda c, its: c["gamma"] and any(it["outcome"] == "split" for it in its),
    "k: gamma-mode split with a staged row, N >= 402": lambda c, its: c["gamma"] and c["n"] >= 402 and any(
        it["outcome"] == "split" for it in its) and any(it["stages"] for it in its),
}
# k asks for three gamma-mode cases
AT_LEAST = {"k: gamma-mode split (stale p)": 3}


def smallest_margins(c):
    """(step-1 gap, smallest step-2 lead, smallest acceptance margin) of a case."""
    tr = oracle_of(c)[3]
    leads = [r["lead"] for r in tr["step2"] if r["divisors"]]
    margins = [m for r in tr["step2"] if r["margins"] for m in r["margins"]]
    return tr["step1_min_gap"], min(leads, default=1.0), min(margins, default=1.0)


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name,gamma", [("m_best_gamma", True), ("m_best", False)])
def test_trace_counts_the_reference_s_own_splits(golden, name, gamma):
    """m_best_split.npz records how often np.insert fired inside the reference (three calls per split): the trace's
    `split` records must be as many, in all ten calls."""
    g = golden("m_best_split")
    assert len(g["cases"]) == 5
    for n, ml, num, w in g["cases"]:
        tag = f"{name}_n{n}_ml{ml}_num{num}_w{w}"
        tr = {}
        per, _, _ = po.m_best(multi_sinusoid_window(int(w), int(n)), int(num), int(ml), 2, gamma, trace=tr)
        assert np.array_equal(per, g[tag + "_periods"]), tag
        assert sum(r["outcome"] == "split" for r in tr["step2"]) == int(g[tag + "_splits"]), tag
        assert {r["outcome"] for r in tr["step2"]} <= {"prime", "present", "nosplit", "split"}


def test_trace_shows_the_large_period_fixture_s_split(golden):
    g = golden("m_best_large_p")
    n, ml, num, _ = g["cases"][0]
    tr = {}
    per, _, _ = po.m_best(g[f"x_n{n}"], int(num), int(ml), 2, False, trace=tr)
    assert np.array_equal(per, g[f"m_best_n{n}_ml{ml}_num{num}_periods"])
    assert any(r["outcome"] == "split" and r["period"] == 454 and r["top_f"] == 227 for r in tr["step2"])
    assert not short_row(int(n), 454)  # the tiled path


def test_trace_leaves_the_result_alone():
    x = multi_sinusoid_window(3, 240)
    a = po.m_best(x, 5, 30, 2, True)
    b = po.m_best(x, 5, 30, 2, True, trace={})
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_predicates_at_their_edges():
    assert short_row(600, 400) and not short_row(600, 401)  # per + per // 2 <= N
    assert not short_row(600, 12, plain64=False)
    # N = 240: so + 128 <= N never holds (so >= 2 + 1 + 256)
    assert not any(staged(240, p, q, 30) for p in range(4, 31) for q in range(4, 31))
    assert staged(700, 36, 12, 40) and pieces(12) == 1
    assert staged(2000, 720, 240, 720) and pieces(240) == 2
    assert not staged(2000, 720, 240, 720, lds_window=False)
    assert not staged(4000, 12, 1680, 1700) and staged(4000, 12, 1536, 1700)  # kStep2Pre * blockDim
    assert not staged(700, 36, 200, 40)  # a piece would leave the compact row (row_stride = 128)
    assert n_divisors(10080) == 70 and not staged(15200, 12, 10080, 10080)


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_every_decision_of_a_case_is_far_from_a_tie(c):
    gap, lead, margin = smallest_margins(c)
    bar = GAP64 if c["dtype"] == np.float64 else GAP32
    print(f"{c['name']}: step-1 gap {gap:.3g}, step-2 lead {lead:.3g}, margin {margin:.3g}")
    assert gap >= bar and lead >= bar and margin >= bar, (gap, lead, margin)
    its = walk_of(c)
    for label in c["items"]:  # what the table says the case is there for
        hits = [k for k in CHECKLIST if k.startswith(label + ":")]
        assert hits and any(CHECKLIST[k](c, its) for k in hits), (c["name"], label)


def test_the_table_contains_every_path():
    seen = {k: [] for k in CHECKLIST}
    for c in CASES:
        its = walk_of(c)
        for k, hit in CHECKLIST.items():
            if hit(c, its):
                seen[k].append(c["name"])
    for k, where in seen.items():
        print(f"{k}: {where}")
    missing = [k for k, where in seen.items() if len(where) < AT_LEAST.get(k, 1)]
    assert not missing, missing


def _mode(c):
    return ("f32" if c["dtype"] == np.float32 else "f64") + ("_trunc" if c["trunc"] else "") + ("_orth" if c["orth"] else "")


def test_float32_and_trunc_cases_split_on_every_kind_of_row():
    """Items b, c and d once more on float32 input (every row tiled) and under trunc (the general path)."""
    for mode in ("f32", "f64_trunc"):
        hit = set()
        for c in CASES:
            if _mode(c) == mode:
                its = walk_of(c)
                hit |= {k for k, f in CHECKLIST.items() if k[0] in "bcd" and f(c, its)}
        assert hit == {k for k in CHECKLIST if k[0] in "bcd"}, (mode, hit)


def test_orth_rows_have_nothing_left_in_their_divisor_subspaces():
    """Why no orth case splits.  With orthogonalize the stored row of period p is P_p x minus its projections onto p / f
    for the prime f | p (Periods.py:208-214), which is orthogonal to the subspace of every proper divisor; step 2 projects
    that row onto the divisors again, so its factor norms are rounding noise (with trunc: the defect of averaging complete
    rows only, a fraction of a percent of the row) and `n_small > floor` cannot hold unless a row of the result is itself
    noise, which the margin rule above excludes.  (A scan of 14 000 composite rows of random signals under orth and
    trunc + orth found no split.)  The two orth cases therefore pin the general path on composite rows that stay."""
    for name, bound in (("orth_rows", 1e-12), ("trunc_orth_rows", 2e-2)):
        c = BY_NAME[name]
        tr = oracle_of(c)[3]
        rows = [r for r in tr["step2"] if r["divisors"]]
        assert len(rows) >= 3 and all(r["outcome"] in ("present", "nosplit") for r in rows)
        assert all(r["n_big"] <= bound * tr["step1_norms"].min() for r in rows), [r["n_big"] for r in rows]
