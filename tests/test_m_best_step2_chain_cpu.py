"""m_best step 2 (k_mbest_step2) with the factor geometry read from the host's table, on the CPU: more small cases for
the row and split paths, and the equality of the table with what the kernel computed itself.

In the fp64 plain path a wavefront folds one factor f of a row at a time on the geometry of (N, f).  The kernel used to
rebuild it per factor (make_geom: an integer and two fp64 divisions in lane 0, handed over through LDS); it now reads
geom[f], the table prepare_geom fills on the host (PH_STEP2_GEOM=0: the old way).  The cases below are small windows --
N = 330 with periods up to 240, so that rows beyond 2N/3 take the tiled path beside short ones and nothing can be
staged; N = 700 with periods up to 48, where composite rows are staged -- and, for what a small window cannot hold
(a divisor list beyond 64 entries, staged rows of several pieces), cases of tests/test_m_best_step2_cpu.py.  `walk` of
that module replays the oracle's step-2 trace through the kernel's predicates; CHECKLIST names the paths the table
must contain, and every decision of every new case is at least 1e-6 from a tie.
tests/test_gpu_m_best_step2_chain.py runs the table with the switch on and off."""

import functools

import numpy as np
import pytest

from oracle import period_oracle as po
from test_m_best_step2_cpu import BY_NAME, GAP64, case, case_signal, n_divisors, smallest_margins, split_chains, walk
from test_m_best_step2_cpu import oracle_of as _table_oracle

# every window of a mixed launch shares N, num and max_length
MIXED_LONG = dict(n=330, num=5, max_length=240)
MIXED_STAGED = dict(n=700, num=5, max_length=48)

NEW_CASES = [
    case("chain_prime_factor", comps=((2, 1.92), (5, 1.84)), seed=764, noise=0.2, items="ace", **MIXED_LONG),
    case("chain_cascade", comps=((15, 2.67), (26, 1.08), (35, 1.36)), seed=273, noise=0.5, items="be", **MIXED_LONG),
    case("chain_present_after_split", comps=((4, 1.8), (8, 2.12), (10, 0.77), (14, 0.44)), seed=558, noise=0.05, items="bce", **MIXED_LONG),
    case("chain_after_prime", comps=((11, 1.49), (18, 1.38)), seed=139, noise=0.5, items="ae", **MIXED_LONG),
    case("chain_long_short", comps=((15, 0.3), (222, 1.35), (235, 1.88)), seed=564, noise=0.5, items="f", **MIXED_LONG),
    case("chain_split_last", comps=((8, 0.99), (9, 2.34), (10, 0.37), (18, 2.28)), seed=348, noise=0.5, items="d", **MIXED_STAGED),
    case("chain_num2", 330, ((18, 1.16),), 946, 2, 240, noise=0.2, items="eg"),
    case("chain_num1", 330, ((21, 2.24), (24, 0.86)), 55, 1, 240, noise=0.05, items="g"),
]
# cases of the older table that run here too: the staged shapes and what a small window cannot hold
OLD_CASES = [BY_NAME[k] for k in ("mix_cascade", "mix_primes", "mix_present", "mix_last", "two_pieces", "tiled_split",
                                  "long_short_row", "many_divisors_short")]
CASES = NEW_CASES + OLD_CASES
NEW_BY_NAME = {c["name"]: c for c in NEW_CASES}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = NEW_BY_NAME[name]
    tr = {}
    per, pw, bs = po.m_best(case_signal(c), c["num"], c["max_length"], c["min_length"], trace=tr)
    for a in (per, pw, bs):
        a.setflags(write=False)
    return per, pw, bs, tr


def oracle_of(c):
    """(periods, powers, bases, trace) of a case: computed once, shared, read-only."""
    return _oracle(c["name"]) if c["name"] in NEW_BY_NAME else _table_oracle(c)


def walk_of(c):
    """The kernel's iterations (walk) with what went before each: a skipped prime row directly above it or not."""
    tr = oracle_of(c)[3]
    its = walk(c["n"], c["max_length"], tr)
    recs, used = tr["step2"], set()
    for it in its:
        k = next(j for j, r in enumerate(recs) if j not in used and r["i"] == it["i"] and r["period"] == it["period"]
                 and r["outcome"] == it["outcome"] and r["divisors"])
        it["after_prime"] = k > 0 and recs[k - 1]["outcome"] == "prime" and recs[k - 1]["i"] == it["i"] - 1
        used.add(k)  # (a row may be visited twice with the same outcome: each record serves once)
    return its


def _prime_factor(c, its):
    """a split whose factor is prime: the remainder (same period, one row down) is what the loop examines next"""
    return any(a["outcome"] == "split" and n_divisors(a["top_f"]) == 0 and b["i"] == a["i"] + 1 and b["period"] == a["period"]
               for a, b in zip(its, its[1:]))


def _long_around_short(c, its):
    pairs = [(a["short"], b["short"]) for a, b in zip(its, its[1:]) if a["outcome"] != "split"]
    return (True, False) in pairs and (False, True) in pairs


CHECKLIST = {
    "a: split whose factor is prime, the remainder examined next": _prime_factor,
    "b: three or more consecutive splits at one position": lambda c, its: any(len(ch) >= 4 for _, ch in split_chains(its)),
    "c: split blocked by `present` right after a split": lambda c, its: any(
        it["after_split"] and it["outcome"] == "present" for it in its),
    "d: split at i == num - 1 (the row falls off, no remainder)": lambda c, its: any(
        it["outcome"] == "split" and it["i"] == c["num"] - 1 for it in its),
    "e: split of the first examined row (unstaged)": lambda c, its: bool(its) and its[0]["outcome"] == "split" and not its[0]["from_stage"],
    "e: split of an unstaged row behind a skipped prime": lambda c, its: any(
        it["after_prime"] and not it["from_stage"] and it["outcome"] == "split" for it in its),
    "e: split of a row whose divisor list exceeds 64 entries (unstaged)": lambda c, its: any(
        len(it["divisors"]) > 64 and it["short"] and not it["from_stage"] and it["outcome"] == "split" for it in its),
    "f: a tiled row directly before and directly after a short one": _long_around_short,
    "g: num = 1": lambda c, its: c["num"] == 1 and len(its) == 1,
    "g: num = 2": lambda c, its: c["num"] == 2 and any(it["outcome"] == "split" for it in its),
    "h: split of a row that arrived through the staging area": lambda c, its: any(
        it["from_stage"] and it["outcome"] == "split" for it in its),
    "h: a factor below 64 and one of 64 or more folded for one row": lambda c, its: any(
        min(it["divisors"]) < 64 <= max(it["divisors"]) for it in its),
}


# ------------------------------------------------------------------------------------------ tests
def test_case_names_are_unique():
    assert len({c["name"] for c in CASES}) == len(CASES) and not set(NEW_BY_NAME) & set(BY_NAME)


@pytest.mark.parametrize("c", NEW_CASES, ids=lambda c: c["name"])
def test_every_decision_of_a_new_case_is_far_from_a_tie(c):
    tr = oracle_of(c)[3]
    leads = [r["lead"] for r in tr["step2"] if r["divisors"]]
    margins = [m for r in tr["step2"] if r["margins"] for m in r["margins"]]
    gap, lead, margin = tr["step1_min_gap"], min(leads, default=1.0), min(margins, default=1.0)
    print(f"{c['name']}: step-1 gap {gap:.3g}, step-2 lead {lead:.3g}, margin {margin:.3g}")
    assert gap >= GAP64 and lead >= GAP64 and margin >= GAP64, (gap, lead, margin)
    assert c["dtype"] == np.float64 and not (c["trunc"] or c["orth"] or c["gamma"]) and 200 <= c["n"] <= 700 and c["num"] <= 6
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
    assert not [k for k, where in seen.items() if not where]


def test_the_older_cases_keep_their_margins():
    for c in OLD_CASES:
        assert min(smallest_margins(c)) >= GAP64, c["name"]


def test_table_geometry_is_the_kernel_s_own():
    """The factor folds take nfull, w_full = 1 / R and w_short = 1 / (R - 1) of geom[f] (the host's table: R from the
    integer ceiling, the quotients in IEEE double precision) where the fallback evaluates make_geom(N, f) on the device
    (the same integer expressions, 1.0 / (double)R: one correctly rounded division).  Both forms, stated as written,
    must agree bit for bit for every f <= 2048 at every window length the tests and the benchmark run, and a quotient
    must lie where a single rounding of the exact quotient puts it."""
    from fractions import Fraction

    lengths = sorted({c["n"] for c in CASES} | {240, 402, 1000, 1024, 4096})
    f = np.arange(1, 2049, dtype=np.int64)
    for n in lengths:
        rows_t = (n + f - 1) // f  # prepare_geom
        table = np.stack([rows_t, f - (rows_t * f - n), 1.0 / rows_t, np.where(rows_t > 1, 1.0 / np.maximum(rows_t - 1, 1), 0.0)])
        rows_k = -(-n // f)  # make_geom: ceil(N / f)
        own = np.stack([rows_k.astype(np.float64), (f - (rows_k * f - n)).astype(np.float64), np.float64(1.0) / rows_k.astype(np.float64),
                        np.where(rows_k > 1, np.float64(1.0) / np.maximum(rows_k - 1, 1).astype(np.float64), 0.0)])
        assert np.array_equal(table.astype(np.float64).view(np.uint64), own.view(np.uint64)), n
        assert np.all((table[1] >= 1) & (table[1] <= f))
    for r in (3, 7, 683, 2047):  # a correctly rounded quotient lies within half an ulp (2^-53 relative) of the exact one
        assert abs(Fraction(float(np.float64(1.0) / np.float64(r))) - Fraction(1, r)) <= Fraction(1, r) / 2 ** 53
