"""The sweep census on the CPU: what tests/sweep_cases.py reaches, what its reference rests on, and whether the GPU
bar has teeth.

`test_table_reaches_every_label` asserts that the frozen table reaches every label of sweep_cases.LABELS under the
engines of sweep_cases.ENGINES, or that the label is listed in UNREACHABLE with its argument, and prints every label with
the (case, engine) pairs that reach it (-s; the printout is the failure message too).  `test_unreachable_by_enumeration`
checks the arguments by running the restatement over every N <= 260 (and a few longer windows) and every plan entry.

The reference: sweep_ref (np.longdouble) against the float64 oracle po.sweep_norms in both norm modes, and against the
reference project's own numbers (tests/golden/sweep.npz, N = 4096), entry by entry in units of A_p.

The bar of those two comparisons, REF_BAR = 1e-12, from N <= 2048 (u = 2^-53):
  * the oracle adds the R <= N / 2 rows of a column in order: |S_j - fl(S_j)| <= (R - 1) u sum_r |x[j + r p]|;
  * the mean S_j / cnt_j and its tiling add one rounding each, the norm (a dot product or nrm2 of N terms) at most N u
    relative in the sum of squares, the square root and the one or two divisions 3 u in the value, i.e. 6 u squared;
  * so |N v^2 [p] - ss_p| <= (2 (R - 1) + 2 + N + 6) u A_p <= (2 N + 8) u A_p = 4104 u A_p = 4.6e-13 A_p at N = 2048 (ss_p <= A_p).
The fixture's N = 4096 with p <= N / 3 gives (2 (N / 2) + 2 + N + 6) u = 8200 u = 9.1e-13: the same bar holds.

Teeth: every mutant of sweep_cases.mutant_moves has to move its entry by more than 10 BAR A_p on the two seeded noise
rows of every case; at most 0.1 % of the (period, mutant) pairs of a case may stay inside (a dropped sample cancels when
2 S_j ~ x_n).  This is a condition on the seeds of the table and is asserted.

Measured: see profiles/sweep_census/README.md.
"""

import collections

import numpy as np
import pytest

import sweep_cases as sc
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


def census(cus=sc.CUS):
    carriers = collections.defaultdict(list)
    for case in sc.CASES:
        for engine in sc.ENGINES:
            for label in sc.case_labels(case["n"], case["p_lo"], case["p_hi"], engine, sc.N_ROWS, cus):
                carriers[label].append(f"{case['name']}/{engine}")
    return carriers


def census_text(carriers):
    lines = []
    for label in sc.LABELS:
        names = carriers.get(label, [])
        cases = sorted({n.split("/")[0] for n in names})
        lines.append(f"{len(names):3d}  {label}: " + (", ".join(cases) if names else "UNREACHABLE: " + sc.UNREACHABLE.get(label, "?")))
    return "\n".join(lines)


def test_table_reaches_every_label():
    carriers = census()
    text = census_text(carriers)
    print(text)
    assert len(set(sc.LABELS)) == len(sc.LABELS)
    assert not set(carriers) - set(sc.LABELS), (set(carriers) - set(sc.LABELS), text)
    missing = [label for label in sc.LABELS if not carriers[label] and label not in sc.UNREACHABLE]
    assert not missing, (missing, text)
    both = [label for label in sc.UNREACHABLE if carriers[label]]
    assert not both, ("listed as unreachable and reached", both)
    assert len(sc.CASES) <= 26 and max(c["n"] for c in sc.CASES) <= sc.N_MAX
    # the m = 0 path is the no-chain engine's alone, and the deterministic flush labels the one-wavefront engine's
    assert all(n.endswith("/nochain") for n in carriers["kind:m=0"])
    assert {n.split("/")[1] for n in carriers["flush:7 pending"]} == {"block64"}


def test_unreachable_by_enumeration():
    """No plan entry of any window length up to 260, or of a few longer ones, reaches a label of UNREACHABLE (all
    classes, all base periods the plans of the engines can hold for p_hi <= 2048)."""
    seen = set()
    for N in list(range(1, 261)) + [385, 449, 512, 513, 1024, 2047, 2048]:
        for p in range(1, 64):
            seen |= sc.entry_labels(N, p, 0)
        for p in range(64, 2049 if N <= 130 or N >= 1024 else 700):
            seen |= sc.entry_labels(N, p, 1)
            if 2 * p <= sc.N_MAX:
                seen |= sc.entry_labels(N, p, 2)
            if 4 * p <= sc.N_MAX:
                seen |= sc.entry_labels(N, p, 4)
    assert not seen & set(sc.UNREACHABLE), seen & set(sc.UNREACHABLE)
    assert not seen - set(sc.LABELS), seen - set(sc.LABELS)


def test_every_period_is_produced_exactly_once():
    """Every range of the table, every plan variant, sorted or mixed: the plan yields each period of [p_lo, p_hi] once;
    mixing only permutes it; every chain halves down from at most 64 and every multi-class pass starts at 64 or above."""
    ranges = {(c["p_lo"], c["p_hi"]) for c in sc.CASES} | {(2, 300), (2, 301), (3, 300)}
    for p_lo, p_hi in sorted(ranges):
        for max_m in (1, 2, 4):
            for chains in (False, True):
                plan = sc.build_plan(p_lo, p_hi, max_m, True, chains)
                got = sorted(q for e in plan for q in sc.produced(*e))
                assert got == list(range(p_lo, p_hi + 1)), (p_lo, p_hi, max_m, chains)
                assert sorted(plan) == sorted(sc.build_plan(p_lo, p_hi, max_m, False, chains))
                for p, m in plan:
                    assert (m >= 8 and p <= 64 and 1 <= m - 8 <= 7) or (m == 0 and p < 64 and not chains) or (m in (1, 2, 4) and p >= 64 and m <= max_m), (p, m)


def test_geometry_and_chunks():
    """PGeom and pick_chunks as restated: counts add up to N, segment A is never empty, chunks never exceed what leaves
    a workgroup 8 periods per wavefront, and a slice that starts past the plan is empty, never negative."""
    for N in (1, 13, 64, 65, 385, 2048):
        for p in (1, 2, 63, 64, 65, N, N + 1, 2 * N + 3):
            rows, nfull = sc.geom(N, p)
            assert 1 <= nfull <= p and nfull * rows + (p - nfull) * (rows - 1) == N
    for case in sc.CASES:
        P = case["p_hi"] - case["p_lo"] + 1
        for engine, (max_m, chains, nw) in sc.VARIANTS.items():
            for W in (1, 2, sc.N_ROWS, 8 * sc.CUS):
                chunks = sc.sweep_chunks(sc.CUS, W, case["p_lo"], case["p_hi"], nw)
                assert chunks == 1 or (chunks * 8 * nw <= P and chunks <= -(-8 * sc.CUS // W))
            assert sc.sweep_chunks(sc.CUS, 8 * sc.CUS, case["p_lo"], case["p_hi"], nw) == 1


def test_planted_rows():
    """The planted row of every case that can hold one spans six decades and more between its strongest and its
    weakest entry (norm mode 0), and the weak entry is the planted one."""
    n = 0
    for case in sc.CASES:
        pw = sc.weak_period(case)
        if pw is None:
            continue
        ss = sc.ref(case)[2][0].astype(np.float64)
        assert np.sqrt(ss.max() / ss[pw - case["p_lo"]]) >= 1e6, (case["name"], pw, ss.max(), ss[pw - case["p_lo"]])
        n += 1
    assert n >= len(sc.CASES) // 2


def test_reference_against_the_oracle():
    """sweep_ref against po.sweep_norms, both norm modes, every float64 row of every case, entry by entry."""
    worst = 0.0
    for case in sc.CASES:
        N, p_lo, p_hi = case["n"], case["p_lo"], case["p_hi"]
        for x, (ss, A) in zip(sc.windows(case), sc.ref(case)):
            for mode in (0, 1):
                got = sc.norm_sq(po.sweep_norms(x, p_lo, p_hi, gamma=bool(mode)), N, p_lo, p_hi, mode)
                err = np.abs(got - ss)
                assert np.all(err <= sc.REF_BAR * A), (case["name"], mode, int(np.argmax(err - sc.REF_BAR * A)) + p_lo)
                worst = max(worst, float(np.max(np.where(A > 0, err / np.where(A > 0, A, 1), 0))))
    print(f"largest |N v^2 [p] - ss_p| / A_p of the oracle: {worst:.2e}")


def test_reference_against_the_fixture(golden):
    """The reference project's own sweep values (N = 4096, p = 2 .. N / 3), entry by entry in units of A_p."""
    g = golden("sweep")
    n = 4096
    for w in range(4):
        ss, A = sc.sweep_ref(multi_sinusoid_window(w, n), 2, n // 3)
        for mode, key in ((0, f"plain_w{w}"), (1, f"gamma_w{w}")):
            err = np.abs(sc.norm_sq(g[key], n, 2, n // 3, mode) - ss)
            assert np.all(err <= sc.REF_BAR * A), (key, float(np.max(err / A)))


def test_teeth():
    total = collections.Counter()
    for case in sc.CASES:
        for w in (0, 1):
            moves = sc.mutant_moves(case, sc.windows(case)[w])
            small = [(p, what, float(v)) for p, what, v in moves if not v > sc.TEETH * sc.BAR]
            kinds = collections.Counter(what.split()[0] for _, what, _ in moves)
            assert kinds["drop"] > 0 and len(small) <= sc.TEETH_CAP * len(moves), (case["name"], w, len(moves), small[:8])
            total.update(kinds)
    print("mutants:", dict(total))
    assert all(total[k] > 0 for k in ("drop", "segment", "select", "wrong")), total
