"""The Ramanujan census on the CPU: what tests/ramanujan_cases.py reaches, and what its expected values rest on.

k_ramanujan (ph_ram.h) picks its code by integers the host derives from (N, q_lo, q_hi): rows per batch and batches of
the root fold, the chunk tail, the mask of the partial last row, the rows of a child in its root's strip, and for every
factor (I - P_d) of a period's projector the coset count d, the prime r and whether the factor is the last one.
ramanujan_cases.classify restates those integers; `test_table_reaches_every_class` asserts that the table reaches every
label of ramanujan_cases.CLASSES and prints how many cases reach each.

The expected values of the GPU test are po.ramanujan_norm_projector_q's (longdouble, the projector as coset means: the
kernel's own algebra), so `test_projector_form_is_pinned_to_the_correlation_form` ties that function to the independent
po.ramanujan_norm_folded_q (c_q correlated twice through a q x q index matrix, float64): every q <= 400 at N = 257 and
N = 811 on two windows, and every q > 400 the table emits from a range of at most 40 periods.  The difference is
measured in units of B_q, the energy in front of the projector, and must stay below TOL / 100 = 1e-12.

Measured (this table, x86-64 longdouble):
  largest |projector form - correlation form| / B_q: 4.0e-14 over 1677 (q, window) pairs (5 s);
  largest |projector form - closed form| / closed form on the impulse windows: 2.2e-16 over 2490 periods;
  oracle time of the whole table, float64 and float32 windows together: 3.2 s; this module: 13 s;
  74 cases; cases per class as test_table_reaches_every_class prints them (-s), from 48 (one and two factors) down to
  2 (five factors; U = 7 or 8 with k >= 2; Q = 2 N) and 1 (children of 9 and more rows, odd and even, which only the
  wide range [64, 768] reaches; q_hi == 1; q_hi == 2).
On an MI355X the kernel's largest error over the table is 1.4e-13 B_q (q = 1 on white noise, where B_1 = N S_1^2 is
itself a cancelled sum) and 1.4e-15 B_q everywhere else, float32 windows included.
"""

import collections
import math
import time
from fractions import Fraction

import numpy as np

import ramanujan_cases as rc
from oracle import period_oracle as po

NARROW = 40


def test_table_reaches_every_class():
    count = collections.Counter()
    for case in rc.CASES:
        for label in rc.classify(case):
            count[label] += 1
    for label in rc.CLASSES:
        print(f"{count[label]:3d}  {label}")
    others = sorted(set(count) - set(rc.CLASSES))
    print("also reached:", ", ".join(f"{label} ({count[label]})" for label in others))
    missing = [label for label in rc.CLASSES if not count[label]]
    assert not missing, missing
    assert len(set(rc.CASES)) == len(rc.CASES)
    assert max(c[0] for c in rc.CASES) <= 5000 and np.median([c[0] for c in rc.CASES]) <= 700
    assert sum(1 for c in rc.CASES if rc.n_windows(c) < len(rc.KINDS)) == 1


def test_classes_left_out_cannot_happen():
    """Two labels the issue's list would suggest do not exist.  U = 4 with rem == 0 and k >= 2: 4 k rows are cut into
    ceil(4 k / 8) < k batches.  A factor with a power of two d < 64 that is not the last one: a later factor has a
    larger prime, and that prime divides d."""
    for rows in range(1, 6000):
        k, u, rem = rc.batches(rows)
        assert 1 <= u <= 8 and 0 <= rem < k and u * k + rem == rows and k == -(-rows // 8)
        assert not (u == 4 and rem == 0 and k >= 2), rows
    for q in range(1, 4000):
        st = rc.steps(q)
        assert math.prod(r for r, _ in st) <= q and len(st) <= 5
        for r, d in st[:-1]:
            assert not (d < 64 and d & (d - 1) == 0), q


def _agree(x, q):
    got, unit = po.ramanujan_norm_projector_q(x, q)
    want = po.ramanujan_norm_folded_q(x, q)
    assert unit > 0 and got <= 2 * unit
    return float(abs(got - np.longdouble(want)) / unit)


def test_projector_form_is_pinned_to_the_correlation_form():
    t0 = time.time()
    worst, pairs = 0.0, 0
    for n in (257, 811):  # q > 257: periods longer than the window
        x = rc.windows((n, 1, 400))
        for q in range(1, 401):
            for w in (0, 1):
                worst = max(worst, _agree(x[w], q))
                pairs += 1
    narrow = [c for c in rc.CASES if 0 <= c[2] - c[1] <= NARROW and c[2] > 400]
    assert any(len(rc.steps(q)) == 5 for c in narrow for q in range(c[1], c[2] + 1))
    for case in narrow:
        x = rc.windows(case)
        for q in range(max(case[1], 401), case[2] + 1):
            worst = max(worst, _agree(x[q % x.shape[0]], q))
            pairs += 1
    print(f"projector form against correlation form: {worst:.3e} B_q at worst over {pairs} pairs, {time.time() - t0:.1f} s")
    assert worst < rc.TOL / 100


def _impulse_exact(n, q):
    """norms[q] of the unit impulse at N - 1 in integers: S_q is the unit vector at j0 = (N - 1) mod q, E_q S_q =
    c_q(j - j0) / q, so norms[q] = q^2 / phi^4 sum_j cnt_q[j] c_q(j - j0)^2."""
    c = [int(v) for v in po.ramanujan_cq_exact(q)]
    j0 = (n - 1) % q
    rows, nfull = rc.geometry(n, q)
    tot = sum((rows if j < nfull else rows - 1) * c[(j - j0) % q] ** 2 for j in range(q))
    return Fraction(q * q * tot, po.phi(q) ** 4)


def test_impulse_window_closed_form():
    worst, seen = 0.0, 0
    for case in rc.CASES:
        n, q_lo, q_hi = case[:3]
        if rc.n_windows(case) < 3:
            continue
        want, unit = rc.ref(case)
        for q in range(q_lo, q_hi + 1):
            exact = _impulse_exact(n, q)
            assert exact > 0
            worst = max(worst, abs(float(want[2, q]) / float(exact) - 1.0))
            rows, nfull = rc.geometry(n, q)
            cnt0 = rows if (n - 1) % q < nfull else rows - 1
            assert abs(float(unit[2, q]) / float(Fraction(q, po.phi(q)) ** 4 * cnt0) - 1.0) < 1e-15
            seen += 1
    print(f"impulse windows: {worst:.3e} relative at worst over {seen} periods")
    assert worst < 1e-15 and seen > 1000


def test_correlation_form_runs_for_periods_of_the_window_length_and_more():
    seen = 0
    for case in rc.CASES:
        n, q_lo, q_hi = case[:3]
        if q_hi < n or q_hi > 400:
            continue
        x = rc.windows(case)
        for q in range(max(q_lo, n), q_hi + 1):
            for w in range(x.shape[0]):
                assert _agree(x[w], q) < rc.TOL / 100, (case, q, w)
                seen += 1
    assert seen >= 100


def test_oracle_time_of_the_table():
    t0 = time.time()
    for case in rc.CASES:
        for dtype in (np.float64, np.float32):
            want, unit = rc.ref(case, dtype)
            assert want.shape == (rc.n_windows(case), case[2] + 1) and np.all(want <= 2 * unit)
            assert not want[:, : case[1]].any() and np.all(np.isfinite(want))
    dt = time.time() - t0
    print(f"oracle time of the table, both dtypes: {dt:.1f} s")
    assert dt < 60
