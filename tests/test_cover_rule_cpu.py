"""The cover rule of the window-pair screen of m_best (ph_pair.h, k_mbest_step1_pair), pinned against the oracle on the CPU.

Plain m_best screens only the "top" periods q in (max_length // 2, max_length]; a smaller period d is looked at only
when one of its multiples m may still hold the maximum.  That rests on E_d <= E_m for d | m (V_d is a subspace of V_m,
E_q = sum_j S_q[j]^2 / cnt_q[j] the squared norm of the orthogonal projection), which holds in fp64 up to rounding
noise that is ABSOLUTE in units of the residual's sum of squares.  For every sweep of the oracle's step 1:

  * E_d <= E_m + 2^-40 ||r||^2 for every top m and every divisor d of it in range;
  * the oracle's winner is among {covering top periods} U {their divisors};
  * on the noisy windows that candidate set stays within the kernel's survivor list (96 entries).

The fp64 values stand in for the float screen values here (the radius of the float screen only widens the set).
"""

import functools

import numpy as np
import pytest

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window, readme_window

SLACK = 2.0 ** -40
LIST_CAP = 96


def _energies(work, lo, hi):
    n = work.size
    return {p: float(np.sum(po.fold_sums(work, p) ** 2 / po.fold_counts(n, p))) for p in range(lo, hi + 1)}


@functools.lru_cache(maxsize=None)
def _divisors(m, lo):
    return [d for d in range(max(lo, 1), m // 2 + 1) if m % d == 0]


def _step1_sweeps(x, num, lo, hi):
    """Step 1 of the oracle's m_best (Periods.py:494-537), one record per sweep: residual, skip set, winner."""
    work = x.copy()
    periods, skip, i, repeats, out = [0] * num, set(), 0, 0, []
    while i < num:
        top_norm, top_p, top_base = 0, 0, None
        for p in range(lo, hi + 1):
            base = po.project(work, p)
            nrm = po.periodic_norm(base)
            if nrm > top_norm and p not in skip:
                top_p, top_norm, top_base = p, nrm, base
        assert top_p, "the oracle ran out of candidates"
        out.append((work, set(skip), top_p))
        present = top_p in periods
        if present and repeats < 10:
            repeats += 1
        elif present:
            skip.add(top_p)
            repeats = 0
        else:
            periods[i] = top_p
            i += 1
            repeats = 0
        work = work - top_base
    return out, periods


def _check_window(x, num, hi, lo=2, noisy=True):
    sweeps, picks = _step1_sweeps(x, num, lo, hi)
    trace = {}
    po.m_best(x, num, max_length=hi, min_length=lo, trace=trace)
    assert list(trace["step1_periods"]) == picks  # the sweeps above ARE the oracle's
    p_scr = max(lo, hi // 2 + 1)
    worst = 0
    for work, skip, winner in sweeps:
        ssq = float(np.sum(work * work))
        e = _energies(work, lo, hi)
        for m in range(p_scr, hi + 1):
            for d in _divisors(m, lo):
                assert e[d] <= e[m] + SLACK * ssq, (m, d, e[d], e[m], ssq)
        live = [m for m in range(p_scr, hi + 1) if m not in skip]
        assert live
        best_lower = max(e[m] for m in live)
        thr = best_lower - abs(best_lower) * 1e-9
        cand = set()
        for m in range(p_scr, hi + 1):
            if e[m] + SLACK * ssq >= thr:  # m covers, skipped or not
                if m not in skip:
                    cand.add(m)
                cand.update(d for d in _divisors(m, lo) if d not in skip)
        assert winner in cand, (winner, sorted(cand))
        worst = max(worst, len(cand))
    if noisy:
        assert worst <= LIST_CAP, worst
    return worst


@pytest.mark.parametrize("w", [0, 1, 2, 3, 17, 640])
def test_config2_windows(w):
    _check_window(multi_sinusoid_window(w, 4096), 10, 4096 // 3)


def test_readme_window():
    _check_window(readme_window(2000), 5, 2000 // 3)


def test_noise_free_integer_period_window():
    """d ties with its multiples exactly (up to rounding); the oracle's winner is a small multiple of the period, no
    top period, and reaches the decision through the divisor list.  A second component makes a second sweep possible:
    there the winner is a multiple that also holds part of the other component."""
    t = np.arange(1024)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(12)[t % 12]
    sweeps, _ = _step1_sweeps(x, 1, 2, 341)
    assert sweeps[0][2] < 341 // 2 + 1 and sweeps[0][2] % 12 == 0
    _check_window(x, 1, 341, noisy=False)
    _check_window(x + 0.5 * rng.standard_normal(35)[t % 35], 2, 341, noisy=False)


def test_min_length_one_and_odd_max_length():
    _check_window(multi_sinusoid_window(5, 600), 4, 199, lo=1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_skipped_top_period_covers_its_divisor(seed):
    """White noise of 97 samples, periods 5 ... 20, twelve rows: a top period is skipped after ten repeats while a
    divisor of it is still eligible and wins a later sweep -- it must be among the candidates through the skipped one."""
    x = np.random.default_rng(seed).standard_normal(97)
    sweeps, _ = _step1_sweeps(x, 12, 5, 20)
    assert any(m > 10 and win < m and m % win == 0 for _, skip, win in sweeps for m in skip)
    _check_window(x, 12, 20, lo=5)
