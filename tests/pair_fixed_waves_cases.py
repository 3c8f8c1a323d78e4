"""Cases of the window-pair kernels with a compile-time wavefront count (ph_device.h: red_combine<.., NW>, block_sum<NW>,
red_argmax<NW>; k_mbest_step1_pair, k_best_correlation_pair and k_small_to_large_pair<16> are compiled for 16 wavefronts
and test no slot of a workgroup reduction, k_small_to_large_pair<0> reads the count from the launch).

A wrong slot count shows where wavefronts hold nothing: N = 97 and N = 500 leave 14 and 8 of the 16 wavefronts of a
workgroup without a sample, so their partial sums are the zeros (or -inf) the reduction must still combine; N = 1100
gives every thread a sample and some two.  W = 1 and W = 3 end in a pair whose second window does not exist.

The windows are the seeded ones of pyperiod_amd.synth.  A comparison of period lists means something only where the
oracle itself is not at a tie; the leads below are how far it is from one, and test_pair_fixed_waves_cpu.py holds them
above MIN_LEAD:

  m_best / m_best_gamma   step 1 sweep by sweep (Periods.py:494-537): the winning norm's relative lead over the
                          best other period
  best_correlation        the oracle's own trace: relative lead of the winning max|S_p[s]|, |gain - ratio|
  small_to_large          the oracle's own trace: smallest |imposed - thresh| / thresh over all periods

MIN_LEAD = 1e-9.  The kernels associate their sums differently from numpy: a sum of N <= 1100 squares carries a relative
error below N 2^-53 ~ 1.2e-13 either way, a rounded norm a few ulp more, so two values 1e-9 apart are ordered the same
by every correct evaluation, with four decimal orders to spare."""

import functools

import numpy as np

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch

MIN_LEAD = 1e-9
NUM = 4
SEED = 7100  # first window of the seeded batches: windows SEED + N .. of multi_sinusoid_batch

# (N, W) of the m_best cases; both norms run on each
MBEST_SHAPES = [(97, 1), (97, 3), (500, 1), (500, 3), (1100, 1), (1100, 3)]
MBEST_CASES = [(n, w, gamma) for n, w in MBEST_SHAPES for gamma in (False, True)]

S2L_N, S2L_W, S2L_THRESH = 500, 3, 0.05
S2L_BLOCKS = (512, 768, 1024)  # PH_S2L_BLOCK: 1024 launches k_small_to_large_pair<16>, the others k_small_to_large_pair<0>

BC_N, BC_W, BC_NUM = 500, 3, 3


@functools.lru_cache(maxsize=None)
def windows(n, w):
    x = multi_sinusoid_batch(SEED + n, w, n)
    x.setflags(write=False)
    return x


def mbest_step1_leads(x, num, lo, hi, gamma):
    """Relative lead of every step-1 winner over the best other period (Periods.py:494-537)."""
    work, periods, skip, repeats, leads = np.array(x, dtype=np.float64), [], set(), 0, []
    while len(periods) < num and len(leads) < 200:
        v = po.sweep_norms(work, lo, hi, gamma)
        for s in skip:
            v[s - lo] = -1.0
        k = int(np.argmax(v))
        assert v[k] > 0.0
        others = np.delete(v, k)
        leads.append(float((v[k] - others.max()) / v[k]))
        top = lo + k
        if top in periods and repeats < 10:
            repeats += 1
        elif top in periods:
            repeats = 0
            skip.add(top)
        else:
            repeats = 0
            periods.append(top)
        work = work - po.project(work, top)
    return leads


@functools.lru_cache(maxsize=None)
def mbest_oracle(n, w, gamma):
    """Per window: (periods, powers, bases) of the oracle; computed once, shared, never written."""
    out = []
    for row in windows(n, w):
        per, pw, bs = po.m_best(row, NUM, gamma=gamma)
        out.append((np.asarray(per), np.asarray(pw), np.asarray(bs)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def s2l_oracle():
    out = []
    for row in windows(S2L_N, S2L_W):
        tr = {}
        res = po.small_to_large(row, S2L_THRESH, trace=tr)
        out.append((res, tr["min_margin"]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def bc_oracle():
    out = []
    for row in windows(BC_N, BC_W):
        tr = []
        res = po.best_correlation(row, BC_NUM, trace=tr)
        out.append((res, tuple(tr)))
    return tuple(out)
