"""Cases of k_mbest_step1_pair's parameter block (pyperiod_amd/csrc/ph_mbest.h, Step1PairArgs).  The kernel takes its
arguments as one block and fetches each of them by a scalar load at the head of the phase that uses it -- the survivor
scan, the exact phase of either window, the output loop -- where it used to hold all 26 from its entry block on; only
what a pass of the screen needs stays in registers.  An argument that reached the wrong phase, or a phase that read
the wrong slot of the block, shows in a case that moves that argument away from the value every other case gives it.

Shapes: N = 97, 500 and 1100 (14, 8 and 0 of the 16 wavefronts without a sample), W = 1 and 3 (the last workgroup holds one
window; the other does not exist).  One group of cases per argument:

  num          1, 4, and a list longer than the window fills: white noise over a narrow band of periods, where present
               periods win again (repeats) until they are skipped (skip bits); and an integer pattern of period 7 whose
               residual is exactly zero after one pick, so the window ends without a period and its other rows stay zero
  min_length   1 (period 1 and the divisor 1 of every period), 2, and 12 / 24: inside the chains 24-12-6-3 / 48-24-12-6-3
               that the screen folds in one pass; max_length below N / 3
  gamma        m_best and m_best_gamma
  switches     PH_PAIR_FOLD_ONCE = 0 and 1 (thin_band's sign), PH_PAIR_FOLD_REPORT = 1 (fold_report: the fold-once count above
               bit 16 of the sweep count), PH_PAIR_COVER = 0 (p_scr = p_lo), PH_PAIR_DUO = 0 (another plan and n_pass)

The windows are the seeded ones of pyperiod_amd.synth (`sin`), seeded white noise (`noise`) and the integer pattern
(`int7`).  A period list compares only where the oracle is at no tie: step1_leads gives, sweep by sweep, the relative lead
of the winning norm over the best other period, and test_pair_args_cpu.py holds every case above MIN_LEAD = 1e-9, the
project's tie bar.  (Sums of N <= 1100 squares carry a relative error below 1.2e-13 in any order.)  No case is dropped:
DROPPED is empty, and the CPU test fails if it ever holds more than one case in ten."""

import functools

import numpy as np

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch

MIN_LEAD = 1e-9
SEED = 9300  # `sin` windows: multi_sinusoid_batch(SEED + N, W, N)
SHAPES = [(97, 1), (97, 3), (500, 1), (500, 3), (1100, 1), (1100, 3)]
DROPPED = ()  # names of cases left out because the oracle is at a tie on one of their windows: none


def _case(name, n, w, num=4, min_length=2, max_length=None, gamma=False, kind="sin", **env):
    return dict(name=name, n=n, w=w, num=num, min_length=min_length, max_length=n // 3 if max_length is None else max_length,
                gamma=gamma, kind=kind, env=tuple(sorted(env.items())))


CASES = (
    # num = 4, min_length = 2, m_best: every shape
    [_case(f"plain_n{n}_w{w}", n, w) for n, w in SHAPES]
    + [_case(f"gamma_n{n}_w{w}", n, w, gamma=True) for n, w in ((97, 3), (500, 1), (1100, 3))]
    + [_case(f"num1_n{n}_w{w}", n, w, num=1) for n, w in ((97, 1), (500, 3), (1100, 1))]
    + [
        # sixteen periods, twelve rows: repeats and skip bits
        _case("num12_noise_n97_w3", 97, 3, num=12, min_length=5, max_length=20, kind="noise"),
        _case("num14_noise_n500_w1", 500, 1, num=14, min_length=150, max_length=166, kind="noise"),
        # one period to find, three rows asked for: the window ends without a period, rows 1 and 2 stay zero
        _case("num3_int7_n97_w3", 97, 3, num=3, min_length=5, max_length=12, kind="int7"),
    ]
    + [_case(f"min1_n{n}_w{w}", n, w, min_length=1) for n, w in ((97, 3), (500, 1), (1100, 3))]
    + [_case("min12_n97_w1", 97, 1, min_length=12), _case("min24_n500_w3", 500, 3, min_length=24),
       _case("min24_n1100_w1", 1100, 1, min_length=24)]
    + [_case("max20_n97_w3", 97, 3, max_length=20), _case("max100_n500_w1", 500, 1, max_length=100),
       _case("max200_n1100_w3", 1100, 3, max_length=200)]
    # the fold-once path needs a winner above 256: N = 1100 (periods up to 366)
    + [_case(f"fold_once{v}_n1100_w{w}", 1100, w, PH_PAIR_FOLD_ONCE=v) for v in ("0", "1") for w in (1, 3)]
    + [_case("fold_report_n1100_w3", 1100, 3, PH_PAIR_FOLD_REPORT="1"), _case("fold_report_n500_w1", 500, 1, PH_PAIR_FOLD_REPORT="1")]
    + [_case(f"cover0_n{n}_w{w}", n, w, PH_PAIR_COVER="0") for n, w in ((97, 3), (500, 1), (1100, 3))]
    + [_case(f"duo0_n{n}_w{w}", n, w, PH_PAIR_DUO="0") for n, w in ((500, 3), (1100, 1))]
)
CASES = tuple(c for c in CASES if c["name"] not in DROPPED)
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def _windows(kind, n, w):
    if kind == "sin":
        x = multi_sinusoid_batch(SEED + n, w, n)
    elif kind == "noise":
        x = np.stack([np.random.default_rng(SEED + n + k).standard_normal(n) for k in range(w)])
    elif kind == "int7":  # integer patterns of period 7: every fold of them is exact in any order
        x = np.stack([np.random.default_rng(SEED + n + k).integers(-9, 10, 7)[np.arange(n) % 7].astype(np.float64) for k in range(w)])
    else:
        raise AssertionError(kind)
    x.setflags(write=False)
    return x


def windows(case):
    return _windows(case["kind"], case["n"], case["w"])


def step1_leads(x, num, lo, hi, gamma, max_sweeps=400):
    """Step 1 of Periods.py:494-537 sweep by sweep: (leads, periods, ended).  leads[i] is the relative lead of sweep i's
    winning norm over the best other period that is not skipped; `ended` says the window ran out of positive norms
    (the reference raises there, the kernels report status 1)."""
    work, periods, skip, repeats, leads = np.array(x, dtype=np.float64), [], set(), 0, []
    while len(periods) < num:
        assert len(leads) < max_sweeps
        v = po.sweep_norms(work, lo, hi, gamma)
        for s in skip:
            v[s - lo] = -1.0
        k = int(np.argmax(v))
        if not v[k] > 0.0:
            return leads, periods, True
        others = np.delete(v, k)
        leads.append(float((v[k] - (others.max() if len(others) else 0.0)) / v[k]))
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
    return leads, periods, False


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, w, num, lo, hi, gamma):
    out = []
    for row in _windows(kind, n, w):
        try:
            with np.errstate(all="ignore"):
                per, pw, bs = po.m_best(row, num, max_length=hi, min_length=lo, gamma=gamma)
            out.append((np.asarray(per), np.asarray(pw), np.asarray(bs)))
        except TypeError:  # no period with a positive norm is left (Periods.py:520/537)
            out.append(None)
    return tuple(out)


def oracle(case):
    """Per window: (periods, powers, bases) of the oracle, or None where the reference raises; computed once per distinct
    request, shared between the cases that differ only in a switch, never written."""
    return _oracle(case["kind"], case["n"], case["w"], case["num"], case["min_length"], case["max_length"], case["gamma"])
