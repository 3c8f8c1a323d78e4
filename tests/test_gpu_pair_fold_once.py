"""The fold-once path of k_mbest_step1_pair (pyperiod_amd/csrc/ph_mbest.h): behind the screen the residual is folded once
at the surviving top period -- the exact value, the values of the listed divisors and the means of the update all come
from those column sums, read straight from the workspace -- where the kernel used to stage the window, fold every
candidate, fold the winner again and fold it a third time for the means.

Three engines on the cases of pair_fold_once_cases.py, whose paths test_pair_fold_once_cpu.py has established (fold-once
on the first sweep and in place, one and two columns per thread, with and without listed divisors; fallback on exact and
near ties, two top periods, short winners, divisors of a skipped period; windows that are not screened at all):

  default               the fold-once path
  PH_PAIR_FOLD_ONCE=0   the phases as they were, for every window-sweep
  PH_STEP1_PAIR=0       the one-window fp64 kernel

All three must give identical periods, status, sweep counts and bases; the first two identical powers as well -- the path
reorders no sum that reaches an output -- and the one-window kernel powers within 1e-13.  The input is not written.

That the path is live, and taken exactly where the restated rule says, shows a fourth engine with PH_PAIR_FOLD_REPORT=1:
its sweep counts carry, above bit 16, the number of window-sweeps of the window that took the fold-once path.  It must
equal the number of "fold:" sweeps of the window's trace -- so a window-sweep that the rule sends to the staged phases
(a tie, two top periods, a short winner, a listed divisor of a skipped period that does not divide m) is seen if it folds,
and a kernel that never folds is seen as well."""

import os
import warnings

import numpy as np
import pytest

import pair_fold_once_cases as fc
from oracle import period_oracle as po

pytestmark = pytest.mark.gpu
TOL = 1e-10  # against the oracle
KTOL = 1e-13  # powers, pair kernel against one-window kernel (test_gpu_pair.py)


def _engine(**env):
    from pyperiod_amd import PeriodEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return PeriodEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge

    ge.build()
    fold = _engine(PH_STEP1_PAIR="1", PH_PAIR_FOLD_ONCE="1")
    off = _engine(PH_STEP1_PAIR="1", PH_PAIR_FOLD_ONCE="0")
    single = _engine(PH_STEP1_PAIR="0")
    report = _engine(PH_STEP1_PAIR="1", PH_PAIR_FOLD_ONCE="1", PH_PAIR_FOLD_REPORT="1")
    report_off = _engine(PH_STEP1_PAIR="1", PH_PAIR_FOLD_ONCE="0", PH_PAIR_FOLD_REPORT="1")
    yield fold, off, single, report, report_off
    for e in (fold, off, single, report, report_off):
        e.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _run(engine, x, case):
    import torch

    out = engine.m_best(x, case["num"], case["max_length"], case["min_length"], case["gamma"], want_sweeps=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c["name"])
def test_three_engines_agree(engines, case):
    import torch

    fold, off, single, report, report_off = engines
    n = case["n"]
    args = (n, case["num"], case["max_length"], case["min_length"])
    assert fold.m_best_info(*args) == (2, 8) and off.m_best_info(*args) == (2, 8) and single.m_best_info(*args)[0] == 1
    xh = fc.windows(case)
    x = torch.from_numpy(np.array(xh)).cuda()
    a, b, c = (_run(e, x, case) for e in (fold, off, single))
    assert np.array_equal(x.cpu().numpy(), xh, equal_nan=True)  # the input is read in place on the first sweep, never written
    ok = a[3] == 0  # (what a window whose step 1 failed leaves in its rows and powers is no contract)
    for other, what in ((b, "PH_PAIR_FOLD_ONCE=0"), (c, "PH_STEP1_PAIR=0")):
        print(case["name"], what, "periods", np.array_equal(a[0], other[0]), "status", np.array_equal(a[3], other[3]), "sweeps",
              np.array_equal(a[4], other[4]), "bases", np.array_equal(a[2][ok], other[2][ok]), "sweeps", a[4].tolist())
        assert np.array_equal(a[3], other[3]), (what, a[3], other[3])
        assert np.array_equal(a[0], other[0]), (what, np.nonzero((a[0] != other[0]).any(1))[0])
        assert np.array_equal(a[4], other[4]), (what, a[4], other[4])
        assert np.array_equal(a[2][ok], other[2][ok]), what
    assert np.array_equal(a[1][ok], b[1][ok])  # no sum that reaches an output is reordered
    if ok.any():
        scale = np.maximum(np.max(np.abs(c[1]), axis=1, keepdims=True), 1e-300)
        dpow = float(np.max((np.abs(a[1] - c[1]) / scale)[ok]))
        print(case["name"], "powers against the one-window kernel", dpow)
        assert dpow <= KTOL
    # the window-sweeps that took the fold-once path: exactly the "fold:" sweeps of the restated rule
    r, r0 = _run(report, x, case), _run(report_off, x, case)
    assert np.array_equal(r[4] & 0xFFFF, a[4]) and np.array_equal(r0[4], a[4])  # (no sweep folds with the path switched off)
    for k in range(4):
        assert np.array_equal(r[k][ok] if k in (1, 2) else r[k], a[k][ok] if k in (1, 2) else a[k]), k
    want_folds = [sum(rec["path"].startswith("fold") for rec in tr) for tr in fc.traces(case)]
    print(case["name"], "fold-once window-sweeps", (r[4] >> 16).tolist(), "of", a[4].tolist())
    assert (r[4] >> 16).tolist() == want_folds, ((r[4] >> 16).tolist(), want_folds)
    # the sweeps are those of the restated step 1, whose paths the CPU census has established, and the picks the oracle's
    for w, tr in enumerate(fc.traces(case)):
        failed = tr[-1]["winner"] == 0
        assert a[3][w] == (1 if failed else 0), (w, a[3][w])
        if failed:  # no positive norm is left: the reference raises (Periods.py:520/537)
            continue
        assert a[4][w] == len(tr), (w, a[4][w], len(tr))
        with np.errstate(all="ignore"):
            want = po.m_best(xh[w], case["num"], max_length=case["max_length"], min_length=case["min_length"], gamma=case["gamma"])
        assert np.array_equal(a[0][w], want[0]), (w, a[0][w], want[0])
        assert np.max(np.abs(a[1][w] - want[1])) <= TOL * np.max(np.abs(want[1]))
        assert np.max(np.abs(a[2][w] - want[2])) <= TOL * np.max(np.abs(want[2]))


def test_the_full_batch_is_bit_identical_with_the_switch_off(engines):
    """The config-2 shape at a size that keeps the test short: 63 windows of 4096 samples, num = 10."""
    import torch

    from pyperiod_amd.synth import multi_sinusoid_batch

    fold, off, _, report, _ = engines
    x = torch.from_numpy(multi_sinusoid_batch(0, 63, 4096)).cuda()
    a = [o.cpu().numpy() for o in fold.m_best(x, 10, want_sweeps=True)]
    b = [o.cpu().numpy() for o in off.m_best(x, 10, want_sweeps=True)]
    for k in range(5):
        assert np.array_equal(a[k], b[k]), k
    assert (a[3] == 0).all()
    # nearly every window-sweep of this data is one survivor and its divisors: the path carries the batch
    r = report.m_best(x, 10, want_sweeps=True)[4].cpu().numpy()
    assert np.array_equal(r & 0xFFFF, a[4])
    print("fold-once window-sweeps", int((r >> 16).sum()), "of", int(a[4].sum()))
    assert (r >> 16).sum() >= 0.9 * a[4].sum()
