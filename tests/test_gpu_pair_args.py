"""k_mbest_step1_pair reads its arguments from one parameter block, each at the head of the phase that uses it
(pyperiod_amd/csrc/ph_mbest.h, Step1PairArgs, pair_args_at_use).  Every case of pair_args_cases.py -- one group per
argument: num, min_length, max_length, gamma, the fold-once switch and its report, the cover rule, the shared-load plan --
goes through the pair kernel and is compared

  * against the oracle: periods equal, powers and bases to 1e-10 of the largest entry (the bar of
    test_gpu_pair_fixed_waves.py); a window on which the reference raises ends with status 1;
  * against the one-window kernel (PH_STEP1_PAIR=0), which takes its arguments one by one as before: periods, status,
    bases and sweep counts identical.

test_pair_args_cpu.py holds the oracle clear of a tie in every sweep of every case."""

import os
import warnings

import numpy as np
import pytest

import pair_args_cases as pa
import pair_fold_once_cases as fc

pytestmark = pytest.mark.gpu
TOL = 1e-10


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
    """engine(env) -> the pair engine with these switches; engine(None) -> the one-window engine.  One of each, shared."""
    import __graft_entry__ as ge

    ge.build()
    made = {}

    def get(env):
        if env not in made:
            made[env] = _engine(PH_STEP1_PAIR="0") if env is None else _engine(PH_STEP1_PAIR="1", **dict(env))
        return made[env]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got) - want))) <= TOL * float(np.max(np.abs(want)))


@pytest.mark.parametrize("case", pa.CASES, ids=lambda c: c["name"])
def test_case_through_the_pair_kernel(engines, case):
    pair, single = engines(case["env"]), engines(None)
    n, num, lo, hi, gamma = case["n"], case["num"], case["min_length"], case["max_length"], case["gamma"]
    assert pair.m_best_info(n, num, hi, lo)[0] == 2 and single.m_best_info(n, num, hi, lo)[0] == 1
    x = np.array(pa.windows(case))
    a = pair.m_best(x, num, hi, lo, gamma, want_sweeps=True)
    b = single.m_best(x, num, hi, lo, gamma, want_sweeps=True)
    report = dict(case["env"]).get("PH_PAIR_FOLD_REPORT") == "1"
    sweeps, folds = (a[4] & 0xFFFF, a[4] >> 16) if report else (a[4], None)
    print(case["name"], "periods", a[0].tolist(), "status", a[3].tolist(), "sweeps", sweeps.tolist(), "folds", None if folds is None else folds.tolist())
    assert np.array_equal(a[3], b[3]), (a[3], b[3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(sweeps, b[4]), (a[0], b[0], sweeps, b[4])
    ok = a[3] == 0  # (what a window whose step 1 failed leaves in its rows is no contract)
    assert np.array_equal(a[2][ok], b[2][ok])
    if report:
        # the count is that of the restated rule (pair_fold_once_cases.trace); a window-sweep folds once only behind a winner
        # above kPairSmallP = 256, which N = 500 (periods up to 166) never has
        want_folds = [sum(rec["path"].startswith("fold") for rec in fc.trace(np.array(row), num, lo, hi, gamma)) for row in x]
        assert folds.tolist() == want_folds and (sum(want_folds) > 0) == (hi > 256), (folds, want_folds)
    for k, want in enumerate(pa.oracle(case)):
        if want is None:  # the reference raises: no period with a positive norm is left
            assert a[3][k] == 1, (k, a[3][k])
            continue
        assert a[3][k] == 0, (k, a[3][k])
        assert np.array_equal(a[0][k], want[0]), (k, a[0][k], want[0])
        assert _close(a[1][k], want[1]) and _close(a[2][k], want[2]), k
