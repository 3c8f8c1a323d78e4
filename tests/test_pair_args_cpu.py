"""The oracle is at no tie on the windows of pair_args_cases.py: in every sweep of step 1 of every case the winning norm
leads the best other period by more than MIN_LEAD = 1e-9 (relative), the project's tie bar, so the kernels of
test_gpu_pair_args.py -- which sum in another order than numpy -- must return the oracle's period lists.  No case is
left out; should one ever have to be, pair_args_cases.DROPPED names it and this file fails above one case in ten."""

import warnings

import numpy as np
import pytest

import pair_args_cases as pa


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def test_at_most_one_case_in_ten_is_dropped():
    print("cases", len(pa.CASES), "dropped", len(pa.DROPPED), list(pa.DROPPED))
    assert 10 * len(pa.DROPPED) <= len(pa.CASES) + len(pa.DROPPED)


def test_every_argument_has_its_cases():
    names = " ".join(c["name"] for c in pa.CASES)
    for group in ("plain", "gamma", "num1_", "num12_", "num14_", "num3_", "min1_", "min12_", "min24_", "max20_", "max100_", "max200_",
                  "fold_once0", "fold_once1", "fold_report", "cover0", "duo0"):
        assert group in names, group
    assert {(c["n"], c["w"]) for c in pa.CASES} == set(pa.SHAPES)


@pytest.mark.parametrize("case", pa.CASES, ids=lambda c: c["name"])
def test_step1_is_at_no_tie(case):
    lo, hi, num = case["min_length"], case["max_length"], case["num"]
    assert lo <= hi < case["n"]  # (the window-pair screen needs max_length < N)
    for k, row in enumerate(pa.windows(case)):
        leads, periods, ended = pa.step1_leads(row, num, lo, hi, case["gamma"])
        print(case["name"], "window", k, "sweeps", len(leads), "periods", periods, "ended", ended, "smallest lead %.3e" % min(leads))
        assert min(leads) > pa.MIN_LEAD, (k, leads)
        want = pa.oracle(case)[k]
        if case["kind"] == "int7":  # one pick, then a residual that is exactly zero
            assert ended and periods == [7] and want is None
            continue
        assert not ended and want is not None
        assert sorted(int(p) for p in want[0]) != [] and (np.asarray(want[0]) > 0).all()
        assert 1 not in periods  # (a list that holds period 1 ends PH_ST_NO_PERIOD in step 2)
        if case["kind"] == "noise":  # the list is filled only through repeats and skipped periods
            assert len(leads) > num + 10, (k, len(leads))
