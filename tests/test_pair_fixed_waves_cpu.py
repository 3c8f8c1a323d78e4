"""The oracle is at no tie on the windows of pair_fixed_waves_cases.py: every period list the GPU tests compare
(test_gpu_pair_fixed_waves.py) is decided with a lead of at least MIN_LEAD, so a kernel that sums in another order than
numpy must still return it."""

import warnings

import numpy as np
import pytest

import pair_fixed_waves_cases as fw


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


@pytest.mark.parametrize("n,w,gamma", fw.MBEST_CASES, ids=lambda v: str(v))
def test_m_best_step1_is_at_no_tie(n, w, gamma):
    hi = n // 3
    assert hi < n  # (the window-pair screen needs max_length < N)
    for k, row in enumerate(fw.windows(n, w)):
        leads = fw.mbest_step1_leads(row, fw.NUM, 2, hi, gamma)
        print("N", n, "window", k, "gamma", gamma, "sweeps", len(leads), "smallest lead %.3e" % min(leads))
        assert min(leads) > fw.MIN_LEAD, (k, leads)
        per = fw.mbest_oracle(n, w, gamma)[k][0]
        assert len(per) == fw.NUM and (np.asarray(per) > 0).all()


def test_small_to_large_is_at_no_tie():
    for k, (res, margin) in enumerate(fw.s2l_oracle()):
        print("small_to_large window", k, "accepted", len(res[0]), "smallest margin %.3e" % margin)
        assert margin > fw.MIN_LEAD, (k, margin)
        assert 0 < len(res[0]) <= 64  # (some periods are accepted; the GPU test's capacity holds them)


def test_best_correlation_is_at_no_tie():
    for k, (res, tr) in enumerate(fw.bc_oracle()):
        print("best_correlation window", k, "periods", list(res[0]), "leads", ["%.3e" % t[0] for t in tr], "gaps", ["%.3e" % t[1] for t in tr])
        assert len(tr) == fw.BC_NUM
        assert min(t[0] for t in tr) > fw.MIN_LEAD and min(t[1] for t in tr) > fw.MIN_LEAD, (k, tr)
