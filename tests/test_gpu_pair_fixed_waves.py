"""The window-pair kernels with their wavefront count as a compile-time fact (ph_device.h: the workgroup reductions'
template parameter NW).  k_mbest_step1_pair, k_best_correlation_pair and k_small_to_large_pair<16> are compiled for
16 wavefronts: their workgroup reductions read exactly 16 slots and test none; k_small_to_large_pair<0>, which the host
launches for every other block (PH_S2L_BLOCK), reads the count from the launch.  A wrong slot count would show where
wavefronts hold no sample (N = 97, N = 500) and in a pair without a second window (W = 1, W = 3): see
pair_fixed_waves_cases.py, whose windows test_pair_fixed_waves_cpu.py holds clear of every tie of the oracle.

  * m_best and m_best_gamma through the pair kernel against the oracle, and periods, status and sweep counts against
    the one-window kernels (PH_STEP1_PAIR=0), which keep the run-time count;
  * small_to_large through the pair kernel with 512, 768 and 1024 threads: the three results identical bit for bit
    (1024 is the fixed instantiation, the others the run-time one) and equal to the oracle's;
  * best_correlation through the pair kernel against the oracle and against PH_BC_PAIR=0."""

import os
import warnings

import numpy as np
import pytest

import pair_fixed_waves_cases as fw

pytestmark = pytest.mark.gpu
TOL = 1e-10  # against the oracle (powers and bases, relative to the largest entry: the bar of test_gpu_pair*.py)


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
def built():
    import __graft_entry__ as ge

    ge.build()


@pytest.fixture(scope="module")
def mbest_engines(built):
    pair = _engine(PH_STEP1_PAIR="1")
    single = _engine(PH_STEP1_PAIR="0")
    yield pair, single
    pair.close()
    single.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got) - want))) <= TOL * float(np.max(np.abs(want)))


@pytest.mark.parametrize("n,w,gamma", fw.MBEST_CASES, ids=lambda v: str(v))
def test_m_best_through_the_pair_kernel(mbest_engines, n, w, gamma):
    pair, single = mbest_engines
    assert pair.m_best_info(n, fw.NUM)[0] == 2 and single.m_best_info(n, fw.NUM)[0] == 1
    x = np.array(fw.windows(n, w))
    a = pair.m_best(x, fw.NUM, gamma=gamma, want_sweeps=True)
    b = single.m_best(x, fw.NUM, gamma=gamma, want_sweeps=True)
    print("N", n, "W", w, "gamma", gamma, "periods", a[0].tolist(), "status", a[3].tolist(), "sweeps", a[4].tolist())
    assert (a[3] == 0).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), (a[0], b[0], a[4], b[4])
    for k, (per, pw, bs) in enumerate(fw.mbest_oracle(n, w, gamma)):
        assert np.array_equal(a[0][k], per), (k, a[0][k], per)
        assert _close(a[1][k], pw) and _close(a[2][k], bs), k


def test_small_to_large_with_fixed_and_run_time_wave_count(built):
    x = np.array(fw.windows(fw.S2L_N, fw.S2L_W))
    res = []
    for block in fw.S2L_BLOCKS:
        e = _engine(PH_S2L_PAIR="1", PH_S2L_BLOCK=str(block))
        try:
            res.append(e.small_to_large(x, fw.S2L_THRESH, None, cap=64))
        finally:
            e.close()
    first = res[0]
    for block, r in zip(fw.S2L_BLOCKS, res):
        print("PH_S2L_BLOCK", block, "counts", r[0].tolist())
        assert (r[4] == 0).all()
        assert np.array_equal(r[0], first[0]) and np.array_equal(r[1], first[1]) and np.array_equal(r[2], first[2]), block
        for k, cnt in enumerate(r[0]):
            assert np.array_equal(r[3][k, :cnt], first[3][k, :cnt]), (block, k)
    for k, ((per, pw, bs), _) in enumerate(fw.s2l_oracle()):
        cnt = int(first[0][k])
        assert list(first[1][k][:cnt]) == list(per), (k, first[1][k][:cnt], per)
        assert _close(first[2][k][:cnt], pw) and _close(first[3][k][:cnt], np.array(bs)), k


def test_best_correlation_through_the_pair_kernel(built):
    x = np.array(fw.windows(fw.BC_N, fw.BC_W))
    pair, single = _engine(PH_BC_PAIR="1"), _engine(PH_BC_PAIR="0")
    try:
        a = pair.best_correlation(x, fw.BC_NUM)
        b = single.best_correlation(x, fw.BC_NUM)
    finally:
        pair.close()
        single.close()
    print("best_correlation periods", a[0].tolist(), "status", a[3].tolist())
    # periods, bases and status bit for bit; the norm gains sum their squares in another order (test_gpu_pair.py: 1e-13)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert float(np.max(np.abs(a[1] - b[1]))) <= 1e-13 * float(np.max(np.abs(b[1])))
    for k, ((per, gains, bs), _) in enumerate(fw.bc_oracle()):
        assert np.array_equal(a[0][k], per), (k, a[0][k], per)
        assert _close(a[1][k], gains) and _close(a[2][k], bs), k
