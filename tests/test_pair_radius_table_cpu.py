"""The radius table of the window-pair screen of m_best (ph_pair_radius_table: what the host uploads next to the float
geometry and k_mbest_step1_pair reads in its survivor scan), pinned on the CPU.

pair_radius(R, q) = 1.5 (2 R + floor(q / 64) + 32) 2^-24 bounds |float screen - fp64 value| of period q in units of the
window's sum of squares; the proof in pyperiod_amd/csrc/ph_pair.h is stated for R = ceil(N / q), the row count of the
period, and that is the entry of the table.  The scan used to estimate the row count on the device,
R' = int(fl32(fl32(fl32(N) * rcp(q)) * 1.000001f)) + 1 with the hardware's approximate reciprocal, and took
pair_radius(R', q): an upper estimate.  Both expressions are restated here in numpy; the table must equal the first
and never exceed the second, so the survivor lists can only shrink towards what the proof allows."""
import ctypes

import numpy as np
import pytest

LENGTHS = (256, 2246, 4096)
U = 2.0 ** -24


def radius(rows, q):
    return 1.5 * (2.0 * rows.astype(np.float64) + (q >> 6).astype(np.float64) + 32.0) * U


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    cache = {}

    def get(n):
        if n not in cache:
            out = np.full(n // 2 + 1, np.nan)
            rc = lib.ph_pair_radius_table(n, n // 2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
            assert rc == _ffi.PH_OK
            cache[n] = out
        return cache[n]

    return get


@pytest.mark.parametrize("n", LENGTHS)
def test_table_is_the_radius_at_the_row_count_of_the_period(table, n):
    q = np.arange(2, n // 2 + 1)
    rows = -(-n // q)
    got = table(n)
    assert got.shape == (n // 2 + 1,) and got[0] == 0.0
    assert np.array_equal(got[q], radius(rows, q))  # 1.5 x integer x 2^-24: exact in fp64, so equality is the bar
    assert np.all(got[1:] > 0.0)


@pytest.mark.parametrize("n", LENGTHS)
def test_table_never_exceeds_the_radius_at_the_estimated_row_count(table, n):
    q = np.arange(2, n // 2 + 1)
    rows = -(-n // q)
    fn, k = np.float32(n), np.float32(1.000001)
    rcp = np.float32(1.0) / q.astype(np.float32)
    # the hardware reciprocal is good to one ulp: the estimate is taken at the correctly rounded value and one ulp to
    # either side of it
    for r in (rcp, np.nextafter(rcp, np.float32(0.0)), np.nextafter(rcp, np.float32(1.0))):
        est = ((fn * r).astype(np.float32) * k).astype(np.float32).astype(np.int64) + 1
        assert np.all(est >= rows)
        assert np.all(table(n)[q] <= radius(est, q))
    assert np.any(radius(((fn * rcp).astype(np.float32) * k).astype(np.float32).astype(np.int64) + 1, q) > table(n)[q])  # (it is an estimate)


def test_arguments_are_checked_on_the_host(table):
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    out = np.zeros(8)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.ph_pair_radius_table(4, 7, ptr) == _ffi.PH_E_ARG  # max_p > N
    assert lib.ph_pair_radius_table(0, 1, ptr) == _ffi.PH_E_ARG
    assert lib.ph_pair_radius_table(7, 7, None) == _ffi.PH_E_ARG
    assert lib.ph_pair_radius_table(7, 7, ptr) == _ffi.PH_OK and out[7] == 1.5 * (2.0 + 32.0) * U
