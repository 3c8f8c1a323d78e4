"""m_best step 2 (k_mbest_step2) against the oracle on every row form and split path.

The cases are the table of tests/test_m_best_step2_cpu.py, whose census says which path of the kernel each of them takes
(staged rows that split, cascades, splits blocked by `present`, staged rows of several pieces, rows beyond the staging
limit, the tiled path, more than 64 divisors, gamma mode, float32, trunc / orth) and holds every decision of every case
at least 1e-6 (float32: 1e-2) away from a tie.  Each case runs through eng.m_best and is compared with po.m_best:
status 0, periods exactly, powers to 1e-10 (element-wise 1e-9), bases row by row to 1e-10 of the row's own maximum
(floored at 1e-5 of the matrix's, as conftest.elem_err does), so that a weak remainder row is not hidden behind the
strongest one; float32 cases to 1e-4 throughout, against the oracle on the float32-rounded input.  The fp64 cases up to
N = 4000 run a second time on an engine whose windows live in HBM (the LW == false instantiation, which stages nothing),
and one launch mixes windows that take different paths."""

import os
import warnings

import numpy as np
import pytest

from conftest import elem_err, rel_err
from test_m_best_step2_cpu import BY_NAME, CASES, MIXED_GAMMA, MIXED_PLAIN, case_signal, oracle_of

pytestmark = pytest.mark.gpu

TOL64, ELEM64, TOL32 = 1e-10, 1e-9, 1e-4
TOL_HBM = 1e-12  # engine against engine, as tests/test_gpu_placement_edges.py
HBM_CASES = [c for c in CASES if c["dtype"] == np.float64 and not (c["trunc"] or c["orth"]) and c["n"] <= 4000]


def _engine(**env):
    """A fresh engine created with `env` set (the variables are read by ph_create) and restored right after."""
    from pyperiod_amd import PeriodEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
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
    from pyperiod_amd import default_engine

    e = dict(eng=default_engine(), hbm=_engine(PH_HBM_WINDOW=1), alone={})
    yield e
    e["hbm"].close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def run(engine, c, x=None):
    x = case_signal(c)[None, :] if x is None else x
    return engine.m_best(x, c["num"], c["max_length"], c["min_length"], c["gamma"], c["trunc"], c["orth"])


def alone(engines, c):
    """The default engine's result for the case as a one-window call: computed once, shared."""
    if c["name"] not in engines["alone"]:
        engines["alone"][c["name"]] = run(engines["eng"], c)
    return engines["alone"][c["name"]]


def row_err(got, want):
    """max over rows of max|got - want| / max(max|want_row|, 1e-5 max|want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.maximum(np.max(np.abs(want), axis=1), max(1e-5 * float(np.max(np.abs(want))), 1e-300))
    return float(np.max(np.max(np.abs(got - want), axis=1) / den))


def check(c, per, pw, bs, st, what):
    rper, rpw, rbs, _ = oracle_of(c)
    tol, etol = (TOL64, ELEM64) if c["dtype"] == np.float64 else (TOL32, TOL32)
    print(f"{c['name']} [{what}]: periods {per.tolist()} oracle {rper.tolist()} powers rel {rel_err(pw, rpw):.2e} "
          f"elem {elem_err(pw, rpw):.2e} bases by row {row_err(bs, rbs):.2e}")
    assert st == 0 and np.array_equal(per, rper), (c["name"], what, st, per, rper)
    assert rel_err(pw, rpw) <= tol and elem_err(pw, rpw) <= etol, (c["name"], what)
    assert bs.dtype == c["dtype"] and row_err(bs, rbs) <= tol, (c["name"], what)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_matches_the_oracle(engines, c):
    from pyperiod_amd import _ffi

    per, pw, bs, st = alone(engines, c)
    check(c, per[0], pw[0], bs[0], st[0], "default")
    plan = engines["eng"].plan_info("m_best", c["n"], (c["num"], c["min_length"], c["max_length"]), c["dtype"], c["trunc"], c["orth"])
    assert plan[1].window == _ffi.PH_PLAN_LDS  # the staging area exists
    assert plan[1].block == (256 if c["trunc"] or c["orth"] else 512)  # the general path has its own block


@pytest.mark.parametrize("c", HBM_CASES, ids=lambda c: c["name"])
def test_case_with_the_window_in_hbm(engines, c):
    """LW == false: the row buffer is an HBM workspace and nothing is staged; the splits are the same."""
    from pyperiod_amd import _ffi

    hbm = engines["hbm"]
    plan = hbm.plan_info("m_best", c["n"], (c["num"], c["min_length"], c["max_length"]), c["dtype"])
    assert plan[1].window == _ffi.PH_PLAN_HBM
    per, pw, bs, st = run(hbm, c)
    check(c, per[0], pw[0], bs[0], st[0], "hbm window")
    dper, dpw, dbs, dst = alone(engines, c)
    assert np.array_equal(per, dper) and np.array_equal(st, dst)
    assert rel_err(pw, dpw) <= TOL_HBM and rel_err(bs, dbs) <= TOL_HBM, (rel_err(pw, dpw), rel_err(bs, dbs))


@pytest.mark.parametrize("shape,names", [(MIXED_PLAIN, ("mix_cascade", "mix_primes", "mix_present", None, "mix_last")),
                                         (MIXED_GAMMA, ("gmix_cascade", "gmix_primes", "gmix_present", None, "gmix_last"))],
                         ids=["plain", "gamma"])
def test_windows_on_different_paths_in_one_launch(engines, shape, names):
    """Five windows of one N in one call: a cascade, planted primes only (step 2 reads no row), a split blocked by
    `present`, an all-zero window (passed through with PH_ST_NO_PERIOD) and, unpaired in the window-pair step 1, one
    that splits.  Every live window must come out bit for bit as it does alone."""
    from pyperiod_amd import _ffi

    cs = [BY_NAME[k] if k else None for k in names]
    live = [c for c in cs if c]
    assert len(cs) % 2 == 1 and all({k: c[k] for k in shape} == shape for c in live)
    x = np.stack([case_signal(c) if c else np.zeros(shape["n"]) for c in cs])
    per, pw, bs, st = run(engines["eng"], live[0], x)
    for w, c in enumerate(cs):
        if c is None:
            assert st[w] == _ffi.PH_ST_NO_PERIOD and not bs[w].any(), (w, st[w])
            continue
        check(c, per[w], pw[w], bs[w], st[w], f"window {w} of {len(cs)}")
        aper, apw, abs_, ast = alone(engines, c)
        assert st[w] == ast[0] and np.array_equal(per[w], aper[0]), (w, c["name"])
        assert np.array_equal(pw[w], apw[0]) and np.array_equal(bs[w], abs_[0]), (w, c["name"])


def test_the_step_2_kernel_is_what_ran(engines):
    eng = engines["eng"]
    eng.profile(True)
    try:
        run(eng, BY_NAME["two_cascades"])
        names = {k for k, _ in eng.profile_read()}
    finally:
        eng.profile(False)
    assert "k_mbest_step2" in names, names
