"""k_mbest_step2 with the factor geometry from the host's table, against the fallback and the oracle.

The cases are the table of tests/test_m_best_step2_chain_cpu.py, whose census says which row and split path each of
them takes.  Every case runs on the default engine (PH_STEP2_GEOM unset: the table) and on one created with
PH_STEP2_GEOM=0 (lane 0 rebuilds the geometry per factor and hands it over through LDS): periods, status,
powers and bases must be equal bit for bit between the two, and both must agree with po.m_best at the bars of
tests/test_gpu_m_best_step2.py (periods exactly, powers 1e-10 / element-wise 1e-9, bases 1e-10 row by row).  Two
launches mix the windows of one shape with an all-zero window, whose step 1 fails and which step 2 passes through."""

import warnings

import numpy as np
import pytest

from conftest import elem_err, rel_err
from test_gpu_m_best_step2 import ELEM64, TOL64, _engine, row_err, run
from test_m_best_step2_chain_cpu import CASES, MIXED_LONG, MIXED_STAGED, case_signal, oracle_of

pytestmark = pytest.mark.gpu

BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    e = dict(on=default_engine(), off=_engine(PH_STEP2_GEOM=0), alone={})
    yield e
    e["off"].close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def alone(engines, which, c):
    """The engine's result for the case as a one-window call: computed once, shared."""
    key = (which, c["name"])
    if key not in engines["alone"]:
        engines["alone"][key] = run(engines[which], c)
    return engines["alone"][key]


def check(c, per, pw, bs, st, what):
    rper, rpw, rbs, _ = oracle_of(c)
    print(f"{c['name']} [{what}]: periods {per.tolist()} oracle {rper.tolist()} powers rel {rel_err(pw, rpw):.2e} "
          f"elem {elem_err(pw, rpw):.2e} bases by row {row_err(bs, rbs):.2e}")
    assert st == 0 and np.array_equal(per, rper), (c["name"], what, st, per, rper)
    assert rel_err(pw, rpw) <= TOL64 and elem_err(pw, rpw) <= ELEM64, (c["name"], what)
    assert bs.dtype == np.float64 and row_err(bs, rbs) <= TOL64, (c["name"], what)


def same_bits(a, b, what):
    for name, u, v in zip(("periods", "powers", "bases", "status"), a, b):
        assert u.dtype == v.dtype and np.array_equal(u, v), (what, name)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_switch_on_and_off_agree_bit_for_bit(engines, c):
    from pyperiod_amd import _ffi

    plan = engines["on"].plan_info("m_best", c["n"], (c["num"], c["min_length"], c["max_length"]), c["dtype"])
    assert plan[1].window == _ffi.PH_PLAN_LDS and plan[1].block == 512  # the path the switch acts on
    on, off = alone(engines, "on", c), alone(engines, "off", c)
    same_bits(on, off, c["name"])
    for which, (per, pw, bs, st) in (("on", on), ("off", off)):
        check(c, per[0], pw[0], bs[0], st[0], which)


@pytest.mark.parametrize("shape,names", [
    (MIXED_LONG, ("chain_prime_factor", "chain_cascade", "chain_present_after_split", None, "chain_after_prime", "chain_long_short", "chain_cascade")),
    (MIXED_STAGED, ("chain_split_last", "mix_cascade", None, "mix_present", "mix_last"))], ids=["long", "staged"])
def test_windows_on_different_paths_in_one_launch(engines, shape, names):
    """Windows of one shape in one call, an all-zero one among them (passed through with PH_ST_NO_PERIOD) and the last
    one unpaired in the window-pair step 1: every live window comes out bit for bit as it does alone, switch on or off."""
    from pyperiod_amd import _ffi

    cs = [BY_NAME[k] if k else None for k in names]
    live = [c for c in cs if c]
    assert len(cs) % 2 == 1 and all({k: c[k] for k in shape} == shape for c in live)
    x = np.stack([case_signal(c) if c else np.zeros(shape["n"]) for c in cs])
    on, off = run(engines["on"], live[0], x), run(engines["off"], live[0], x)
    alive = [w for w, c in enumerate(cs) if c]  # (the powers of a window without a period are 0 / 0)
    same_bits([a[alive] for a in on], [a[alive] for a in off], names)
    assert np.array_equal(on[3], off[3])
    per, pw, bs, st = on
    for w, c in enumerate(cs):
        if c is None:
            assert st[w] == _ffi.PH_ST_NO_PERIOD and not bs[w].any() and not off[2][w].any(), (w, st[w])
            continue
        check(c, per[w], pw[w], bs[w], st[w], f"window {w} of {len(cs)}")
        same_bits([a[w] for a in on], [a[0] for a in alone(engines, "on", c)], (w, c["name"]))
