"""best_correlation (k_best_correlation_pair, k_best_correlation) against the reference and the oracle on every screen
and event path of both kernels (case table and restatements: bc_cases.py, census: test_bc_census_cpu.py).

Four engines: the default (the pair kernel wherever plan_best_correlation allows it), the one-window kernel
(PH_BC_PAIR=0), the same with 256 threads (PH_SWEEP_BLOCK=256) and with the window in HBM (PH_HBM_WINDOW=1).  Every window
of every case on every engine: status 1 exactly where the reference raises, else 0; the period row equal to the expected
one (every window of the table passes the margin rule or is exact, the CPU census asserts it); gain k within
TOL ||r_k|| / ||x|| and base row k within TOL max|r_k| element by element, r_k the residual before round k -- a gain of
1e-12 after a collapse does not hide under the first one; a rejected or unreached row is exactly zero.  TOL = 1e-10;
float32 windows 1e-4.  The expected values are the reference's own (tests/golden/best_correlation_edges.npz) where the
table names a fixture tag, the oracle's elsewhere.  Windows whose arithmetic is exact in any order (impulses: ties of all
periods; near ties of 2^-51) are held bit for bit in periods and bases and to 1e-13 relative in the gain.

The engines among each other, the two windows of a pair swapped, and every window alone against itself in its batch:
status, periods and bases bit for bit, gains to 1e-13 ||r_k|| / ||x|| (the pair kernel adds its squares in another
order; a gain is the difference of two norms of that size, so that is what its rounding error is relative to).

Measured on an MI355X: largest error 4.0e-6 of the gain bar and 0 of the base bar for float64 on every engine (trunc / orth
5.6e-6 and 0), 6.3e-5 and 8.7e-4 for float32.  The module takes 1.5 s, 0.7 s of them the creation of the four engines.
Before the one-window kernel skipped its screen on a non-finite sum|x| it reported status 1 on the single-NaN window on
all three one-window engines (and for float32 input on the default one), while the pair kernel returned the reference's
zeros.
"""

import os
import warnings

import numpy as np
import pytest

import bc_cases as bc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "best_correlation_edges.npz")
REL = 1e-13


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
    assert not any(k in os.environ for env in bc.ENGINES.values() for k in env)
    e = {name: _engine(**env) for name, env in bc.ENGINES.items()}
    e["runs"] = {}
    e["fixture"] = bc.load_fixture(GOLDEN)
    for case in bc.CASES:  # the expected answers of the whole table, once for every test of the module
        bc.ref(case)
    yield e
    for name in bc.ENGINES:
        e[name].close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def call(engine, case, x):
    return engine.best_correlation(np.ascontiguousarray(x), case["num"], bc.max_length_of(case), case["ratio"], case["trunc"], case["orth"])


def run(engines, name, case):
    key = (name, case["name"])
    if key not in engines["runs"]:
        engines["runs"][key] = call(engines[name], case, bc.windows(case))
    return engines["runs"][key]


def expected(engines, case, w):
    """-> (status, periods, norms, bases): the reference's answer where window w has a fixture tag, the oracle's elsewhere.
    Where the reference raises, the rounds before the raise are the oracle's and the rest is zero."""
    r = bc.ref(case)[w]
    tag = case["fixture"][w]
    if tag is not None and engines["fixture"][tag][0] == "ok":
        f = engines["fixture"][tag]
        assert r["raised"] is None
        return 0, f[1], f[2], f[3]
    if tag is not None:
        assert r["raised"] is not None
    return (0 if r["raised"] is None else 1), r["periods"], r["norms"], r["bases"]


def close(a, b, rel=REL):
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def gain_units(case):
    """(W, num): ||r_k|| / ||x|| of the residual before round k, the size of the two norms a gain is the difference of
    (0 where the expected row is zero: equal exactly).  Two engines that add the squares in different orders differ by a
    few 1e-16 of it, however small the gain itself is."""
    u = np.zeros((len(case["kinds"]), case["num"]))
    for w, r in enumerate(bc.ref(case)):
        for k, rd in enumerate(r["rounds"]):
            if r["periods"][k]:
                u[w, k] = rd["rnorm"] / r["rounds"][0]["rnorm"]
    return u


def same(case, a, b, what, rows=slice(None)):
    """a against rows `rows` of b: periods, bases, status bit for bit; gains to 1e-13 of gain_units."""
    b = [v[rows] for v in b]
    assert np.array_equal(a[3], b[3]), (what, "status", a[3], b[3])
    assert np.array_equal(a[0], b[0]), (what, "periods", a[0], b[0])
    assert np.array_equal(a[2].view(np.uint8), b[2].view(np.uint8)), (what, "bases")
    assert np.all(np.abs(a[1] - b[1]) <= REL * gain_units(case)[rows]), (what, "gains", a[1] - b[1], gain_units(case)[rows])


def held(engines, case, got, what, only=None):
    """Every window of the case against its expected answer.  -> the largest gain and base error as fractions of their
    bars."""
    per, nr, bs, st = got
    tol = bc.TOL if case["dtype"] == np.float64 else bc.TOL32
    assert bs.dtype == case["dtype"] and per.shape == (len(case["kinds"]) if only is None else 1, case["num"])
    worst = [0.0, 0.0]
    for w in range(len(case["kinds"])) if only is None else [only]:
        g = w if only is None else 0
        want_st, wper, wnr, wbs = expected(engines, case, w)
        r = bc.ref(case)[w]
        print(what, w, case["kinds"][w], "status", int(st[g]), "periods", per[g].tolist(), "expected", want_st, np.asarray(wper).tolist())
        assert st[g] == want_st, (what, w, "status", st[g], want_st)
        assert bc.admitted(case, w), (what, w)
        assert list(per[g]) == list(wper), (what, w, "periods", list(per[g]), list(wper))
        og = r["rounds"][0]["rnorm"] if r["rounds"] else 0.0
        for k in range(case["num"]):
            if wper[k] == 0:  # rejected, or not reached: the row is zero, not a leftover projection
                assert nr[g, k] == 0.0 and not bs[g, k].any(), (what, w, k, "zero row")
                continue
            rd = r["rounds"][k]
            unit_g, unit_b = rd["rnorm"] / og, rd["rmax"]
            eg = abs(float(nr[g, k]) - float(wnr[k]))
            eb = float(np.max(np.abs(bs[g, k].astype(np.float64) - wbs[k])))
            print(f"    round {k}: p {int(wper[k])} gain {float(nr[g, k])!r} expected {float(wnr[k])!r} error {eg / unit_g:.2e} of ||r_k||/||x||, "
                  f"base error {eb / unit_b:.2e} of max|r_k|")
            assert eg <= tol * unit_g, (what, w, k, "gain", float(nr[g, k]), float(wnr[k]), eg / unit_g)
            assert eb <= tol * unit_b, (what, w, k, "base", eb / unit_b)
            worst = [max(worst[0], eg / (tol * unit_g)), max(worst[1], eb / (tol * unit_b))]
            if case["exact"][w]:
                assert np.array_equal(bs[g, k].astype(np.float64), wbs[k]), (what, w, k, "base bits")
                assert close(nr[g, k], wnr[k]), (what, w, k, "gain", float(nr[g, k]), float(wnr[k]))
    return worst


def test_plans(engines):
    """Each engine runs the variant bc_cases.plan_variant predicts for each case, the pair kernel with the LDS bytes of
    bc_cases.pair_lds_bytes and 1024 threads, the one-window kernel with 512 or 256 and the window where asked."""
    from pyperiod_amd import _ffi

    seen = set()
    for case in bc.CASES:
        for name, env in bc.ENGINES.items():
            (k,) = engines[name].plan_info("best_correlation", case["n"], (bc.max_length_of(case),), case["dtype"], case["trunc"], case["orth"])
            got = "pair" if k.variant == _ffi.PH_PLAN_PAIR else "one"
            assert got == bc.plan_variant(case["dtype"], bc.general(case), case["n"], bc.max_length_of(case), env), (case["name"], name, k)
            if got == "pair":
                assert k.lds_bytes == bc.pair_lds_bytes(case["n"]) and k.block == bc.K_PAIR_BLOCK, (case["name"], name, k)
            else:
                assert k.block == int(env.get("PH_SWEEP_BLOCK", 512)), (case["name"], name, k)
                assert (k.window == _ffi.PH_PLAN_HBM) == bool(env.get("PH_HBM_WINDOW")), (case["name"], name, k)
            seen.add((name, got))
    assert seen == {("pair", "pair"), ("pair", "one"), ("one", "one"), ("one256", "one"), ("hbm", "one")}, seen


@pytest.mark.parametrize("name", list(bc.ENGINES))
def test_every_case_against_the_reference(engines, name):
    worst = {}
    for case in bc.CASES:
        w = held(engines, case, run(engines, name, case), (case["name"], name))
        key = np.dtype(case["dtype"]).name + (" trunc/orth" if bc.general(case) else "")
        worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0.0, 0.0]), w)]
    for key, (wg, wb) in worst.items():
        print(f"{name} {key}: largest gain error {wg:.2e} of its bar, largest base error {wb:.2e} of its bar")


def test_engines_equal_each_other(engines):
    for case in bc.CASES:
        for name in ("one", "one256", "hbm"):
            same(case, run(engines, name, case), run(engines, "pair", case), (case["name"], name, "against the default engine"))


@pytest.mark.parametrize("name", list(bc.ENGINES))
def test_halves(engines, name):
    """Swapping the two windows of a pair swaps the outputs, and every window alone equals the same window in its batch:
    nothing of a neighbour -- a stale staging buffer, a NaN, a scale, a status -- leaks."""
    n = 0
    for case in bc.CASES:
        x = bc.windows(case)
        both = run(engines, name, case)
        if len(x) == 2:
            sw = call(engines[name], case, x[::-1])
            same(case, tuple(a[::-1] for a in sw), both, (case["name"], name, "swapped"))
            n += 1
        if len(x) > 1:
            for w in range(len(x)):
                same(case, call(engines[name], case, x[w:w + 1]), both, (case["name"], name, "alone", w), rows=slice(w, w + 1))
    assert n >= 40


def test_periods_class(engines):
    """Periods().best_correlation: a batch with a single-NaN (+Inf, -Inf) window returns the reference's zeros for it and
    the healthy window's answer beside it; a batch with a window the reference raises on raises TypeError."""
    from pyperiod_amd import Periods

    fx = engines["fixture"]
    for kind in bc.DEGENERATE:
        for place in ("first", "second"):
            case = bc.BY_NAME[f"deg_{kind}_{place}"]
            w = 0 if place == "first" else 1
            x = bc.windows(case)
            if fx["deg_" + kind][0] == "raises":
                with pytest.raises(TypeError):
                    Periods().best_correlation(x, num=case["num"])
                with pytest.raises(TypeError):
                    Periods().best_correlation(x[w], num=case["num"])
                continue
            per, nr, bs = Periods().best_correlation(x, num=case["num"])
            got = (per, nr, bs, np.zeros(2, np.int32))
            held(engines, case, got, (case["name"], "Periods"))
            one = Periods().best_correlation(x[w], num=case["num"])
            assert np.array_equal(one[0], per[w]) and np.array_equal(one[2], bs[w]) and close(one[1], nr[w])
            if kind in bc.ZEROS_REF:
                assert not per[w].any() and not nr[w].any() and not bs[w].any() and per[1 - w].any()
