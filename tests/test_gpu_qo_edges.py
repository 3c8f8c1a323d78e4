"""QOPeriods.find_periods device loops (k_qo_find, its trunc instantiation, k_qo_greedy) at their limits, against the
reference and the oracle: the fixed-weight quirks, 16 / 17 / 40-block dictionaries (LDS pair table, then the inline
gcd), the 64-block exit, the row capacity at R and R - 1, the residual's LDS / HBM placement on both sides of every
boundary ph_qo_plan_info reports, and a seeded fuzz.  Reference cases come from tests/golden/qoperiods_edges.npz
(make_golden_qo_edges.py)."""

import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from test_oracle_golden import qo_edge_case

pytestmark = pytest.mark.gpu

F64_TOL = dict(norms=1e-10, weights=1e-8, residual=1e-8)
F32_TOL = dict(norms=1e-4, weights=1e-4, residual=1e-4)
VARIANTS = [(False, True), (True, True), (False, False), (True, False)]  # (trunc, update_weights)
VARIANT_IDS = ["default", "trunc", "keep", "keep_trunc"]
MARGIN = {np.float64: 1e-9, np.float32: 1e-5}  # as in make_golden_qo_edges.py


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


@pytest.fixture(scope="module")
def hbm_eng():
    """An engine whose k_qo_find / k_qo_greedy always keep the residual in HBM (PH_QO_HBM_WINDOW is read when the
    context is created; the variable is restored right after)."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import PeriodEngine

    old = os.environ.get("PH_QO_HBM_WINDOW")
    os.environ["PH_QO_HBM_WINDOW"] = "1"
    try:
        e = PeriodEngine(0)
    finally:
        if old is None:
            del os.environ["PH_QO_HBM_WINDOW"]
        else:
            os.environ["PH_QO_HBM_WINDOW"] = old
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _qo(trunc=False):
    from pyperiod_amd import QOPeriods

    return QOPeriods(trunc_to_integer_multiple=trunc)


def _rows(periods, keeps, nb):
    """Dictionary rows of the first nb blocks of a device result (a keep of 0 holds all p rows)."""
    return sum(int(k) if k else int(q) for q, k in zip(periods[:nb], keeps[:nb]))


def _check(got, want, tol, what):
    """got = (output_bases, residual) of the class; want = dict with periods, norms, weights, dict_keys, dict_vals,
    residual."""
    gb, gr = got
    assert np.array_equal(np.asarray(gb["periods"]), want["periods"]), (what, gb["periods"], want["periods"])
    assert [int(k) for k in gb["basis_dictionary"]] == [int(k) for k in want["dict_keys"]], what
    assert [int(v) for v in gb["basis_dictionary"].values()] == [int(v) for v in want["dict_vals"]], what
    assert rel_err(gb["norms"], want["norms"]) <= tol["norms"], what
    assert np.asarray(gb["weights"]).shape == np.asarray(want["weights"]).shape, what
    assert rel_err(gb["weights"], want["weights"]) <= tol["weights"], what
    assert rel_err(gr, want["residual"]) <= tol["residual"], what


def _fixture(g, tag):
    return {k: g[f"{tag}_{k}"] for k in ("periods", "norms", "weights", "dict_keys", "dict_vals", "residual")}


def _oracle(x, kw, trunc, uw, trace=None):
    out, res = po.qo_find_periods(np.asarray(x, dtype=np.float64), trunc=trunc, update_weights=uw, trace=trace, **kw)
    return {"periods": out["periods"], "norms": out["norms"], "weights": out["weights"],
            "dict_keys": [int(k) for k in out["basis_dictionary"]],
            "dict_vals": list(out["basis_dictionary"].values()), "residual": res, "subspaces": out["subspaces"]}


def _gram_cond(want):
    a = np.asarray(want["subspaces"])
    return float(np.linalg.cond(a @ a.T))


# ---------------------------------------------------------------------------- reference fixtures
def test_fixtures_batch_and_rows(eng, golden):
    """Every case of qoperiods_edges.npz through QOPeriods().find_periods: a batch of two copies of the window (one
    launch of k_qo_find / k_qo_greedy, fallbacks included) and the 1-D call.  The 1-D call is left out where it runs
    what the batch ran: blocks40 / blocks40_t (the same k_qo_find launch, seconds each) and blocks70 (PH_ST_CAP, then
    the host loop on its 1686-row dictionary, which the batch of one row already ran)."""
    g = golden("qoperiods_edges")
    for tag in (str(t) for t in g["tags"]):
        x, kw, trunc, uw = qo_edge_case(g, tag)
        tol = F32_TOL if x.dtype == np.float32 else F64_TOL
        want = _fixture(g, tag)
        copies = 1 if tag == "blocks70" else 2
        batch = _qo(trunc).find_periods(np.vstack([x] * copies), update_weights=uw, **kw)
        for w in range(copies):
            _check(batch[w], want, tol, (tag, "batch row", w))
        if tag not in ("blocks40", "blocks40_t", "blocks70"):
            _check(_qo(trunc).find_periods(x, update_weights=uw, **kw), want, tol, (tag, "1-D"))


# ---------------------------------------------------------------------------- block limits
@pytest.mark.parametrize("tag,blocks", [("blocks16", 16), ("blocks17", 17), ("blocks40", 40), ("blocks40_t", 40)])
def test_pair_table_and_inline_gcd(eng, golden, tag, blocks):
    """16 blocks keep their pair constants in the LDS table (kQoPairTab); 17 and 40 compute them inline."""
    g = golden("qoperiods_edges")
    x, kw, trunc, uw = qo_edge_case(g, tag)
    per, nrm, keeps, counts, wts, res, st = eng.qo_find_periods(x[None, :], kcap=2048, trunc=trunc, **kw)
    assert st[0] == 0 and counts[0, 0] == blocks and counts[0, 1] == blocks, (tag, st, counts)
    assert np.array_equal(per[0, :blocks], g[f"{tag}_periods"]), tag
    assert list(keeps[0, :blocks]) == list(g[f"{tag}_dict_vals"]), tag
    rows = int(g[f"{tag}_rows"])
    assert _rows(per[0], keeps[0], blocks) == rows, tag
    assert rel_err(nrm[0, :blocks], g[f"{tag}_norms"]) <= F64_TOL["norms"], tag
    assert rel_err(wts[0, :rows], g[f"{tag}_weights"]) <= F64_TOL["weights"], tag
    assert rel_err(res[0], g[f"{tag}_residual"]) <= F64_TOL["residual"], tag


def test_block_limit_exit_and_greedy(eng, golden):
    """blocks70: k_qo_find stops at kQoMaxBlocks (64) with PH_ST_CAP although 2048 rows would hold the dictionary (the
    class re-runs the row on the host: test_fixtures_batch_and_rows); k_qo_greedy has no block limit and finishes 70
    blocks."""
    from pyperiod_amd import _ffi

    g = golden("qoperiods_edges")
    x, kw, trunc, uw = qo_edge_case(g, "blocks70")
    assert uw and int(g["blocks70_rows"]) <= 2048
    per, nrm, keeps, counts, wts, res, st = eng.qo_find_periods(x[None, :], kcap=2048, **kw)
    assert st[0] == _ffi.PH_ST_CAP and counts[0, 1] == 64, (st, counts)  # kQoMaxBlocks, not the 2048 rows

    x, kw, trunc, uw = qo_edge_case(g, "blocks70_k")
    rows = int(g["blocks70_k_rows"])
    assert not uw and rows > 2048
    per, nrm, keeps, counts, wts, res, st = eng.qo_find_periods(x[None, :], kcap=4096, update_weights=False, **kw)
    assert st[0] == 0 and counts[0, 0] == 70 and counts[0, 1] == 70, (st, counts)
    assert np.array_equal(per[0], g["blocks70_k_periods"]) and _rows(per[0], keeps[0], 70) == rows
    assert rel_err(wts[0, :rows], g["blocks70_k_weights"]) <= F64_TOL["weights"]
    assert rel_err(res[0], g["blocks70_k_residual"]) <= F64_TOL["residual"]


# ---------------------------------------------------------------------------- row capacity
@pytest.mark.parametrize("trunc,uw", VARIANTS, ids=VARIANT_IDS)
def test_row_capacity_edge(eng, monkeypatch, trunc, uw):
    """kcap = R (the rows the window needs) runs with status 0 and the large-kcap answer; kcap = R - 1 ends with
    PH_ST_CAP, and the class, handed that kcap on its first launch, still returns the oracle's answer."""
    from pyperiod_amd import _ffi
    from pyperiod_amd.synth import multi_sinusoid_window

    x = multi_sinusoid_window(5, 1537)
    kw = dict(num=6, thresh=0.02, min_length=2, max_length=200)
    big = eng.qo_find_periods(x[None, :], kcap=2048, trunc=trunc, update_weights=uw, **kw)
    assert big[6][0] == 0, big[6]
    nb = int(big[3][0, 1])
    r = _rows(big[0][0], big[2][0], nb)
    assert 64 < r < 2048
    edge = eng.qo_find_periods(x[None, :], kcap=r, trunc=trunc, update_weights=uw, **kw)
    assert edge[6][0] == 0, (r, edge[6])
    assert np.array_equal(edge[3], big[3])
    assert np.array_equal(edge[0][0, :nb], big[0][0, :nb]) and np.array_equal(edge[2][0, :nb], big[2][0, :nb])
    assert rel_err(edge[1][0, :nb], big[1][0, :nb]) <= 1e-12
    assert rel_err(edge[4][0, :r], big[4][0, :r]) <= 1e-12 and rel_err(edge[5], big[5]) <= 1e-12
    short = eng.qo_find_periods(x[None, :], kcap=r - 1, trunc=trunc, update_weights=uw, **kw)
    assert short[6][0] == _ffi.PH_ST_CAP, (r, short[6])

    seen = []
    launch = eng.qo_find_periods

    def first_launch_short(xs, num, thresh, min_length, max_length, kcap, **k):
        out = launch(xs, num, thresh, min_length, max_length, r - 1 if not seen else kcap, **k)
        seen.append((r - 1 if not seen else kcap, int(out[6][0])))
        return out

    monkeypatch.setattr(eng, "qo_find_periods", first_launch_short)
    got = _qo(trunc).find_periods(x[None, :], update_weights=uw, **kw)[0]
    assert seen[0] == (r - 1, _ffi.PH_ST_CAP), seen
    _check(got, _oracle(x, kw, trunc, uw), F64_TOL, ("class after PH_ST_CAP", trunc, uw, r))


# ---------------------------------------------------------------------------- LDS / HBM placement
PLACE_KW = dict(num=3, thresh=0.01, min_length=2, max_length=80)  # at most 3 blocks of <= 80 rows: fits kcap 256


def _place_window(n, seed):
    """Three sinusoids with integer periods in [8, 70] and a little noise: the periods are inside [2, 80]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.05 * rng.standard_normal(n)
    for T in rng.choice(np.arange(8, 71), size=3, replace=False):
        x += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * t / T + rng.uniform(0, 2 * np.pi))
    return x


def _boundaries(eng, dtype, kcap, trunc, uw, hi=50000, step=64):
    """Every N (up to hi) where qo_plan_info's placement differs from that of N - 1: a scan in steps of `step`,
    then bisection inside each step that changes.  Host only."""
    place = lambda n: eng.qo_plan_info(n, dtype, kcap, PLACE_KW["max_length"], trunc, uw)[0]  # noqa: E731
    out = []
    lo, plo = 3 * PLACE_KW["max_length"], None
    plo = place(lo)
    n = lo
    while n < hi:
        m = min(n + step, hi)
        pm = place(m)
        if pm != plo:
            a, b = n, m  # place(a) == plo != place(b)
            while b - a > 1:
                c = (a + b) // 2
                if place(c) == plo:
                    a = c
                else:
                    b = c
            out.append(b)
            n, plo = b, place(b)
            continue
        n, plo = m, pm
    return out


@pytest.mark.parametrize("trunc,uw", VARIANTS, ids=VARIANT_IDS)
def test_placement_boundaries(eng, hbm_eng, trunc, uw):
    """Windows of N* - 1, N* and N* + 1 samples at every placement boundary N* (fp64 and fp32, kcap 256 and 1024):
    the placement changes inside the triple, the result equals that of an engine that keeps every residual in HBM,
    and for fp64 the oracle's."""
    from pyperiod_amd import _ffi

    for dtype in (np.float64, np.float32):
        for kcap in (256, 1024):
            bounds = _boundaries(eng, dtype, kcap, trunc, uw)
            # k_qo_find: window in LDS behind the work vectors, overlaid by them, then in HBM; k_qo_greedy: LDS, HBM
            visited = {eng.qo_plan_info(n, dtype, kcap, PLACE_KW["max_length"], trunc, uw)[0]
                       for b in bounds for n in (b - 1, b)}
            want = {_ffi.PH_QO_LDS_BEHIND, _ffi.PH_QO_HBM} | ({_ffi.PH_QO_LDS_OVERLAY} if uw else set())
            assert visited == want, (dtype, kcap, trunc, uw, bounds, visited)
            for nstar in bounds:
                what = (dtype.__name__, kcap, trunc, uw, nstar)
                places = {eng.qo_plan_info(n, dtype, kcap, PLACE_KW["max_length"], trunc, uw)[0]
                          for n in (nstar - 1, nstar, nstar + 1)}
                assert len(places) == 2, (what, places)
                assert hbm_eng.qo_plan_info(nstar, dtype, kcap, PLACE_KW["max_length"], trunc, uw)[0] == _ffi.PH_QO_HBM
                for n in (nstar - 1, nstar, nstar + 1):
                    x = _place_window(n, nstar + n).astype(dtype)
                    a = eng.qo_find_periods(x[None, :], kcap=kcap, trunc=trunc, update_weights=uw, **PLACE_KW)
                    b = hbm_eng.qo_find_periods(x[None, :], kcap=kcap, trunc=trunc, update_weights=uw, **PLACE_KW)
                    assert a[6][0] == 0 and b[6][0] == 0, (what, n, a[6], b[6])
                    nb = int(a[3][0, 1])
                    assert np.array_equal(a[3], b[3]), (what, n)  # counts
                    assert np.array_equal(a[0][0, :nb], b[0][0, :nb]) and np.array_equal(a[2][0, :nb], b[2][0, :nb]), (what, n)
                    r = _rows(a[0][0], a[2][0], nb)
                    assert rel_err(a[1][0, :nb], b[1][0, :nb]) <= 1e-12, (what, n)
                    assert rel_err(a[4][0, :r], b[4][0, :r]) <= 1e-12, (what, n)
                    assert rel_err(a[5], b[5]) <= 1e-12, (what, n)
                    if dtype == np.float64:
                        want = _oracle(x, PLACE_KW, trunc, uw)
                        nr = len(want["periods"])
                        assert int(a[3][0, 0]) == nr and r == len(want["weights"]), (what, n, a[3], r)
                        assert np.array_equal(a[0][0, :nr], want["periods"]), (what, n, a[0][0], want["periods"])
                        if uw:  # distinct periods: the dictionary lists every block's rows in order
                            assert list(a[2][0, :nb]) == want["dict_vals"], (what, n)
                        assert rel_err(a[1][0, :nr], want["norms"]) <= F64_TOL["norms"], (what, n)
                        assert rel_err(a[4][0, :r], want["weights"]) <= F64_TOL["weights"], (what, n)
                        assert rel_err(a[5][0], want["residual"]) <= F64_TOL["residual"], (what, n)


# ---------------------------------------------------------------------------- seeded fuzz
def _fuzz_windows(seed, n, hi, count, dtype):
    """`count` windows of n samples: three sinusoids with periods in [2.5, hi] and a little noise."""
    r2 = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    base = np.empty((count, n))
    for d in range(count):
        base[d] = 0.05 * r2.standard_normal(n)
        for _ in range(3):
            base[d] += r2.uniform(0.3, 1.0) * np.sin(2 * np.pi * t / r2.uniform(2.5, max(3.0, hi)) + r2.uniform(0, 6.3))
    return base.astype(dtype)


def _fuzz_draws(seed=2026):
    """Endless seeded draws: (trial index, params, find_periods keywords, distinct windows)."""
    rng = np.random.default_rng(seed)
    i = 0
    while True:
        trunc, uw = VARIANTS[i % 4]
        dtype = (np.float64, np.float32)[(i // 4) % 2]
        n = int(rng.integers(8, 6001)) if i % 5 else int(rng.integers(8, 200))
        w = (1, 3, 7, 257)[i % 4 if i % 3 else 0]
        hi = n - 1 if (trunc and n <= 400 and rng.random() < 0.5) else min(n // 3, 300)
        num = int(rng.integers(1, 25))
        if uw:  # the re-solved dictionary grows with every block: keep the oracle's dense solves small
            hi = min(hi, 600 // num)
        hi = max(hi, 2)
        params = dict(n=n, dtype=dtype.__name__, trunc=trunc, uw=uw, w=w, num=num,
                      thresh=float(rng.choice([0.02, 0.05, 0.1, 0.2])), min_length=2, max_length=hi, seed=int(rng.integers(1 << 30)))
        kw = dict(num=num, thresh=params["thresh"], min_length=2, max_length=hi)
        accepted = yield params, kw, _fuzz_windows(params["seed"], n, hi, min(w, 2), dtype)
        i += bool(accepted)


def _well_posed(x, kw, trunc, uw):
    """-> (oracle result, whether the reference's answer is determined by the input).  Not determined: a near-tie
    selection (best and second-best gamma norm closer than MARGIN relative) or one at rounding level; a re-solved
    dictionary (update_weights=True) that takes a period again or a divisor of an earlier one -- its block then keeps
    0 rows, Pp hands it all p rows (QOPeriods.py:970-974), the Gram matrix is singular, and whether
    numpy.linalg.solve raises (:552-559) depends on rounding (only trunc selection reaches such periods above
    rounding level); a re-solved dictionary that is rank-deficient (at least as many rows as samples, or a Gram
    condition number of 1e12 or more), whose weights are not unique; non-finite outputs."""
    trace = []
    want = _oracle(x, kw, trunc, uw, trace)
    ok = all(b - s >= MARGIN[x.dtype.type] * b and b >= 1e-6 * trace[0][0] for b, s, _ in trace)
    picked = [p for _, _, p in trace]
    ok &= all(np.all(np.isfinite(want[k])) for k in ("norms", "weights", "residual"))
    if uw and ok:
        ok &= all(all(q % p for q in picked[:i]) for i, p in enumerate(picked))
        ok &= len(want["weights"]) < x.size and _gram_cond(want) < 1e12
    return want, ok


def _fuzz_trials(count=30, seed=2026):
    """Seeded trials: (params, keywords, batch, oracle results of its distinct windows); a draw that is not well posed
    (_well_posed) is replaced by the next one."""
    trials = []
    draws = _fuzz_draws(seed)
    params, kw, base = next(draws)
    while len(trials) < count:
        wants = [_well_posed(b, kw, params["trunc"], params["uw"]) for b in base]
        ok = all(o for _, o in wants)
        if ok:
            trials.append((params, kw, base[np.arange(params["w"]) % len(base)], [w for w, _ in wants]))
        params, kw, base = draws.send(ok)
    return trials


# Well-posed fuzz draws whose re-solved dictionary has a Gram condition number of 1e7 - 1e8 (nearly as many rows as
# samples).  k_qo_find's conjugate-gradient solve need not converge there; it used to end the loop as if the
# dictionary were singular, with status OK and one period short, where numpy.linalg.solve goes on.
ILL_CONDITIONED = [
    dict(n=365, dtype=np.float32, seed=13806051, window=1, num=12, thresh=0.05, max_length=50),  # 330 rows
    dict(n=424, dtype=np.float64, seed=984903968, window=1, num=14, thresh=0.2, max_length=42),  # 342 rows
]


@pytest.mark.parametrize("case", ILL_CONDITIONED, ids=["n365_f32", "n424_f64"])
def test_ill_conditioned_dictionary(eng, case):
    """Trunc selection, re-solved weights, Gram condition 1e7 - 1e8: the kernel either converges to the reference's
    answer or hands the window back with PH_ST_ITER_CAP -- never a silent short answer -- and the class (batch and
    1-D call) returns the oracle's answer."""
    from pyperiod_amd import _ffi

    x = _fuzz_windows(case["seed"], case["n"], case["max_length"], 2, case["dtype"])[case["window"]]
    kw = dict(num=case["num"], thresh=case["thresh"], min_length=2, max_length=case["max_length"])
    want, ok = _well_posed(x, kw, True, True)
    assert ok and 1e6 <= _gram_cond(want) < 1e12, case
    tol = F32_TOL if x.dtype == np.float32 else F64_TOL
    per, nrm, keeps, counts, wts, res, st = eng.qo_find_periods(x[None, :], kcap=2048, trunc=True, **kw)
    assert st[0] in (_ffi.PH_ST_OK, _ffi.PH_ST_ITER_CAP), (case, st)
    if st[0] == _ffi.PH_ST_OK:
        nr = len(want["periods"])
        assert int(counts[0, 0]) == nr and np.array_equal(per[0, :nr], want["periods"]), (case, counts, per[0])
        assert rel_err(wts[0, : len(want["weights"])], want["weights"]) <= tol["weights"], case
    for got in _qo(True).find_periods(np.vstack([x, x]), **kw):
        _check(got, want, tol, (case, "batch"))
    _check(_qo(True).find_periods(x, **kw), want, tol, (case, "1-D"))


def test_seeded_fuzz(eng):
    """About 30 seeded trials over N in [8, 6000], the four variants, fp64 and fp32, num <= 24, max_length up to
    N - 1 for trunc, W in {1, 3, 7, 257} (rows repeat two distinct windows): every row against the oracle."""
    for params, kw, x, wants in _fuzz_trials():
        tol = F32_TOL if x.dtype == np.float32 else F64_TOL
        got = _qo(params["trunc"]).find_periods(x, update_weights=params["uw"], **kw)
        assert len(got) == x.shape[0], params
        for w, r in enumerate(got):
            _check(r, wants[w % len(wants)], tol, (params, w))
