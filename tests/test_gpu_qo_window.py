"""QOPeriods under an analysis window on the device: ph_qo_fit_win (k_qo_fit_win) against the reference fixture
tests/golden/qo_window.npz and numpy solves of the oracle's dictionary rows, its reduction to ph_qo_fit, the shapes at
which its folds change path, both placements of its staging vector u (a default engine and one created under
PH_HBM_WINDOW=1), and the class surface: compute_reconstruction(x(W, N), lists, window=win) and find_periods with
``window`` set.

Bars: 1e-8 on weights and residual against the reference (the project's bar for the fit, tests/test_gpu_ram_fit.py) on
rows with cond <= 1e7 -- every non-singular row of the fixture; 1e-4 for float32 input against the windowed solve of the
rounded input; 1e-12 between two runs of the same arithmetic in another order (the two placements of u, ones(N) against
ph_qo_fit, a scaled window)."""

import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window
from test_qo_window_cpu import fit_case, windowed_solve

pytestmark = pytest.mark.gpu
TOL, TOL32, TOL_SAME = 1e-8, 1e-4, 1e-12


@pytest.fixture(scope="module")
def engines():
    """(default engine, engine whose staging vector always lives in HBM); PH_HBM_WINDOW is read when the context is
    created and restored right after."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import PeriodEngine, default_engine

    old = os.environ.get("PH_HBM_WINDOW")
    os.environ["PH_HBM_WINDOW"] = "1"
    try:
        hbm = PeriodEngine(0)
    finally:
        if old is None:
            del os.environ["PH_HBM_WINDOW"]
        else:
            os.environ["PH_HBM_WINDOW"] = old
    yield default_engine(), hbm
    hbm.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _pack(lists, pcap=None):
    pcap = max(1, max(len(p) for p in lists)) if pcap is None else pcap
    per = np.zeros((len(lists), pcap), dtype=np.int32)
    for w, p in enumerate(lists):
        per[w, : len(p)] = p
    return per, np.array([len(p) for p in lists], dtype=np.int32)


def _solve(x, win, lst):
    rows, dims = po.qo_get_subspaces(lst, x.size)
    w, recon = windowed_solve(x.astype(np.float64), win, rows)
    return list(dims.values()), w, x.astype(np.float64) - recon


def _check_rows(got, xs, win, lists, tol, what):
    keeps, wts, resid, st = got
    for w, lst in enumerate(lists):
        dims, want_w, want_r = _solve(xs[w], win, lst)
        k = sum(dims)
        print(f"{what} row {w} {lst}: status {st[w]} weights {rel_err(wts[w, :k], want_w):.2e} residual {rel_err(resid[w], want_r):.2e}")
        assert st[w] == 0 and list(keeps[w, : len(lst)]) == dims, (what, w)
        assert rel_err(wts[w, :k], want_w) <= tol and not wts[w, k:].any(), (what, w)
        assert rel_err(resid[w], want_r) <= tol, (what, w)


# ---------------------------------------------------------------------------- 1. the engine against the fixture
def test_engine_against_reference_fixture(engines, golden):
    from pyperiod_amd import _ffi

    g = golden("qo_window")
    groups = {}
    for k in range(int(g["fit_count"])):
        groups.setdefault(tuple(int(v) for v in g[f"fit{k}_case"][[0, 2]]), []).append(k)
    seen = 0
    for (n, code), ks in groups.items():
        cases = [fit_case(g, k) for k in ks]
        xs = np.stack([c[0] for c in cases])
        win = cases[0][1]
        per, cnt = _pack([c[2] for c in cases])
        for name, eng in zip(("lds", "hbm"), engines):
            keeps, wts, resid, st = eng.qo_fit(xs, per, cnt, kcap=512, window=win)
            r32 = eng.qo_fit(xs.astype(np.float32), per, cnt, kcap=512, window=win)
            for w, (x, _, lst, want) in enumerate(cases):
                if want is None:  # [128, 64]: the second block has no rows
                    assert st[w] == _ffi.PH_ST_ITER_CAP and not wts[w].any()
                    assert r32[3][w] == _ffi.PH_ST_ITER_CAP and not r32[1][w].any()
                    continue
                assert float(want["cond"]) <= 1e7  # (the fixture holds no other non-singular row: none is skipped)
                k = want["weights"].size
                ew, er = rel_err(wts[w, :k], want["weights"]), rel_err(resid[w], x - want["recon"])
                print(f"N={n} window {code} {lst} u in {name}: status {st[w]} weights {ew:.2e} residual {er:.2e}")
                assert st[w] == _ffi.PH_ST_OK and list(keeps[w, : len(lst)]) == list(want["dict_vals"])
                assert ew <= TOL and er <= TOL and not wts[w, k:].any()
                seen += name == "lds"
            ok = [w for w, c in enumerate(cases) if c[3] is not None]
            _check_rows(tuple(a[ok] for a in r32), xs.astype(np.float32)[ok], win, [cases[w][2] for w in ok], TOL32, f"float32 N={n}")
    assert seen == 25


# ---------------------------------------------------------------------------- 2. reduction to the unwindowed kernel
@pytest.mark.parametrize("n", [36, 600, 4097])
def test_ones_window_is_the_unwindowed_fit(engines, n):
    lists = {36: [[2, 3], [4, 6], [5, 7, 12]], 600: [[7, 12], [5, 6, 10, 30], [64, 96], [3, 9, 27], [13, 17, 19, 23]],
             4097: [[7, 12, 100], [64, 96], [4, 6, 9, 100], [1000, 37]]}[n]
    xs = np.stack([multi_sinusoid_window(40 + w, n) for w in range(len(lists))])
    per, cnt = _pack(lists)
    plain = engines[0].qo_fit(xs, per, cnt, kcap=1280)
    assert not plain[3].any()
    for eng in engines:
        got = eng.qo_fit(xs, per, cnt, kcap=1280, window=np.ones(n))
        assert not got[3].any() and np.array_equal(got[0], plain[0])
        assert rel_err(got[1], plain[1]) <= TOL_SAME and rel_err(got[2], plain[2]) <= TOL_SAME


def test_scaled_window_gives_the_same_fit(engines):
    n, lists = 600, [[7, 12], [5, 6, 10, 30], [64, 96]]
    xs = np.stack([multi_sinusoid_window(50 + w, n) for w in range(len(lists))])
    per, cnt = _pack(lists)
    for eng in engines:
        one = eng.qo_fit(xs, per, cnt, kcap=256, window=np.hanning(n))
        three = eng.qo_fit(xs, per, cnt, kcap=256, window=3.0 * np.hanning(n))
        assert not one[3].any() and not three[3].any()
        assert rel_err(three[1], one[1]) <= TOL_SAME and rel_err(three[2], one[2]) <= TOL_SAME


# ---------------------------------------------------------------------------- 3. shapes
def test_shapes(engines):
    """W = 5: a shared list and per-row lists of different lengths (one empty); N = 601 is a multiple of no period;
    [64, 96] at N = 600 has at most 10 samples per residue; periods below and above 64 in one list; keep < p blocks
    ([5, 6, 10, 30]: 5, 5, 4 and 16 rows); a single block."""
    from pyperiod_amd import _ffi

    for eng in engines:
        for n in (600, 601):
            win = np.hanning(n)
            xs = np.stack([multi_sinusoid_window(60 + w, n) for w in range(5)])
            shared = [5, 6, 10, 30]
            _check_rows(eng.qo_fit(xs, shared, kcap=64, window=win), xs, win, [shared] * 5, TOL, f"shared N={n}")
            lists = [[7, 12], [64, 96], [4, 6, 9, 100], [], [13]]
            per, cnt = _pack(lists)
            keeps, wts, resid, st = eng.qo_fit(xs, per, cnt, kcap=256, window=win)
            assert st[3] == _ffi.PH_ST_NO_PERIOD and not wts[3].any() and not keeps[3].any()
            ok = [0, 1, 2, 4]
            _check_rows((keeps[ok], wts[ok], resid[ok], st[ok]), xs[ok], win, [lists[w] for w in ok], TOL, f"per-row N={n}")


def test_capacity_and_singular_window(engines):
    from pyperiod_amd import _ffi

    n, lst = 600, [5, 6, 10, 30]
    xs = np.stack([multi_sinusoid_window(70 + w, n) for w in range(5)])
    win = np.hanning(n)
    rows = sum(po.qo_get_subspaces(lst, n)[1].values())
    assert rows == 30
    first3 = np.zeros(n)
    first3[:3] = 1.0
    for eng in engines:
        _check_rows(eng.qo_fit(xs, lst, kcap=rows, window=win), xs, win, [lst] * 5, TOL, "kcap == rows")
        keeps, wts, _, st = eng.qo_fit(xs, lst, kcap=rows - 1, window=win)
        assert np.all(st == _ffi.PH_ST_CAP) and not wts.any() and list(keeps[0]) == [5, 5, 4, 16]
        keeps, wts, _, st = eng.qo_fit(xs, lst, kcap=64, window=first3)  # most residues never meet the window
        assert np.all(st == _ffi.PH_ST_ITER_CAP) and not wts.any()
        with pytest.raises(ValueError):
            eng.qo_fit(xs, lst, kcap=64, window=np.ones(n - 1))


def test_indefinite_window_ends_on_the_curvature_test(engines):
    """A window with a negative sample whose folds are all positive (diagonal 1, 3, 3, 3) but whose matrix is indefinite
    (eigenvalues -1.17, 2.62, 3, 5.55): the diagonal test passes and the solve meets non-positive curvature.  x is
    chosen so that the first preconditioned residual z = (1, 0, -1, -1) has z^T G z = -1: the solver's curvature test
    ends the window in its first iteration on either placement, fp64 and fp32 (every number here is exact in fp32 but
    x[2] = -4/3, which moves z^T G z by 1e-7).  The reference's LU solve has no such limit (cond 4.7): the class hands
    the row to the 1-D call and returns its answer, held to the windowed solve of the oracle's rows at the 1e-8 bar."""
    from pyperiod_amd import QOPeriods, _ffi

    win = np.array([2.0, 1.0, -3.0, 1.0, 2.0, 1.0])
    x = np.array([[-1.5, -3.0, -4.0 / 3.0, 0.0, 0.0, 3.0]])
    rows, _ = po.qo_get_subspaces([2, 3], 6)
    g = rows @ np.diag(win) @ rows.T
    z = (rows @ (win * x[0])) / np.diag(g)
    assert np.all(np.diag(g) > 0) and np.linalg.eigvalsh(g)[0] < -1 and abs(z @ g @ z + 1.0) < 1e-12
    for eng in engines:
        for xs in (x, x.astype(np.float32)):
            keeps, wts, _, st = eng.qo_fit(xs, [2, 3], kcap=64, window=win)
            assert st[0] == _ffi.PH_ST_ITER_CAP and list(keeps[0]) == [2, 2] and not wts.any()
    recon, bases = QOPeriods().compute_reconstruction(x, [2, 3], type="solve", window=win)[0]
    _, want_w, want_r = _solve(x[0], win, [2, 3])
    assert rel_err(bases["weights"], want_w) <= TOL and rel_err(x[0] - recon, want_r) <= TOL


def test_device_tensors_give_the_same_bits(engines):
    import torch

    n, lists = 600, [[7, 12], [64, 96], [4, 6, 9, 100], [], [13]]
    xs = np.stack([multi_sinusoid_window(80 + w, n) for w in range(5)])
    win = np.hanning(n)
    per, cnt = _pack(lists)
    for eng in engines:
        host = eng.qo_fit(xs, per, cnt, kcap=256, window=win)
        dev = eng.qo_fit(torch.as_tensor(xs, device="cuda"), torch.as_tensor(per, device="cuda"), torch.as_tensor(cnt, device="cuda"),
                         kcap=256, max_period=100, window=torch.as_tensor(win, device="cuda"))
        st = dev[3].cpu().numpy()
        assert np.array_equal(st, host[3])
        ok = st == 0
        assert np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(dev[1].cpu().numpy(), host[1])
        assert np.array_equal(dev[2].cpu().numpy()[ok], host[2][ok])


# ---------------------------------------------------------------------------- 4. plan
def test_plan_and_both_placements_at_the_switch(engines):
    from pyperiod_amd import _ffi

    eng, hbm = engines
    kcap, mp = 512, 100

    def where(e, n):
        (k,) = e.plan_info("qo_fit_win", n, (kcap, mp))
        assert k.window == _ffi.PH_PLAN_HBM and k.block in (256, 512, 1024)
        return k

    lo, hi = 1, 1 << 20
    assert where(eng, lo).second == _ffi.PH_PLAN_LDS and where(eng, hi).second == _ffi.PH_PLAN_HBM
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if where(eng, mid).second == _ffi.PH_PLAN_LDS else (lo, mid)
    n_star = lo
    lds_limit = eng.lds_bytes
    solver = eng.plan_info("qo_fit", n_star, (kcap, mp))[0].lds_bytes
    assert where(eng, n_star).lds_bytes <= lds_limit < where(eng, n_star).lds_bytes + 16
    assert where(eng, n_star + 1).lds_bytes == solver == where(hbm, 64).lds_bytes
    for n in (1, 64, n_star, n_star + 1):
        assert where(hbm, n).second == _ffi.PH_PLAN_HBM
    assert eng.qo_fit_feasible(kcap, mp, n_star, window=True) and eng.qo_fit_feasible(kcap, mp, 1 << 20, window=True)
    # a kcap whose vectors do not fit the LDS
    big = 4096
    assert not eng.qo_fit_feasible(big, mp) and not eng.qo_fit_feasible(big, mp, 600, window=True)
    with pytest.raises(ValueError):
        eng.plan_info("qo_fit_win", 600, (big, mp))
    with pytest.raises(ValueError):
        eng.qo_fit(np.zeros((1, 600)), [7, 12], kcap=big, window=np.hanning(600))
    lst = [7, 12, 100]
    for n in (n_star, n_star + 1):
        xs = np.stack([multi_sinusoid_window(90 + w, n) for w in range(2)])
        win = np.hanning(n)
        a = eng.qo_fit(xs, lst, kcap=kcap, max_period=mp, window=win)
        b = hbm.qo_fit(xs, lst, kcap=kcap, max_period=mp, window=win)
        assert not a[3].any() and not b[3].any()
        assert rel_err(a[1], b[1]) <= TOL_SAME and rel_err(a[2], b[2]) <= TOL_SAME
        _check_rows(a, xs, win, [lst] * 2, TOL, f"N={n}")


# ---------------------------------------------------------------------------- 5. class surface
def _names(eng):
    return [name for name, _ in eng.profile_read()]


def test_compute_reconstruction_batch(engines, golden, monkeypatch):
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    g = golden("qo_window")
    ks = [k for k in range(int(g["fit_count"])) if tuple(g[f"fit{k}_case"][[0, 2]]) == (600, 0)]
    cases = [fit_case(g, k) for k in ks]
    xs = np.stack([c[0] for c in cases])
    win = cases[0][1]
    lists = [c[2] for c in cases]
    qo = QOPeriods()
    rows_1d = [qo.compute_reconstruction(xs[w], lists[w], "solve", win) for w in range(len(cases))]
    dense = []
    monkeypatch.setattr(QOPeriods, "solve_quadratic", staticmethod(lambda *a, **k: dense.append(1)))
    eng.profile(True)
    try:
        batch = qo.compute_reconstruction(xs, lists, type="solve", window=win)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert names.count("k_qo_fit_win") == 1 and "k_fold_sums" not in names and "k_qo_fit" not in names and not dense
    for w, (x, _, lst, want) in enumerate(cases):
        recon, bases = batch[w]
        assert rel_err(recon, want["recon"]) <= TOL and rel_err(bases["weights"], want["weights"]) <= TOL
        assert list(bases["basis_dictionary"].values()) == list(want["dict_vals"])
        assert np.array_equal(bases["subspaces"], rows_1d[w][1]["subspaces"]) and list(bases["periods"]) == lst
        assert rel_err(recon, rows_1d[w][0]) <= TOL and rel_err(bases["weights"], rows_1d[w][1]["weights"]) <= TOL


def test_compute_reconstruction_shared_list_and_fallback_row(engines):
    """One list for every row; a list whose second block has no rows goes to the 1-D call and is None as there."""
    from pyperiod_amd import QOPeriods

    n = 1024
    xs = np.stack([multi_sinusoid_window(100 + w, n) for w in range(3)])
    win = np.hanning(n)
    qo = QOPeriods()
    batch = qo.compute_reconstruction(xs, [4, 6, 9, 100], type="solve", window=win)
    for w in range(3):
        _, want_w, want_r = _solve(xs[w], win, [4, 6, 9, 100])
        assert rel_err(batch[w][1]["weights"], want_w) <= TOL and rel_err(xs[w] - batch[w][0], want_r) <= TOL
    mixed = qo.compute_reconstruction(xs, [[4, 6, 9, 100], [128, 64], [7]], type="solve", window=win)
    assert mixed[1] is None and qo.compute_reconstruction(xs[1], [128, 64], "solve", win) is None
    assert rel_err(mixed[0][0], batch[0][0]) <= TOL_SAME and mixed[2][1]["weights"].size == 7


def test_unwindowed_batches_launch_what_they_did(engines):
    """window=None stays one k_qo_fit launch; window=False stays the 1-D call per row (no fit kernel at all)."""
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    n = 600
    xs = np.stack([multi_sinusoid_window(110 + w, n) for w in range(3)])
    qo = QOPeriods()
    eng.profile(True)
    try:
        a = qo.compute_reconstruction(xs, [7, 12], type="solve", window=None)
        names_none = _names(eng)
        eng.profile(False)
        eng.profile(True)
        b = qo.compute_reconstruction(xs, [7, 12], type="solve", window=False)
        names_false = _names(eng)
    finally:
        eng.profile(False)
    assert names_none == ["k_qo_fit"] and "k_qo_fit" not in names_false and "k_qo_fit_win" not in names_false
    for w in range(3):
        assert rel_err(a[w][0], b[w][0]) <= TOL


def test_find_periods_batch_against_reference_fixture(engines, golden):
    from pyperiod_amd import QOPeriods

    eng = engines[0]
    g = golden("qo_window")
    n, num, thresh, lo, hi = g["fp_kw"]
    n, kw = int(n), dict(num=int(num), thresh=float(thresh), min_length=int(lo), max_length=int(hi))
    seeds = [int(g[f"fp{w}_seed"]) for w in range(8)]
    # + the first seed the generator replaced (its run reaches a block without rows: the 1-D call) + an all-zero row
    forced = next(s for s in range(max(seeds)) if s not in seeds)
    xs = np.stack([multi_sinusoid_window(s, n) for s in seeds + [forced]] + [np.zeros(n)])
    qo = QOPeriods()
    qo.window = np.hanning(n)
    eng.profile(True)
    try:
        batch = qo.find_periods(xs[:8], **kw)
        names = _names(eng)
    finally:
        eng.profile(False)
    assert len(batch) == 8 and isinstance(qo._output_bases, list)
    # four rounds: one sweep and one fit each, nothing from the host-driven loop
    assert names.count("k_qo_fit_win") == 4 and names.count("k_sweep") == 4 and len(names) == 8
    for w in range(8):
        bases, res = batch[w]
        want = {k: g[f"fp{w}_{k}"] for k in ("periods", "norms", "weights", "dict_keys", "dict_vals", "residual")}
        assert np.array_equal(bases["periods"], want["periods"]) and len(bases["periods"]) == want["periods"].size
        assert [int(q) for q in bases["basis_dictionary"]] == list(want["dict_keys"])
        assert list(bases["basis_dictionary"].values()) == list(want["dict_vals"])
        assert np.array_equal(bases["subspaces"], po.qo_get_subspaces(list(want["dict_keys"]), n)[0])
        ew, er = rel_err(bases["weights"], want["weights"]), rel_err(res, want["residual"])
        print(f"find_periods row {w}: weights {ew:.2e} residual {er:.2e} norms {rel_err(bases['norms'], want['norms']):.2e}")
        assert ew <= TOL and er <= TOL and rel_err(bases["norms"], want["norms"]) <= TOL
    tail = qo.find_periods(xs[7:], **kw)
    for w, got in zip((7, 8, 9), tail):
        one = qo.find_periods(xs[w], **kw)
        assert np.array_equal(got[0]["periods"], one[0]["periods"]) and got[0]["basis_dictionary"] == one[0]["basis_dictionary"]
        assert rel_err(got[0]["weights"], one[0]["weights"]) <= TOL and rel_err(got[1], one[1]) <= TOL
    assert list(tail[2][0]["periods"]) == [1] and not tail[2][1].any()
    assert rel_err(tail[0][0]["weights"], batch[7][0]["weights"]) <= TOL_SAME


def test_find_periods_rows_the_test_function_stops(engines):
    """thresh = 0.6: the reconstruction of some rows falls below it after a round; those rows report one period fewer
    than their dictionary holds (QOPeriods.py:560-594), exactly as the 1-D call does."""
    from pyperiod_amd import QOPeriods

    n, kw = 600, dict(num=4, thresh=0.6, min_length=2, max_length=100)
    xs = np.stack([multi_sinusoid_window(s, n) for s in (0, 1, 3, 4, 6)])
    qo = QOPeriods()
    qo.window = np.hanning(n)
    batch = qo.find_periods(xs, **kw)
    short = [len(b["periods"]) < len(b["basis_dictionary"]) for b, _ in batch]
    assert any(short) and not all(short)
    for w in range(xs.shape[0]):
        one = qo.find_periods(xs[w], **kw)
        assert np.array_equal(batch[w][0]["periods"], one[0]["periods"]) and batch[w][0]["basis_dictionary"] == one[0]["basis_dictionary"]
        assert rel_err(batch[w][0]["norms"], one[0]["norms"]) <= TOL
        assert rel_err(batch[w][0]["weights"], one[0]["weights"]) <= TOL and rel_err(batch[w][1], one[1]) <= TOL
