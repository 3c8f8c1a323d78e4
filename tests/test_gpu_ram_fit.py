"""GPU tests of the batched fit: RamanujanPeriods.find_periods_with_weights and QOPeriods.compute_reconstruction on
(W, N) batches, the engine entry points ph_ramanujan_fit / ph_qo_fit behind them, and the PH_OP_QO_FIT plan.

Value bars.  Weights and residuals are compared at 1e-8 (the bar test_gpu_configs.py holds the 1-D path to) on rows
whose dictionary has cond(A A^T) <= 1e7, taken from the fixture / the oracle's dictionary, never from the code under
test; above that cut the reference's own weights are LAPACK rounding noise (windows 1 and 25 of batch A: cond 8e16 and
1e14).  Periods, dictionaries and finiteness are held on every row.  float32 batches are compared against the fp64
oracle on the rounded input at 1e-4 (the project's fp32 bar) on rows with cond <= 1e5: the fp32 kernel stops at a
relative residual of 1e-9, which bounds the weight error by cond x 1e-9."""

import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch, multi_sinusoid_window

pytestmark = pytest.mark.gpu
COND_CUT = 1e7
COND_CUT_F32 = 1e5


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _batch(g, tag, dtype=np.float64):
    n, lo, hi, thresh = g[f"{tag}_kw"]
    x = np.stack([multi_sinusoid_window(int(s), int(n)) for s in g[f"{tag}_seeds"]]).astype(dtype)
    return x, dict(min_length=int(lo), max_length=int(hi), thresh=float(thresh))


def _oracle_fit(sig, periods):
    a, dims = po.qo_get_subspaces(periods, len(sig))
    w, recon = po.qo_solve_quadratic(sig, a)
    return a, dims, w, recon


@pytest.mark.parametrize("tag", ["A", "B"])
def test_batch_against_reference_fixture(eng, golden, tag):
    """1. The class surface on batch A / B against the reference's answers, row by row."""
    from pyperiod_amd import RamanujanPeriods

    g = golden("ramanujan_fit")
    x, kw = _batch(g, tag)
    ram = RamanujanPeriods()
    got = ram.find_periods_with_weights(x, **kw)
    assert isinstance(got, list) and len(got) == x.shape[0]
    assert isinstance(ram._output, list) and all(ram._output[w] is got[w][0] for w in range(len(got)))
    worst = {}
    for w, (out, res) in enumerate(got):
        key = f"{tag}{w}"
        assert set(out.keys()) == {"periods", "norms", "subspaces", "weights", "basis_dictionary"}
        assert np.array_equal(out["periods"], g[f"{key}_periods"]), key
        assert [int(k) for k in out["basis_dictionary"]] == list(g[f"{key}_dict_keys"]), key
        assert list(out["basis_dictionary"].values()) == list(g[f"{key}_dict_vals"]), key
        assert res.dtype == np.float64 and res.shape == (x.shape[1],)
        assert np.all(np.isfinite(out["weights"])) and np.all(np.isfinite(res)), key
        assert out["weights"].shape == (int(g[f"{key}_dict_vals"].sum()),), key
        assert rel_err(out["norms"], g[f"{key}_norms"][g[f"{key}_periods"]]) < 1e-5, key
        if g[f"{tag}_cond"][w] <= COND_CUT:
            ew, er = rel_err(out["weights"], g[f"{key}_weights"]), rel_err(res, g[f"{key}_residual"])
            worst[key] = (ew, er)
            print(f"{key}: cond {g[f'{tag}_cond'][w]:.2e} weights {ew:.2e} residual {er:.2e}")
            assert ew < 1e-8 and er < 1e-8, (key, ew, er, g[f"{tag}_cond"][w])
    assert len(worst) >= (28 if tag == "A" else 5)
    # "subspaces" is built on first read and is the 1-D array
    out0 = got[0][0]
    assert out0["subspaces"].shape == (int(g[f"{tag}0_dict_vals"].sum()), x.shape[1])
    a0, _ = po.qo_get_subspaces(g[f"{tag}0_periods"], x.shape[1])
    assert np.array_equal(out0["subspaces"], a0)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_engine_solves_on_the_device(eng, golden, tag):
    """2. Through the engine: every well-conditioned row that fits comes back PH_ST_OK -- the class surface may not pass
    by handing everything to the host -- with the reference's weights."""
    from pyperiod_amd import _ffi

    g = golden("ramanujan_fit")
    x, kw = _batch(g, tag)
    kcap = 1024
    norms, per, counts, keeps, wts, resid, st = eng.ramanujan_fit(x, kw["min_length"], kw["max_length"], kw["thresh"], 64, kcap)
    hard = {w: int(st[w]) for w in range(x.shape[0]) if g[f"{tag}_cond"][w] > COND_CUT}
    for w in range(x.shape[0]):
        key = f"{tag}{w}"
        n = int(counts[w])
        assert list(per[w, :n]) == list(g[f"{key}_periods"]) and not per[w, n:].any(), key
        assert rel_err(norms[w], g[f"{key}_norms"]) < 1e-5, key
        if g[f"{tag}_cond"][w] <= COND_CUT and g[f"{tag}_rows"][w] <= kcap:
            assert st[w] == _ffi.PH_ST_OK, f"{key}: status {st[w]}; ill-conditioned rows came back as {hard}"
            assert list(keeps[w, :n]) == list(g[f"{key}_dict_vals"]) and not keeps[w, n:].any(), key
            k = int(keeps[w].sum())
            assert rel_err(wts[w, :k], g[f"{key}_weights"]) < 1e-8 and not wts[w, k:].any(), key
            assert rel_err(resid[w], g[f"{key}_residual"]) < 1e-8, key
        else:
            assert st[w] in (_ffi.PH_ST_OK, _ffi.PH_ST_ITER_CAP, _ffi.PH_ST_CAP), f"{key}: status {st[w]}; {hard}"
            if st[w] != _ffi.PH_ST_OK:
                assert not wts[w].any(), key
    print(f"batch {tag}: statuses of the rows above the cond cut: {hard}")


def test_engine_device_tensors_equal_host_arrays(eng, golden):
    """The torch path (device pointers on torch's stream) gives the bits of the numpy path."""
    import torch

    g = golden("ramanujan_fit")
    x, kw = _batch(g, "B")
    host = eng.ramanujan_fit(x, kw["min_length"], kw["max_length"], kw["thresh"], 64, 512)
    dev = eng.ramanujan_fit(torch.from_numpy(x).to(f"cuda:{eng.device}"), kw["min_length"], kw["max_length"], kw["thresh"], 64, 512)
    torch.cuda.synchronize()
    ok = host[6] == 0
    assert np.array_equal(dev[6].cpu().numpy(), host[6])
    for h, d in zip(host[:5], dev[:5]):
        assert np.array_equal(d.cpu().numpy(), h)
    assert np.array_equal(dev[5].cpu().numpy()[ok], host[5][ok])
    lists = torch.tensor([7, 12], dtype=torch.int32, device=f"cuda:{eng.device}")
    xt = torch.from_numpy(x).to(f"cuda:{eng.device}")
    kd, wd, rd, sd = eng.qo_fit(xt, lists, kcap=64, max_period=12)
    kh, wh, rh, sh = eng.qo_fit(x, [7, 12], kcap=64)
    torch.cuda.synchronize()
    assert not sh.any() and np.array_equal(sd.cpu().numpy(), sh)
    assert np.array_equal(kd.cpu().numpy(), kh) and np.array_equal(wd.cpu().numpy(), wh) and np.array_equal(rd.cpu().numpy(), rh)


def test_batch_rows_equal_one_dimensional_calls(eng, golden):
    """3. Each row of the batch result is what the 1-D call on that row returns."""
    from pyperiod_amd import RamanujanPeriods

    g = golden("ramanujan_fit")
    for tag in ("A", "B"):
        x, kw = _batch(g, tag)
        got = RamanujanPeriods().find_periods_with_weights(x, **kw)
        for w in range(x.shape[0]):
            out1, res1 = RamanujanPeriods().find_periods_with_weights(x[w], **kw)
            out, res = got[w]
            assert np.array_equal(out["periods"], out1["periods"]) and out["periods"].dtype == out1["periods"].dtype
            assert np.array_equal(out["norms"], out1["norms"])
            assert out["basis_dictionary"] == out1["basis_dictionary"]
            assert list(out["basis_dictionary"]) == list(out1["basis_dictionary"])
            if g[f"{tag}_cond"][w] <= COND_CUT:
                assert rel_err(out["weights"], out1["weights"]) < 1e-8 and rel_err(res, res1) < 1e-8, (tag, w)
        assert np.array_equal(got[3][0]["subspaces"], RamanujanPeriods().find_periods_with_weights(x[3], **kw)[0]["subspaces"])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_float32_batch_against_oracle(eng, golden, tag):
    """3. float32 batches run the float kernels and return float64 residuals; against the fp64 oracle on the rounded input."""
    from pyperiod_amd import RamanujanPeriods, _ffi

    g = golden("ramanujan_fit")
    x32, kw = _batch(g, tag, np.float32)
    got = RamanujanPeriods().find_periods_with_weights(x32, **kw)
    st = eng.ramanujan_fit(x32, kw["min_length"], kw["max_length"], kw["thresh"], 64, 1024)[6]
    compared = 0
    for w in range(x32.shape[0]):
        out, res = got[w]
        want, wres = po.ramanujan_find_periods_with_weights(x32[w].astype(np.float64), **kw)
        assert np.array_equal(out["periods"], want["periods"]), (tag, w)
        assert list(out["basis_dictionary"].values()) == list(want["basis_dictionary"].values())
        assert res.dtype == np.float64 and np.all(np.isfinite(res)) and np.all(np.isfinite(out["weights"]))
        if g[f"{tag}_cond"][w] <= COND_CUT_F32:
            compared += 1
            assert st[w] == _ffi.PH_ST_OK, (tag, w, st[w])  # (the fp32 kernel itself answered)
            ew, er = rel_err(out["weights"], want["weights"]), rel_err(res, wres)
            print(f"{tag}{w} fp32: weights {ew:.2e} residual {er:.2e}")
            assert ew < 1e-4 and er < 1e-4, (tag, w, ew, er)
    assert compared >= 5


def test_qo_fit_explicit_lists(eng):
    """4. ph_qo_fit with explicit lists: bookkeeping, sharing, statuses, edges."""
    from pyperiod_amd import _ffi

    n = 240
    sig = multi_sinusoid_window(0, n)
    x = sig[None, :]
    keeps, wts, resid, st = eng.qo_fit(x, [7, 12], kcap=64)
    assert st[0] == _ffi.PH_ST_OK and list(keeps[0]) == [7, 11]
    _, dims, w_o, recon = _oracle_fit(sig, [7, 12])
    assert list(dims.values()) == [7, 11]
    assert rel_err(wts[0, :18], w_o) < 1e-8 and not wts[0, 18:].any() and rel_err(resid[0], sig - recon) < 1e-8
    # a shared list (per_stride == 0) equals per-window copies bit for bit
    xb = multi_sinusoid_batch(0, 5, n)
    shared = eng.qo_fit(xb, [7, 12, 30], kcap=64)
    copies = eng.qo_fit(xb, np.tile(np.array([7, 12, 30], dtype=np.int32), (5, 1)), np.full(5, 3, dtype=np.int32), kcap=64)
    assert not shared[3].any()
    for a, b in zip(shared, copies):
        assert np.array_equal(a, b)
    # n_periods selects a prefix per window
    mixed = eng.qo_fit(xb, np.tile(np.array([7, 12, 30], dtype=np.int32), (5, 1)), np.array([3, 2, 1, 0, 3], dtype=np.int32), kcap=64)
    assert list(mixed[3]) == [0, 0, 0, _ffi.PH_ST_NO_PERIOD, 0]
    assert list(mixed[0][1]) == [7, 11, 0] and list(mixed[0][2]) == [7, 0, 0] and list(mixed[0][3]) == [0, 0, 0]
    assert np.array_equal(mixed[1][0], shared[1][0]) and np.array_equal(mixed[2][4], shared[2][4])
    two = eng.qo_fit(xb[1:2], [7, 12], kcap=64)
    assert np.array_equal(mixed[1][1], two[1][0]) and np.array_equal(mixed[2][1], two[2][0])
    # a repeated period / periods whose divisors are all present: the reference's matrix is singular
    for bad, want_keeps in (([7, 7], [7, 0]), ([6, 2, 3], [6, 0, 0]), ([12, 5, 4], [12, 4, 0])):
        keeps, wts, resid, st = eng.qo_fit(x, bad, kcap=64)
        assert st[0] == _ffi.PH_ST_ITER_CAP and list(keeps[0]) == want_keeps and not wts.any(), bad
    # periods outside 1 .. max_period
    for bad in ([0], [7, -3], [7, 13]):
        assert eng.qo_fit(x, bad, kcap=64, max_period=12)[3][0] == _ffi.PH_ST_ITER_CAP, bad
    # more than 64 blocks
    many = [int(p) for p in po.primes_upto(400)[:65]]
    keeps, wts, resid, st = eng.qo_fit(multi_sinusoid_window(1, 4096)[None, :], many, kcap=2048)
    assert st[0] == _ffi.PH_ST_CAP and not wts.any()
    # capacity: sum(keep) == kcap runs, kcap - 1 does not
    exact = eng.qo_fit(x, [7, 12], kcap=18)
    assert exact[3][0] == _ffi.PH_ST_OK and np.array_equal(exact[1][0], eng.qo_fit(x, [7, 12], kcap=64)[1][0, :18])
    keeps, wts, resid, st = eng.qo_fit(x, [7, 12], kcap=17)
    assert st[0] == _ffi.PH_ST_CAP and list(keeps[0]) == [7, 11] and not wts.any()
    # empty list
    assert eng.qo_fit(x, [], kcap=64)[3][0] == _ffi.PH_ST_NO_PERIOD
    # period 1 alone: the mean
    keeps, wts, resid, st = eng.qo_fit(x, [1], kcap=64)
    assert st[0] == _ffi.PH_ST_OK and list(keeps[0]) == [1]
    assert abs(wts[0, 0] - sig.mean()) <= 1e-13 * np.abs(sig).max() and rel_err(resid[0], sig - sig.mean()) < 1e-12
    # N / 2 < p <= N: rows with one or two samples (p = 151), every row one sample (p = N: the fit is the window)
    for p in (151, n):
        keeps, wts, resid, st = eng.qo_fit(x, [p], kcap=256)
        _, dims, w_o, recon = _oracle_fit(sig, [p])
        assert st[0] == _ffi.PH_ST_OK and list(keeps[0]) == list(dims.values()) == [p]
        assert rel_err(wts[0, :p], w_o) < 1e-8 and np.max(np.abs(resid[0] - (sig - recon))) <= 1e-8 * np.abs(sig).max()
    keeps, wts, resid, st = eng.qo_fit(x, [151, 7], kcap=256)
    _, dims, w_o, recon = _oracle_fit(sig, [151, 7])
    assert st[0] == _ffi.PH_ST_OK and list(keeps[0]) == list(dims.values())
    assert rel_err(wts[0, : w_o.size], w_o) < 1e-8 and rel_err(resid[0], sig - recon) < 1e-8
    # a prime period above N keeps more rows than there are samples: handed back, nothing divided by zero
    for p in (241, 251):
        keeps, wts, resid, st = eng.qo_fit(x, [p], kcap=512)
        assert st[0] == _ffi.PH_ST_ITER_CAP and list(keeps[0]) == [p] and not wts.any()
    keeps, wts, resid, st = eng.qo_fit(x, [7, 251], kcap=512)  # 251 keeps phi(251) = 250 > N rows
    assert st[0] == _ffi.PH_ST_ITER_CAP and list(keeps[0]) == [7, 250] and not wts.any() and np.all(np.isfinite(wts))
    # 241 keeps phi(241) = 240 <= N rows, but 7 + 240 rows on 240 samples are rank deficient: singular in the reference
    keeps, wts, resid, st = eng.qo_fit(x, [7, 241], kcap=512)
    assert st[0] == _ffi.PH_ST_ITER_CAP and list(keeps[0]) == [7, 240] and not wts.any()
    assert np.linalg.matrix_rank(po.qo_get_subspaces([7, 241], n)[0]) < 247
    # argument errors
    with pytest.raises(ValueError):
        eng.qo_fit(x, [7, 12], kcap=0)
    with pytest.raises(ValueError):
        eng.qo_fit(x, [7, 12], kcap=64, max_period=(1 << 20) + 1)
    with pytest.raises(ValueError):
        eng.ramanujan_fit(x, 2, 80, 0.0)


def test_qo_fit_pair_table_and_inline_gcd(eng):
    """4b. k_qo_fit's product with 16 blocks (pair constants from the LDS table, kQoPairTab) and with 17 (computed
    inline): the shared product of k_qo_find, whose own 16 / 17-block test is in test_gpu_qo_edges.py.  N = 500 is a
    multiple of no period; cond(A A^T) is about 3e3, so the bar is the 1e-8 of the tests above."""
    from pyperiod_amd import _ffi

    n, lst = 500, [2, 3, 4, 5, 7, 8, 9, 11, 13, 16, 17, 19, 23, 25, 27, 29, 31]
    x = multi_sinusoid_batch(5, 2, n)
    for blocks in (16, 17):
        keeps, wts, resid, st = eng.qo_fit(x, lst[:blocks], kcap=256)
        for w in range(2):
            a, dims, w_o, recon = _oracle_fit(x[w], lst[:blocks])
            assert np.linalg.cond(a @ a.T) <= COND_CUT
            assert st[w] == _ffi.PH_ST_OK and list(keeps[w]) == list(dims.values()), (blocks, w)
            ew, er = rel_err(wts[w, : w_o.size], w_o), rel_err(resid[w], x[w] - recon)
            print(f"{blocks} blocks, window {w}: weights {ew:.2e} residual {er:.2e}")
            assert ew < 1e-8 and er < 1e-8 and not wts[w, w_o.size :].any(), (blocks, w, ew, er)


@pytest.mark.parametrize("n, lanes", [(2048, 4), (4096, 8)])
def test_qo_fit_lane_split_four_and_eight(eng, n, lanes):
    """4b. The lanes-per-row split of the product at 4 and at 8 lanes per row (the fixtures reach 1, 2 and 16): a row
    of block 64 walks min(105, terms) + min(175, terms) steps against blocks 210 and 350, terms = n / 64 samples, and
    the split doubles its lanes while steps / lanes > 24 -- 64 steps give 4 lanes at n = 2048, 128 steps give 8 at
    n = 4096, the smallest windows at which this dictionary gets there.  cond(A A^T) is 519 / 256: the 1e-8 bar."""
    from pyperiod_amd import _ffi

    lst = [210, 350, 64]
    steps = sum(min(p // np.gcd(p, 64), (n - 1) // 64 + 1) for p in lst[:2])
    assert steps // (lanes // 2) > 24 >= steps // lanes  # (the rule of qo_lane_split; all items fit the 1024 threads)
    x = multi_sinusoid_batch(9, 2, n)
    keeps, wts, resid, st = eng.qo_fit(x, lst, kcap=552)
    for w in range(2):
        a, dims, w_o, recon = _oracle_fit(x[w], lst)
        assert np.linalg.cond(a @ a.T) <= COND_CUT
        assert st[w] == _ffi.PH_ST_OK and list(keeps[w]) == list(dims.values()) == [210, 280, 62]
        ew, er = rel_err(wts[w], w_o), rel_err(resid[w], x[w] - recon)
        print(f"n {n}, window {w}: weights {ew:.2e} residual {er:.2e}")
        assert ew < 1e-8 and er < 1e-8, (n, w, ew, er)


def test_qo_fit_non_finite_sample(eng):
    """4c. A NaN sample makes the right-hand side, hence the solver's sums, NaN: no comparison of the solver accepts one,
    so the window is handed back with PH_ST_ITER_CAP and zero weights; its neighbour in the batch is untouched.
    Without a window (k_qo_fit) and under one (k_qo_fit_win: the folds of the window itself stay finite)."""
    from pyperiod_amd import _ffi

    n = 240
    x = multi_sinusoid_batch(0, 2, n)
    clean = eng.qo_fit(x, [7, 12], kcap=64)
    xb = x.copy()
    xb[0, 100] = np.nan
    for window in (None, np.ones(n)):
        keeps, wts, resid, st = eng.qo_fit(xb, [7, 12], kcap=64, window=window)
        assert list(st) == [_ffi.PH_ST_ITER_CAP, _ffi.PH_ST_OK] and list(keeps[0]) == [7, 11] and not wts[0].any()
        if window is None:
            assert np.array_equal(wts[1], clean[1][1]) and np.array_equal(resid[1], clean[2][1])
        else:  # (the same arithmetic in another order: the bar of test_gpu_qo_window.py)
            assert rel_err(wts[1], clean[1][1]) < 1e-12 and rel_err(resid[1], clean[2][1]) < 1e-12


def test_compute_reconstruction_batch(eng):
    """5. QOPeriods.compute_reconstruction on a batch against get_subspaces + solve_quadratic of the oracle."""
    from pyperiod_amd import QOPeriods

    n = 600
    x = multi_sinusoid_batch(3, 6, n)
    lists = [[7, 12], [5, 9, 16], [30], [4, 6, 9, 25], [11, 13], [8, 12, 18]]
    qo = QOPeriods()
    for periods in ([7, 12, 30], lists):
        got = qo.compute_reconstruction(x, periods)
        assert isinstance(got, list) and len(got) == 6
        for w in range(6):
            pl = periods[w] if periods is lists else periods
            recon, bases = got[w]
            a, dims, w_o, recon_o = _oracle_fit(x[w], pl)
            assert np.linalg.cond(a @ a.T) <= COND_CUT
            assert bases["periods"] == pl and bases["basis_dictionary"] == dims
            assert set(bases.keys()) == {"periods", "subspaces", "weights", "basis_dictionary"}
            assert rel_err(bases["weights"], w_o) < 1e-8 and rel_err(recon, recon_o) < 1e-8, (w, pl)
            assert np.array_equal(bases["subspaces"], a)
    # a singular list takes the 1-D call of the row (lstsq by default), the others stay on the device
    got = qo.compute_reconstruction(x[:2], [[6, 2, 3], [7, 12]])
    one = qo.compute_reconstruction(x[0], [6, 2, 3])
    assert np.array_equal(got[0][0], one[0]) and np.array_equal(got[0][1]["weights"], one[1]["weights"])
    assert rel_err(got[1][0], _oracle_fit(x[1], [7, 12])[3]) < 1e-8
    # type="solve" on a singular list: the 1-D call returns None, so does the row
    assert (qo.compute_reconstruction(x[:1], [[7, 7]], type="solve")[0] is None) == (qo.compute_reconstruction(x[0], [7, 7], type="solve") is None)
    # float32 batch
    got32 = qo.compute_reconstruction(x.astype(np.float32), [7, 12, 30])
    for w in range(6):
        _, _, w_o, recon_o = _oracle_fit(x[w].astype(np.float32).astype(np.float64), [7, 12, 30])
        assert rel_err(got32[w][1]["weights"], w_o) < 1e-4 and rel_err(got32[w][0], recon_o) < 1e-4
    # 1-D input takes the path it always took
    recon, bases = qo.compute_reconstruction(x[0], [7, 12])
    assert rel_err(recon, _oracle_fit(x[0], [7, 12])[3]) < 1e-8


def test_test_function_batch(eng):
    """6. test_function= on a batch: called once per row on that row's 1-D norms; rows equal the 1-D calls."""
    from pyperiod_amd import RamanujanPeriods

    x = multi_sinusoid_batch(0, 6, 240)
    calls = []

    def pick(norms):
        calls.append(np.ndim(norms))
        order = np.argsort(-norms, kind="stable")[:2]
        return np.sort(order)

    got = RamanujanPeriods().find_periods_with_weights(x, 2, 80, test_function=pick)
    assert calls == [1] * 6
    for w in range(6):
        out1, res1 = RamanujanPeriods().find_periods_with_weights(x[w], 2, 80, test_function=pick)
        out, res = got[w]
        assert np.array_equal(out["periods"], out1["periods"]) and np.array_equal(out["norms"], out1["norms"])
        assert out["basis_dictionary"] == out1["basis_dictionary"]
        a, _ = po.qo_get_subspaces(out1["periods"], 240)
        assert np.linalg.cond(a @ a.T) <= COND_CUT
        assert rel_err(out["weights"], out1["weights"]) < 1e-8 and rel_err(res, res1) < 1e-8
    got = RamanujanPeriods().find_periods_with_weights(x[:2], 2, 80, test_function=lambda v: np.array([7, 12]))
    assert all(list(o["periods"]) == [7, 12] and list(o["basis_dictionary"].values()) == [7, 11] for o, _ in got)


def test_plan_pins(eng):
    """7. PH_OP_QO_FIT: the LDS grows with kcap, the last feasible kcap launches, the next is refused by the plan query and
    by the launch alike."""
    from pyperiod_amd import _ffi

    prev = 0
    for kcap in (1, 64, 65, 128, 129, 512, 513, 1024, 2048):
        (k,) = eng.plan_info("qo_fit", 1024, (kcap, 128))
        assert k.window == _ffi.PH_PLAN_HBM and k.second == _ffi.PH_PLAN_NONE and k.variant == _ffi.PH_PLAN_ONE
        assert k.lds_bytes >= prev and k.lds_bytes <= eng.lds_bytes and k.block in (256, 512, 1024)
        assert k.block == (1024 if kcap > 512 else 512 if kcap > 128 else 256)
        prev = k.lds_bytes
    # N and dtype do not enter; a long period range does once its bitset outgrows the vectors
    assert eng.plan_info("qo_fit", 100, (512, 128), np.float32) == eng.plan_info("qo_fit", 1 << 20, (512, 128))
    assert eng.plan_info("qo_fit", 1024, (64, 1 << 20))[0].lds_bytes > eng.plan_info("qo_fit", 1024, (64, 128))[0].lds_bytes
    assert eng.qo_fit_feasible(2048, 512) and not eng.qo_fit_feasible(1 << 20, 512)
    lo, hi = 2048, 1 << 14
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if eng.qo_fit_feasible(mid, 512) else (lo, mid)
    last = lo
    assert eng.plan_info("qo_fit", 1024, (last, 512))[0].lds_bytes <= eng.lds_bytes
    x = multi_sinusoid_batch(0, 2, 1024)
    keeps, wts, resid, st = eng.qo_fit(x, [7, 12], kcap=last, max_period=512)
    assert not st.any() and wts.shape == (2, last)
    small = eng.qo_fit(x, [7, 12], kcap=64, max_period=512)
    assert rel_err(wts[:, :64], small[1]) < 1e-12 and rel_err(resid, small[2]) < 1e-12 and not wts[:, 64:].any()
    with pytest.raises(ValueError):
        eng.plan_info("qo_fit", 1024, (last + 1, 512))
    with pytest.raises(ValueError):
        eng.qo_fit(x, [7, 12], kcap=last + 1, max_period=512)


def test_scale_batch(eng):
    """8. 256 windows x 8192 samples, periods 2 .. 512, in one call; every 16th row against the oracle."""
    from pyperiod_amd import RamanujanPeriods

    x = multi_sinusoid_batch(0, 256, 8192)
    kw = dict(min_length=2, max_length=512, thresh=0.2)
    got = RamanujanPeriods().find_periods_with_weights(x, **kw)
    assert len(got) == 256
    for out, res in got:
        assert np.all(np.isfinite(out["weights"])) and np.all(np.isfinite(res))
        assert out["weights"].size == sum(out["basis_dictionary"].values())
    compared = 0
    for w in range(0, 256, 16):
        want, wres = po.ramanujan_find_periods_with_weights(x[w], **kw)
        out, res = got[w]
        assert np.array_equal(out["periods"], want["periods"]), w
        assert {k: int(v) for k, v in out["basis_dictionary"].items()} == want["basis_dictionary"], w
        a = want["subspaces"]
        ev = np.linalg.eigvalsh(a @ a.T)  # (symmetric: cheaper than the SVD of numpy.linalg.cond at 3000 rows)
        cond = ev[-1] / ev[0] if ev[0] > 0 else np.inf
        if cond <= COND_CUT:
            compared += 1
            ew, er = rel_err(out["weights"], want["weights"]), rel_err(res, wres)
            print(f"scale row {w}: rows {a.shape[0]} cond {cond:.2e} weights {ew:.2e} residual {er:.2e}")
            assert ew < 1e-8 and er < 1e-8, (w, a.shape[0], cond, ew, er)
    assert compared >= 8
