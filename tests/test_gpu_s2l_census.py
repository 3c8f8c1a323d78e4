"""small_to_large (k_small_to_large_pair, k_small_to_large) against the oracle on every event path of both kernels
(case table and restatements: s2l_cases.py, census: test_s2l_census_cpu.py).

Five engines: the pair kernel with 16 wavefronts (default) and with 8 (PH_S2L_BLOCK=512), the one-window kernel
(PH_S2L_PAIR=0), the same with 256 threads (PH_SWEEP_BLOCK=256: every boundary of split_row_means and of the flat loops
moves) and with the window in HBM (PH_HBM_WINDOW=1).  Every window of every case on every engine: status 0; count and
period list equal to the oracle's (every case of the table passes the margin rule, the CPU census asserts it); power k
within TOL ||r_k|| / ||x|| and base row k within TOL max|r_k| element by element, r_k the oracle's residual before
accept k (from its trace) -- a small late base does not hide under the first one.  TOL = 1e-10; float32 windows 1e-4.
float32, trunc and orth cases run on the one-window engines only.

Between the engines the float64 plain cases are equal bit for bit; so are the two windows of a pair when they are
swapped, every window alone, the same call again, and a batch that starts 8 bytes off a 16-byte boundary.

Measured on an MI355X: largest error 8.0e-6 of the power bar and 1.3e-5 of the base bar for float64 on every engine
(trunc / orth 3.4e-6 and 0), 1.2e-4 and 1.5e-3 for float32.  The module takes 16 s alone, 11 s of them one-time start-up in the first test
(torch's import for the device-tensor case, the first launch of each kernel); in the whole suite no test of it takes 2 s.
"""

import os
import warnings

import numpy as np
import pytest

import s2l_cases as sc

pytestmark = pytest.mark.gpu


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
    assert not any(k in os.environ for env in sc.ENGINES.values() for k in env)
    e = {name: _engine(**env) for name, env in sc.ENGINES.items()}
    e["runs"] = {}
    for case in sc.CASES:  # the oracle on the whole table, once for every test of the module
        sc.ref(case, n_windows(e, case))
    yield e
    for name in sc.ENGINES:
        e[name].close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def n_windows(engines, case):
    return 8 * engines["pair"].num_cu + 3 if case["kinds"] == "persistent" else None


def plain64(case):
    return case["dtype"] == np.float64 and not sc.general(case)


def call(engine, case, x, thresh=None, **kw):
    out = engine.small_to_large(x, case["thresh"] if thresh is None else thresh, sc.n_periods_of(case), case["trunc"], case["orth"], **kw)
    return tuple(a.cpu().numpy() if hasattr(a, "cpu") else a for a in out)


def device_batch(x, engine, misaligned):
    """The batch as a device tensor whose first sample sits at 0 or at 8 mod 16 bytes."""
    import torch

    store = torch.zeros(x.size + 2, dtype=torch.float64, device=f"cuda:{engine.device}")
    off = (store.data_ptr() // 8 + (1 if misaligned else 0)) % 2  # allocations are 16-byte aligned and more; be sure
    xt = store[off:off + x.size].view(x.shape)
    xt.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert xt.data_ptr() % 16 == (8 if misaligned else 0) and xt.is_contiguous()
    return xt


def run(engines, name, case):
    """The engine's answer for the whole case: computed once, shared.  A misaligned case goes in as a device tensor that
    starts one double into its storage."""
    key = (name, case["name"])
    if key not in engines["runs"]:
        x = sc.windows(case, n_windows(engines, case))
        xin = device_batch(x, engines[name], True) if case["misaligned"] else x
        engines["runs"][key] = call(engines[name], case, xin)
    return engines["runs"][key]


def same_bits(a, b, what):
    """counts, periods, powers, the base rows the kernels wrote, status: bit for bit."""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[4], b[4]), (what, a[0], b[0], a[4], b[4])
    for w, k in enumerate(a[0]):
        assert np.array_equal(a[1][w, :k], b[1][w, :k]), (what, w, a[1][w, :k], b[1][w, :k])
        assert np.array_equal(a[2][w, :k].view(np.uint64), b[2][w, :k].view(np.uint64)), (what, w, "powers")
        assert np.array_equal(a[3][w, :k].view(np.uint8), b[3][w, :k].view(np.uint8)), (what, w, "bases")


def held(case, got, refs, x, what, lists=True, rows=None):
    """Status, count, periods, and the two value bars for every window; `rows`: only the first so many accepts were
    written (capacity test).  -> the largest power and base error as fractions of their bars."""
    counts, per, pw, bs, st = got
    tol = sc.TOL if case["dtype"] == np.float64 else sc.TOL32
    assert bs.dtype == case["dtype"] and len(counts) == len(refs)
    worst = [0.0, 0.0]
    for w, r in enumerate(refs):
        k, want = int(counts[w]), r["periods"]
        if rows is None:
            assert st[w] == 0, (what, w, "status", st[w])
        if lists:
            assert k == len(want) and list(per[w, :min(k, rows or k)]) == want[:rows], (what, w, k, list(per[w, :k]), want)
        elif k != len(want) or list(per[w, :k]) != want:
            continue  # below the margin bar the lists may differ: nothing to compare the values with
        scales = sc.accept_scales(r, np.asarray(x[w], dtype=np.float64))
        for i in range(min(k, rows or k)):
            unit_p, unit_b = scales[i]
            ep = abs(float(pw[w, i]) - float(r["powers"][i]))
            eb = float(np.max(np.abs(bs[w, i].astype(np.float64) - r["bases"][i])))
            assert ep <= tol * unit_p, (what, w, want[i], "power", float(pw[w, i]), float(r["powers"][i]), ep / unit_p)
            assert eb <= tol * unit_b, (what, w, want[i], "base", eb / unit_b if unit_b else eb)
            worst[0] = max(worst[0], ep / (tol * unit_p) if unit_p else 0.0)
            worst[1] = max(worst[1], eb / (tol * unit_b) if unit_b else 0.0)
    return worst


def test_plans(engines):
    """Each engine runs the variant, the block and the window placement s2l_cases.plan_variant predicts for each case,
    and the persistent case has more pairs than workgroups at both block sizes."""
    from pyperiod_amd import _ffi

    assert engines["pair"].lds_bytes >= sc.LDS_LIMIT
    seen = set()
    for case in sc.CASES:
        for name, env in sc.ENGINES.items():
            (k,) = engines[name].plan_info("small_to_large", case["n"], (sc.n_periods_of(case),), case["dtype"], case["trunc"], case["orth"])
            got = ("pair" if k.variant == _ffi.PH_PLAN_PAIR else "one", k.block, "hbm" if k.window == _ffi.PH_PLAN_HBM else "lds")
            assert got == sc.plan_variant(case["dtype"], sc.general(case), case["n"], sc.n_periods_of(case), env), (case["name"], name, k)
            assert k.variant in (_ffi.PH_PLAN_PAIR, _ffi.PH_PLAN_ONE) and k.window in (_ffi.PH_PLAN_LDS, _ffi.PH_PLAN_HBM)
            if got[0] == "pair":
                assert k.lds_bytes == sc.pair_lds_bytes(case["n"]), (case["name"], name)
            seen.add((name,) + got)
    assert seen == {("pair", "pair", 1024, "lds"), ("pair", "one", 512, "lds"), ("pair512", "pair", 512, "lds"), ("pair512", "one", 512, "lds"),
                    ("one", "one", 512, "lds"), ("one256", "one", 256, "lds"), ("hbm", "one", 512, "hbm")}, seen
    cus = engines["pair"].num_cu
    pairs = (8 * cus + 3 + 1) // 2
    assert pairs > sc.resident_pairs(48, 512, cus) > sc.resident_pairs(48, 1024, cus)


@pytest.mark.parametrize("name", list(sc.ENGINES))
def test_every_case_against_the_oracle(engines, name):
    worst = {}
    for case in sc.CASES:
        if name in sc.PAIR_ENGINES and not plain64(case):
            continue
        W = n_windows(engines, case)
        got = run(engines, name, case)
        assert sc.admitted(case, W), case["name"]
        w = held(case, got, sc.ref(case, W), sc.windows(case, W), (case["name"], name))
        key = np.dtype(case["dtype"]).name + (" trunc/orth" if sc.general(case) else "")
        worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0.0, 0.0]), w)]
    for key, (wp, wb) in worst.items():
        print(f"{name} {key}: largest power error {wp:.2e} of its bar, largest base error {wb:.2e} of its bar")


def test_pair_engines_equal_the_one_window_kernel(engines):
    n = 0
    for case in sc.CASES:
        if plain64(case):
            for name in sc.PAIR_ENGINES:
                same_bits(run(engines, name, case), run(engines, "one", case), (case["name"], name))
            n += 1
    assert n >= 40


def test_knife_edges(engines):
    """thresh 1e-12 either side of an accepted period's own drop, for a period whose rows are split 16 ways and more, one
    with its means in prt and one that takes the column loop: the pair engines equal the one-window kernel bit for bit,
    and where the period list is the oracle's the values are held to it."""
    for what, case, w, p, thresh, accepts in sc.knife_cases():
        x = np.ascontiguousarray(sc.windows(case)[[w, 1 - w]])
        one = call(engines["one"], case, x, thresh)
        for name in sc.PAIR_ENGINES:
            same_bits(call(engines[name], case, x, thresh), one, (what, name))
        refs = [sc.oracle_window(row, case, thresh) for row in x]
        print(what, "kernel", list(one[1][0, :one[0][0]]), "oracle", refs[0]["periods"], "accepts" if accepts else "rejects")
        held(case, one, refs, x, what, lists=False)


def test_halves(engines):
    """Swapping the two windows of a pair swaps the outputs, and every window alone equals the same window in its pair,
    bit for bit: nothing of a neighbour -- a stale staging buffer, a NaN, a scale -- leaks."""
    n = 0
    for case in sc.CASES:
        if not plain64(case) or case["kinds"] == "persistent":
            continue
        x = sc.windows(case)
        for name in sc.PAIR_ENGINES:
            both = run(engines, name, case)
            if len(x) == 2:
                sw = call(engines[name], case, np.ascontiguousarray(x[::-1]))
                same_bits(tuple(a[::-1] for a in sw), both, (case["name"], name, "swapped"))
            for w in range(len(x)):
                alone = call(engines[name], case, x[w:w + 1])
                same_bits(alone, tuple(a[w:w + 1] for a in both), (case["name"], name, "alone", w))
        n += 1
    assert n >= 40


def test_persistent_case_twice(engines):
    """More pairs than workgroups, so workgroups draw second pairs from the device counter; the host zeroes it before
    every launch: the same call again gives the same bits (the first call is held to the oracle above)."""
    case = sc.BY_NAME["persistent"]
    x = sc.windows(case, n_windows(engines, case))
    assert len(x) % 2 == 1
    for name in sc.PAIR_ENGINES:
        same_bits(call(engines[name], case, x), run(engines, name, case), (name, "again"))
        half = call(engines[name], case, x[:len(x) // 2])  # fewer pairs than workgroups
        same_bits(half, tuple(a[:len(x) // 2] for a in run(engines, name, case)), (name, "half the batch"))


def test_misaligned_base(engines):
    """A device tensor that starts one double into its storage (even N: every row then sits at 8 mod 16 and s2l_copy
    takes its scalar path) against the aligned tensor and the numpy call."""
    for cname in ("planted_misaligned", "accept_4100", "planted_lone"):
        case = sc.BY_NAME[cname]
        x = sc.windows(case)
        assert case["n"] % 2 == 0
        for name in sc.PAIR_ENGINES + ("one",):
            e = engines[name]
            off = call(e, case, device_batch(x, e, True))
            same_bits(off, call(e, case, device_batch(x, e, False)), (cname, name, "aligned tensor"))
            same_bits(off, call(e, case, x), (cname, name, "numpy"))


@pytest.mark.parametrize("name", ["pair", "pair512", "one"])
def test_capacity(engines, name):
    """cap = 3 on a pair that accepts 39 periods each: the ABI call returns PH_E_CAP, counts are the oracle's, status is
    PH_ST_CAP, the first three periods, powers and base rows are right; the engine's retry returns everything; with
    PH_FLAG_NOSYNC on a device tensor the status word alone reports it."""
    import torch

    from pyperiod_amd import _ffi

    e = engines[name]
    case = sc.BY_NAME["accept_4100"]
    x, refs, cap = sc.windows(case), sc.ref(case), 3
    want = [len(r["periods"]) for r in refs]
    assert min(want) > sc.DEFAULT_CAP > cap
    for nosync in (False, True):
        xin = device_batch(x, e, False) if nosync else x
        xc, code, W, N, fl, mk = e._prep(xin)
        counts, per, pw = mk.empty((W,), np.int32), mk.empty((W, cap), np.int32), mk.empty((W, cap), np.float64)
        bs, st = mk.empty((W, cap, N), np.float64), mk.empty((W,), np.int32)
        rc = e._call(mk, W, e._lib.ph_small_to_large, mk.addr(xc), code, W, N, float(case["thresh"]), sc.n_periods_of(case), None, None, 0,
                     fl | (_ffi.PH_FLAG_NOSYNC if nosync else 0), cap, mk.addr(counts), mk.addr(per), mk.addr(pw), mk.addr(bs), mk.addr(st), check=False)
        if nosync:
            torch.cuda.synchronize()
        got = tuple(a.cpu().numpy() if nosync else a for a in (counts, per, pw, bs, st))
        assert rc == (_ffi.PH_OK if nosync else _ffi.PH_E_CAP), (name, nosync, rc)
        assert list(got[0]) == want and list(got[4]) == [_ffi.PH_ST_CAP] * W, (name, nosync, got[0], got[4])
        held(case, got, refs, x, (name, "cap 3", nosync), rows=cap)
    full = call(e, case, x, cap=cap)
    assert full[1].shape[1] == max(want)
    held(case, full, refs, x, (name, "retry"))
    same_bits(full, run(engines, name, case), (name, "retry against the default capacity"))
