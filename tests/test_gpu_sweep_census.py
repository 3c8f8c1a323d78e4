"""The fp64 pass-plan folds (wave_sweep_plan and everything it runs, ph_device.h) against a longdouble reference on
every pass shape (case table, restatement and reference: sweep_cases.py, census: test_sweep_census_cpu.py).

Six engines: default, the window in HBM (PH_HBM_WINDOW=1), the periods below 64 one m = 0 pass each (PH_PAIR_CHAIN=0),
single and two-class passes only (PH_PLAN_MAX_M=1 and 2), and one wavefront per workgroup (PH_SWEEP_BLOCK=64: eight
times the workgroups per window, and a wavefront's passes -- hence its butterfly at the flush -- fixed by the plan alone).

Norm modes 0 and 1, every case, row, engine, float64 and float32: every entry holds |N got^2 [p] - ss_p| <= 1e-10 A_p
against sweep_ref of the values the kernel was given; zero rows give +0.0; output (W, P) float64.  Mode 2 (wave_sweep):
po.sweep_maxabs bit for bit from p = 2 (p = 1 within 1e-13: numpy sums a contiguous axis pairwise).

Bit for bit, as the code says (read before asserting): a period is produced whole by ONE wavefront -- the pass code is a
function of (window, N, p, geom) alone -- and Butterfly8 pairs the same lanes (l ^ 32, l ^ 16, l ^ 8, then lanes 7 - i,
i ^ 1, i ^ 2 of a group of 8) with a commutative add whatever slot the period lands in, and never adds two periods.  So
the chunking (a row alone against the row in a batch of 8 CUs' worth), the workgroup size, a repeated call, the
alignment of the batch and the stream cannot change a bit.  Win<T, false> reads the HBM copy of the window (zero pad
included) through plain loads into the same expressions -- additions, explicit fma, no contraction across them -- so the
HBM engine equals the default bit for bit too.  PH_PLAN_MAX_M and PH_PAIR_CHAIN=0 produce a period by another pass
(another association) and are held to the bar only.

Measured on an MI355X: profiles/sweep_census/README.md.
"""

import os
import warnings

import numpy as np
import pytest

import sweep_cases as sc
from oracle import period_oracle as po

pytestmark = pytest.mark.gpu

SAME_BITS = ("hbm", "block64")  # engines whose norm sweeps equal the default engine's bit for bit


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
    assert "PH_PLAN_SORTED" not in os.environ and "PH_PLAN_ONLY_M" not in os.environ
    e = {name: _engine(**env) for name, env in sc.ENGINES.items()}
    e["runs"] = {}
    for case in sc.CASES:  # the reference of the whole table, once for every test of the module
        sc.ref(case, np.float64)
        sc.ref(case, np.float32)
    yield e
    for name in sc.ENGINES:
        e[name].close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def sweep(engine, case, x, mode):
    out = engine.sweep(x, case["p_lo"], case["p_hi"], mode)
    return out.cpu().numpy() if hasattr(out, "cpu") else out


def run(engines, name, case, mode, dtype=np.float64):
    """The engine's answer for the rows of the case: computed once, shared."""
    key = (name, case["name"], mode, np.dtype(dtype).name)
    if key not in engines["runs"]:
        engines["runs"][key] = sweep(engines[name], case, sc.windows(case, dtype), mode)
    return engines["runs"][key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, np.argwhere(bits(a) != bits(b))[:4])


def held(case, got, refs, mode, what):
    """Every entry of every row within BAR A_p of the reference -> the largest error in units of A_p, for the periods
    below 64, from 64 to N - 1 and from N on."""
    N, p_lo, p_hi = case["n"], case["p_lo"], case["p_hi"]
    assert got.dtype == np.float64 and got.shape == (len(refs), p_hi - p_lo + 1), (what, got.dtype, got.shape)
    worst = np.zeros(3)
    periods = np.arange(p_lo, p_hi + 1)
    bands = [periods < 64, (periods >= 64) & (periods < N), (periods >= 64) & (periods >= N)]
    for w, (ss, A) in enumerate(refs):
        err = np.abs(sc.norm_sq(got[w], N, p_lo, p_hi, mode) - ss)
        bad = ~(err <= sc.BAR * A)
        assert not bad.any(), (what, "row", w, "p", int(np.argmax(bad)) + p_lo, float(got[w][np.argmax(bad)]), float(err[np.argmax(bad)] / A[np.argmax(bad)]))
        if np.all(A == 0):
            assert not got[w].any() and not np.signbit(got[w]).any(), (what, "row", w, "a zero row gives +0.0")
        else:
            worst = np.maximum(worst, [float(np.max(err[b] / A[b], initial=0.0)) for b in bands])
    return worst


def test_plans_and_counts(engines):
    """Each engine runs what its variables ask for, ph_sweep_plan_info equals the restatement's counts on every range of
    the table, and with this device's CU count the table still reaches every label."""
    from pyperiod_amd import _ffi

    import test_sweep_census_cpu as cpu

    for name, (max_m, chains, nw) in sc.VARIANTS.items():
        e = engines[name]
        for case in sc.CASES:
            plan = sc.build_plan(case["p_lo"], case["p_hi"], max_m, True, chains)
            assert e.sweep_plan_info(case["p_lo"], case["p_hi"]) == (len(plan), case["p_hi"] - case["p_lo"] + 1), (name, case["name"])
            (k,) = e.plan_info("sweep", case["n"], (case["p_lo"], case["p_hi"], 0))
            assert k.block == 64 * nw and k.window == (_ffi.PH_PLAN_HBM if name == "hbm" else _ffi.PH_PLAN_LDS), (name, case["name"], k)
    carriers = cpu.census(engines["default"].num_cu)
    missing = [label for label in sc.LABELS if not carriers[label] and label not in sc.UNREACHABLE]
    assert not missing, (engines["default"].num_cu, missing)


@pytest.mark.parametrize("name", list(sc.ENGINES))
def test_norm_modes_against_the_reference(engines, name):
    worst = {}
    for case in sc.CASES:
        for dtype in (np.float64, np.float32):
            for mode in (0, 1):
                got = run(engines, name, case, mode, dtype)
                w = held(case, got, sc.ref(case, dtype), mode, (case["name"], name, np.dtype(dtype).name, mode))
                key = np.dtype(dtype).name
                worst[key] = np.maximum(worst.get(key, 0.0), w)
    for key, w in worst.items():
        print(f"{name} {key}: largest |N got^2 [p] - ss_p| / A_p: {w[0]:.2e} (p < 64), {w[1]:.2e} (64 <= p < N), {w[2]:.2e} (p >= N); "
              f"{w.max() / sc.BAR:.1e} of the bar")


def test_engines_that_run_the_same_instructions(engines):
    """HBM window, one wavefront per workgroup, and the same call again: the default engine's bits."""
    for case in sc.CASES:
        for dtype in (np.float64, np.float32):
            for mode in (0, 1):
                want = run(engines, "default", case, mode, dtype)
                for name in SAME_BITS:
                    same_bits(run(engines, name, case, mode, dtype), want, (case["name"], name, mode))
                if dtype == np.float64:
                    same_bits(sweep(engines["default"], case, sc.windows(case), mode), want, (case["name"], "again", mode))


@pytest.mark.parametrize("name", ["default", "hbm", "block64"])
def test_maxabs(engines, name):
    """Mode 2 runs wave_sweep over the period range split in chunks: row-order sums, the oracle's bits."""
    from pyperiod_amd import _ffi

    for case in sc.CASES:
        x = sc.windows(case)
        got = sweep(engines[name], case, x, _ffi.PH_SWEEP_MAXABS)
        assert got.dtype == np.float64 and got.shape == (len(x), case["p_hi"] - case["p_lo"] + 1)
        key = ("maxabs", case["name"])
        if key not in engines["runs"]:
            engines["runs"][key] = np.stack([po.sweep_maxabs(row, case["p_lo"], case["p_hi"]) for row in x])
        want = engines["runs"][key]
        lo = 1 if case["p_lo"] == 1 else 0
        same_bits(got[:, lo:], want[:, lo:], (case["name"], name))
        # p = 1: 1e-13 of the oracle's value -- but the planted row cancels at p = 1 by construction (|sum x| ~ 1e-8 of
        # sum |x|) and numpy's own pairwise sum is only good to u sum |x| there: that row is held to 1e-13 sum |x|
        unit = np.abs(want[:, :lo])
        if sc.weak_period(case) is not None:
            unit[sc.ROW_KINDS.index("planted")] = np.sum(np.abs(x[sc.ROW_KINDS.index("planted")]))
        assert np.all(np.abs(got[:, :lo] - want[:, :lo]) <= 1e-13 * unit), (case["name"], name, "p = 1", got[:, :lo], want[:, :lo])


def device_batch(x, engine, misaligned):
    """The batch as a device tensor whose first sample sits at 0 or at 8 mod 16 bytes."""
    import torch

    store = torch.zeros(x.size + 2, dtype=torch.float64, device=f"cuda:{engine.device}")
    off = (store.data_ptr() // 8 + (1 if misaligned else 0)) % 2
    xt = store[off:off + x.size].view(x.shape)
    xt.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert xt.data_ptr() % 16 == (8 if misaligned else 0) and xt.is_contiguous()
    return xt


def test_alone_and_in_a_large_batch(engines):
    """W = 1 takes the most chunks, W = 8 CUs' worth takes one: the row's bits do not depend on it."""
    e = engines["default"]
    W = 8 * e.num_cu
    done = 0
    for case in sc.CASES:
        if case["n"] > 512 or case["p_hi"] - case["p_lo"] < 128:
            continue
        assert sc.sweep_chunks(e.num_cu, 1, case["p_lo"], case["p_hi"], 8) > 1 and sc.sweep_chunks(e.num_cu, W, case["p_lo"], case["p_hi"], 8) == 1
        x = sc.windows(case)
        batch = np.ascontiguousarray(np.tile(x, (W // len(x) + 1, 1))[:W])
        for mode in (0, 1):
            big = sweep(e, case, batch, mode)
            for w in (0, 1, 2):
                alone = sweep(e, case, x[w:w + 1], mode)
                same_bits(alone[0], run(engines, "default", case, mode)[w], (case["name"], "alone against the case", w))
                for at in (w, w + len(x) * ((W - 1 - w) // len(x))):  # row i of the batch is x[i mod 5]: first and last copy
                    same_bits(alone[0], big[at], (case["name"], "alone against row", at))
        done += 1
        if done == 2:
            break
    assert done == 2


def test_alignment_and_stream(engines):
    """A device tensor 8 bytes off a 16-byte boundary (load_window's scalar path), an aligned one, a tensor on a side
    stream: the bits of the host array."""
    import torch

    e = engines["default"]
    done = 0
    for case in sc.CASES:
        if case["n"] % 2 or done == 3:
            continue
        x = sc.windows(case)
        for mode in (0, 1, 2):
            want = sweep(e, case, x, mode)
            same_bits(sweep(e, case, device_batch(x, e, True), mode), want, (case["name"], "misaligned", mode))
            same_bits(sweep(e, case, device_batch(x, e, False), mode), want, (case["name"], "aligned tensor", mode))
            side = torch.cuda.Stream(device=e.device)
            with torch.cuda.stream(side):
                xt = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{e.device}")
                got = e.sweep(xt, case["p_lo"], case["p_hi"], mode)
            side.synchronize()
            same_bits(got.cpu().numpy(), want, (case["name"], "side stream", mode))
        done += 1
    assert done == 3


def test_scaling(engines):
    """Powers of two pass through every sum, square, weight and root exactly: sweep(2^200 x) = 2^200 sweep(x), bit for bit."""
    assert len(sc.SCALED) >= 2
    for cname in sc.SCALED:
        case = sc.BY_NAME[cname]
        x = sc.special_windows(case, "scaled")
        for name in sc.ENGINES:
            for mode in (0, 1):
                got = sweep(engines[name], case, x, mode)
                assert np.all(np.isfinite(got)) and np.all(got[0] > 0)
                same_bits(got[1], got[0] * 2.0 ** 200, (cname, name, mode, "2^200"))
                same_bits(got[2], got[0] * 2.0 ** -200, (cname, name, mode, "2^-200"))


def test_nonfinite_rows(engines):
    """A NaN and an Inf sample: NaN wherever the reference has NaN, +Inf wherever it has +Inf, and the healthy rows on
    either side keep the bits they have alone."""
    assert len(sc.NONFINITE) >= 2
    for cname in sc.NONFINITE:
        case = sc.BY_NAME[cname]
        x = sc.special_windows(case, "nonfinite")
        refs = [sc.sweep_ref(row, case["p_lo"], case["p_hi"])[0].astype(np.float64) for row in x[1:3]]
        assert np.isnan(refs[0]).all() and np.isposinf(refs[1]).all()
        for name in sc.ENGINES:
            for mode in (0, 1):
                got = sweep(engines[name], case, x, mode)
                assert np.array_equal(np.isnan(got[1]), np.isnan(refs[0])), (cname, name, mode, "NaN row")
                assert np.array_equal(np.isposinf(got[2]), np.isposinf(refs[1])) and not np.isnan(got[2]).any(), (cname, name, mode, "Inf row")
                same_bits(got[0], sweep(engines[name], case, x[0:1], mode)[0], (cname, name, mode, "healthy row 0"))
                same_bits(got[3], got[0], (cname, name, mode, "healthy row 3"))


def test_host_caches(engines):
    """One engine through ranges and window lengths that reuse and replace the cached plan and geometry (prepare_plan's
    key; prepare_geom under geom_max_p >= max_p with another N; m_best and best_correlation put their own plans into
    the same slot): every sweep equals the same call on a fresh engine, bit for bit."""
    rng = np.random.default_rng(7)
    x1, x2 = rng.standard_normal((3, 700)), rng.standard_normal((3, 450))
    e = engines["default"]
    steps = [(x1, 2, 300), (x1, 2, 301), (x2, 2, 300), "m_best", "best_correlation", (x1, 3, 300), (x1, 2, 300)]
    for step in steps:
        if step == "m_best":
            e.m_best(x1, num=3)
        elif step == "best_correlation":
            e.best_correlation(x1, num=3)
        else:
            x, p_lo, p_hi = step
            fresh = _engine()
            try:
                for mode in (0, 1, 2):
                    same_bits(e.sweep(x, p_lo, p_hi, mode), fresh.sweep(x, p_lo, p_hi, mode), (x.shape, p_lo, p_hi, mode))
            finally:
                fresh.close()
