"""k_ramanujan, k_ram_select and k_dict_project against the oracle on every fold shape and factor set (case table:
ramanujan_cases.py, census: test_ramanujan_census_cpu.py).

Norms.  Every case runs as float64 and as float32 on the default engine and on one that keeps every window in HBM
(PH_HBM_WINDOW=1).  Each entry is held on its own: |got[w, q] - want[w, q]| <= TOL B_q(w) with TOL = 1e-10, `want` and
the unit B_q (the energy in front of the projector) from po.ramanujan_norm_projector_q in longdouble.  float32 windows
get the same bound against the oracle on the rounded samples: the kernel promotes every sample to double before the
first add.  Outside the range the row is zero, and word 0 -- the root queue of the workgroup -- is +0.0 bit for bit.
A window alone, the same call again and (to TOL_HBM) the other engine give the same row.

Selection and dictionary projection are held to the reference's numpy expressions: k_ram_select to the rule of
test_ram_fit_cpu.py applied to the device's own norms, k_dict_project to one float32 ulp of the longdouble value."""

import os

import numpy as np
import pytest

import ramanujan_cases as rc
from conftest import rel_err
from oracle import period_oracle as po
from test_ram_fit_cpu import ram_select_rule

pytestmark = pytest.mark.gpu
TOL = rc.TOL
TOL_HBM = {np.float64: 1e-12, np.float32: 1e-5}  # test_gpu_placement_edges.py's bars between the two engines
DTYPES = (np.float64, np.float32)


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

    assert "PH_HBM_WINDOW" not in os.environ
    hbm = _engine(PH_HBM_WINDOW=1)
    yield {"default": default_engine(), "hbm": hbm}
    hbm.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def held(got, want, unit, q_lo, what):
    """The per-entry bound and the entries outside the range; -> the largest error in units of B_q."""
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert not bits(got[:, 0]).any(), (what, "word 0 is not +0.0", got[:, 0])
    assert not got[:, :q_lo].any(), (what, "entries below q_lo")
    err = np.abs(got.astype(np.longdouble) - want)
    bad = np.argwhere(~(err <= TOL * unit))
    worst = float(np.max(err[:, q_lo:] / unit[:, q_lo:], initial=0.0)) if q_lo < want.shape[1] else 0.0
    assert bad.size == 0, (what, f"{len(bad)} entries beyond {TOL} B_q, first (window, q):", bad[:8].tolist(),
                           [(float(got[w, q]), float(want[w, q]), float(unit[w, q])) for w, q in bad[:4]], worst)
    return worst


def run_case(engines, case, dtypes=DTYPES):
    n, q_lo, q_hi = case[:3]
    worst = 0.0
    for dtype in dtypes:
        x = rc.windows(case, dtype)
        want, unit = rc.ref(case, dtype)
        rows = {}
        for name, e in engines.items():
            what = (case, np.dtype(dtype).name, name)
            got = e.ramanujan_norms(x, q_lo, q_hi)
            worst = max(worst, held(got, want, unit, q_lo, what))
            assert np.array_equal(bits(e.ramanujan_norms(x, q_lo, q_hi)), bits(got)), (what, "the same call again")
            for w in range(x.shape[0]):
                alone = e.ramanujan_norms(x[w:w + 1], q_lo, q_hi)
                assert np.array_equal(bits(alone[0]), bits(got[w])), (what, "window alone", w)
            rows[name] = got
        assert rel_err(rows["default"], rows["hbm"]) <= TOL_HBM[dtype], (case, np.dtype(dtype).name, "default against hbm")
    return worst


@pytest.mark.parametrize("group", list(rc.GROUPS))
def test_norms(engines, group):
    worst = 0.0
    for case in rc.GROUPS[group]:
        worst = max(worst, run_case(engines, case))
    print(f"{group}: {len(rc.GROUPS[group])} cases, largest error {worst:.2e} B_q")


def test_empty_range_launches_nothing(engines):
    """q_lo > q_hi: zeros, and the profile shows no k_ramanujan."""
    ran = [c for c in rc.CASES if c[1] > c[2]]
    assert len(ran) >= 2
    for case in ran:
        n, q_lo, q_hi = case[:3]
        for dtype in DTYPES:
            for name, e in engines.items():
                e.profile(True)
                try:
                    got = e.ramanujan_norms(rc.windows(case, dtype), q_lo, q_hi)
                    names = [k for k, _ in e.profile_read()]
                finally:
                    e.profile(False)
                assert "k_ramanujan" not in names and not bits(got).any() and got.shape == (4, q_hi + 1), (case, name)
    # the same query on a range that is not empty does show the kernel
    e = engines["default"]
    e.profile(True)
    try:
        e.ramanujan_norms(rc.windows((300, 50, 100)), 50, 100)
        names = [k for k, _ in e.profile_read()]
    finally:
        e.profile(False)
    assert "k_ramanujan" in names


def _plan(e, n, q_lo, q_hi, dtype):
    (k,) = e.plan_info("ramanujan", n, (q_lo, q_hi), dtype)
    return k


def _first_without_pad(e, q_hi, dtype, lo=1024, hi=40000):
    for n in range(lo, hi):
        if _plan(e, n, 2, q_hi, dtype).pad == 0:
            return n
    raise AssertionError(("no window length without pad", q_hi, dtype))


def test_placements(engines):
    """What the plans of the table's cases are between them on the default engine: the window in LDS behind a zeroed
    pad, in LDS without it and in HBM, wave counts below, at and above the root count (the HBM engine plans HBM for
    every case).  Without the pad the folds read past the window into the strips; which of the table's lengths drop
    it is an accident of the LDS arithmetic, so the first N that does is also found on the host for q_hi = 128 and
    q_hi = 704 and run here."""
    from pyperiod_amd import _ffi

    e = engines["default"]
    seen, waves = set(), set()
    for case in rc.CASES:
        n, q_lo, q_hi = case[:3]
        if q_lo > q_hi:
            continue
        roots = len(rc.assign(n, q_lo, q_hi))
        for dtype in DTYPES:
            k = _plan(e, n, q_lo, q_hi, dtype)
            assert _plan(engines["hbm"], n, q_lo, q_hi, dtype).window == _ffi.PH_PLAN_HBM
            seen.add(("hbm" if k.window == _ffi.PH_PLAN_HBM else "lds", "pad" if k.pad else "no pad"))
            seen.add("waves < roots" if k.waves < roots else "waves == roots" if k.waves == roots else "waves > roots")
            waves.add(k.waves)
    print(sorted(str(s) for s in seen), "wave counts", sorted(waves))
    assert {("lds", "pad"), ("lds", "no pad"), ("hbm", "pad"), "waves < roots", "waves == roots", "waves > roots"} <= seen
    assert 16 in waves and min(waves) < 16
    for q_hi, q_lo, dtype in ((128, 1, np.float64), (704, 300, np.float64), (704, 300, np.float32)):
        n = _first_without_pad(e, q_hi, dtype)
        k = _plan(e, n, q_lo, q_hi, dtype)
        assert k.pad == 0 and k.window == _ffi.PH_PLAN_LDS and 2 <= k.waves <= 16, (q_hi, n, k)
        worst = run_case(engines, (n, q_lo, q_hi, 2), (dtype,))
        print(f"no pad: q_hi {q_hi} {np.dtype(dtype).name} N {n} waves {k.waves}: largest error {worst:.2e} B_q")


def test_device_tensor_on_a_side_stream(engines):
    """A wide-range case as a device tensor on a stream that is not torch's default: the bits of the numpy call."""
    import torch

    case = (1000, 1, 256)
    assert case in rc.CASES
    e = engines["default"]
    for dtype in DTYPES:
        x = rc.windows(case, dtype)
        host = e.ramanujan_norms(x, case[1], case[2])
        side = torch.cuda.Stream(device=e.device)
        with torch.cuda.stream(side):
            xt = torch.from_numpy(np.array(x)).to(f"cuda:{e.device}", non_blocking=False)
            dev = e.ramanujan_norms(xt, case[1], case[2])
        side.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(host)), np.dtype(dtype).name
        assert np.array_equal(bits(e.ramanujan_norms(x, case[1], case[2])), bits(host))  # and back on the own stream


# ------------------------------------------------------------------------------------------------ k_ram_select
def _select_batch(n, dtype=np.float64):
    """(4, n): a plain window, one with a NaN sample, all zeros, and a plain one again."""
    rng = np.random.default_rng([rc.SEED, n, 7])
    x = rng.standard_normal((4, n)) + np.sin(2 * np.pi * np.arange(n) / 12)[None, :]
    x[1, n // 3] = np.nan
    x[2] = 0.0
    return x.astype(dtype)


@pytest.mark.parametrize("q_hi", [62, 63, 64, 65, 127, 128])
def test_ram_select(engines, q_hi):
    """The selection rule apart from the norms: periods and counts of ph_ramanujan_fit against the numpy rule applied
    to the norms the same call returned.  The row has q_hi + 1 entries, one below to one above a wavefront (and two);
    thresh is put between two neighbouring ratios so that the count is 0, pcap - 1, pcap and pcap + 1 where the row has
    that many periods, and below every ratio so that every norm passes."""
    e = engines["default"]
    n, q_lo = 400, 1
    x = _select_batch(n)
    norms0 = e.ramanujan_norms(x, q_lo, q_hi)
    assert np.isnan(norms0[1, 1:]).all() and not norms0[2].any() and np.all(norms0[0, 1:] > 0)
    ratio = np.sort(norms0[0] / np.abs(np.max(norms0[0])))[::-1]  # descending; the last one is word 0
    assert np.all(np.diff(ratio) < 0)
    reached = set()
    for pcap in (1, 64):
        targets = {0: 1.0, q_hi: 1e-300}
        for c in (pcap - 1, pcap, pcap + 1):
            if 1 <= c <= q_hi:
                targets[c] = 0.5 * (ratio[c - 1] + ratio[c])
        for c, thresh in sorted(targets.items()):
            norms, per, counts, keeps, wts, resid, st = e.ramanujan_fit(x, q_lo, q_hi, thresh, pcap, 64)
            assert np.array_equal(bits(norms), bits(norms0)), (q_hi, pcap, c)
            assert per.shape == (4, pcap) and per.dtype == np.int32 and counts.dtype == np.int32
            for w in range(4):
                count, want = ram_select_rule(norms[w], thresh, pcap)
                assert counts[w] == count and np.array_equal(per[w], want), (q_hi, pcap, c, w, counts[w], count, per[w], want)
                assert not per[w, min(count, pcap):].any()
            assert counts[0] == c and counts[1] == 0 and counts[2] == 0, (q_hi, pcap, c, counts)
            reached.add((pcap, "below" if c < pcap else "at" if c == pcap else "above"))
            if c == q_hi:
                assert list(per[0, :min(pcap, q_hi)]) == list(range(1, min(pcap, q_hi) + 1))
    assert {(1, "below"), (1, "at"), (1, "above"), (64, "below")} <= reached
    if q_hi >= 65:
        assert {(64, "at"), (64, "above")} <= reached


# ------------------------------------------------------------------------------------------------ k_dict_project
def _dict_want(x, basis):
    """RamanujanPeriods.project in longdouble, rounded once to float32."""
    ld = np.longdouble
    out = np.zeros(basis.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i, row in enumerate(basis.astype(ld)):
            row = row / np.max(row)
            out[i] = (np.sum(x.astype(ld) * row) * row).astype(np.float32)
    return out


def _dictionaries(rows, n, rng):
    out = {}
    with np.errstate(all="ignore"):
        for q in (7, 8, 30):  # a prime, a power of two, three primes
            full = po.ramanujan_dictionary(q, n)
            out[f"Cq_complete({q})"] = full[np.arange(rows) % q]
    neg = -np.abs(rng.standard_normal((rows, n))) - 0.25
    out["negative everywhere"] = neg
    zero_max = neg.copy()
    zero_max[:, :: max(1, n // 3)] = 0.0
    out["largest entry 0"] = zero_max
    return out


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (3, 64), (5, 65), (2, 255), (2, 256), (2, 257), (7, 1000)])
def test_dict_project(engines, shape):
    """Each element within one float32 ulp of the longdouble value rounded to float32: the kernel's double dot product
    errs far below half an ulp, so it can differ from the correctly rounded value only next to a rounding boundary.
    A row whose largest entry is 0 is inf / nan in numpy (row / max(row)) and must be here."""
    rows, n = shape
    rng = np.random.default_rng([rc.SEED, rows, n])
    x = rng.standard_normal(n)
    e = engines["default"]
    for name, basis in _dictionaries(rows, n, rng).items():
        want = _dict_want(x, basis)
        got = e.dict_project(x, basis)
        assert got.dtype == np.float32 and got.shape == (rows, n), name
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (shape, name)
        if name == "largest entry 0":
            assert nan.all()
        elif n > 1 or name == "negative everywhere":
            assert not nan.any(), (shape, name)
        g, w = got[~nan].astype(np.float64), want[~nan].astype(np.float64)
        ulp = np.spacing(np.abs(want[~nan])).astype(np.float64)
        assert np.all(np.isinf(g) == np.isinf(w)) and np.all(np.abs(g - w)[np.isfinite(w)] <= ulp[np.isfinite(w)]), (
            shape, name, float(np.max(np.abs(g - w) / ulp, initial=0.0)))
