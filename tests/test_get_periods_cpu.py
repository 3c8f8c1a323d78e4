"""QOPeriods.get_periods without a GPU: the closed form that k_qo_extract evaluates, restated in numpy, against the
repaired reference's results (tests/golden/qo_get_periods.npz, written by tests/golden/make_golden_get_periods.py); the
host helpers of the reference surface; the C ABI's argument checks; and what the class packs for the engine."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

TYPES = ("rr", "lu", "qr", "lstsq")
FP64_BAR = 1e-10  # the project's fp64 parity bar (the differences observed when the fixture was made were <= 2e-14)


def mobius(n):
    mu, m, f = 1, n, 2
    while f * f <= m:
        if m % f == 0:
            m //= f
            if m % f == 0:
                return 0
            mu = -mu
        f += 1
    return -mu if m > 1 else mu


def concatenate(keys, vals, weights):
    segs, read = [], 0
    for p, r in zip(keys, vals):
        seg = np.zeros(p)
        seg[:r] = weights[read : read + r]
        read += r
        segs.append(seg)
    return segs


def closed_form(keys, vals, weights):
    """actual = c - P c by fold-means and Moebius sums; one period alone: c - mean(c)."""
    segs = concatenate(keys, vals, weights)
    if len(keys) == 1:
        return np.concatenate(segs) - np.mean(segs[0])
    out = [s.copy() for s in segs]
    for d in range(1, max(keys) + 1):
        members = [a for a, p in enumerate(keys) if p % d == 0]
        if len(members) < 2:
            continue
        u = {}
        for a in members:
            u[a] = np.zeros(d)
            for e in range(1, d + 1):
                if d % e == 0 and mobius(d // e) != 0:
                    u[a] += mobius(d // e) * np.tile(segs[a].reshape(-1, e).mean(axis=0), d // e)
        v = sum(u[a] for a in members) / sum(d / keys[a] for a in members)
        for a in members:
            out[a] += np.tile((d / keys[a]) * v - u[a], keys[a] // d)
    return np.concatenate(out)


def cases(g):
    for k in range(int(g["count"])):
        yield k, [int(v) for v in g[f"c{k}_keys"]], [int(v) for v in g[f"c{k}_vals"]], g[f"c{k}_weights"]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("qo_get_periods")


def test_fixture_holds_data_only(fixture):
    assert int(fixture["count"]) == 25
    for name in fixture:
        a = fixture[name]
        assert a.dtype.kind in "fiU", (name, a.dtype)  # numbers and exception class names, nothing pickled
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "qo_get_periods.npz"))
    assert size < 1 << 20


def test_closed_form_reproduces_the_reference(fixture):
    worst = 0.0
    for k, keys, vals, wts in cases(fixture):
        got = closed_form(keys, vals, wts)
        want = fixture[f"c{k}_lstsq"]  # always returned
        scale = max(1.0, float(np.max(np.abs(want))))
        for t in TYPES:
            if f"c{k}_{t}" in fixture:
                dev = float(np.max(np.abs(got - fixture[f"c{k}_{t}"]))) / scale
            else:  # raised, or a singular solve that went astray: the projector's result is 'lstsq'
                assert f"c{k}_{t}_raised" in fixture or f"c{k}_{t}_singular" in fixture, (k, t)
                dev = float(np.max(np.abs(got - want))) / scale
            worst = max(worst, dev)
            assert dev <= FP64_BAR, (k, keys, t, dev)
        if len(keys) == 1:  # (the lone period loses its mean: the reference's ones((1, p)))
            continue
        # the redistribution keeps the reconstruction
        n = int(np.lcm.reduce(keys))
        tile = lambda flat: sum(np.tile(s, n // p) for s, p in zip(np.split(flat, np.cumsum(keys)[:-1]), keys))  # noqa: E731
        assert np.max(np.abs(tile(got) - tile(np.concatenate(concatenate(keys, vals, wts))))) <= 1e-12 * scale * len(keys)
    print("closed form vs reference: worst relative difference", worst)


def test_raising_patterns_recorded(fixture):
    """'row reduction' raises on rank-1 matrices only; 'lu' / 'qr' misbehave only where their solve is singular."""
    for k, keys, _, _ in cases(fixture):
        rank1 = len(keys) == 1 or (len(keys) == 2 and np.gcd(keys[0], keys[1]) == 1)
        assert (f"c{k}_rr_raised" in fixture) == rank1
        assert f"c{k}_rr_singular" not in fixture
        for t in ("lu", "qr"):
            assert f"c{k}_{t}" in fixture or len(keys) >= 3, (k, t)
        for t in TYPES:
            if f"c{k}_{t}_raised" in fixture:
                assert str(fixture[f"c{k}_{t}_raised"]) == "LinAlgError"


def test_stack_pairwise_gcd_subspaces_bit_for_bit(fixture):
    from pyperiod_amd import QOPeriods, RamanujanPeriods

    seen = 0
    for k, keys, _, _ in cases(fixture):
        if f"c{k}_matrix" not in fixture:
            assert sum(keys) > 100
            continue
        want = fixture[f"c{k}_matrix"]
        got = QOPeriods.stack_pairwise_gcd_subspaces(np.array(keys))
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (k, keys)
        assert np.array_equal(RamanujanPeriods.stack_pairwise_gcd_subspaces(keys), want)
        seen += 1
    assert seen >= 10
    assert np.array_equal(QOPeriods.stack_pairwise_gcd_subspaces([]), np.ones((1, 1)))


def test_reduce_rows_keeps_a_maximal_independent_subset(fixture):
    from pyperiod_amd.QOPeriods import reduce_rows

    for k, keys, _, _ in cases(fixture):
        if f"c{k}_matrix" not in fixture:
            continue
        a = fixture[f"c{k}_matrix"]
        r = reduce_rows(a)
        rank = np.linalg.matrix_rank(a)
        assert r.ndim == 2 and r.shape[0] == rank == np.linalg.matrix_rank(r), (k, r.shape, rank)
        rows = {row.tobytes() for row in a}
        assert all(row.tobytes() in rows for row in r)  # a subset of the rows ...
        assert np.array_equal(r[0], a[0])  # ... in order, from the first
        # the same subset as the greedy rule of the reference: a row is kept iff it raises the rank of the rows above it
        kept, cur = [], 0
        for i in range(a.shape[0]):
            now = np.linalg.matrix_rank(a[: i + 1])
            if now > cur:
                kept.append(i)
                cur = now
        assert np.array_equal(r, a[kept]), k
    assert reduce_rows(np.ones((1, 5))).shape == (1, 5)


def test_header_and_binding_agree():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    m = re.search(r"#define PH_OP_QO_GET_PERIODS (\d+)", text)
    assert m and int(m.group(1)) == _ffi.PH_OP_QO_GET_PERIODS == 12
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int ph_qo_get_periods\((.*?)\);", code, flags=re.S)
    assert decl, "ph_qo_get_periods not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(_ffi.SIGNATURES["ph_qo_get_periods"]) == 13
    for a, ct in zip(args, _ffi.SIGNATURES["ph_qo_get_periods"]):
        if "*" in a:
            assert ct is ctypes.c_void_p, a
        elif a.startswith("int64_t"):
            assert ct is ctypes.c_int64, a
        elif a.startswith("unsigned"):
            assert ct is ctypes.c_uint, a
        else:
            assert ct is ctypes.c_int, a


def test_null_and_range_errors_without_gpu():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    per = np.array([[12, 18]], dtype=np.int32)
    rws = np.array([[12, 12]], dtype=np.int32)
    cnt = np.array([2], dtype=np.int32)
    wts = np.zeros((1, 24))
    out = np.zeros((1, 30))
    st = np.zeros(1, dtype=np.int32)
    a = lambda x: x.ctypes.data  # noqa: E731
    assert lib.ph_qo_get_periods(None, a(per), a(rws), a(cnt), 1, 2, a(wts), 24, 18, 30, 0, a(out), a(st)) == _ffi.PH_E_ARG
    assert b"ctx" in lib.ph_last_error()
    with pytest.raises(ValueError):
        _ffi.check(_ffi.PH_E_ARG)
    rec = (ctypes.c_int32 * _ffi.PH_PLAN_LEN)()
    prm = np.array([30, 18], dtype=np.int32)
    assert lib.ph_plan_info(None, _ffi.PH_OP_QO_GET_PERIODS, _ffi.PH_F64, 30, a(prm), 2, 0, ctypes.addressof(rec)) == _ffi.PH_E_ARG


class _FakeEngine:
    """Records what the class hands to PeriodEngine.qo_get_periods and answers with the numpy restatement."""

    def __init__(self):
        self.calls = []

    def qo_get_periods(self, periods, rows, counts, weights, max_period=None, ccap=None):
        self.calls.append((periods.copy(), rows.copy(), counts.copy(), weights.copy()))
        W = len(counts)
        ccap = int(max(periods[w, : counts[w]].sum() for w in range(W)))
        out = np.zeros((W, ccap))
        for w in range(W):
            k = int(counts[w])
            flat = closed_form([int(p) for p in periods[w, :k]], [int(r) for r in rows[w, :k]], weights[w])
            out[w, : flat.size] = flat
        return out, np.zeros(W, dtype=np.int32)


def test_class_packs_lists_counts_and_offsets(fixture, monkeypatch):
    from pyperiod_amd import QOPeriods, RamanujanPeriods

    import sys

    mod = sys.modules[QOPeriods.__module__]
    fake = _FakeEngine()
    monkeypatch.setattr(mod, "default_engine", lambda: fake)
    ks = (20, 6, 18)  # {12:12, 18:12}, a five-period dictionary, {12:12}
    dicts = [{str(p): r for p, r in zip(fixture[f"c{k}_keys"], fixture[f"c{k}_vals"])} for k in ks]
    wlist = [fixture[f"c{k}_weights"] for k in ks]
    dicts.append({"1": 36})  # the all-zero answer of find_periods: more rows than the period, one weight
    wlist.append(np.array([0]))
    qo = QOPeriods.__new__(QOPeriods)
    res = qo.get_periods(wlist, dicts)
    assert len(fake.calls) == 1  # one launch for the batch
    per, rws, cnt, wts = fake.calls[0]
    assert per.dtype == rws.dtype == cnt.dtype == np.int32 and wts.dtype == np.float64
    assert per.shape == rws.shape == (4, 5) and cnt.tolist() == [2, 5, 1, 1]
    assert wts.shape == (4, max(int(fixture[f"c{k}_vals"].sum()) for k in ks))
    for w, k in enumerate(ks):
        n = cnt[w]
        assert per[w, :n].tolist() == fixture[f"c{k}_keys"].tolist() and not per[w, n:].any()
        assert rws[w, :n].tolist() == fixture[f"c{k}_vals"].tolist() and not rws[w, n:].any()
        nw = int(fixture[f"c{k}_vals"].sum())
        assert np.array_equal(wts[w, :nw], fixture[f"c{k}_weights"]) and not wts[w, nw:].any()  # blocks back to back
    assert per[3, 0] == 1 and rws[3, 0] == 1 and wts[3, 0] == 0.0  # normalised to rows <= period
    assert isinstance(res, list) and len(res) == 4
    for w, k in enumerate(ks):
        assert isinstance(res[w], tuple) and [len(a) for a in res[w]] == fixture[f"c{k}_keys"].tolist()
        assert all(a.dtype == np.float64 for a in res[w])
        want = fixture[f"c{k}_lstsq"]
        assert np.max(np.abs(np.concatenate(res[w]) - want)) <= FP64_BAR * max(1.0, np.max(np.abs(want)))
    assert len(res[3]) == 1 and np.array_equal(res[3][0], np.zeros(1))
    # the 1-D call is a batch of one and returns the tuple itself; every decomp_type gives the projector's result
    for t in ("row reduction", "lu", "qr", "lstsq"):
        one = qo.get_periods(wlist[0], dicts[0], decomp_type=t)
        assert isinstance(one, tuple) and all(np.array_equal(a, b) for a, b in zip(one, res[0]))
    assert fake.calls[-1][0].shape == (1, 2)
    # RamanujanPeriods inherits the method
    assert RamanujanPeriods.get_periods is QOPeriods.get_periods or issubclass(RamanujanPeriods, QOPeriods)


def test_class_raises_value_error_on_an_empty_dictionary(monkeypatch):
    import sys

    from pyperiod_amd import QOPeriods

    monkeypatch.setattr(sys.modules[QOPeriods.__module__], "default_engine", lambda: _FakeEngine())
    qo = QOPeriods.__new__(QOPeriods)
    with pytest.raises(ValueError):
        qo.get_periods(np.zeros(0), {})
    with pytest.raises(ValueError, match="row 1"):
        qo.get_periods([np.ones(3), np.zeros(0)], [{"3": 3}, {}])
    with pytest.raises(ValueError, match="row 0"):  # concatenate_periods' own broadcast error, with the row named
        qo.get_periods([np.ones(5)], [{"2": 5}])
