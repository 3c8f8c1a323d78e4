"""Every entry point at the sample counts N* where its launch plan changes: the variant (one window or a window pair
per workgroup; FFT, chirp or direct spectrum), the window's and the second buffer's placement (LDS or HBM workspace),
m_best's small_means, the block size, Ramanujan's wave count and pad.  The switch points are found on the host with
engine.plan_info (ph_plan_info, the planning functions the launches use), the states visited are pinned against
hand-written sets, and at N* - 1, N*, N* + 1 the results are checked against the oracle (fp64; fp32 on the fp32-rounded
input at the DESIGN.md section 4 bar), against an engine that keeps every window in HBM (PH_HBM_WINDOW=1) and, at the
pair boundaries, against the one-window kernels (PH_STEP1_PAIR=0, PH_S2L_PAIR=0, PH_BC_PAIR=0)."""

import os
import time

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po

pytestmark = pytest.mark.gpu

MAX_LEN = 300  # candidate periods / n_periods / max_p: keeps the oracle cheap at N = 41 000
NUM = 3
HI = 45000  # past the last switch (fp32 windows leave the LDS near 40 600)
FLAGS = {"plain": (False, False), "trunc": (True, False), "orth": (False, True)}
TOL64, TOL32 = 1e-10, 1e-4
# against the all-HBM engine: fp64 1e-12; fp32 1e-5, because that engine's m_best step 1 runs without small_means
# (as every window too long for it does): split_row_means rounds a short winner's float sums differently, and the
# later periods' bases (W, num, N) carry that rounding through two subtractions (3.4e-6 seen at N = 39 800)
TOL_HBM = {np.float64: 1e-12, np.float32: 1e-5}


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

    e = dict(eng=default_engine(), hbm=_engine(PH_HBM_WINDOW=1),
             one=_engine(PH_STEP1_PAIR=0, PH_S2L_PAIR=0, PH_BC_PAIR=0))
    yield e
    e["hbm"].close()
    e["one"].close()


# ---------------------------------------------------------------------------- plan states and switch points
def _names():
    from pyperiod_amd import _ffi

    var = {_ffi.PH_PLAN_ONE: "one", _ffi.PH_PLAN_PAIR: "pair", _ffi.PH_PLAN_FFT: "fft", _ffi.PH_PLAN_CHIRP: "chirp",
           _ffi.PH_PLAN_DIRECT: "direct"}
    place = {_ffi.PH_PLAN_NONE: "-", _ffi.PH_PLAN_LDS: "lds", _ffi.PH_PLAN_HBM: "hbm"}
    return var, place


def state(recs):
    """Everything a plan decides except the LDS byte count (which moves with every N): one string per kernel."""
    var, place = _names()
    out = []
    for r in recs:
        s = f"{var[r.variant]} win={place[r.window]} buf={place[r.second]} b={r.block}"
        if r.small_means:
            s += " sm"
        if r.waves:
            s += f" nw={r.waves} pad={r.pad}"
        out.append(s)
    return " / ".join(out)


OPS = {  # op -> (params as a function of N, flag modes it has)
    "project": (lambda n: (MAX_LEN,), ("plain", "trunc", "orth")),
    "sweep": (lambda n: (2, MAX_LEN, 0), ("plain", "trunc", "orth")),
    "m_best": (lambda n: (NUM, 2, MAX_LEN), ("plain", "trunc", "orth")),
    "small_to_large": (lambda n: (MAX_LEN,), ("plain", "trunc", "orth")),
    "best_correlation": (lambda n: (MAX_LEN,), ("plain", "trunc", "orth")),
    "best_frequency": (lambda n: (MAX_LEN,), ("plain",)),
    "orth_powers": (lambda n: (MAX_LEN,), ("plain",)),
    "fold_sums": (lambda n: (), ("plain",)),
}
RAM_Q = {"q64": lambda n: (2, 64), "q128": lambda n: (2, 128), "q512": lambda n: (2, 512), "qN3": lambda n: (2, n // 3)}


def plan_of(eng, op, n, params, dtype, mode):
    trunc, orth = FLAGS[mode]
    return eng.plan_info(op, n, params, dtype, trunc, orth)


def switch_points(f, lo, hi, step=64):
    """Every x in (lo, hi] with f(x) != f(x - 1), for a piecewise-constant f: a scan in steps of `step`, then
    bisection inside each step that changes; the scan restarts at every switch found."""
    out = []
    x, fx = lo, f(lo)
    while x < hi:
        m = min(x + step, hi)
        fm = f(m)
        if fm == fx:
            x = m
            continue
        a, b = x, m  # f(a) == fx != f(b)
        while b - a > 1:
            c = (a + b) // 2
            if f(c) == fx:
                a = c
            else:
                b = c
        out.append(b)
        x, fx = b, f(b)
    return out


def scan(eng, op, dtype, mode, params=None, lo=3 * MAX_LEN + 3, hi=HI):
    params = params or OPS[op][0]
    return switch_points(lambda n: state(plan_of(eng, op, n, params(n), dtype, mode)), lo, hi)


def _signal(n, seed, dtype=np.float64):
    """Integer periods 7 (short: split_row_means and the chains below 64), 60 and 283 (near MAX_LEN), amplitudes well
    apart, a little noise: every selection has a clear margin."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.02 * rng.standard_normal(n)
    for amp, p in ((1.0, 283), (0.7, 7), (0.45, 60)):
        x += amp * np.sin(2 * np.pi * t / p + rng.uniform(0, 2 * np.pi))
    return x.astype(dtype)


def _run(eng, op, x, mode):
    """One call of `op` on the (W, N) batch x -> (lists that must match exactly, float arrays)."""
    trunc, orth = FLAGS[mode]
    if op == "project":
        return [], [eng.project_batch(x, [7, 60, MAX_LEN], trunc, orth)]
    if op == "sweep":
        return [], [eng.sweep(x, 2, MAX_LEN, 0, trunc, orth)]
    if op == "m_best":
        per, pw, bs, st = eng.m_best(x, NUM, MAX_LEN, 2, False, trunc, orth)
        return [per, st], [pw, bs]
    if op == "small_to_large":
        cnt, per, pw, bs, st = eng.small_to_large(x, 0.05, MAX_LEN, trunc, orth)
        k = int(cnt.max())
        return [cnt, per[:, :k], st], [pw[:, :k], bs[:, :k]]
    if op == "best_correlation":
        per, nr, bs, st = eng.best_correlation(x, NUM, MAX_LEN, 0.01, trunc, orth)
        return [per, st], [nr, bs]
    if op == "best_frequency":
        per, pw, bs, st = eng.best_frequency(x, MAX_LEN, NUM, trunc, orth)
        return [per, st], [pw, bs]
    if op == "orth_powers":
        return [], [eng.orth_powers(x, MAX_LEN, True)]
    if op == "fold_sums":
        return [], [eng.fold_sums(x, [7, 60, MAX_LEN], [7, 59, MAX_LEN])]
    raise AssertionError(op)


def _oracle(op, x, mode):
    """The oracle's answer for one window in _run's layout (float64)."""
    trunc, orth = FLAGS[mode]
    x = x.astype(np.float64)
    if op == "project":
        return [], [np.stack([po.project(x, p, trunc, orth) for p in (7, 60, MAX_LEN)])]
    if op == "sweep":
        return [], [po.sweep_norms(x, 2, MAX_LEN, trunc=trunc, orth=orth)]
    if op == "m_best":
        per, pw, bs = po.m_best(x, NUM, MAX_LEN, 2, False, trunc, orth)
        return [np.asarray(per), 0], [pw, bs]
    if op == "small_to_large":
        per, pw, bs = po.small_to_large(x, 0.05, MAX_LEN, trunc, orth)
        return [len(per), np.asarray(per, dtype=np.int64), 0], [pw, np.asarray(bs)]
    if op == "best_correlation":
        per, nr, bs = po.best_correlation(x, NUM, MAX_LEN, 0.01, trunc, orth)
        return [np.asarray(per), 0], [nr, bs]
    if op == "best_frequency":
        per, pw, bs = po.best_frequency(x, MAX_LEN, NUM, trunc, orth)
        return [np.asarray(per), 0], [pw, bs]
    if op == "orth_powers":
        return [], [po.orth_powers(x, MAX_LEN, True)]
    if op == "fold_sums":
        return [], [np.concatenate([po.fold_sums(x, p)[:k] for p, k in ((7, 7), (60, 59), (MAX_LEN, MAX_LEN))])]
    raise AssertionError(op)


def _same_lists(a, b, what):
    assert len(a) == len(b), what
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u).astype(np.int64).reshape(-1), np.asarray(v).astype(np.int64).reshape(-1)), \
            (what, u, v)


def check_triple(engines, op, dtype, mode, nstar, pair=False):
    """N* - 1, N*, N* + 1: the plan changes inside the triple; every result equals the all-HBM engine's (and the
    one-window engine's at a pair boundary) and the oracle's."""
    eng = engines["eng"]
    params = OPS[op][0]
    plans = {state(plan_of(eng, op, n, params(n), dtype, mode)) for n in (nstar - 1, nstar, nstar + 1)}
    assert len(plans) == 2, (op, dtype, mode, nstar, plans)
    others = ["hbm"] + (["one"] if pair else [])
    for n in (nstar - 1, nstar, nstar + 1):
        what = (op, dtype.__name__, mode, nstar, n)
        w = 3 if pair else 1  # odd batch at a pair boundary: the last window runs unpaired
        x = np.stack([_signal(n, 1000 * nstar + 10 * n + i, dtype) for i in range(w)])
        lists, vals = _run(eng, op, x, mode)
        for name in others:
            l2, v2 = _run(engines[name], op, x, mode)
            _same_lists(lists, l2, (what, name))
            for a, b in zip(vals, v2):
                assert rel_err(a, b) <= TOL_HBM[dtype], (what, name, rel_err(a, b))
        for i in range(w):
            rl, rv = _oracle(op, x[i], mode)
            _same_lists([u[i] for u in lists], rl, (what, "oracle", i))
            tol = TOL64 if dtype == np.float64 else TOL32
            for a, b in zip(vals, rv):
                a = np.asarray(a[i], dtype=np.float64)
                b = np.asarray(b, dtype=np.float64).reshape(a.shape)
                if op == "project" and dtype == np.float64 and not FLAGS[mode][1]:
                    assert np.array_equal(a, b), what  # row-order sums, one division: bit-identical
                assert rel_err(a, b) <= tol, (what, i, rel_err(a, b))


EXPECTED = {  # (op, dtype, flag mode or Ramanujan range) -> [(N*, plan at N* - 1, plan at N*)]
    ('project', 'float64', 'plain'): [
        (20181, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (20481, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('project', 'float64', 'trunc'): [
        (20181, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (20481, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('project', 'float64', 'orth'): [
        (10241, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (20481, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('project', 'float32', 'plain'): [
        (40661, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (40961, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('project', 'float32', 'trunc'): [
        (40661, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (40961, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('project', 'float32', 'orth'): [
        (20481, 'one win=lds buf=lds b=256',
         'one win=lds buf=hbm b=256'),
        (40961, 'one win=lds buf=hbm b=256',
         'one win=hbm buf=hbm b=256'),
    ],
    ('sweep', 'float64', 'plain'): [
        (6537, 'one win=lds buf=- b=512',
         'one win=lds buf=- b=1024'),
        (20191, 'one win=lds buf=- b=1024',
         'one win=hbm buf=- b=1024'),
    ],
    ('sweep', 'float64', 'trunc'): [
        (3269, 'one win=lds buf=lds b=512',
         'one win=lds buf=lds b=1024'),
        (10095, 'one win=lds buf=lds b=1024',
         'one win=lds buf=hbm b=1024'),
        (20191, 'one win=lds buf=hbm b=1024',
         'one win=hbm buf=hbm b=1024'),
    ],
    ('sweep', 'float64', 'orth'): [
        (3269, 'one win=lds buf=lds b=512',
         'one win=lds buf=lds b=1024'),
        (10095, 'one win=lds buf=lds b=1024',
         'one win=lds buf=hbm b=1024'),
        (20191, 'one win=lds buf=hbm b=1024',
         'one win=hbm buf=hbm b=1024'),
    ],
    ('sweep', 'float32', 'plain'): [
        (13329, 'one win=lds buf=- b=512',
         'one win=lds buf=- b=1024'),
        (40637, 'one win=lds buf=- b=1024',
         'one win=hbm buf=- b=1024'),
    ],
    ('sweep', 'float32', 'trunc'): [
        (6665, 'one win=lds buf=lds b=512',
         'one win=lds buf=lds b=1024'),
        (20317, 'one win=lds buf=lds b=1024',
         'one win=lds buf=hbm b=1024'),
        (40637, 'one win=lds buf=hbm b=1024',
         'one win=hbm buf=hbm b=1024'),
    ],
    ('sweep', 'float32', 'orth'): [
        (6665, 'one win=lds buf=lds b=512',
         'one win=lds buf=lds b=1024'),
        (20317, 'one win=lds buf=lds b=1024',
         'one win=lds buf=hbm b=1024'),
        (40637, 'one win=lds buf=hbm b=1024',
         'one win=hbm buf=hbm b=1024'),
    ],
    ('m_best', 'float64', 'plain'): [
        (9509, 'pair win=lds buf=- b=1024 / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 sm / one win=lds buf=hbm b=512'),
        (19389, 'one win=lds buf=- b=1024 sm / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 / one win=lds buf=hbm b=512'),
        (20073, 'one win=lds buf=- b=1024 / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 / one win=hbm buf=hbm b=512'),
        (20157, 'one win=lds buf=- b=1024 / one win=hbm buf=hbm b=512',
         'one win=hbm buf=- b=1024 / one win=hbm buf=hbm b=512'),
    ],
    ('m_best', 'float64', 'trunc'): [
        (3072, 'one win=lds buf=lds b=512 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256'),
        (10037, 'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256'),
        (10079, 'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256'),
        (20073, 'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
        (20157, 'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256',
         'one win=hbm buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
    ],
    ('m_best', 'float64', 'orth'): [
        (3072, 'one win=lds buf=lds b=512 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256'),
        (10037, 'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256'),
        (10079, 'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256'),
        (20073, 'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
        (20157, 'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256',
         'one win=hbm buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
    ],
    ('m_best', 'float32', 'plain'): [
        (3072, 'one win=lds buf=- b=512 sm / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 sm / one win=lds buf=hbm b=512'),
        (39801, 'one win=lds buf=- b=1024 sm / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 / one win=lds buf=hbm b=512'),
        (40401, 'one win=lds buf=- b=1024 / one win=lds buf=hbm b=512',
         'one win=lds buf=- b=1024 / one win=hbm buf=hbm b=512'),
        (40569, 'one win=lds buf=- b=1024 / one win=hbm buf=hbm b=512',
         'one win=hbm buf=- b=1024 / one win=hbm buf=hbm b=512'),
    ],
    ('m_best', 'float32', 'trunc'): [
        (3072, 'one win=lds buf=lds b=512 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256'),
        (20201, 'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256'),
        (20285, 'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256'),
        (40401, 'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
        (40569, 'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256',
         'one win=hbm buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
    ],
    ('m_best', 'float32', 'orth'): [
        (3072, 'one win=lds buf=lds b=512 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256'),
        (20201, 'one win=lds buf=lds b=1024 / one win=lds buf=lds b=256',
         'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256'),
        (20285, 'one win=lds buf=lds b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256'),
        (40401, 'one win=lds buf=hbm b=1024 / one win=lds buf=hbm b=256',
         'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
        (40569, 'one win=lds buf=hbm b=1024 / one win=hbm buf=hbm b=256',
         'one win=hbm buf=hbm b=1024 / one win=hbm buf=hbm b=256'),
    ],
    ('small_to_large', 'float64', 'plain'): [
        (9705, 'pair win=lds buf=- b=1024',
         'one win=lds buf=- b=512'),
        (19647, 'one win=lds buf=- b=512',
         'one win=hbm buf=- b=512'),
    ],
    ('small_to_large', 'float64', 'trunc'): [
        (10079, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (20159, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('small_to_large', 'float64', 'orth'): [
        (10079, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (20159, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('small_to_large', 'float32', 'plain'): [
        (40061, 'one win=lds buf=- b=512',
         'one win=hbm buf=- b=512'),
    ],
    ('small_to_large', 'float32', 'trunc'): [
        (20285, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (40573, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('small_to_large', 'float32', 'orth'): [
        (20285, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (40573, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('best_correlation', 'float64', 'plain'): [
        (9901, 'pair win=lds buf=- b=1024',
         'one win=lds buf=- b=512'),
        (19783, 'one win=lds buf=- b=512',
         'one win=hbm buf=- b=512'),
    ],
    ('best_correlation', 'float64', 'trunc'): [
        (9891, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (19783, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('best_correlation', 'float64', 'orth'): [
        (9891, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (19783, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('best_correlation', 'float32', 'plain'): [
        (39821, 'one win=lds buf=- b=512',
         'one win=hbm buf=- b=512'),
    ],
    ('best_correlation', 'float32', 'trunc'): [
        (19909, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (39821, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('best_correlation', 'float32', 'orth'): [
        (19909, 'one win=lds buf=lds b=512',
         'one win=lds buf=hbm b=512'),
        (39821, 'one win=lds buf=hbm b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('best_frequency', 'float64', 'plain'): [
        (10225, 'chirp win=hbm buf=- b=512 / one win=lds buf=lds b=512',
         'chirp win=hbm buf=- b=512 / one win=lds buf=hbm b=512'),
        (20449, 'chirp win=hbm buf=- b=512 / one win=lds buf=hbm b=512',
         'chirp win=hbm buf=- b=512 / one win=hbm buf=hbm b=512'),
    ],
    ('best_frequency', 'float32', 'plain'): [
        (20449, 'chirp win=hbm buf=- b=512 / one win=lds buf=lds b=512',
         'chirp win=hbm buf=- b=512 / one win=lds buf=hbm b=512'),
        (40897, 'chirp win=hbm buf=- b=512 / one win=lds buf=hbm b=512',
         'chirp win=hbm buf=- b=512 / one win=hbm buf=hbm b=512'),
    ],
    ('orth_powers', 'float64', 'plain'): [
        (10091, 'one win=lds buf=lds b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('orth_powers', 'float32', 'plain'): [
        (13453, 'one win=lds buf=lds b=512',
         'one win=hbm buf=hbm b=512'),
    ],
    ('fold_sums', 'float64', 'plain'): [
        (20481, 'one win=lds buf=- b=256',
         'one win=hbm buf=- b=256'),
    ],
    ('fold_sums', 'float32', 'plain'): [
        (40961, 'one win=lds buf=- b=256',
         'one win=hbm buf=- b=256'),
    ],
    ('ramanujan', 'float64', 'q64'): [
        (18689, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=960 nw=15 pad=256'),
        (18785, 'one win=lds buf=- b=960 nw=15 pad=256',
         'one win=lds buf=- b=896 nw=14 pad=256'),
        (18881, 'one win=lds buf=- b=896 nw=14 pad=256',
         'one win=lds buf=- b=832 nw=13 pad=256'),
        (18977, 'one win=lds buf=- b=832 nw=13 pad=256',
         'one win=lds buf=- b=768 nw=12 pad=256'),
        (19073, 'one win=lds buf=- b=768 nw=12 pad=256',
         'one win=lds buf=- b=704 nw=11 pad=256'),
        (19169, 'one win=lds buf=- b=704 nw=11 pad=256',
         'one win=lds buf=- b=640 nw=10 pad=256'),
        (19265, 'one win=lds buf=- b=640 nw=10 pad=256',
         'one win=lds buf=- b=576 nw=9 pad=256'),
        (19361, 'one win=lds buf=- b=576 nw=9 pad=256',
         'one win=lds buf=- b=512 nw=8 pad=256'),
        (19457, 'one win=lds buf=- b=512 nw=8 pad=256',
         'one win=lds buf=- b=448 nw=7 pad=256'),
        (19553, 'one win=lds buf=- b=448 nw=7 pad=256',
         'one win=lds buf=- b=384 nw=6 pad=256'),
        (19649, 'one win=lds buf=- b=384 nw=6 pad=256',
         'one win=lds buf=- b=320 nw=5 pad=256'),
        (19745, 'one win=lds buf=- b=320 nw=5 pad=256',
         'one win=lds buf=- b=256 nw=4 pad=256'),
        (19841, 'one win=lds buf=- b=256 nw=4 pad=256',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
    ('ramanujan', 'float32', 'q64'): [
        (37633, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=960 nw=15 pad=256'),
        (37825, 'one win=lds buf=- b=960 nw=15 pad=256',
         'one win=lds buf=- b=896 nw=14 pad=256'),
        (38017, 'one win=lds buf=- b=896 nw=14 pad=256',
         'one win=lds buf=- b=832 nw=13 pad=256'),
        (38209, 'one win=lds buf=- b=832 nw=13 pad=256',
         'one win=lds buf=- b=768 nw=12 pad=256'),
        (38401, 'one win=lds buf=- b=768 nw=12 pad=256',
         'one win=lds buf=- b=704 nw=11 pad=256'),
        (38593, 'one win=lds buf=- b=704 nw=11 pad=256',
         'one win=lds buf=- b=640 nw=10 pad=256'),
        (38785, 'one win=lds buf=- b=640 nw=10 pad=256',
         'one win=lds buf=- b=576 nw=9 pad=256'),
        (38977, 'one win=lds buf=- b=576 nw=9 pad=256',
         'one win=lds buf=- b=512 nw=8 pad=256'),
        (39169, 'one win=lds buf=- b=512 nw=8 pad=256',
         'one win=lds buf=- b=448 nw=7 pad=256'),
        (39361, 'one win=lds buf=- b=448 nw=7 pad=256',
         'one win=lds buf=- b=384 nw=6 pad=256'),
        (39553, 'one win=lds buf=- b=384 nw=6 pad=256',
         'one win=lds buf=- b=320 nw=5 pad=256'),
        (39745, 'one win=lds buf=- b=320 nw=5 pad=256',
         'one win=lds buf=- b=256 nw=4 pad=256'),
        (39937, 'one win=lds buf=- b=256 nw=4 pad=256',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
    ('ramanujan', 'float64', 'q128'): [
        (17153, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=1024 nw=16 pad=0'),
        (17409, 'one win=lds buf=- b=1024 nw=16 pad=0',
         'one win=lds buf=- b=960 nw=15 pad=0'),
        (17601, 'one win=lds buf=- b=960 nw=15 pad=0',
         'one win=lds buf=- b=896 nw=14 pad=0'),
        (17793, 'one win=lds buf=- b=896 nw=14 pad=0',
         'one win=lds buf=- b=832 nw=13 pad=0'),
        (17985, 'one win=lds buf=- b=832 nw=13 pad=0',
         'one win=lds buf=- b=768 nw=12 pad=0'),
        (18177, 'one win=lds buf=- b=768 nw=12 pad=0',
         'one win=lds buf=- b=704 nw=11 pad=0'),
        (18369, 'one win=lds buf=- b=704 nw=11 pad=0',
         'one win=lds buf=- b=640 nw=10 pad=0'),
        (18561, 'one win=lds buf=- b=640 nw=10 pad=0',
         'one win=lds buf=- b=576 nw=9 pad=0'),
        (18753, 'one win=lds buf=- b=576 nw=9 pad=0',
         'one win=lds buf=- b=512 nw=8 pad=0'),
        (18945, 'one win=lds buf=- b=512 nw=8 pad=0',
         'one win=lds buf=- b=448 nw=7 pad=0'),
        (19137, 'one win=lds buf=- b=448 nw=7 pad=0',
         'one win=lds buf=- b=384 nw=6 pad=0'),
        (19329, 'one win=lds buf=- b=384 nw=6 pad=0',
         'one win=lds buf=- b=320 nw=5 pad=0'),
        (19521, 'one win=lds buf=- b=320 nw=5 pad=0',
         'one win=lds buf=- b=256 nw=4 pad=0'),
        (19713, 'one win=lds buf=- b=256 nw=4 pad=0',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
    ('ramanujan', 'float32', 'q128'): [
        (34561, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=1024 nw=16 pad=0'),
        (34817, 'one win=lds buf=- b=1024 nw=16 pad=0',
         'one win=lds buf=- b=960 nw=15 pad=256'),
        (34945, 'one win=lds buf=- b=960 nw=15 pad=256',
         'one win=lds buf=- b=960 nw=15 pad=0'),
        (35201, 'one win=lds buf=- b=960 nw=15 pad=0',
         'one win=lds buf=- b=896 nw=14 pad=256'),
        (35329, 'one win=lds buf=- b=896 nw=14 pad=256',
         'one win=lds buf=- b=896 nw=14 pad=0'),
        (35585, 'one win=lds buf=- b=896 nw=14 pad=0',
         'one win=lds buf=- b=832 nw=13 pad=256'),
        (35713, 'one win=lds buf=- b=832 nw=13 pad=256',
         'one win=lds buf=- b=832 nw=13 pad=0'),
        (35969, 'one win=lds buf=- b=832 nw=13 pad=0',
         'one win=lds buf=- b=768 nw=12 pad=256'),
        (36097, 'one win=lds buf=- b=768 nw=12 pad=256',
         'one win=lds buf=- b=768 nw=12 pad=0'),
        (36353, 'one win=lds buf=- b=768 nw=12 pad=0',
         'one win=lds buf=- b=704 nw=11 pad=256'),
        (36481, 'one win=lds buf=- b=704 nw=11 pad=256',
         'one win=lds buf=- b=704 nw=11 pad=0'),
        (36737, 'one win=lds buf=- b=704 nw=11 pad=0',
         'one win=lds buf=- b=640 nw=10 pad=256'),
        (36865, 'one win=lds buf=- b=640 nw=10 pad=256',
         'one win=lds buf=- b=640 nw=10 pad=0'),
        (37121, 'one win=lds buf=- b=640 nw=10 pad=0',
         'one win=lds buf=- b=576 nw=9 pad=256'),
        (37249, 'one win=lds buf=- b=576 nw=9 pad=256',
         'one win=lds buf=- b=576 nw=9 pad=0'),
        (37505, 'one win=lds buf=- b=576 nw=9 pad=0',
         'one win=lds buf=- b=512 nw=8 pad=256'),
        (37633, 'one win=lds buf=- b=512 nw=8 pad=256',
         'one win=lds buf=- b=512 nw=8 pad=0'),
        (37889, 'one win=lds buf=- b=512 nw=8 pad=0',
         'one win=lds buf=- b=448 nw=7 pad=256'),
        (38017, 'one win=lds buf=- b=448 nw=7 pad=256',
         'one win=lds buf=- b=448 nw=7 pad=0'),
        (38273, 'one win=lds buf=- b=448 nw=7 pad=0',
         'one win=lds buf=- b=384 nw=6 pad=256'),
        (38401, 'one win=lds buf=- b=384 nw=6 pad=256',
         'one win=lds buf=- b=384 nw=6 pad=0'),
        (38657, 'one win=lds buf=- b=384 nw=6 pad=0',
         'one win=lds buf=- b=320 nw=5 pad=256'),
        (38785, 'one win=lds buf=- b=320 nw=5 pad=256',
         'one win=lds buf=- b=320 nw=5 pad=0'),
        (39041, 'one win=lds buf=- b=320 nw=5 pad=0',
         'one win=lds buf=- b=256 nw=4 pad=256'),
        (39169, 'one win=lds buf=- b=256 nw=4 pad=256',
         'one win=lds buf=- b=256 nw=4 pad=0'),
        (39425, 'one win=lds buf=- b=256 nw=4 pad=0',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
    ('ramanujan', 'float64', 'q512'): [
        (7937, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=1024 nw=16 pad=0'),
        (8193, 'one win=lds buf=- b=1024 nw=16 pad=0',
         'one win=lds buf=- b=960 nw=15 pad=256'),
        (8705, 'one win=lds buf=- b=960 nw=15 pad=256',
         'one win=lds buf=- b=960 nw=15 pad=0'),
        (8961, 'one win=lds buf=- b=960 nw=15 pad=0',
         'one win=lds buf=- b=896 nw=14 pad=256'),
        (9473, 'one win=lds buf=- b=896 nw=14 pad=256',
         'one win=lds buf=- b=896 nw=14 pad=0'),
        (9729, 'one win=lds buf=- b=896 nw=14 pad=0',
         'one win=lds buf=- b=832 nw=13 pad=256'),
        (10241, 'one win=lds buf=- b=832 nw=13 pad=256',
         'one win=lds buf=- b=832 nw=13 pad=0'),
        (10497, 'one win=lds buf=- b=832 nw=13 pad=0',
         'one win=lds buf=- b=768 nw=12 pad=256'),
        (11009, 'one win=lds buf=- b=768 nw=12 pad=256',
         'one win=lds buf=- b=768 nw=12 pad=0'),
        (11265, 'one win=lds buf=- b=768 nw=12 pad=0',
         'one win=lds buf=- b=704 nw=11 pad=256'),
        (11777, 'one win=lds buf=- b=704 nw=11 pad=256',
         'one win=lds buf=- b=704 nw=11 pad=0'),
        (12033, 'one win=lds buf=- b=704 nw=11 pad=0',
         'one win=lds buf=- b=640 nw=10 pad=256'),
        (12545, 'one win=lds buf=- b=640 nw=10 pad=256',
         'one win=lds buf=- b=640 nw=10 pad=0'),
        (12801, 'one win=lds buf=- b=640 nw=10 pad=0',
         'one win=lds buf=- b=576 nw=9 pad=256'),
        (13313, 'one win=lds buf=- b=576 nw=9 pad=256',
         'one win=lds buf=- b=576 nw=9 pad=0'),
        (13569, 'one win=lds buf=- b=576 nw=9 pad=0',
         'one win=lds buf=- b=512 nw=8 pad=256'),
        (14081, 'one win=lds buf=- b=512 nw=8 pad=256',
         'one win=lds buf=- b=512 nw=8 pad=0'),
        (14337, 'one win=lds buf=- b=512 nw=8 pad=0',
         'one win=lds buf=- b=448 nw=7 pad=256'),
        (14849, 'one win=lds buf=- b=448 nw=7 pad=256',
         'one win=lds buf=- b=448 nw=7 pad=0'),
        (15105, 'one win=lds buf=- b=448 nw=7 pad=0',
         'one win=lds buf=- b=384 nw=6 pad=256'),
        (15617, 'one win=lds buf=- b=384 nw=6 pad=256',
         'one win=lds buf=- b=384 nw=6 pad=0'),
        (15873, 'one win=lds buf=- b=384 nw=6 pad=0',
         'one win=lds buf=- b=320 nw=5 pad=256'),
        (16385, 'one win=lds buf=- b=320 nw=5 pad=256',
         'one win=lds buf=- b=320 nw=5 pad=0'),
        (16641, 'one win=lds buf=- b=320 nw=5 pad=0',
         'one win=lds buf=- b=256 nw=4 pad=256'),
        (17153, 'one win=lds buf=- b=256 nw=4 pad=256',
         'one win=lds buf=- b=256 nw=4 pad=0'),
        (17409, 'one win=lds buf=- b=256 nw=4 pad=0',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
    ('ramanujan', 'float32', 'q512'): [
        (16129, 'one win=lds buf=- b=1024 nw=16 pad=256',
         'one win=lds buf=- b=1024 nw=16 pad=0'),
        (16385, 'one win=lds buf=- b=1024 nw=16 pad=0',
         'one win=lds buf=- b=960 nw=15 pad=256'),
        (17665, 'one win=lds buf=- b=960 nw=15 pad=256',
         'one win=lds buf=- b=960 nw=15 pad=0'),
        (17921, 'one win=lds buf=- b=960 nw=15 pad=0',
         'one win=lds buf=- b=896 nw=14 pad=256'),
        (19201, 'one win=lds buf=- b=896 nw=14 pad=256',
         'one win=lds buf=- b=896 nw=14 pad=0'),
        (19457, 'one win=lds buf=- b=896 nw=14 pad=0',
         'one win=lds buf=- b=832 nw=13 pad=256'),
        (20737, 'one win=lds buf=- b=832 nw=13 pad=256',
         'one win=lds buf=- b=832 nw=13 pad=0'),
        (20993, 'one win=lds buf=- b=832 nw=13 pad=0',
         'one win=lds buf=- b=768 nw=12 pad=256'),
        (22273, 'one win=lds buf=- b=768 nw=12 pad=256',
         'one win=lds buf=- b=768 nw=12 pad=0'),
        (22529, 'one win=lds buf=- b=768 nw=12 pad=0',
         'one win=lds buf=- b=704 nw=11 pad=256'),
        (23809, 'one win=lds buf=- b=704 nw=11 pad=256',
         'one win=lds buf=- b=704 nw=11 pad=0'),
        (24065, 'one win=lds buf=- b=704 nw=11 pad=0',
         'one win=lds buf=- b=640 nw=10 pad=256'),
        (25345, 'one win=lds buf=- b=640 nw=10 pad=256',
         'one win=lds buf=- b=640 nw=10 pad=0'),
        (25601, 'one win=lds buf=- b=640 nw=10 pad=0',
         'one win=lds buf=- b=576 nw=9 pad=256'),
        (26881, 'one win=lds buf=- b=576 nw=9 pad=256',
         'one win=lds buf=- b=576 nw=9 pad=0'),
        (27137, 'one win=lds buf=- b=576 nw=9 pad=0',
         'one win=lds buf=- b=512 nw=8 pad=256'),
        (28417, 'one win=lds buf=- b=512 nw=8 pad=256',
         'one win=lds buf=- b=512 nw=8 pad=0'),
        (28673, 'one win=lds buf=- b=512 nw=8 pad=0',
         'one win=lds buf=- b=448 nw=7 pad=256'),
        (29953, 'one win=lds buf=- b=448 nw=7 pad=256',
         'one win=lds buf=- b=448 nw=7 pad=0'),
        (30209, 'one win=lds buf=- b=448 nw=7 pad=0',
         'one win=lds buf=- b=384 nw=6 pad=256'),
        (31489, 'one win=lds buf=- b=384 nw=6 pad=256',
         'one win=lds buf=- b=384 nw=6 pad=0'),
        (31745, 'one win=lds buf=- b=384 nw=6 pad=0',
         'one win=lds buf=- b=320 nw=5 pad=256'),
        (33025, 'one win=lds buf=- b=320 nw=5 pad=256',
         'one win=lds buf=- b=320 nw=5 pad=0'),
        (33281, 'one win=lds buf=- b=320 nw=5 pad=0',
         'one win=lds buf=- b=256 nw=4 pad=256'),
        (34561, 'one win=lds buf=- b=256 nw=4 pad=256',
         'one win=lds buf=- b=256 nw=4 pad=0'),
        (34817, 'one win=lds buf=- b=256 nw=4 pad=0',
         'one win=hbm buf=- b=1024 nw=16 pad=256'),
    ],
}


@pytest.mark.parametrize("op", list(OPS))
def test_plan_switch_points(engines, op):
    """Host only: the switch points and the plan states on both sides of each, per dtype and flag mode, are the pinned
    ones (a change that removes or shifts a boundary must update this table on purpose)."""
    eng = engines["eng"]
    for dtype in (np.float64, np.float32):
        for mode in OPS[op][1]:
            got = [(n, state(plan_of(eng, op, n - 1, OPS[op][0](n - 1), dtype, mode)),
                    state(plan_of(eng, op, n, OPS[op][0](n), dtype, mode))) for n in scan(eng, op, dtype, mode)]
            assert got == EXPECTED[(op, dtype.__name__, mode)], (op, dtype.__name__, mode, got)
            hbm = {state(plan_of(engines["hbm"], op, n, OPS[op][0](n), dtype, mode)) for n, _, _ in got}
            assert all("win=lds" not in s and "buf=lds" not in s and "pair" not in s for s in hbm), hbm


@pytest.mark.parametrize("op", list(OPS))
def test_results_at_switch_points(engines, op):
    """Every triple N* - 1, N*, N* + 1 of every dtype and flag mode, three ways (module docstring)."""
    t0 = time.time()
    for (o, dt, mode), sw in EXPECTED.items():
        if o != op:
            continue
        for nstar, before, after in sw:
            check_triple(engines, op, np.dtype(dt).type, mode, nstar, pair="pair" in before + after)
    print(f"{op}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("q", ["q64", "q128", "q512"])
def test_ramanujan_switch_points(engines, q):
    """Ramanujan's wave count, pad and window placement as functions of N at a fixed q_hi: pinned on the host, and the
    norms at every triple where the window or the pad moves equal the all-HBM engine's and the oracle's (1e-10; fp32
    windows against the oracle on the rounded input at the same bar: the kernel's arithmetic is double throughout, as
    test_gpu_ramanujan_census.py holds it entry by entry)."""
    eng, hbm = engines["eng"], engines["hbm"]
    pf = RAM_Q[q]
    for dtype in (np.float64, np.float32):
        want = EXPECTED[("ramanujan", dtype.__name__, q)]
        got = [(n, state(plan_of(eng, "ramanujan", n - 1, pf(n - 1), dtype, "plain")),
                state(plan_of(eng, "ramanujan", n, pf(n), dtype, "plain"))) for n in scan(eng, "ramanujan", dtype, "plain", pf, lo=1024)]
        assert got == want, (q, dtype.__name__, got)
        for nstar, before, after in want:
            if before.split(" b=")[0] == after.split(" b=")[0] and before.split("pad=")[1] == after.split("pad=")[1]:
                continue  # only the wave count moves: every wave count below 16 is already covered by the neighbours
            for n in (nstar - 1, nstar, nstar + 1):
                x = _signal(n, n, dtype)[None, :]
                lo, hi = pf(n)
                a = eng.ramanujan_norms(x, lo, hi)[0]
                b = hbm.ramanujan_norms(x, lo, hi)[0]
                assert rel_err(a, b) <= TOL_HBM[dtype], (q, n)
                assert rel_err(a, po.ramanujan_norms_folded(x[0].astype(np.float64), lo, hi)) <= TOL64, (q, n)


def test_ramanujan_refusals(engines):
    """q_hi = N / 3 grows until one wavefront's strips (12 q_hi bytes) no longer fit the LDS: from that N on,
    plan_info and the launch both refuse with PH_E_ARG on the host, and nothing is launched."""
    eng = engines["eng"]
    pf = RAM_Q["qN3"]
    for dtype in (np.float64, np.float32):
        ok = lambda n: _plan_ok(eng, n, pf(n), dtype)  # noqa: E731
        lo, hi = 30000, 45000
        assert ok(lo) and not ok(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        assert plan_of(eng, "ramanujan", lo, pf(lo), dtype, "plain")[0].window == _ffi().PH_PLAN_HBM
        eng.profile(True)
        with pytest.raises(ValueError):
            eng.ramanujan_norms(_signal(hi, 1, dtype)[None, :], 2, hi // 3)
        assert eng.profile_read() == []
        eng.profile(False)
        x = _signal(lo, 2, dtype)[None, :]
        assert rel_err(eng.ramanujan_norms(x, 2, lo // 3)[0], engines["hbm"].ramanujan_norms(x, 2, lo // 3)[0]) <= TOL_HBM[dtype]
    with pytest.raises(ValueError):
        eng.plan_info("ramanujan", 100000, (2, 30030))  # beyond the record format


def _ffi():
    from pyperiod_amd import _ffi

    return _ffi


def _plan_ok(eng, n, params, dtype):
    try:
        eng.plan_info("ramanujan", n, params, dtype)
        return True
    except ValueError:
        return False


def test_max_window_is_the_sweep_switch(engines):
    """ph_max_window reports exactly the last N whose sweep window stays in LDS, for both dtypes and every mode."""
    f = _ffi()
    eng = engines["eng"]
    for dtype in (np.float64, np.float32):
        m = eng.max_window(dtype)
        for mode in FLAGS:
            assert plan_of(eng, "sweep", m, (2, MAX_LEN, 0), dtype, mode)[0].window == f.PH_PLAN_LDS
            assert plan_of(eng, "sweep", m + 1, (2, MAX_LEN, 0), dtype, mode)[0].window == f.PH_PLAN_HBM
    assert engines["hbm"].max_window() == 0


def test_m_best_queries_report_the_kernel_that_runs(engines):
    """Host only: with every window in HBM m_best runs the one-window step 1, and the info query says so as the plan does
    (a default engine answers (2, 8) and PH_PLAN_PAIR for the same arguments)."""
    hbm = engines["hbm"]
    assert hbm.m_best_info(4096, 10) == (1, 8)
    assert hbm.plan_info("m_best", 4096, (10, 2, -1))[0].variant == _ffi().PH_PLAN_ONE


def _bf_variant(eng, n, L, dtype=np.float64):
    return plan_of(eng, "best_frequency", n, (L,), dtype, "plain")[0].variant


@pytest.mark.parametrize("n", [4096, 12000])
def test_best_frequency_spectrum_limits(engines, n):
    """Each spectrum path on both sides of its limit in win_size L, at a window in LDS (4096) and one whose update
    kernel works from HBM (12 000 fp64): FFT up to L = 8192 (its complex work array fills the LDS), the chirp for any
    other L whose FFT size 2^ceil(log2(min(N, L) + L/2 + 1)) fits, the direct DFT beyond.  Periods equal the oracle's,
    powers and bases within 1e-10, and the kernel the profile names is the one plan_info reports."""
    f = _ffi()
    eng, hbm = engines["eng"], engines["hbm"]
    names = {f.PH_PLAN_FFT: "k_bf_fft", f.PH_PLAN_CHIRP: "k_bf_chirp", f.PH_PLAN_DIRECT: "k_bf_spectrum"}
    # last odd L that runs the chirp (odd L: never the FFT)
    odd = switch_points(lambda k: _bf_variant(eng, n, 2 * k + 1), 2, 20000, step=32)
    assert len(odd) == 1
    lc = 2 * odd[0] - 1
    assert _bf_variant(eng, n, lc) == f.PH_PLAN_CHIRP and _bf_variant(eng, n, lc + 2) == f.PH_PLAN_DIRECT
    cases = [lc - 2, lc, lc + 1, lc + 2, 4096, 8192, 8191, 8193, 16384]
    seen = set()
    for L in cases:
        v = _bf_variant(eng, n, L)
        seen.add(v)
        x = _signal(n, L)[None, :]
        eng.profile(True)
        per, pw, bs, st = eng.best_frequency(x, L, 2)
        prof = {k for k, _ in eng.profile_read()}
        eng.profile(False)
        assert names[v] in prof and not (set(names.values()) - {names[v]}) & prof, (n, L, v, prof)
        p2, w2, b2, s2 = hbm.best_frequency(x, L, 2)
        assert np.array_equal(per, p2) and np.array_equal(st, s2) and rel_err(bs, b2) <= TOL_HBM[np.float64], (n, L)
        rper, rpw, rbs = po.best_frequency(x[0], L, 2)
        assert st[0] == 0 and np.array_equal(per[0], rper), (n, L, per[0], rper)
        assert rel_err(pw[0], rpw) <= TOL64 and rel_err(bs[0], rbs) <= TOL64, (n, L)
    assert seen == {f.PH_PLAN_FFT, f.PH_PLAN_CHIRP, f.PH_PLAN_DIRECT}
