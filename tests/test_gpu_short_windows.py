"""Every transform against the oracle at window lengths 1 to 200 (case table: short_windows_cases.py, census:
test_short_windows_cpu.py).  Between N = 1 and N = 200 the kernels enter each of their paths for the first time --
periods below and above 64, one or two rows per residue, N below a wavefront, a window that is mostly pad, fewer periods
than wavefronts -- and an off-by-one in a tail is the result, not one sample in 4096.

One test per entry point.  Each runs three engines: the default one, one with the one-window kernels
(PH_STEP1_PAIR=0 PH_S2L_PAIR=0 PH_BC_PAIR=0) and one that keeps windows in HBM (PH_HBM_WINDOW=1).  One call per length
and parameter set carries windows (a)-(e) as one batch; plain float64 runs on the dense set 1..200, the flags and float32
input (oracle on the float32-rounded window in float64; 1e-5 norms and powers, 1e-4 bases) on the flag subset.

Status is held in every row: non-zero (or the call refused with ValueError, then the oracle must raise for every row)
exactly where the oracle raises; it never returns numbers there.  Period lists are compared where every decision of the
oracle's trace has a relative margin of 1e-9 (float64) or 1e-3 (float32).  Below that bar another list is accepted, but
the row is then replayed -- the engine's own bases against po.project of its own periods -- and the share of such rows is
capped per test at the census' caps; where the lists agree, powers and bases are held to the oracle's.  The narrow
exceptions (picks on the rounding noise of an exactly fitted window, step-1 ties of m_best, the tie set of m_best) are
stated at _compare_picks, test_m_best and test_qo_find_periods, and pinned by the census.
A test collects every mismatch and reports them together."""

import os
import warnings

import numpy as np
import pytest

import short_windows_cases as sw
from oracle import period_oracle as po

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL32_VAL, TOL32_BASE = 1e-5, 1e-4
PLAIN = (False, False)
FLAG_SETS = ((True, False), (False, True), (True, True))
ENV_SINGLE = dict(PH_STEP1_PAIR=0, PH_S2L_PAIR=0, PH_BC_PAIR=0)
ENV_HBM = dict(PH_HBM_WINDOW=1)


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
    from pyperiod_amd import _ffi, default_engine

    for var in list(ENV_SINGLE) + list(ENV_HBM):
        assert var not in os.environ, var
    dflt, single, hbm = default_engine(), _engine(**ENV_SINGLE), _engine(**ENV_HBM)
    try:
        # the three engines really plan different kernels at these lengths
        for n in (24, 65, 200):
            assert dflt.m_best_info(n, 3) == (2, 8) and single.m_best_info(n, 3) == (1, 8), n
            for op, prm in (("small_to_large", (n // 2,)), ("best_correlation", (n // 3,))):
                assert dflt.plan_info(op, n, prm)[0].variant == _ffi.PH_PLAN_PAIR, (op, n)
                assert single.plan_info(op, n, prm)[0].variant == _ffi.PH_PLAN_ONE, (op, n)
                assert hbm.plan_info(op, n, prm)[0].window == _ffi.PH_PLAN_HBM, (op, n)
            for op, prm in (("sweep", (1, n + 2, 0)), ("project", (n,)), ("ramanujan", (1, n // 2)), ("orth_powers", (n // 2,))):
                assert dflt.plan_info(op, n, prm)[0].window == _ffi.PH_PLAN_LDS, (op, n)
                assert hbm.plan_info(op, n, prm)[0].window == _ffi.PH_PLAN_HBM, (op, n)
            assert [k.window for k in single.plan_info("m_best", n, (3,))] == [_ffi.PH_PLAN_LDS] * 2
            assert [k.window for k in hbm.plan_info("m_best", n, (3,))] == [_ffi.PH_PLAN_HBM] * 2
            assert dflt.plan_info("best_frequency", n, (n,))[1].window == _ffi.PH_PLAN_LDS
            assert hbm.plan_info("best_frequency", n, (n,))[1].window == _ffi.PH_PLAN_HBM
        yield (("default", dflt), ("one-window", single), ("hbm", hbm))
    finally:
        single.close()
        hbm.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


class Bag:
    """Collects mismatches so that one run names all of them."""

    def __init__(self):
        self.bad, self.seen, self.waived, self.rows, self.ties = [], 0, 0, 0, 0

    def check(self, ok, *what):
        self.seen += 1
        if not ok:
            self.bad.append(what)

    def done(self, cap=None, least=1):
        """`cap`: the largest share of the rows compared whose period list may differ from the oracle's under the margin
        rule (the census' caps: every such row still passed its status and self-consistency checks)."""
        print(f"{self.seen} checks, {len(self.bad)} mismatches; of {self.rows} rows {self.waived} with another period list "
              f"under the margin rule, {self.ties} step-1 ties with the same list")
        assert self.seen >= least
        if cap is not None:
            assert self.waived <= cap * self.rows, (self.waived, self.rows, cap)
        for b in self.bad[:60]:
            print("MISMATCH", b)
        assert not self.bad, f"{len(self.bad)} of {self.seen} checks failed, first: {self.bad[:12]}"


def close(got, want, tol):
    """max |got - want| <= tol * max |want| over the finite entries, the NaN entries in the same places; a reference
    that is all zero must be met exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    if nan.all():
        return True
    g, w = got[~nan], want[~nan]
    return bool(np.max(np.abs(g - w)) <= tol * np.max(np.abs(w)))


# part -> (lengths, dtype, flag sets, value bar, base bar, margin bar, parameter sets): plain float64 with the default
# parameters ("dense") and with the second parameter set ("wide") on all lengths -- in four chunks of about equal oracle
# time each, so that every case stays at a few seconds -- the flags and float32 input on the subset
CHUNKS = (range(1, 101), range(101, 146), range(146, 176), range(176, 201))
assert tuple(n for c in CHUNKS for n in c) == sw.DENSE
PARTS = {
    "flags": (sw.FLAGS, np.float64, FLAG_SETS, TOL, TOL, sw.MARGIN64, (0,)),
    "f32": (sw.FLAGS, np.float32, (PLAIN,) + FLAG_SETS, TOL32_VAL, TOL32_BASE, sw.MARGIN32, (0, 1, 2)),
}
for _i, _c in enumerate(CHUNKS):
    PARTS[f"dense{_i}"] = (tuple(_c), np.float64, (PLAIN,), TOL, TOL, sw.MARGIN64, (0,))
    PARTS[f"wide{_i}"] = (tuple(_c), np.float64, (PLAIN,), TOL, TOL, sw.MARGIN64, (1, 2))
DENSE_PARTS = tuple(f"dense{i}" for i in range(len(CHUNKS)))
LEAF_PARTS = DENSE_PARTS + ("flags", "f32")
ALL_PARTS = DENSE_PARTS + tuple(f"wide{i}" for i in range(len(CHUNKS))) + ("flags", "f32")


def cases(part, sets):
    """(parameter set, trunc, orth) of a part; the further parameter sets (None: not at this length) run plain only."""
    return [(kw, t, o) for i, kw in enumerate(sets) if i in PARTS[part][6] and kw is not None for t, o in PARTS[part][2]
            if i == 0 or (t, o) == PLAIN]


def cap_of(part):
    return sw.CAP32 if PARTS[part][1] == np.float32 else sw.CAP64


def x64(n, dtype):
    return sw.windows(n, dtype).astype(np.float64)


def isolated(bag, call, x, what, pair=False, status=None):
    """Rows (a)-(c) must be bit-identical whether or not (d), (e) ride in the batch; for the window-pair kernels also
    with (d) or (e) as the partner of (a) in one workgroup, in the even and in the odd position.  `call(batch)` -> tuple
    of arrays with the window index first; `status`: the index of the status array among them -- a row that ends with
    a status holds nothing else to compare."""
    def fn(b):
        out = tuple(np.asarray(a) for a in call(b))
        if status is None:
            return out
        bad = out[status] != 0
        return tuple(np.where(bad.reshape((-1,) + (1,) * (a.ndim - 1)), np.zeros((), a.dtype), a) if k != status else a
                     for k, a in enumerate(out))

    full = fn(x)
    alone = fn(x[:3])
    for k, (f, a) in enumerate(zip(full, alone)):
        bag.check(np.array_equal(np.asarray(f)[:3], np.asarray(a), equal_nan=True), what, "abc alone", k)
    if pair:
        for other in (3, 4):
            for order in ((0, other), (other, 0)):
                got = fn(np.ascontiguousarray(x[list(order)]))
                for k, (f, g) in enumerate(zip(full, got)):
                    bag.check(np.array_equal(np.asarray(f)[0], np.asarray(g)[order.index(0)], equal_nan=True), what,
                              "partner", order, k)
    return full


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", LEAF_PARTS)
def test_project_batch(engines, part):
    """Bit for bit in float64, except p = 1 at N >= 8: numpy reduces the (N, 1) rectangle along its contiguous axis, where
    it sums pairwise, and the kernel in row order (1e-12 there, as test_gpu_parity.py holds it).  p = 1 with
    orthogonalize is left out: the reference raises KeyError (get_factors(1, True))."""
    bag = Bag()
    lens, dtype, flagsets, tol, tolb = PARTS[part][:5]
    for n in lens:
        x, xr = sw.windows(n, dtype), x64(n, dtype)
        for trunc, orth in flagsets:
            pl = sorted({p for p in (1, 2, 3, n // 2, n - 1, n, n + 1, 63, 64, 65) if p >= (2 if orth else 1)})
            want = np.stack([[po.project(xr[w], p, trunc, orth) for p in pl] for w in range(5)])
            for name, e in engines:
                got = e.project_batch(x, pl, trunc, orth)
                if dtype == np.float64:
                    k0 = 1 if pl[0] == 1 and n >= 8 else 0
                    bag.check(np.array_equal(got[:, k0:], want[:, k0:], equal_nan=True), name, n, trunc, orth)
                    bag.check(close(got[:, :k0], want[:, :k0], 1e-12), name, n, trunc, orth, "p = 1")
                else:
                    for k, p in enumerate(pl):
                        for w in range(5):
                            bag.check(close(got[w, k], want[w, k], tolb), name, n, p, sw.KINDS[w], trunc, orth, "f32")
                if part == "flags":
                    one = e.project_batch(x, pl, trunc, orth, single=True)
                    for k, p in enumerate(pl):
                        m = min(p, n)
                        bag.check(np.array_equal(one[:, k, :m], got[:, k, :m], equal_nan=True), name, n, p, "single")
        if part.startswith("dense"):
            isolated(bag, lambda b, pl=pl: (engines[0][1].project_batch(b, pl),), x, ("project", n))
        if part == "flags":  # return_single_period without a flag too
            pl = sorted({p for p in (1, 2, 3, n // 2, n - 1, n, n + 1, 63, 64, 65) if p >= 1})
            for name, e in engines:
                full, one = e.project_batch(x, pl), e.project_batch(x, pl, single=True)
                for k, p in enumerate(pl):
                    bag.check(np.array_equal(one[:, k, :min(p, n)], full[:, k, :min(p, n)], equal_nan=True), name, n, p,
                              "single, plain")
    bag.done()


def test_periodic_norm(engines):
    bag = Bag()
    for lens, dtype in ((sw.DENSE, np.float64), (sw.FLAGS, np.float32)):
        for n in lens:
            x, xr = sw.windows(n, dtype), x64(n, dtype)
            for p in (None, 2, n):
                want = np.array([po.periodic_norm(xr[w], p) for w in range(5)])
                for name, e in engines:
                    got = e.periodic_norm(x, p)
                    bag.check(np.all(np.abs(got - want) <= 1e-14 * got), name, n, p, np.dtype(dtype).name)
    bag.done()


@pytest.mark.parametrize("part", LEAF_PARTS)
def test_sweep(engines, part):
    """p = 1 .. N + 2 (periods above N have a NaN norm in the reference; with orthogonalize the range starts at 2: the
    reference raises KeyError at p = 1)."""
    from pyperiod_amd import _ffi

    bag = Bag()
    lens, dtype, flagsets, tol = PARTS[part][:4]
    for n in lens:
        x, xr = sw.windows(n, dtype), x64(n, dtype)
        for trunc, orth in flagsets:
            lo = 2 if orth else 1
            ps = np.arange(lo, n + 3)
            norm = np.stack([po.sweep_norms(xr[w], lo, n + 2, False, trunc, orth) for w in range(5)])
            wants = {_ffi.PH_SWEEP_NORM: norm, _ffi.PH_SWEEP_NORM_GAMMA: norm / np.sqrt(ps)[None, :]}  # periodic_norm(., p)
            if (trunc, orth) == PLAIN:
                wants[_ffi.PH_SWEEP_MAXABS] = np.stack([po.sweep_maxabs(xr[w], lo, n + 2) for w in range(5)])
            for mode, want in wants.items():
                for name, e in engines:
                    got = e.sweep(x, lo, n + 2, mode, trunc, orth)
                    for w in range(5):
                        if mode == _ffi.PH_SWEEP_MAXABS:  # p = 1 left out as in test_random_sweeps (one long sum)
                            ok = np.array_equal(got[w, 1:], want[w, 1:]) if dtype == np.float64 else close(got[w, 1:], want[w, 1:], tol)
                        else:
                            ok = close(got[w], want[w], tol)
                        bag.check(ok, name, n, sw.KINDS[w], mode, trunc, orth, np.dtype(dtype).name)
        if part.startswith("dense"):
            for mode in (_ffi.PH_SWEEP_NORM, _ffi.PH_SWEEP_NORM_GAMMA, _ffi.PH_SWEEP_MAXABS):
                isolated(bag, lambda b, n=n, mode=mode: (engines[0][1].sweep(b, 1, n + 2, mode),), x, ("sweep", n, mode))
    bag.done()


# ---------------------------------------------------------------------------------------------------------------------
def _replay(x, per, bases, powers, trunc, orth, chain, tolb, tol):
    """Self-consistency of a row whose period list is not the oracle's: the engine's own bases against po.project of its own
    periods.  chain "frequency" / "correlation": base i is the projection of the residual left by the bases before it
    (both subtract every base), its power the norm of the base over the window's / the gain in the residual norm; a
    period of 0 (a pick best_correlation rejected: its base is not returned) ends the replay.  chain None (m_best, whose
    rows may have been added to or split): every base is periodic with its period."""
    x = np.asarray(x, dtype=np.float64)
    work, og = x.copy(), po.periodic_norm(x)
    old, top = og, float(np.max(np.abs(x)))

    def near(a, b, t):  # to t of the window's largest sample: a base fitted to a residual of 1e-17 is itself noise
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return a.shape == b.shape and bool(np.all(np.abs(a - b) <= t * top))

    for i, p in enumerate(int(v) for v in per):
        b = np.asarray(bases[i], dtype=np.float64)
        if chain is None:
            if p < 1 or not near(po.project(b, p, trunc, False), b, max(tolb, 1e-9)):
                return False
            continue
        if p == 0:
            return not b.any()
        want = po.project(work, p, trunc, orth)
        if not near(b, want, tolb):
            return False
        work = work - want
        if chain == "frequency":
            ok = abs(powers[i] - po.periodic_norm(want) / og) <= max(tol, 1e-9)  # (powers are fractions of the window's norm)
        else:
            this = po.periodic_norm(work)
            ok = abs(powers[i] - (old - this) / og) <= max(tol, 1e-7)  # (a difference of two norms)
            old = this
        if not ok:
            return False
    return True


def _compare_picks(bag, tag, n, dtype, refs, got, st, tol, tolb, bar, x=None, flags=PLAIN, chain=None, noisy=None,
                   gaps=None):
    """Rows of m_best / best_correlation / best_frequency against the oracle's (state, result, margin) per window.
    `got` is None when the engine refused the call with ValueError.

    Status is held in every row: non-zero exactly where the oracle raises.  Two narrow exceptions, both pinned by the
    census: a row in which a later round of the oracle's best_correlation, or a step-1 pick of its m_best, ran on the
    rounding noise of an exactly fitted window (`noisy`), and for float32 input a row the oracle ends "raises late" (short_windows_cases.ref) -- there the
    oracle's own outcome hangs on whether sums are 1e-17 or exactly zero, and a row that ends with a status is accepted.
    The period list is held where the margin is at least `bar`; below it another list is accepted, counted
    (Bag.waived, capped in done()) and the row is replayed: the engine's bases against po.project of its own periods.
    Where the lists agree powers and bases are held to the oracle's.  One exception: a step-1 gap of m_best below `bar`
    (`gaps`) -- tied candidates taken in another order can end in the same list with a period added to another row --
    where a row that misses the values is counted (Bag.ties) and replayed instead."""
    trunc, orth = flags
    for w, (state, want, margin) in enumerate(refs):
        what = tag + (n, sw.KINDS[w], np.dtype(dtype).name)
        if got is None:
            bag.check(state.startswith("raises"), what, "refused a call the oracle answers")
            continue
        loose = bool(noisy and noisy[w]) or (state == "raises late" and dtype == np.float32)
        if state.startswith("raises"):
            if not loose:
                bag.check(st[w] != 0, what, "numbers where the oracle raises")
            elif st[w] == 0:
                bag.check(_replay(x[w], got[0][w], got[2][w], got[1][w], trunc, orth, chain, tolb, tol), what, "replay")
            continue
        if loose and st[w] != 0:
            continue
        bag.check(st[w] == 0, what, "status", int(st[w]))
        if st[w] != 0:
            continue
        bag.rows += 1
        same = np.array_equal(got[0][w], want[0])
        if not same:
            if margin >= bar and not loose:
                bag.check(False, what, "periods", got[0][w].tolist(), want[0].tolist(), margin)
                continue
            bag.waived += 1
            bag.check(_replay(x[w], got[0][w], got[2][w], got[1][w], trunc, orth, chain, tolb, tol), what, "replay",
                      got[0][w].tolist(), want[0].tolist())
            continue
        vals = close(got[1][w], want[1], tol) and close(got[2][w], want[2], tolb)
        if not vals and gaps is not None and gaps[w] < bar:
            bag.ties += 1
            bag.check(_replay(x[w], got[0][w], got[2][w], got[1][w], trunc, orth, None, tolb, tol), what, "replay (tie)")
            continue
        bag.check(close(got[1][w], want[1], tol), what, "powers")
        bag.check(close(got[2][w], want[2], tolb), what, "bases")
        if chain == "correlation":
            bag.check(not np.asarray(got[2][w])[want[0] == 0].any(), what, "zero rows")


def _try(fn, *a, **k):
    try:
        return fn(*a, **k)
    except ValueError:
        return None


@pytest.mark.parametrize("part", ALL_PARTS)
@pytest.mark.parametrize("gamma", [False, True])
def test_m_best(engines, gamma, part):
    """Three parameter sets: the defaults; the issue's num=3, min_length=1, max_length=N-1; and num=3, min_length=2,
    max_length=N//2.  Without gamma the second set is a set of ties: once period N - 1 is taken the residual is two
    spikes and every p > N / 2 has the same norm, so 545 of its 585 answered cases (a)-(c) have a margin below 1e-9
    (census).  Its rows are held like all others -- status, the oracle's values wherever the list agrees, the replay
    where it does not -- but the share of other lists is not capped for it; the third set reaches the same periods
    (64 and more from N = 128) with every margin above the bar and is capped."""
    bag, ties = Bag(), Bag()
    lens, dtype, _, tol, tolb, bar, _ = PARTS[part]
    for n in lens:
        x = sw.windows(n, dtype)
        sets = [dict(num=3), sw.second_set("m_best", n), sw.second_set("m_best_mid", n)]
        for kw, trunc, orth in cases(part, sets):
            kw = {k: v for k, v in kw.items() if k != "gamma"}
            rk = dict(gamma=gamma, trunc=trunc, orth=orth, **kw)
            refs = [sw.ref("m_best", n, k, dtype, **rk) for k in sw.KINDS]
            gaps = [sw.step1_gap(n, k, dtype, **rk) for k in sw.KINDS]
            noisy = [sw.noisy("m_best", n, k, dtype, **rk) for k in sw.KINDS]
            into = ties if (kw.get("max_length") == n - 1 and not gamma) else bag
            for name, e in engines:
                out = _try(e.m_best, x, gamma=gamma, trunc=trunc, orth=orth, **kw)
                _compare_picks(into, (name, "m_best", gamma, trunc, orth, kw.get("max_length")), n, dtype, refs, out,
                               None if out is None else out[3], tol, tolb, bar, x, (trunc, orth), None, noisy, gaps)
            if part[:-1] in ("dense", "wide") and n >= 6:
                isolated(bag, lambda b, kw=kw: engines[0][1].m_best(b, gamma=gamma, **kw), x,
                         ("m_best", n, gamma, kw.get("max_length")), True, 3)
    ties.done(least=0)
    bag.done(cap_of(part))


@pytest.mark.parametrize("part", ALL_PARTS)
def test_small_to_large(engines, part):
    bag = Bag()
    lens, dtype, _, tol, tolb, bar, _ = PARTS[part]
    for n in lens:
        x = sw.windows(n, dtype)
        sets = [dict(thresh=0.05), sw.second_set("small_to_large", n)]
        for kw, trunc, orth in cases(part, sets):
            refs = [sw.ref("small_to_large", n, k, dtype, trunc=trunc, orth=orth, **kw) for k in sw.KINDS]
            for name, e in engines:
                what = (name, "s2l", n, np.dtype(dtype).name, trunc, orth, len(kw))
                out = _try(e.small_to_large, x, kw["thresh"], kw.get("n_periods"), trunc, orth, cap=4)
                bag.check(out is not None, what, "refused")
                if out is None:
                    continue
                counts, per, pw, bs, st = out
                for w, (state, want, margin) in enumerate(refs):
                    assert state == "ok"
                    k = int(counts[w])
                    bag.check(st[w] == 0, what, w, "status", int(st[w]))
                    same = list(per[w, :k]) == list(want[0])
                    if margin >= bar:
                        bag.check(same, what, w, "periods", list(per[w, :k]), want[0], margin)
                    elif not same:
                        bag.waived += 1  # replay: every accepted base is the projection of the residual before it
                        work, good = np.asarray(x[w], dtype=np.float64).copy(), True
                        for i in range(k):
                            base = po.project(work, int(per[w, i]), trunc, orth)
                            good = good and close(bs[w, i], base, tolb)
                            work = work - base
                        bag.check(good, what, w, "replay", list(per[w, :k]), want[0])
                    bag.rows += 1
                    if same:
                        bag.check(close(pw[w, :k], np.array(want[1], dtype=np.float64), tol), what, w, "powers")
                        if k:
                            bag.check(close(bs[w, :k], np.array(want[2]), tolb), what, w, "bases")
            if part[:-1] in ("dense", "wide"):
                def call(b, kw=kw):
                    c, p, w_, b_, s_ = engines[0][1].small_to_large(b, kw["thresh"], kw.get("n_periods"), cap=64)
                    live = np.arange(64)[None, :] < c[:, None]  # (rows behind the count are not written)
                    return c, np.where(live, p, 0), np.where(live, w_, 0.0), np.where(live[:, :, None], b_, 0.0), s_
                isolated(bag, call, x, ("s2l", n, len(kw)), True)
    bag.done(cap_of(part))


@pytest.mark.parametrize("part", ALL_PARTS)
def test_best_correlation(engines, part):
    bag = Bag()
    lens, dtype, _, tol, tolb, bar, _ = PARTS[part]
    for n in lens:
        x = sw.windows(n, dtype)
        sets = [dict(num=2), sw.second_set("best_correlation", n)]
        for kw, trunc, orth in cases(part, sets):
            refs = [sw.ref("best_correlation", n, k, dtype, trunc=trunc, orth=orth, **kw) for k in sw.KINDS]
            noisy = [sw.noisy("best_correlation", n, k, dtype, trunc=trunc, orth=orth, **kw) for k in sw.KINDS]
            for name, e in engines:
                out = _try(e.best_correlation, x, trunc=trunc, orth=orth, **kw)
                _compare_picks(bag, (name, "bc", trunc, orth, len(kw)), n, dtype, refs, out,
                               None if out is None else out[3], tol, tolb, bar, x, (trunc, orth), "correlation", noisy)
            if part[:-1] in ("dense", "wide") and n >= 9:
                isolated(bag, lambda b, kw=kw: engines[0][1].best_correlation(b, **kw), x, ("bc", n, len(kw)), True, 3)
    bag.done(cap_of(part))


@pytest.mark.parametrize("part", ALL_PARTS)
def test_best_frequency(engines, part):
    bag = Bag()
    lens, dtype, _, tol, tolb, bar, _ = PARTS[part]
    for n in lens:
        x = sw.windows(n, dtype)
        sets = [dict(num=2), sw.second_set("best_frequency", n)]
        for kw, trunc, orth in cases(part, sets):
            refs = [sw.ref("best_frequency", n, k, dtype, trunc=trunc, orth=orth, **kw) for k in sw.KINDS]
            for name, e in engines:
                out = _try(e.best_frequency, x, kw.get("win_size"), kw["num"], trunc, orth)
                _compare_picks(bag, (name, "bf", trunc, orth, len(kw)), n, dtype, refs, out,
                               None if out is None else out[3], tol, tolb, bar, x, (trunc, orth), "frequency")
            if part[:-1] in ("dense", "wide") and n >= 2:
                isolated(bag, lambda b, kw=kw: engines[0][1].best_frequency(b, kw.get("win_size"), kw["num"]), x,
                         ("bf", n, len(kw)), False, 3)
    bag.done(cap_of(part))


# ---------------------------------------------------------------------------------------------------------------------
def test_ramanujan_norms(engines):
    bag = Bag()
    for lens, dtype in ((sw.DENSE, np.float64), (sw.FLAGS, np.float32)):
        for n in lens:
            x, xr = sw.windows(n, dtype), x64(n, dtype)
            ranges = {(1, max(1, n // 2)), (2, max(2, n // 3))}
            if n // 2 >= n // 4 + 1:
                ranges.add((n // 4 + 1, n // 2))
            for q_lo, q_hi in sorted(ranges):
                want = np.stack([po.ramanujan_norms_folded(xr[w], q_lo, q_hi) for w in range(5)])
                for name, e in engines:
                    got = e.ramanujan_norms(x, q_lo, q_hi)
                    for w in range(5):
                        scale = max(np.max(np.abs(want[w])), 1e-300)
                        bar = 1e-9  # float32 windows too: the kernel's arithmetic is double throughout
                        bag.check(got[w].shape == want[w].shape and np.max(np.abs(got[w] - want[w])) / scale < bar,
                                  name, n, sw.KINDS[w], q_lo, q_hi, np.dtype(dtype).name)
                if dtype == np.float64:
                    isolated(bag, lambda b, q_lo=q_lo, q_hi=q_hi: (engines[0][1].ramanujan_norms(b, q_lo, q_hi),), x,
                             ("ramanujan", n, q_lo, q_hi))
    bag.done()


def test_orth_powers(engines):
    bag = Bag()
    for lens, dtype, tol in ((sw.DENSE, np.float64, TOL), (sw.FLAGS, np.float32, TOL32_VAL)):
        for n in lens:
            x, xr = sw.windows(n, dtype), x64(n, dtype)
            max_p = max(2, n // 2)
            want = np.stack([po.orth_powers(xr[w], max_p, True) for w in range(5)])
            for name, e in engines:
                got = e.orth_powers(x, max_p, True)
                for w in range(5):
                    bag.check(close(got[w], want[w], tol), name, n, sw.KINDS[w], np.dtype(dtype).name)
            if dtype == np.float64:
                isolated(bag, lambda b, max_p=max_p: (engines[0][1].orth_powers(b, max_p, True),), x, ("orth_powers", n))
    bag.done()


def test_fold_sums_and_tile_sum(engines):
    bag = Bag()
    for lens, dtype, tol in ((sw.DENSE, np.float64, TOL), (sw.FLAGS, np.float32, TOL32_VAL)):
        for n in lens:
            x, xr = sw.windows(n, dtype), x64(n, dtype)
            pl = sorted({p for p in (2, 3, n // 2, n - 1) if p >= 1})
            for keep in (pl, [p - 1 for p in pl]):
                if sum(keep) < 1:
                    continue
                want = np.stack([np.concatenate([po.fold_sums(xr[w], p)[:k] for p, k in zip(pl, keep)]) for w in range(5)])
                t = np.arange(n)
                for name, e in engines:
                    got = e.fold_sums(x, pl, keep)
                    for w in range(5):
                        bag.check(close(got[w], want[w], tol), name, "fold_sums", n, sw.KINDS[w], keep, np.dtype(dtype).name)
                    if dtype == np.float64:  # the reconstruction A^T w of the sums just computed
                        tiled = np.zeros((5, n))
                        off = 0
                        for p, k in zip(pl, keep):
                            blk = np.concatenate([want[:, off:off + k], np.zeros((5, p - k))], axis=1)
                            tiled += blk[:, t % p]
                            off += k
                        back = e.tile_sum(want, n, pl, keep)
                        for w in range(5):
                            bag.check(close(back[w], tiled[w], tol), name, "tile_sum", n, sw.KINDS[w], keep)
    bag.done()


def test_qo_find_periods(engines):
    """Every row (a), (b), (c), (e) is held to: status 0 -- a hand-back (status != 0, the class layer then runs the row on
    the host) is accepted only where a selection of the oracle ran on rounding noise or below the margin, and counted;
    the oracle's period list -- in full where every decision is clear, otherwise up to the oracle's first selection on
    noise (the engine may stop there or go on); and, wherever the lists agree that far, the oracle's residual to `tol`
    of the window's largest sample: the fit is the same whatever a pick on noise adds.  (e) is thus compared in its
    first pick and its zero residual.  (d), all zeros, is the class layer's fixed answer (QOPeriods.py:394-406): here it
    must end with a status or a zero residual."""
    bag = Bag()
    for lens, dtype, bar, tol in ((sw.DENSE, np.float64, sw.MARGIN64, 1e-7), (sw.FLAGS, np.float32, sw.MARGIN32, TOL32_BASE)):
        for n in lens:
            if n < 6:
                continue
            x = sw.windows(n, dtype)
            lo, hi = 2, max(2, n // 3)
            for upd in (True, False):
                kw = dict(num=3, thresh=0.1, min_length=lo, max_length=hi, update_weights=upd)
                refs = [sw.ref("qo_find_periods", n, k, dtype, **kw) for k in sw.KINDS]
                for name, e in engines:
                    per, nrm, keeps, counts, wts, resid, st = e.qo_find_periods(x, 3, 0.1, lo, hi, update_weights=upd)
                    for w, (state, want, margin) in enumerate(refs):
                        kind = sw.KINDS[w]
                        what = (name, "qo", n, kind, upd, np.dtype(dtype).name)
                        assert state == "ok"
                        if w == 3:
                            bag.check(st[w] != 0 or not np.asarray(resid[w]).any(), what, "zero window")
                            continue
                        out, res = want
                        want_per = [int(v) for v in out["periods"]]
                        unclear = margin < bar or sw.noisy("qo_find_periods", n, kind, dtype, **kw)
                        bag.rows += 1
                        if st[w] != 0:
                            bag.waived += 1
                            bag.check(unclear, what, "status", int(st[w]))
                            continue
                        nrep, nb = (int(v) for v in counts[w])
                        got_per = [int(v) for v in per[w, :nrep]]
                        held = len(want_per) if not unclear else min(sw.qo_real_picks(n, kind, dtype, **kw), len(want_per))
                        if margin < bar:  # a tie between two real candidates: the list may part there
                            held = 0
                        agree = got_per[:held] == want_per[:held] and (unclear or got_per == want_per)
                        bag.check(agree, what, "periods", got_per, want_per, held, margin)
                        if not agree or margin < bar:
                            continue
                        scale = float(np.max(np.abs(x[w])))
                        bag.check(np.max(np.abs(np.asarray(resid[w], dtype=np.float64) - res)) <= tol * scale, what, "residual")
                        if got_per == want_per and not unclear:
                            if upd:
                                bag.check(list(keeps[w, :nb]) == list(out["basis_dictionary"].values()), what, "keeps")
                            k = len(out["weights"])  # (fixed weights: the blocks concatenate, the re-fitted last one included)
                            bag.check(close(wts[w, :k], out["weights"], tol), what, "weights")
    bag.done()  # (a hand-back is accepted only in a row with an unclear decision; the census pins and caps those)


# ---------------------------------------------------------------------------------------------------------------------
def test_class_methods_raise_where_the_oracle_raises(engines):
    """The 1-D class methods at five lengths at which the oracle raises for window (a): they raise too."""
    from pyperiod_amd import Periods

    for n in (1, 2, 5, 8, 11):
        x = sw.windows(n)[0].copy()
        assert sw.ref("m_best", n, "a", num=3)[0] == "raises"
        with pytest.raises((TypeError, ValueError)):
            Periods().m_best(x, num=3)
        with pytest.raises((TypeError, ValueError)):
            Periods().m_best_gamma(x, num=3)
    for n, kind in ((4, "a"), (5, "c"), (8, "c"), (36, "c"), (29, "a")):  # period 1 wins: get_factors(1, True) in step 2
        x = sw.windows(n)[sw.KINDS.index(kind)].copy()
        assert sw.ref("m_best", n, kind, num=3, min_length=1, max_length=n - 1, gamma=True)[0] == "raises"
        with pytest.raises(KeyError):
            Periods().m_best_gamma(x, num=3, min_length=1, max_length=n - 1)
    for n in (1, 2, 5, 8, 10):
        x = sw.windows(n)[0].copy()
        assert sw.ref("best_correlation", n, "a", num=2)[0].startswith("raises")
        with pytest.raises((TypeError, ValueError)):
            Periods().best_correlation(x, num=2)
    for n in (1, 2, 5, 13, 33):
        x = sw.windows(n)[0].copy()
        assert sw.ref("best_frequency", n, "a", num=2)[0] == "raises"
        with pytest.raises((OverflowError, ValueError)):
            Periods().best_frequency(x, num=2)


def test_ramanujan_and_qo_class_methods_at_the_shortest_lengths(engines):
    """RamanujanPeriods.find_periods and QOPeriods.find_periods at N = 1 .. 5, where max_length = N // 3 leaves no period
    to look at: the reference does not raise there -- its loops do not run and it returns a zero vector, an empty
    dictionary and the window as the residual -- so the 1-D class methods are held to that answer."""
    from pyperiod_amd import QOPeriods, RamanujanPeriods

    for n in (1, 2, 3, 4, 5):
        x = sw.windows(n)[0].copy()
        want = po.ramanujan_find_periods(x)
        got = RamanujanPeriods().find_periods(x)
        assert got.shape == want.shape and not want.any() and not np.asarray(got).any(), n
        out, res = po.qo_find_periods(x, 3, 0.1)
        gout, gres = QOPeriods().find_periods(x, num=3, thresh=0.1)
        assert len(out["periods"]) == 0 and len(gout["periods"]) == 0 and dict(gout["basis_dictionary"]) == {}, n
        assert np.array_equal(gres, res) and np.array_equal(res, x), n
        # the batch form gives every row the 1-D call's answer, the zero row its fixed one (QOPeriods.py:394-406)
        batch = QOPeriods().find_periods(sw.windows(n).copy(), num=3, thresh=0.1)
        for w, (bout, bres) in enumerate(batch):
            rout, rres = po.qo_find_periods(sw.windows(n)[w], 3, 0.1)
            assert [int(v) for v in bout["periods"]] == [int(v) for v in rout["periods"]], (n, w)
            assert dict(bout["basis_dictionary"]) == rout["basis_dictionary"] and np.array_equal(bres, rres), (n, w)
        rb = RamanujanPeriods().find_periods(sw.windows(n).copy())
        assert rb.shape == (5,) + want.shape and not rb.any(), n


def test_short_time_frames_of_16_and_24_samples(engines):
    """ShortTime with frames far below a wavefront: analyze against the Periods methods on the host-built batch of the same
    frames, as test_gpu_short_time.py compares."""
    from pyperiod_amd import Periods, ShortTime
    from pyperiod_amd.synth import readme_window
    from test_short_time_cpu import frames_ref, ola_bound, overlap_add_ref

    L = 300
    x = readme_window(L, seed=3)
    for N, hop in ((16, 5), (24, 7)):
        st = ShortTime(N, hop)
        batch = frames_ref(x, N, hop, st.frame_count(L))
        per, pw, bases = Periods().m_best(batch, num=2)
        for f in range(batch.shape[0]):  # the host route itself against the oracle
            want = po.m_best(batch[f], 2)
            assert np.array_equal(per[f], want[0]) and close(pw[f], want[1], TOL) and close(bases[f], want[2], TOL), (N, f)
        res = st.analyze(x, "m_best", num=2)
        assert np.array_equal(res.periods, per) and np.array_equal(res.powers, pw)
        ref, mag, den = overlap_add_ref(bases, hop, L, None, None, None, True)
        pos = den > 0
        err, bound = np.abs(res.periodic - ref), ola_bound(mag, den, bases.shape[1], N, hop)
        assert np.all(err[pos] <= bound[pos]) and np.all(res.periodic[~pos] == 0.0)
        assert np.array_equal(res.residual, x.astype(np.float64) - res.periodic)
