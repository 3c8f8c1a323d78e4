"""The host-stepped greedy loop of the batched QOPeriods.find_periods (``_find_periods_stepped`` with its two
selectors) and the capacity ladder of ph_qo_find_periods (``_qo_capacities``), on the CPU.  Two fake engines stand in
for the device: one computes what the kernels compute from the oracle's pieces and is run against the committed
fixtures, one does no arithmetic and scripts every selection and fit to pin who stops when and who is handed back."""

import sys

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd import QOPeriods, _ffi
from pyperiod_amd.QOPeriods import _qo_capacities, _qo_fit_start, _ram_capacities
from pyperiod_amd.synth import multi_sinusoid_window
from test_qo_orth_cpu import group_kw
from test_qo_window_cpu import windowed_solve
from test_qo_window_keep_cpu import o_group_kw

TOL_NORM, TOL_SOLVE = 1e-10, 1e-8  # the bounds of test_oracle_pieces_reproduce_the_fixture for the same pieces


# ---------------------------------------------------------------------------- the oracle-backed engine
class OracleEngine:
    """sweep, qo_orth_select and qo_fit as the oracle's pieces compute them, row by row."""

    def sweep(self, x, p_lo, p_hi, mode, trunc, orth):
        assert mode == _ffi.PH_SWEEP_NORM_GAMMA and not orth
        return np.stack([po.sweep_norms(row, p_lo, p_hi, gamma=True, trunc=trunc) for row in x])

    def qo_orth_select(self, x, max_p, trunc=False):
        p = np.array([po.best_period_orthogonal(row, max_p, True) for row in x], dtype=np.int32)
        g = np.array([po.periodic_norm(po.project(row, q, trunc, True), q) for row, q in zip(x, p)])
        return p, g, np.zeros(len(x), dtype=np.int32)

    def qo_fit_feasible(self, kcap, max_period, n=None, window=False):
        return kcap <= 2048

    def qo_fit(self, x, periods, n_periods, kcap, max_period, window):
        W, N = x.shape
        keeps = np.zeros(periods.shape, dtype=np.int32)
        wts = np.zeros((W, kcap))
        res = x.copy()
        st = np.zeros(W, dtype=np.int32)
        for w in range(W):
            rows, dims = po.qo_get_subspaces([int(q) for q in periods[w, : n_periods[w]]], N)
            keeps[w, : n_periods[w]] = list(dims.values())
            if 0 in dims.values():  # a block without rows: the device hands the list back
                st[w] = _ffi.PH_ST_ITER_CAP
            elif rows.shape[0] > kcap:
                st[w] = _ffi.PH_ST_CAP
            else:
                sol, rec = po.qo_solve_quadratic(x[w], rows) if window is None else windowed_solve(x[w], window, rows)
                wts[w, : sol.size], res[w] = sol, x[w] - rec
        return keeps, wts, res, st


def _check_rows(g, keys, x, out):
    """Every row of `out` against the fixture entries `keys`; -> per row whether it reports fewer periods than blocks."""
    short = []
    for key, row, got in zip(keys, x, out):
        assert got is not None, key
        bases, res = got
        assert np.array_equal(bases["periods"], g[f"{key}_periods"]) and bases["periods"].dtype == np.uint32, key
        assert [int(q) for q in bases["basis_dictionary"]] == list(g[f"{key}_dict_keys"]), key
        assert list(bases["basis_dictionary"].values()) == list(g[f"{key}_dict_vals"]), key
        assert np.array_equal(bases["subspaces"], po.qo_get_subspaces(list(g[f"{key}_dict_keys"]), row.size)[0]), key
        en = rel_err(bases["norms"], g[f"{key}_norms"])
        ew, er = rel_err(bases["weights"], g[f"{key}_weights"]), rel_err(res, g[f"{key}_residual"])
        print(f"{key}: periods {list(bases['periods'])} norms {en:.2e} weights {ew:.2e} residual {er:.2e}")
        assert en <= TOL_NORM and ew <= TOL_SOLVE and er <= TOL_SOLVE, key
        short.append(len(bases["periods"]) < len(bases["basis_dictionary"]))
    return short


@pytest.mark.parametrize("tag", list("ABCDE"))
def test_orthogonal_selector_reproduces_the_fixture(golden, tag):
    g = golden("qo_orth")
    n, num, thresh, max_length, trunc = group_kw(g, tag)
    keys = [f"{tag}{w}" for w in range(8)]
    x = np.stack([multi_sinusoid_window(int(g[f"{k}_seed"]), n) for k in keys])
    qo, eng = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True), OracleEngine()
    short = _check_rows(g, keys, x, qo._find_periods_stepped(eng, x, qo._select_orthogonal(eng, max_length), num, thresh, max_length))
    if tag == "E":  # the mixed-fate batch
        assert any(short) and not all(short)


def test_gamma_selector_under_a_window_reproduces_the_fixture(golden):
    g = golden("qo_window")
    n, num, lo, hi = (int(g["fp_kw"][k]) for k in (0, 1, 3, 4))
    thresh = float(g["fp_kw"][2])
    keys = [f"fp{w}" for w in range(8)]
    x = np.stack([multi_sinusoid_window(int(g[f"{k}_seed"]), n) for k in keys])
    qo, eng = QOPeriods(), OracleEngine()
    _check_rows(g, keys, x, qo._find_periods_stepped(eng, x, qo._select_gamma(eng, lo, hi), num, thresh, hi, window=np.hanning(n)))


@pytest.mark.parametrize("tag", ["OB", "OC", "OE"])
def test_orthogonal_selector_under_a_window_reproduces_the_fixture(golden, tag):
    g = golden("qo_window_keep")
    n, win, num, thresh, max_length, trunc = o_group_kw(g, tag)
    keys = [f"{tag}{w}" for w in range(6)]
    x = np.stack([multi_sinusoid_window(int(g[f"{k}_seed"]), n) for k in keys])
    qo, eng = QOPeriods(trunc_to_integer_multiple=trunc, orthogonalize=True), OracleEngine()
    short = _check_rows(g, keys, x, qo._find_periods_stepped(eng, x, qo._select_orthogonal(eng, max_length), num, thresh,
                                                             max_length, window=win))
    if tag == "OE":
        assert any(short) and not all(short)


# ---------------------------------------------------------------------------- the scripted engine
N = 8
NOTHING, BAD = 0, -1  # script entries next to a period: no gamma norm is positive / the select's status is not OK


def stub_rows(W, zero=()):
    """Row w is [1, w + 2, 1, ...]: a residual is the row times a power of two, so x[1] / x[0] names the row exactly."""
    x = np.ones((W, N))
    x[:, 1] = np.arange(W) + 2
    x[list(zero)] = 0.0
    return x


class StubEngine:
    """`picks[r][w]`: what round r's select says of row w.  A fit of k periods gives row w k blocks of one row each, the
    weights 100 w + k and the residual ``x * scales.get((w, k), 0.5 ** k)``; its status is not OK for (w, k) in `bad`."""

    def __init__(self, picks, scales=None, bad=()):
        self.picks, self.scales, self.bad = picks, scales or {}, set(bad)
        self.selected, self.fitted = [], []  # the rows of every select / fit call

    @staticmethod
    def _ids(x):
        assert np.all(x[:, 0] != 0), "an all-zero row reached the engine"
        return [int(v) - 2 for v in x[:, 1] / x[:, 0]]

    def _script(self, x):
        ids = self._ids(x)
        self.selected.append(ids)
        return np.array([self.picks[len(self.selected) - 1][w] for w in ids])

    def sweep(self, x, p_lo, p_hi, mode, trunc, orth):
        vals = np.full((len(x), p_hi - p_lo + 1), -1.0)
        vals[:, 0] = np.nan  # (ordered below every number)
        for i, p in enumerate(self._script(x)):
            assert p != BAD
            if p != NOTHING:
                vals[i, p - p_lo :] = 0.25  # the first maximum is p
        return vals

    def qo_orth_select(self, x, max_p, trunc=False):
        p = self._script(x)
        assert NOTHING not in p
        st = np.where(p == BAD, _ffi.PH_ST_NO_PERIOD, _ffi.PH_ST_OK).astype(np.int32)
        return np.maximum(p, 1).astype(np.int32), np.full(len(x), 0.25), st

    def qo_fit_feasible(self, kcap, max_period, n=None, window=False):
        return kcap <= 512

    def qo_fit(self, x, periods, n_periods, kcap, max_period, window):
        ids = self._ids(x)
        self.fitted.append(ids)
        keeps = np.zeros(periods.shape, dtype=np.int32)
        wts = np.zeros((len(x), kcap))
        res = x.copy()
        st = np.zeros(len(x), dtype=np.int32)
        for i, (w, k) in enumerate(zip(ids, n_periods)):
            keeps[i, :k], wts[i, :k] = 1, 100 * w + k
            res[i] = x[i] * self.scales.get((w, int(k)), 0.5 ** int(k))
            if (w, int(k)) in self.bad:
                st[i] = _ffi.PH_ST_ITER_CAP
        return keeps, wts, res, st


def selector(qo, kind, eng, max_length=5):
    return qo._select_gamma(eng, 2, max_length) if kind == "gamma" else qo._select_orthogonal(eng, max_length)


KINDS = ("gamma", "orthogonal")


@pytest.mark.parametrize("kind", KINDS)
def test_num_below_one_hands_every_row_back(kind):
    qo, eng = QOPeriods(), StubEngine([])
    for num in (0, -3):
        assert qo._find_periods_stepped(eng, stub_rows(3), selector(qo, kind, eng), num, 0.1, 5, window=np.hanning(N)) == [None] * 3
    assert eng.selected == [] and eng.fitted == []


@pytest.mark.parametrize("orthogonalize", (False, True))
def test_batch_with_num_zero_under_a_window_returns(monkeypatch, orthogonalize):
    """find_periods(x2d, num=0) under an analysis window: what the 1-D call gives for every row, nothing raised."""
    eng = StubEngine([])
    monkeypatch.setattr(sys.modules[QOPeriods.__module__], "default_engine", lambda: eng)
    qo = QOPeriods(orthogonalize=orthogonalize)
    qo.window = np.hanning(N)
    x = stub_rows(3)
    out = qo.find_periods(x, num=0, thresh=0.1, max_length=5)
    one = QOPeriods(orthogonalize=orthogonalize)
    one.window = np.hanning(N)
    for w in range(3):
        want, wres = one.find_periods(x[w], num=0, thresh=0.1, max_length=5)
        assert out[w][0] == want and len(out[w][0]["periods"]) == 0 and np.array_equal(out[w][1], wres)
    assert eng.selected == [] and eng.fitted == []


@pytest.mark.parametrize("kind", KINDS)
def test_a_failed_fit_hands_its_row_back_alone(kind):
    """Row 1's two-period fit comes back not OK: it is None, and round 3 selects and fits rows 0 and 2 only."""
    qo, eng = QOPeriods(), StubEngine([[2, 3, 4], [3, 3, 5], [5, 5, 2]], bad={(1, 2)})
    out = qo._find_periods_stepped(eng, stub_rows(3), selector(qo, kind, eng), 3, 0.1, 5)
    assert eng.selected == [[0, 1, 2], [0, 1, 2], [0, 2]] and eng.fitted == [[0, 1, 2], [0, 1, 2], [0, 2]]
    assert out[1] is None
    for w, periods in ((0, [2, 3, 5]), (2, [4, 5, 2])):
        bases, res = out[w]
        assert list(bases["periods"]) == periods and bases["periods"].dtype == np.uint32
        assert list(bases["basis_dictionary"].items()) == [(str(p), 1) for p in periods]
        assert np.array_equal(bases["weights"], np.full(3, 100.0 * w + 3)) and np.array_equal(bases["norms"], np.full(3, 0.25))
        assert np.array_equal(res, stub_rows(3)[w] * 0.125)


@pytest.mark.parametrize("kind", KINDS)
def test_an_all_zero_row_is_never_selected_or_fitted(kind):
    qo, eng = QOPeriods(), StubEngine([[2, 0, 3], [3, 0, 4]])
    out = qo._find_periods_stepped(eng, stub_rows(3, zero=[1]), selector(qo, kind, eng), 2, 0.1, 5)
    assert eng.selected == [[0, 2]] * 2 and eng.fitted == [[0, 2]] * 2  # (StubEngine._ids asserts it as well)
    assert out[1] is None and list(out[0][0]["periods"]) == [2, 3] and list(out[2][0]["periods"]) == [3, 4]


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_the_test_function_stops_reports_one_period_fewer(kind):
    """Row 0's two-period fit leaves a reconstruction below thresh * rms(data): the test function stops it at the start
    of round 3 with one period reported and the weights, dictionary and residual of the two-period fit.  Row 1 runs on."""
    scale = 1.0 - 2.0**-10
    qo, eng = QOPeriods(), StubEngine([[2, 3], [3, 4], [None, 5]], scales={(0, 2): scale})
    out = qo._find_periods_stepped(eng, stub_rows(2), selector(qo, kind, eng), 3, 0.1, 5)
    assert eng.selected == [[0, 1], [0, 1], [1]] and eng.fitted == [[0, 1], [0, 1], [1]]
    bases, res = out[0]
    assert list(bases["periods"]) == [2] and np.array_equal(bases["norms"], [0.25])
    assert list(bases["basis_dictionary"].items()) == [("2", 1), ("3", 1)]
    assert np.array_equal(bases["weights"], [2.0, 2.0]) and np.array_equal(res, stub_rows(2)[0] * scale)
    assert list(out[1][0]["periods"]) == [3, 4, 5] and np.array_equal(out[1][0]["weights"], np.full(3, 103.0))


def test_gamma_nothing_left_finishes_a_fitted_row_and_hands_back_an_unfitted_one():
    """Row 0 finds no positive gamma norm in round 2 and is finished with its one period; row 1 finds none in round 1,
    was never fitted and is None; row 2 takes all three rounds."""
    qo, eng = QOPeriods(), StubEngine([[2, NOTHING, 3], [NOTHING, None, 4], [None, None, 5]])
    out = qo._find_periods_stepped(eng, stub_rows(3), selector(qo, "gamma", eng), 3, 0.1, 5, window=np.hanning(N))
    assert eng.selected == [[0, 1, 2], [0, 2], [2]] and eng.fitted == [[0, 2], [2], [2]]
    bases, res = out[0]
    assert list(bases["periods"]) == [2] and np.array_equal(bases["weights"], [1.0]) and np.array_equal(res, stub_rows(3)[0] * 0.5)
    assert out[1] is None and list(out[2][0]["periods"]) == [3, 4, 5]


def test_orthogonal_select_status_hands_the_row_back():
    """A select status that is not PH_ST_OK in round 2: None, although the row has a fit behind it."""
    qo, eng = QOPeriods(), StubEngine([[2, 3], [BAD, 4]])
    out = qo._find_periods_stepped(eng, stub_rows(2), selector(qo, "orthogonal", eng), 2, 0.1, 5)
    assert eng.fitted == [[0, 1], [1]] and out[0] is None and list(out[1][0]["periods"]) == [3, 4]


@pytest.mark.parametrize("kind", KINDS)
def test_a_65th_period_hands_the_row_back(kind):
    """Row 0 is picked a period in each of 65 rounds: None.  Row 1 stops after two and keeps its result.  The rule is
    tested after the select: round 65 selects, and fits nothing."""
    picks = [[2, 3], [3, BAD if kind == "orthogonal" else NOTHING]] + [[2 + r % 4, None] for r in range(2, 65)]
    qo, eng = QOPeriods(), StubEngine(picks)
    out = qo._find_periods_stepped(eng, stub_rows(2), selector(qo, kind, eng), 70, 0.1, 5)
    assert len(eng.selected) == 65 and len(eng.fitted) == 64 and eng.selected[64] == [0]
    assert out[0] is None
    if kind == "gamma":
        assert list(out[1][0]["periods"]) == [3]
    # with exactly 64 rounds the same row is finished with its 64 periods
    eng = StubEngine(picks)
    out = qo._find_periods_stepped(eng, stub_rows(2), selector(qo, kind, eng), 64, 0.1, 5)
    assert len(out[0][0]["periods"]) == 64 and np.array_equal(out[0][0]["weights"], np.full(64, 64.0))


def test_selector_preconditions_hand_every_row_back_without_a_launch():
    qo, eng = QOPeriods(), StubEngine([])
    for select in (qo._select_gamma(eng, 6, 5), qo._select_gamma(eng, 0, 5), qo._select_orthogonal(eng, 1)):
        assert qo._find_periods_stepped(eng, stub_rows(2), select, 3, 0.1, 5) == [None, None]
    assert eng.selected == [] and eng.fitted == []


# ---------------------------------------------------------------------------- the capacity ladder
class PlanStub:
    """qo_feasible of an engine whose LDS holds dictionaries of up to `rows` rows."""

    def __init__(self, rows):
        self.rows, self.asked = rows, []

    def qo_feasible(self, n, dtype, kcap, max_length):
        self.asked.append(kcap)
        return kcap <= self.rows

    def qo_fit_feasible(self, kcap, max_period, n=None, window=False):
        self.asked.append(kcap)
        return kcap <= self.rows


# (num, max_length, update_weights, max_rows, feasible up to) -> the capacities, worked out by hand: bound = num *
# max_length, room = bound rounded up to a multiple of 64 and at least 64
LADDERS = [
    # re-solved weights: start min(2048, room) for bound <= 2048, x2 up to 2048
    ((4, 100, True, None, 2048), [448, 896, 1792]),  # room 448; 3584 > 2048
    ((1, 10, True, None, 2048), [64, 128, 256, 512, 1024, 2048]),  # room 64
    ((16, 128, True, None, 2048), [2048]),  # bound 2048 exactly: still the first branch
    ((30, 100, True, None, 1024), [512, 1024]),  # bound 3000 > 2048: start 512; 2048 is not feasible
    ((4, 100, True, None, 300), [224]),  # 448 halved once; 448 is not feasible
    ((4, 100, True, None, 63), [56]),  # 448 -> 224 -> 112 -> 56, which is not halved again and is feasible; 112 is not
    ((4, 100, True, None, 0), []),  # nothing is feasible
    # fixed weights: start min(4096, room), x4 up to 2^20, the plan query is not asked (it would refuse: 0 rows)
    ((4, 100, False, None, 0), [448, 1792, 7168, 28672, 114688, 458752]),  # 1835008 > 2^20
    ((64, 100, False, None, 0), [4096, 16384, 65536, 262144, 1048576]),  # room 6400; 2^20 itself is in
    # max_rows clamps the start and the limit
    ((4, 100, True, 1000, 2048), [448, 896]),  # 1792 > 1000
    ((4, 100, True, 100, 2048), [100]),  # below the unclamped start 448, no multiple of 64
    ((4, 100, True, 10, 2048), [10]),  # below 64
    ((4, 100, True, 100, 60), [50]),  # 100 halved once; 100 <= limit but not feasible
    ((4, 100, False, 1000, 0), [448]),  # 1792 > 1000
    ((64, 100, False, 3000, 0), [3000]),  # room 6400 -> 4096 -> clamped
]


@pytest.mark.parametrize("case,want", LADDERS)
def test_capacity_ladder(case, want):
    num, max_length, update_weights, max_rows, rows = case
    eng = PlanStub(rows)
    assert list(_qo_capacities(eng, 600, np.float64, num, max_length, update_weights, max_rows)) == want
    if not update_weights:
        assert eng.asked == []


def test_capacity_ladder_asks_only_as_far_as_the_caller_goes():
    eng = PlanStub(2048)
    caps = _qo_capacities(eng, 600, np.float64, 4, 100, True)
    assert next(caps) == 448 and max(eng.asked) == 448  # nothing beyond the start was planned


# (max_rows, feasible up to) -> the capacities decompose_ramanujan gives ph_qo_fit, worked out by hand: 512, halved while
# above 1 and over max_rows or not feasible, then doubled while <= max_rows and feasible, max_rows itself the last step
INF = 1 << 30
RAM_LADDERS = [
    ((2048, INF), [512, 1024, 2048]),
    ((3000, INF), [512, 1024, 2048, 3000]),  # 4096 > 3000: max_rows itself
    ((512, INF), [512]),
    ((50, INF), [32, 50]),  # 512 -> ... -> 32 <= 50; 64 > 50: max_rows itself
    ((1, INF), [1]),
    ((2048, 700), [512]),  # 1024 is not feasible
    ((2048, 100), [64]),  # 512 -> 256 -> 128 -> 64; 128 is not feasible
    ((2048, 0), []),  # halved down to 1, which is not feasible either
]


@pytest.mark.parametrize("case,want", RAM_LADDERS)
def test_ramanujan_capacity_ladder(case, want):
    max_rows, rows = case
    assert list(_ram_capacities(PlanStub(rows), 600, 200, max_rows)) == want


@pytest.mark.parametrize("rows,want", [(INF, 512), (100, 64), (10, None)])
def test_qo_fit_start(rows, want):
    """The 512-to-64 start that RamanujanPeriods' batch and QOPeriods._fit_lists_device share; None: infeasible."""
    eng = PlanStub(rows)
    assert _qo_fit_start(lambda k: eng.qo_fit_feasible(k, 200)) == want
    assert min(eng.asked) >= 64  # never halved below the floor
