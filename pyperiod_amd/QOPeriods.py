"""Drop-in ``QOPeriods`` (quadratic-optimisation period finder) on the MI355X engine.

Mirrors the reference surface (pyPeriod/QOPeriods.py:148-1310).  The v1 reference class cannot
even be constructed (QOPeriods.py:190) and only its non-orthogonal ``find_periods`` branch runs
(SURVEY.md section 0); that branch is what is implemented here:

  * plain projection, default test function: the whole greedy loop (gamma sweep, phi-mass row
    bookkeeping, right-hand side by folds, matrix-free conjugate-gradient solve, reconstruction,
    residual) runs in ONE kernel launch per window batch -> ph_qo_find_periods
  * a (W, N) batch: one launch per batch, a greedy loop stepped from the host with two launches per round, or the
    1-D call row by row -- the table in ``QOPeriods._batch_path`` says which settings run where
  * other 1-D settings (custom test_function, update_weights=False, trunc, window, Ramanujan basis):
    the loop is driven from the host with the heavy pieces on the GPU -- the sweep (ph_sweep,
    QOPeriods.py:470-478), W = A x and A A^T as folds (ph_fold_sums, :781-782), A^T w
    (ph_tile_sum, :795) -- and the small dense solve on host LAPACK like the reference (:794).
"""

from __future__ import annotations

import warnings

import numpy as np

from . import _ffi
from ._factors import PRIMES, get_factors, get_primes, phi  # noqa: F401
from .engine import default_engine
from .Periods import Periods, _as_window, rms


def flatten(t: list) -> list:
    return [item for sublist in t for item in sublist]


def reduce_rows(A):
    """The rows of `A` that are not in the span of the rows above them, in order: a maximal independent subset
    (QOPeriods.py:86-94, which takes one SVD per row).  Here every row is tested against an orthonormal basis of the
    rows kept so far (two Gram-Schmidt passes, one matrix-vector product each).  Always 2-D -- the reference hands a
    rank-1 input back as its 1-D first row, which is what breaks its own ``get_periods``."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    basis = np.zeros((0, A.shape[1]))
    kept = []
    tol = max(A.shape) * np.finfo(np.float64).eps
    for i, row in enumerate(A):
        scale = np.linalg.norm(row)
        r = row - basis.T @ (basis @ row)
        r = r - basis.T @ (basis @ r)
        n = np.linalg.norm(r)
        if (n > tol * scale and scale > 0.0) or i == 0:
            kept.append(i)
            if n > 0.0:
                basis = np.vstack((basis, r / n))
    return A[kept]


def normalize(x, level: int = 1):
    """Scale so that max |x| == level (QOPeriods.py:119-145)."""
    x = np.asarray(x)
    return (x / np.max(np.abs(x))) * level


def ramanujan_sum(q: int) -> np.ndarray:
    """c_q(n) for n < q as exact integers: c_q(n) = sum_{d | gcd(n,q)} mu(q/d) d.  The reference
    evaluates the same numbers through complex exponentials (QOPeriods.py:1035-1044) and carries
    ~1e-12 of rounding noise on top of these integers."""
    q = int(q)
    mu = np.ones(q + 1, dtype=np.int64)
    is_comp = np.zeros(q + 1, dtype=bool)
    for i in range(2, q + 1):
        if not is_comp[i]:
            is_comp[2 * i :: i] = True
            mu[i::i] *= -1
            mu[i * i :: i * i] = 0
    n = np.arange(q)
    g = np.gcd(n, q)
    out = np.zeros(q, dtype=np.int64)
    for d in range(1, q + 1):
        if q % d == 0 and mu[q // d] != 0:
            out[g % d == 0] += mu[q // d] * d
    return out


def _to_f64(a):
    """float32 -> float64 copy of a (possibly large) residual batch, on torch's CPU threads when available."""
    try:
        import torch

        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64).numpy()
    except ImportError:
        return a.astype(np.float64)


def _device_window(window, n):
    """The analysis window as the float64 array ph_qo_fit_win takes, or None when it is not a finite 1-D array of n
    samples (None and False, the reference's "no window", among them)."""
    if window is None or window is False:
        return None
    try:
        win = np.ascontiguousarray(window, dtype=np.float64)
    except (TypeError, ValueError):
        return None
    return win if win.shape == (n,) and np.all(np.isfinite(win)) else None


_PICKED, _NOTHING_LEFT, _HAND_BACK = range(3)  # what a selector of QOPeriods._find_periods_stepped says of a row


def _hand_back_all(w):
    """A selector's answer when its precondition fails: (period, norm, fate) with all `w` rows handed back."""
    return np.zeros(w, dtype=np.int32), np.zeros(w), np.full(w, _HAND_BACK)


def _qo_capacities(eng, n, dtype, num, max_length, update_weights, max_rows=None):
    """The dictionary-row capacities (kcap) ph_qo_find_periods is given for windows of `n` samples, one after the other:
    the caller launches at each and asks for the next while rows end PH_ST_CAP.  Nothing is yielded when no capacity is
    feasible.  A block adds at most `max_length` rows, so the start has room for all `num` of them when that is at most
    2048 rows.  Re-solved weights live in LDS: the start is halved until the plan query accepts it, and doubles while
    that holds, up to 2048.  The fixed-weight loop keeps its weights in HBM only, where every capacity is feasible: up
    to 2^20 rows in steps of 4.  `max_rows` caps the start and the limit (the start may then be below 64, or no
    multiple of 64)."""
    bound = int(num) * int(max_length)
    room = max(64, -(-bound // 64) * 64)
    if update_weights:
        kcap, limit, step = (min(2048, room) if bound <= 2048 else 512), 2048, 2
    else:
        kcap, limit, step = min(4096, room), 1 << 20, 4
    if max_rows is not None:
        kcap, limit = min(kcap, max_rows), min(limit, max_rows)

    def feasible(k):
        return not update_weights or eng.qo_feasible(n, dtype, k, max_length)

    while kcap > 64 and not feasible(kcap):
        kcap //= 2
    while kcap <= limit and feasible(kcap):
        yield kcap
        kcap *= step


def _qo_fit_start(feasible):
    """The first capacity (kcap) ph_qo_fit / ph_ramanujan_fit are given where nothing caps it: 512 rows, halved while
    above 64 and not `feasible`.  -> that capacity, or None when it is not feasible either."""
    kcap = 512
    while kcap > 64 and not feasible(kcap):
        kcap //= 2
    return kcap if feasible(kcap) else None


def _ram_capacities(eng, n, max_period, max_rows):
    """The dictionary-row capacities (kcap) ph_qo_fit is given by ``ShortTime.decompose_ramanujan`` for frames of `n`
    samples and periods up to `max_period`, one after the other: 512 rows, halved until `max_rows` and the plan query
    accept them (down to 1, not 64 as in ``_qo_fit_start``: `max_rows` may ask for less), then doubled while both still
    do -- with `max_rows` itself as the last step when the doubling passes it.  Nothing is yielded when no capacity is
    feasible."""
    kcap = 512
    while kcap > 1 and (kcap > max_rows or not eng.qo_fit_feasible(kcap, max_period, n)):
        kcap //= 2
    while kcap <= max_rows and eng.qo_fit_feasible(kcap, max_period, n):
        yield kcap
        if kcap == max_rows:
            return
        kcap = min(2 * kcap, max_rows)


class _LazyBases(dict):
    """The output_bases dict of one row of a batched find_periods.  Its "subspaces" entry -- the stacked
    natural-basis rows of the dictionary blocks, rows x N doubles -- is built from the blocks on first read and
    kept; every other key is plain.  The accessors that read values build it: ``d[k]``, ``get``, ``pop``,
    ``setdefault``, ``items``, ``values``, ``copy``, ``==`` and copies by ``dict(d)`` / ``{**d}`` (iteration goes
    through keys() and ``d[k]``).  ``items`` and ``values`` return lists, not views; ``keys``, ``in`` and ``len``
    need nothing built."""

    def __init__(self, blocks, n, basis_type, **items):
        head = {k: items[k] for k in ("periods", "norms") if k in items}  # (compute_reconstruction reports no norms)
        super().__init__(**head, subspaces=None, weights=items["weights"], basis_dictionary=items["basis_dictionary"])
        self._blocks, self._n, self._basis_type = blocks, n, basis_type

    def _subspaces(self):
        if self._blocks is not None:
            rows = np.vstack([QOPeriods.Pp(q, self._n, k, self._basis_type) for q, k in self._blocks])
            dict.__setitem__(self, "subspaces", rows)
            self._blocks = None
        return dict.__getitem__(self, "subspaces")

    def __getitem__(self, key):
        if key == "subspaces":
            return self._subspaces()
        return dict.__getitem__(self, key)

    def __setitem__(self, key, value):
        if key == "subspaces":
            self._blocks = None
        dict.__setitem__(self, key, value)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __iter__(self):  # (a dict subclass with its own __iter__ is copied through keys() / __getitem__)
        return iter(dict.keys(self))

    def items(self):
        return [(k, self[k]) for k in dict.keys(self)]

    def values(self):
        return [self[k] for k in dict.keys(self)]

    def pop(self, key, *default):
        if key == "subspaces" and key in self:
            self._subspaces()
        return dict.pop(self, key, *default)

    def setdefault(self, key, default=None):
        if key in self:
            return self[key]
        return dict.setdefault(self, key, default)

    def __eq__(self, other):
        for d in (self, other):
            if isinstance(d, _LazyBases) and d._blocks is not None:
                d._subspaces()
        return dict.__eq__(self, other)

    __hash__ = None

    def copy(self):
        return dict(self)

    def __repr__(self):
        built = "built" if self._blocks is None else f"{sum(k if k else q for q, k in self._blocks)} x {self._n}, built on read"
        inner = ", ".join(f"{k!r}: {('<subspaces ' + built + '>') if k == 'subspaces' else repr(dict.__getitem__(self, k))}" for k in dict.keys(self))
        return "{" + inner + "}"


class QOPeriods(Periods):
    PRIMES = PRIMES  # QOPeriods.py:149-151

    def __init__(self, basis_type="natural", trunc_to_integer_multiple=False, orthogonalize=False):
        super().__init__(trunc_to_integer_multiple, orthogonalize)
        # attribute list of QOPeriods.py:191-199
        self._output = None
        self._basis_type = basis_type
        self._verbose = False
        self._k = 0
        self._window = False
        self._output_bases = None
        self._container = []

    # ------------------------------------------------------------------ detection
    def find_periods(self, data, num=None, thresh=None, min_length=2, max_length=None, update_weights=True, **kwargs):
        """Greedy period selection with re-solved weights (QOPeriods.py:313-596).
        Returns ``(dict(periods, norms, subspaces, weights, basis_dictionary), residual)``; a ``(W, N)``
        ndarray returns a list of W such tuples (see ``_find_periods_batch``; ``subspaces`` is built on first read).

        ``orthogonalize=True``: the v1 reference dies on this branch (``best_base`` is never
        assigned, QOPeriods.py:427-448).  Offered here as its commented-out lines intend: the
        period is chosen by the orthogonal (Muresan-Parks) powers -- ``get_best_period_orthogonal``
        on the device -- and its norm is that of the orthogonalised projection of the residual
        (QOPeriods.py:443-448); the solve is the same as in the plain branch."""
        if isinstance(data, np.ndarray) and data.ndim == 2:
            return self._find_periods_batch(data, num, thresh, min_length, max_length, update_weights, kwargs)
        data = _as_window(data)
        N = len(data)
        if max_length is None:
            max_length = int(np.floor(N / 3))
        if num is None:
            num = N
        if np.sum(np.abs(data)) <= 1e-16:  # QOPeriods.py:394-406
            self._output = {
                "periods": np.array([1]),
                "norms": np.array([0]),
                "subspaces": np.ones((1, N)),
                "weights": np.array([0]),
                "basis_dictionary": {"1": N},
            }
            return (self._output, np.zeros(N))
        custom_test = kwargs.get("test_function")
        windowed = not (self.window is None or self.window is False)
        if self._no_candidate(min_length, max_length, num, thresh, update_weights, windowed, kwargs):
            # windows of fewer than 3 * min_length samples with the default range: the reference's selection loop finds
            # nothing, fits an empty dictionary and stops at its second iteration (QOPeriods.py:470-478, :560-594) --
            # nothing is launched
            self._output_bases = {"periods": np.zeros(0, dtype=np.uint32), "norms": np.zeros(0), "subspaces": np.zeros((0, N)),
                                  "weights": np.zeros(0), "basis_dictionary": {}}
            return (self._output_bases, data.copy())
        on_device = (
            update_weights and custom_test is None and thresh is not None and not self._orthogonalize
            and not self._trunc_to_integer_multiple and self._basis_type == "natural" and not windowed
        )
        if on_device:  # the whole greedy loop in one launch, as a batch of one
            done = self._find_periods_device_batch(default_engine(), data[None, :], num, thresh, min_length, max_length, True)[0]
            if done is not None:  # (None: the dictionary does not fit the kernel's LDS layout or workspace)
                bases, residual = done
                # a plain dict, with "subspaces" built and the views into the launch's arrays copied
                self._output_bases = {k: v.copy() if k in ("periods", "norms", "weights") else v for k, v in bases.items()}
                return (self._output_bases, residual.copy())
        return self._find_periods_host(data, N, num, thresh, min_length, max_length, update_weights, custom_test)

    def _no_candidate(self, min_length, max_length, num, thresh, update_weights, windowed, kwargs):
        """The plain route (re-solved weights, default test function, natural basis, no window, not orthogonal) with an
        empty period range: the one case in which the reference returns its empty answer instead of selecting."""
        return (max_length < min_length and num >= 1 and thresh is not None and kwargs.get("test_function") is None
                and update_weights and not windowed and not self._orthogonalize and self._basis_type == "natural")

    def _batch_path(self, W, windowed, win, thresh, update_weights, kwargs):
        """Where a (W, N) batch runs.  ``common`` = default test function, `thresh` set, natural basis, not verbose;
        "device window" = ``self.window`` is a finite 1-D array of N samples (`win`):

            settings                                                              path
            common, orthogonal, update_weights, no window or device window        "orthogonal": stepped, ph_qo_orth_select
            common, plain, update_weights, device window                          "gamma": stepped, ph_sweep
            common, plain, no window -- or device window with fixed weights       "one launch"
            anything else                                                         None: the 1-D call on every row
        """
        common = kwargs.get("test_function") is None and thresh is not None and self._basis_type == "natural" and not self._verbose
        if not common or W == 0 or (windowed and win is None):
            return None
        if self._orthogonalize:
            return "orthogonal" if update_weights else None
        return "gamma" if windowed and update_weights else "one launch"

    def _find_periods_batch(self, data, num, thresh, min_length, max_length, update_weights, kwargs):
        """find_periods over a (W, N) batch: a list of W ``(output_bases, residual)`` tuples, each what the
        1-D call on that row returns (``output_bases`` becomes the list of the per-row dicts).  ``_batch_path`` has the
        table of which settings run where: in ONE launch per batch (``_find_periods_device_batch``: float32 batches in
        the fp32 kernels, residuals returned as float64), in a greedy loop stepped from the host with two launches per
        round (``_find_periods_stepped``), or row by row.  Every row a device path hands back -- a fallback status, a
        dictionary beyond the device's capacity -- runs the 1-D call too; all-zero rows get the reference's fixed
        answer there.

        ``"subspaces"`` of a device row is built from its ``basis_dictionary`` blocks on first read (W x rows
        x N doubles for the whole batch would not fit the host's memory at scale); reading it gives the array
        of the 1-D result."""
        W, N = data.shape
        windowed = not (self.window is None or self.window is False)
        win = _device_window(self.window, N) if windowed else None
        path = self._batch_path(W, windowed, win, thresh, update_weights, kwargs)
        if self._no_candidate(min_length, int(np.floor(N / 3)) if max_length is None else int(max_length),
                              N if num is None else int(num), thresh, update_weights, windowed, kwargs):
            path = None  # every row takes the 1-D call's empty answer
        out = [None] * W
        if path is not None:
            eng = default_engine()
            ml = int(np.floor(N / 3)) if max_length is None else int(max_length)
            n = N if num is None else int(num)
            # (the 1-D call works on the float64 copy of a row; only the one-launch kernels have an fp32 form)
            x = np.ascontiguousarray(data, dtype=np.float32 if path == "one launch" and data.dtype == np.float32 else np.float64)
        if path == "orthogonal":
            out = self._find_periods_stepped(eng, x, self._select_orthogonal(eng, ml), n, thresh, ml, window=win)
        elif path == "gamma":
            out = self._find_periods_stepped(eng, x, self._select_gamma(eng, int(min_length), ml), n, thresh, ml, window=win)
        elif path == "one launch":
            for w, r in enumerate(self._find_periods_device_batch(eng, x, n, thresh, min_length, ml, update_weights, window=win)):
                # all-zero rows (QOPeriods.py:394-406) go to the 1-D call.  A gamma norm is at most rms(x) <=
                # sum|x| / sqrt(N), so only rows whose first norm is <= 1e-16 need the sum of the 1-D test.
                if r is not None:
                    nrm = r[0]["norms"]
                    if (nrm.size == 0 or nrm[0] <= 1e-16) and np.sum(np.abs(x[w].astype(np.float64))) <= 1e-16:
                        r = None
                out[w] = r
        for w in range(W):
            if out[w] is None:  # the 1-D call on the row, whatever it is
                out[w] = self.find_periods(data[w], num, thresh, min_length, max_length, update_weights, **kwargs)
        self._output_bases = [r[0] for r in out]
        return out

    def _row_bases(self, blocks, n, periods, norms, weights):
        """The output_bases of one device row from its (period, rows kept) `blocks`."""
        return _LazyBases(blocks, n, self._basis_type, periods=periods, norms=norms, weights=weights,
                          basis_dictionary={str(q): k for q, k in blocks})

    def _find_periods_device_batch(self, eng, x, num, thresh, min_length, max_length, update_weights, window=None):
        """One ph_qo_find_periods launch for the batch `x` (and one more per capacity of ``_qo_capacities``, for the rows
        that needed it); with the float64 analysis window `window` (N, ``update_weights=False`` only) the launch is
        ph_qo_greedy_win.  -> list of (output_bases, residual) or None (the row goes to the 1-D call)."""
        W, N = x.shape
        trunc = bool(self._trunc_to_integer_multiple)
        results = [None] * W
        todo = np.arange(W)
        for kcap in _qo_capacities(eng, N, x.dtype, num, max_length, update_weights):
            xs = x if todo.size == W else x[todo]
            per, nrm, keeps, counts, wts, resid, st = eng.qo_find_periods(
                xs, num, thresh, min_length, max_length, kcap, trunc=trunc, update_weights=update_weights, window=window
            )
            if resid.dtype != np.float64:
                resid = _to_f64(resid)
            for i, w in enumerate(todo):
                if st[i] != _ffi.PH_ST_OK or counts[i, 1] == 0:
                    continue
                n_report, n_blocks = int(counts[i, 0]), int(counts[i, 1])
                blocks = [(int(per[i, b]), int(keeps[i, b])) for b in range(n_blocks)]
                n_rows = sum(k if k else q for q, k in blocks)
                # (views into the batch's output arrays)
                results[w] = (self._row_bases(blocks, N, per[i, :n_report], nrm[i, :n_report], wts[i, :n_rows]), resid[i])
            todo = todo[st == _ffi.PH_ST_CAP]
            if not todo.size:
                break
        return results

    def _select_gamma(self, eng, min_length, max_length):
        """The selector of the plain branch for ``_find_periods_stepped``: one ph_sweep launch, the gamma norms of the
        residuals over min_length .. max_length, and per row the first maximum if it is > 0 (NaN ordered below every
        number: the strict '>' scan of ``_strongest_period``), else nothing left."""
        trunc = bool(self._trunc_to_integer_multiple)

        def select(res):
            if max_length < min_length or min_length < 1:
                return _hand_back_all(res.shape[0])
            rows = np.arange(res.shape[0])
            vals = eng.sweep(res, min_length, max_length, _ffi.PH_SWEEP_NORM_GAMMA, trunc, False)
            order = np.where(np.isnan(vals), -np.inf, vals)
            k = np.argmax(order, axis=1)
            return min_length + k, vals[rows, k], np.where(order[rows, k] > 0, _PICKED, _NOTHING_LEFT)

        return select

    def _select_orthogonal(self, eng, max_length):
        """The selector of orthogonal (Muresan-Parks) selection for ``_find_periods_stepped``: one ph_qo_orth_select
        launch, per row the period by the normalised orthogonal powers over q < max_length and the norm of the
        orthogonalised projection (``_strongest_period`` for every row at once; ``min_length`` does not enter, as in the
        1-D call).  A status that is not PH_ST_OK (a non-finite power) hands the row back."""
        trunc = bool(self._trunc_to_integer_multiple)

        def select(res):
            if max_length < 2:  # (ph_qo_orth_select needs max_p >= 2)
                return _hand_back_all(res.shape[0])
            p, g, st = eng.qo_orth_select(res, max_length, trunc)
            return p, g, np.where(st == _ffi.PH_ST_OK, _PICKED, _HAND_BACK)

        return select

    def _find_periods_stepped(self, eng, x, select, num, thresh, max_length, window=None):
        """The greedy loop with re-solved weights for the float64 batch `x`, stepped from the host: per round one launch
        of `select` on the residuals of the rows still active and one ph_qo_fit launch on those rows with their lists so
        far -- ph_qo_fit_win under the float64 analysis window `window` (N), which only the fit sees -- instead of a
        dense dictionary, its uploads and a host solve per row and round.  ``select(residuals)`` -> (period, norm, fate)
        per row: _PICKED, _NOTHING_LEFT (the row is finished with the fit it has) or _HAND_BACK.  A row also stops when
        ``rms(reconstruction) > rms(data) * thresh`` fails -- its result is the last fit with one period fewer reported
        (QOPeriods.py:560-594) -- or after `num` rounds.
        -> per row (output_bases, residual), or None: the row is rerun whole by the 1-D call (all-zero rows, `num` < 1,
        a row handed back or with nothing left before its first fit, a fit that came back not PH_ST_OK -- a block
        without rows such as a period picked twice, an indefinite matrix, a dictionary beyond the largest feasible
        capacity -- and a 65th period, which is tested after the select)."""
        W, N = x.shape
        out = [None] * W
        if num < 1:
            return out
        per = np.zeros((W, 64), dtype=np.int32)
        counts = np.zeros(W, dtype=np.int32)
        gnorm = np.zeros((W, 64))
        fits = [None] * W  # (blocks, weights, residual) of the row's last fit
        res = x.copy()
        rms_data = np.sqrt(np.sum(x * x, axis=1) / N)
        active = np.flatnonzero(np.sum(np.abs(x), axis=1) > 1e-16)  # (QOPeriods.py:394-406: the 1-D call's fixed answer)

        def finish(w, n_report):
            blocks, wts, resid = fits[w]
            out[w] = (self._row_bases(blocks, N, per[w, :n_report].astype(np.uint32), gnorm[w, :n_report].copy(), wts), resid)

        for i in range(num):
            if i > 0:  # the test function on the reconstruction of the last fit
                rec = x[active] - res[active]
                go = np.sqrt(np.sum(rec * rec, axis=1) / N) > rms_data[active] * thresh
                for w in active[~go]:
                    finish(w, int(counts[w]) - 1)
                active = active[go]
            if active.size == 0:
                break
            p, g, fate = select(np.ascontiguousarray(res[active]))
            for w in active[fate == _NOTHING_LEFT]:  # every later round would repeat this one
                if fits[w] is not None:
                    finish(w, int(counts[w]))
            picked = (fate == _PICKED) & (counts[active] < 64)  # (a 65th period: the 1-D call)
            active, p, g = active[picked], p[picked], g[picked]
            if active.size == 0:
                break
            per[active, counts[active]] = p
            gnorm[active, counts[active]] = g
            counts[active] += 1
            fit = self._fit_lists_device(eng, np.ascontiguousarray(x[active]), np.ascontiguousarray(per[active]),
                                         np.ascontiguousarray(counts[active]), max_length, window=window)
            for w, r in zip(active, fit):
                if r is not None:
                    fits[w] = r
                    res[w] = r[2]
            active = active[np.array([r is not None for r in fit], dtype=bool)]
        for w in active:
            finish(w, int(counts[w]))
        return out

    def _strongest_period(self, eng, res, found, min_length, max_length, update_weights):
        """(period, gamma norm) of the residual `res`; period 0 = stop (QOPeriods.py:425-478)."""
        if not self._orthogonalize:  # plain gamma sweep, first maximum == strict '>' scan (:470-478)
            vals = eng.sweep(res[None, :], min_length, max_length, _ffi.PH_SWEEP_NORM_GAMMA, self._trunc_to_integer_multiple, False)[0]
            order = np.where(np.isnan(vals), -np.inf, vals)
            k = int(np.argmax(order))
            return (min_length + k, vals[k]) if order[k] > 0 else (0, 0)
        pows = eng.orth_powers(res[None, :], int(max_length), True)[0]
        if update_weights:  # :435-448
            best = int(np.argmax(pows))
            best = best if best > 0 else 1
        else:  # strongest power not found yet (:450-460)
            best = next((int(q) for q in np.argsort(-pows, kind="stable") if q not in found), 0)
        if best < 1:
            return 0, 0
        base = eng.project_batch(res[None, :], [best], self._trunc_to_integer_multiple, True)[0, 0]
        return best, eng.periodic_norm(base[None, :], best)[0]

    def _find_periods_host(self, data, N, num, thresh, min_length, max_length, update_weights, custom_test):
        """Host-driven greedy loop for the variants the single-launch kernel does not cover (custom
        test function, update_weights=False, trunc, window, Ramanujan basis, orthogonal selection).
        Heavy pieces stay on the GPU: the sweep (ph_sweep) or orthogonal powers (ph_orth_powers),
        W = A x and A A^T as folds (ph_fold_sums), A^T w (ph_tile_sum); the small dense solve uses
        host LAPACK like the reference (QOPeriods.py:794)."""
        eng = default_engine()
        keep_going = custom_test if custom_test is not None else (lambda _self, x, y: rms(y) > rms(data) * thresh)
        found = np.zeros(num, dtype=np.uint32)
        gnorm = np.zeros(num)
        state = {"A": np.empty((0, N)), "dims": {}, "w": np.array([]), "recon": None}
        res = data.copy()
        result = {"periods": [], "norms": [], "subspaces": [], "weights": [], "basis_dictionary": {}}

        def resolve(active):
            # update_weights: dictionary of all periods so far, weights re-solved against the data
            # (:598-643); otherwise only the newest period's rows are fitted to the residual (:645-714)
            if update_weights:
                state["A"], state["dims"], state["w"], state["recon"] = self._update_weights(data, N, active)
            else:
                state["A"], state["dims"], state["w"], state["recon"] = self._dont_update_weights(
                    res, N, active, state["w"], state["A"], state["dims"]
                )

        def report(active, count):
            return {
                "periods": active[:count],
                "norms": gnorm[:count],
                "subspaces": state["A"],
                "weights": state["w"],
                "basis_dictionary": state["dims"],
            }

        active = found[:0]
        for i in range(num):
            if i > 0 and not keep_going(self, data, state["recon"]):
                # the period added last broke the test: weights / dictionary of everything found are kept,
                # the period list drops its last entry (:560-594)
                resolve(active)
                result = report(active, len(active) - 1)
                self._output_bases = result
                break
            p, g = self._strongest_period(eng, res, found, min_length, max_length, update_weights)
            if self._orthogonalize and p < 1:
                break  # :441-442
            found[i], gnorm[i] = p, g
            if self._verbose:
                print(f"New period: {p}")
            active = found[found > 0]
            try:
                resolve(active)
            except np.linalg.LinAlgError:  # singular dictionary: keep the previous result (:552-559)
                break
            res = (data - state["recon"]) if update_weights else (res - state["recon"])
            result = report(active, len(active))
            self._output_bases = result
        return (result, res)

    def _solve_structured(self, x, basis_matrix, dictionary):
        """solve_quadratic for a natural-basis dictionary without touching the dense matrix
        on the compute side: W = A x and A A^T are folds, A^T w is a tile-sum."""
        if self._basis_type != "natural":
            return self.solve_quadratic(x, basis_matrix, window=self.window)
        eng = default_engine()
        p_list = [int(q) for q in dictionary.keys()]
        keep = [int(v) for v in dictionary.values()]
        win = self.window
        if win is None or win is False:
            rhs = eng.fold_sums(x[None, :], p_list, keep)[0]
            gram = eng.fold_sums(basis_matrix, p_list, keep)  # row (q,j) folded by p == (A A^T)^T
        else:
            rhs = eng.fold_sums((x * win)[None, :], p_list, keep)[0]
            gram = eng.fold_sums(basis_matrix * win, p_list, keep)
        weights = np.linalg.solve(gram.T, rhs)  # QOPeriods.py:794 (raises LinAlgError when singular)
        recon = eng.tile_sum(weights[None, :], x.size, p_list, keep)[0]
        return weights, recon

    def _update_weights(self, data, N, nonzero_periods):
        """QOPeriods.py:598-643."""
        basis_matricies, basis_dictionary = self.get_subspaces(nonzero_periods, N)
        output_weights, reconstruction = self._solve_structured(data, basis_matricies, basis_dictionary)
        return (basis_matricies, basis_dictionary, output_weights, reconstruction)

    def _dont_update_weights(self, data, N, nonzero_periods, output_weights, basis_matricies, basis_dictionary):
        """QOPeriods.py:645-714 (the v1 reference overflows here under numpy 2: uint32 periods
        reach Pp_column; periods are converted to int first)."""
        last = int(nonzero_periods[-1])
        keep = last
        factors = get_factors(last)
        existing = set()
        for p in nonzero_periods[:-1]:
            existing = existing.union(get_factors(int(p)))
        for f in sorted(existing.intersection(factors)):
            keep -= phi(f)
        basis_matrix = self.Pp(last, N, keep=keep, type=self._basis_type)
        weights, reconstruction = self._solve_structured(data, basis_matrix, {str(last): basis_matrix.shape[0]})
        basis_dictionary.update({str(last): keep})
        basis_matricies = np.vstack((basis_matricies, basis_matrix))
        output_weights = np.concatenate((output_weights, weights))
        return (basis_matricies, basis_dictionary, output_weights, reconstruction)

    # ------------------------------------------------------------------ linear algebra
    @staticmethod
    def solve_quadratic(x, A, type: str = "solve", window=None, k: int = 0):
        """Generic dense form (QOPeriods.py:743-805): A' = A A^T, W = A x, solve, A^T w.
        The two dense products are plain library GEMMs and run through rocBLAS
        (torch.matmul on the GPU); the small solve uses host LAPACK like the reference."""
        import torch

        eng = default_engine()
        dev = torch.device("cuda", eng.device)
        At = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float64), device=dev)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
        Aw = At if (window is None or window is False) else At * torch.as_tensor(np.asarray(window, dtype=np.float64), device=dev)
        A_prime = (Aw @ At.T).cpu().numpy()
        W = (Aw @ xt).cpu().numpy()
        if type == "solve":
            output = np.linalg.solve(A_prime, W)
        else:
            if type != "lstsq":
                warnings.warn("type ({}) unrecognized. Defaulting to lstsq.".format(type))
            output = np.linalg.lstsq(A_prime, W, rcond=None)[0]
        reconstructed = (At.T @ torch.as_tensor(output, device=dev)).cpu().numpy()
        return (output, reconstructed)

    def get_subspaces(self, Q, N: int):
        """Stacked natural-basis rows and the {period: rows kept} dictionary
        (QOPeriods.py:807-852)."""
        old_dimensionality = 0
        d = {}
        R = set()
        for q in Q:
            R = R.union(get_factors(int(q)))
            s = int(np.sum([phi(r) for r in R]))
            d[str(q)] = s - old_dimensionality
            old_dimensionality = s
        blocks = [self.Pp(int(q), N, keep, self._basis_type) for q, keep in d.items()]
        A = np.vstack(blocks) if blocks else np.array([]).reshape((0, N))
        return (A, d)

    def _fit_lists_device(self, eng, x, per, counts, max_period, first=None, window=None):
        """Fit the period lists per[w, :counts[w]] (int32, at most 64 columns) to the rows of the float32 / float64 batch
        `x` with ph_qo_fit, or under the float64 analysis window `window` (N) with ph_qo_fit_win.  `first` = (kcap,
        keeps, weights, residual, status) of a launch that already ran on these lists (ph_ramanujan_fit).  Capacity grows
        by re-running only the PH_ST_CAP rows while the plan query says the larger kcap fits.  -> per row None (the
        caller runs its 1-D call) or (blocks, weights, float64 residual)."""
        W, N = x.shape
        out = [None] * W

        def feasible(kcap):
            return eng.qo_fit_feasible(kcap, max_period, N, window is not None)

        def take(todo, kcap, keeps, wts, resid, st):
            if resid.dtype != np.float64:
                resid = _to_f64(resid)
            for i, w in enumerate(todo):
                if st[i] != _ffi.PH_ST_OK:
                    continue
                blocks = [(int(per[w, b]), int(keeps[i, b])) for b in range(int(counts[w]))]
                out[w] = (blocks, wts[i, : sum(k for _, k in blocks)], resid[i])
            # a list longer than the device's 64 blocks stays PH_ST_CAP at every capacity
            return todo[(st == _ffi.PH_ST_CAP) & (counts[todo] <= per.shape[1])]

        if first is None:
            kcap = _qo_fit_start(feasible)
            if kcap is None:
                return out
            todo = np.arange(W)
            todo = take(todo, kcap, *eng.qo_fit(x, per, counts, kcap, max_period, window))
        else:
            kcap = first[0]
            todo = take(np.arange(W), *first)
        while todo.size:
            nxt = 2 * kcap
            if not feasible(nxt):  # the last feasible capacity below the doubling, in steps of 64
                lo, hi = kcap // 64, nxt // 64
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (mid, hi) if feasible(64 * mid) else (lo, mid)
                nxt = 64 * lo
            if nxt <= kcap:
                break
            kcap = nxt
            todo = take(todo, kcap, *eng.qo_fit(np.ascontiguousarray(x[todo]), np.ascontiguousarray(per[todo]),
                                                np.ascontiguousarray(counts[todo]), kcap, max_period, window))
        return out

    def _compute_reconstruction_batch(self, x, periods, type, window):
        """compute_reconstruction over a (W, N) batch: `periods` is one list for every row or a list of W lists.  A list
        of W ``(reconstruction, output_bases)`` tuples (``None`` where the 1-D call returns ``None``), each what the 1-D
        call on that row returns.  Natural basis: one launch per batch -- ph_qo_fit without an analysis window
        (``window=None``), ph_qo_fit_win under one (a finite 1-D array of N samples) -- float32 batches in the fp32
        kernel, ``subspaces`` built on first read; rows the kernel hands back (singular, indefinite or ill-conditioned
        dictionaries, more than 64 periods or more rows than the LDS holds) and every other setting (``window=False``
        among them) run the 1-D call on the row.  ``type`` only reaches the 1-D calls."""
        W, N = x.shape
        per_row = len(periods) == W and W > 0 and all(np.ndim(p) == 1 for p in periods)
        lists = [periods[w] if per_row else periods for w in range(W)]
        out = [None] * W
        done = [False] * W
        win = _device_window(window, N)
        if (window is None or win is not None) and self._basis_type == "natural" and W > 0:
            xs = np.ascontiguousarray(x if x.dtype in (np.float32, np.float64) else x.astype(np.float64))
            arrs = [np.asarray(p).astype(np.int64).reshape(-1) for p in lists]
            counts = np.array([a.size for a in arrs], dtype=np.int32)
            per = np.zeros((W, 64), dtype=np.int32)
            for w, a in enumerate(arrs):
                per[w, : min(a.size, 64)] = np.clip(a[:64], -1, (1 << 20) + 1)  # (out-of-range entries stay out of range)
            max_period = int(min(max(1, per.max()), 1 << 20))
            x64 = xs if xs.dtype == np.float64 else _to_f64(xs)
            for w, r in enumerate(self._fit_lists_device(default_engine(), xs, per, counts, max_period, window=win)):
                if r is None:
                    continue
                blocks, wts, resid = r
                bases = _LazyBases(blocks, N, self._basis_type, periods=lists[w], weights=wts,
                                   basis_dictionary={str(q): k for q, k in zip(lists[w], (k for _, k in blocks))})
                out[w], done[w] = (x64[w] - resid, bases), True
        for w in range(W):
            if not done[w]:  # the 1-D call on the row, whatever it is
                out[w] = self.compute_reconstruction(x[w], lists[w], type, window)
        return out

    def compute_reconstruction(self, x, periods, type: str = "lstsq", window=None):
        """QOPeriods.py:1054-1116.  A ``(W, N)`` ndarray with one period list or a list of W lists returns a list of W
        results (see ``_compute_reconstruction_batch``)."""
        if isinstance(x, np.ndarray) and x.ndim == 2:
            return self._compute_reconstruction_batch(x, periods, type, window)
        basis_matricies, basis_dictionary = self.get_subspaces(periods, len(x))
        try:
            output_weights, reconstruction = self.solve_quadratic(x, basis_matricies, window=window, type=type)
        except np.linalg.LinAlgError:
            return None
        output_bases = {
            "periods": periods,
            "subspaces": basis_matricies,
            "weights": output_weights,
            "basis_dictionary": basis_dictionary,
        }
        return (reconstruction, output_bases)

    def get_periods(self, weights, dictionary, decomp_type="row reduction"):
        """One waveform per period from the weights of a fit (QOPeriods.py:719-741): the dictionary's segments with
        what two or more periods share redistributed among them, ``c - P c`` with ``P`` the orthogonal projector onto
        the rows of ``stack_pairwise_gcd_subspaces``.  Returns a tuple of float64 arrays, one of ``int(q)`` samples per
        key ``q`` of `dictionary` in its order; tiling and adding them reproduces the reconstruction.  The 1-D call is
        a batch of one through k_qo_extract (ph_qo_get_periods, closed form); there is no CPU path.

        Batch form: `weights` a list / tuple of W arrays and `dictionary` a list / tuple of W dicts -- e.g.
        ``[b["weights"] for b in qo.output_bases], [b["basis_dictionary"] for b in qo.output_bases]`` after a batched
        ``find_periods`` -- returns a list of W tuples from one launch.  A row that would raise in the 1-D call makes
        the batch raise the same exception with the row named.

        Deviations from the reference, which cannot run this method in v1 (``self._k`` lands in the positional ``type``
        of solve_quadratic: TypeError) and, with that call repaired, raises ``LinAlgError`` for the default
        ``decomp_type="row reduction"`` on one period or two coprime periods (``reduce_rows`` returns a 1-D row) and for
        ``"lu"`` with three or more periods (singular ``U``): every `decomp_type` is a factorisation of the same
        projector, and all of them return the projector's result here; ``self._k`` is ignored as the reference ignores
        it.  Mirrored: one period alone returns ``c - mean(c)`` and an empty dictionary raises ValueError."""
        batch = isinstance(dictionary, (list, tuple))
        dicts = list(dictionary) if batch else [dictionary]
        wlist = list(weights) if batch else [weights]
        if len(wlist) != len(dicts):
            raise ValueError(f"get_periods: {len(wlist)} weight arrays for {len(dicts)} dictionaries")
        W = len(dicts)
        if W == 0:
            return []

        def named(w, exc):
            return type(exc)(f"get_periods: row {w}: {exc}") if batch else exc

        keys, rows, blocks = [], [], []
        for w, (wt, d) in enumerate(zip(wlist, dicts)):
            if len(d) == 0:
                raise named(w, ValueError("empty dictionary (the reference's matmul has nothing to multiply)"))
            wt = np.asarray(wt, dtype=np.float64).reshape(-1)
            per = [int(q) for q in d.keys()]
            kp, bl, read = [], [], 0
            for q, r in zip(per, d.values()):
                # concatenate_periods' own slice semantics: an entry with more rows than its period keeps what the
                # slice assignment keeps (the all-zero answer {"1": N} with one weight among them)
                try:
                    seg = self.concatenate_periods(wt[read:], {str(q): r})
                except ValueError as exc:
                    raise named(w, exc) from None
                k = int(r) if 0 <= int(r) <= q else q
                read += int(r)
                kp.append(k)
                bl.append(seg[:k])
            keys.append(per)
            rows.append(kp)
            blocks.append(np.concatenate(bl) if bl else np.zeros(0))
        pcap = max(len(k) for k in keys)
        kcap = max(1, max(b.size for b in blocks))
        per = np.zeros((W, pcap), dtype=np.int32)
        rws = np.zeros((W, pcap), dtype=np.int32)
        wts = np.zeros((W, kcap), dtype=np.float64)
        counts = np.array([len(k) for k in keys], dtype=np.int32)
        for w in range(W):
            per[w, : counts[w]] = np.clip(keys[w], -1, (1 << 20) + 1)  # (out-of-range entries stay out of range)
            rws[w, : counts[w]] = rows[w]
            wts[w, : blocks[w].size] = blocks[w]
        out, status = default_engine().qo_get_periods(per, rws, counts, wts)
        result = []
        for w in range(W):
            if status[w] != _ffi.PH_ST_OK:
                why = "a repeated period, or a period outside 1 .. 2^20" if status[w] == _ffi.PH_ST_ITER_CAP else f"status {int(status[w])}"
                raise named(w, ValueError(f"dictionary {dicts[w]!r} cannot be extracted ({why})"))
            edges = np.concatenate(([0], np.cumsum(keys[w])))
            result.append(tuple(out[w, a:b].copy() for a, b in zip(edges[:-1], edges[1:])))
        return result if batch else result[0]

    @staticmethod
    def stack_pairwise_gcd_subspaces(periods):
        """The rows whose span get_periods projects out (QOPeriods.py:889-938): for every pair a < b of `periods` and
        every shift i < g = gcd(p_a, p_b) one row over the concatenated segments with -1 on segment a and +1 on
        segment b at the indices = i (mod g), zeros elsewhere.  One period gives ones((1, p)), none ones((1, 1)).
        A host table like ``Pp`` (the device path never builds it)."""
        per = np.asarray(periods, dtype=np.int64).reshape(-1)
        if per.size == 0:
            return np.ones((1, 1))
        if per.size == 1:
            return np.ones((1, int(per[0])))
        ia, ib = np.triu_indices(per.size, 1)  # the pairs in itertools.combinations order
        g = np.gcd(per[ia], per[ib])
        pair = np.repeat(np.arange(ia.size), g)  # pair of every row
        shift = np.arange(g.sum()) - np.repeat(np.cumsum(g) - g, g)  # its shift
        seg = np.repeat(np.arange(per.size), per)  # segment of every column
        idx = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)  # index inside it
        hit = idx[None, :] % g[pair][:, None] == shift[:, None]
        sign = (seg[None, :] == ib[pair][:, None]).astype(np.float64) - (seg[None, :] == ia[pair][:, None])
        return np.where(hit, sign, sign * 0.0)

    @staticmethod
    def concatenate_periods(weights, dictionary):
        """QOPeriods.py:854-887."""
        read_idx = 0
        output = []
        for q, r in dictionary.items():
            v = np.zeros(int(q))
            v[0:r] = weights[read_idx : read_idx + r]
            read_idx += r
            output.append(v)
        return np.array(flatten(output))

    # ------------------------------------------------------------------ dictionaries (host tables)
    @staticmethod
    def Pp(p: int, N: int = 1, keep: int = None, type: str = "natural") -> np.ndarray:
        """Natural (indicator) or Ramanujan basis rows (QOPeriods.py:940-974)."""
        p, N = int(p), int(N)
        if type == "natural":
            matrix = (np.arange(N)[None, :] % p == np.arange(p)[:, None]).astype(np.float64)
        elif type == "ramanujan":
            reps = int(np.ceil(N / p))
            matrix = np.stack([QOPeriods.Cq(p, i, reps, "real")[:N] for i in range(p)])
        else:
            matrix = np.zeros((p, N))
        return matrix[:keep] if keep else matrix

    @staticmethod
    def Pp_column(p: int, s: int, repetitions: int = 1):
        """[.., 1 at (index - s) % p == 0, ..] tiled (QOPeriods.py:976-1003)."""
        p, s = int(p), int(s)
        vec = ((np.arange(p) - s) % p == 0).astype(np.float64)
        return np.tile(vec, repetitions)

    @staticmethod
    def Cq(q: int, s: int = 0, repetitions: int = 1, type: str = "real"):
        """Ramanujan sum c_q rolled by s and tiled (QOPeriods.py:1005-1052)."""
        vec = np.tile(np.roll(ramanujan_sum(q).astype(np.float64), s), repetitions)
        return vec.astype(complex) if type == "complex" else vec

    # ------------------------------------------------------------------ orthogonal period powers
    def auto_corr(self, x, k):
        """sum_n x[n] x[n+k] (QOPeriods.py:1151-1173)."""
        x = _as_window(x)
        return np.float64(default_engine().orth_powers(x[None, :], 2, want_autocorr=True)[1][0, int(k)])

    def eq_3(self, x, P):
        """Equation 3 of Muresan & Parks (QOPeriods.py:1122-1149)."""
        x = _as_window(x)
        P = int(P)
        return np.float64(default_engine().orth_powers(x[None, :], max(P + 1, 2), want_eq3=True)[1][0, P])

    def get_best_period_orthogonal(self, x, max_p=None, normalize=False, return_powers=False):
        """Strongest period by orthogonal (factor-subtracted) powers (QOPeriods.py:1175-1232)."""
        x = _as_window(x)
        if max_p is None:
            max_p = len(x) // 2
        pows = default_engine().orth_powers(x[None, :], int(max_p), normalize)[0]
        if return_powers:
            return pows
        best = int(np.argmax(pows))
        return best if best > 0 else 1  # Q[argmax] - 1 == argmax (QOPeriods.py:1227-1232)

    # ------------------------------------------------------------------ properties (QOPeriods.py:1237-1310)
    @property
    def basis_type(self):
        return self._basis_type

    @basis_type.setter
    def basis_type(self, value):
        self._basis_type = value

    @property
    def verbose(self):
        return self._verbose

    @verbose.setter
    def verbose(self, value):
        self._verbose = value

    @property
    def k(self):
        return self._k

    @k.setter
    def k(self, value):
        self._k = value

    @property
    def window(self):
        return self._window

    @window.setter
    def window(self, value):
        self._window = value

    @property
    def output_bases(self):
        return self._output_bases
