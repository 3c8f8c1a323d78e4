"""Case table of the short-window tests (test_short_windows_cpu.py, test_gpu_short_windows.py): window lengths 1 to 200,
the windows of every length, and the oracle calls with their decision margins.

Every length N has five windows, all seeded by N alone so that the CPU census and the GPU tests build the same arrays:
  (a) Gaussian noise;  (b) sin(2 pi n / 5 + 0.3) + 0.3 noise;  (c) a random max(2, N // 4)-periodic pattern + 0.2 noise;
  (d) all zeros;  (e) the constant 0.75 (k copies of it add up exactly, so the residual after the first projection is
  exactly zero: rsq == 0 in small_to_large, the status path of best_correlation).

`ref(op, x, **kw)` runs the oracle once per (op, window, parameters) and keeps the answer: ("ok", result, margin) or
("raises", None, None).  The margin is the smallest relative distance of any decision in the oracle's trace from
flipping; a case takes part in the "same period list" comparison only if it is at least MARGIN64 (float64 input) or
MARGIN32 (float32 input), and is held to status, and to every value bar wherever its list agrees, either way.
"""

import warnings

import numpy as np

from oracle import period_oracle as po

DENSE = tuple(range(1, 201))
FLAGS = tuple(range(1, 25)) + (31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 130, 191, 192, 193, 200)
SEED = 20260
MARGIN64, MARGIN32 = 1e-9, 1e-3
CAP64, CAP32 = 0.02, 0.10  # largest share of cases the margin rule may leave out, per op
KINDS = "abcde"
CONST = 0.75
NOISE = 1e-12  # a norm this far below the window's first winner is rounding noise (fp64: 1e-16 per operation)
RAISES = (TypeError, ValueError, OverflowError, ZeroDivisionError, IndexError, KeyError)  # KeyError: get_factors(1, True)


class LateRaise(Exception):
    pass


_WIN = {}
_NOISY = {}
_QO_TRACE = {}
_QO_CLEAR = {}
_REF = {}


def windows(n, dtype=np.float64):
    """(5, n) windows (a)-(e) of length n; float32: the float64 windows rounded (the oracle then runs on
    windows(n, np.float32).astype(np.float64))."""
    key = (n, np.dtype(dtype).name)
    if key not in _WIN:
        rng = np.random.default_rng([SEED, n])
        t = np.arange(n)
        a = rng.standard_normal(n)
        b = np.sin(2 * np.pi * t / 5 + 0.3) + 0.3 * rng.standard_normal(n)
        q = max(2, n // 4)
        c = rng.standard_normal(q)[t % q] + 0.2 * rng.standard_normal(n)
        x = np.stack([a, b, c, np.zeros(n), np.full(n, CONST)]).astype(dtype)
        x.setflags(write=False)
        _WIN[key] = x
    return _WIN[key]


def _m_best_margin(tr):
    leads = [r["lead"] for r in tr["step2"] if r["divisors"]]
    margins = [m for r in tr["step2"] if r["margins"] for m in r["margins"]]
    return min([tr["step1_min_gap"]] + leads + margins)


def _call(op, x, kw):
    if op == "m_best":
        tr = {}
        out = po.m_best(x, trace=tr, **kw)
        nrm = tr["step1_norms"]  # a step-1 winner at the rounding noise of an exactly fitted window: see noisy()
        return out, _m_best_margin(tr), (tr["step1_min_gap"], bool(np.min(nrm) <= NOISE * np.max(nrm)))
    if op == "small_to_large":
        tr = {}
        out = po.small_to_large(x, trace=tr, **kw)
        return out, tr["min_margin"], False
    if op == "best_correlation":
        tr = []
        try:
            out = po.best_correlation(x, trace=tr, **kw)
        except RAISES:
            if tr:  # a later round found every fold sum of the residual EXACTLY zero: see ref()
                raise LateRaise from None
            raise
        return out, min(min(lead, gap) for lead, gap, _ in tr), any(not best > NOISE * tr[0][2] for _, _, best in tr)
    if op == "best_frequency":
        tr = []
        out = po.best_frequency(x, trace=tr, **kw)
        return out, min(tr), False
    if op == "qo_find_periods":
        tr = []
        out = po.qo_find_periods(x, trace=tr, **kw)
        _QO_TRACE[id(x)] = tr
        return (out, min([(b - s) / b if b > 0 else 0.0 for b, s, _ in tr], default=1.0),
                not tr or any(not b > NOISE * tr[0][0] for b, _, _ in tr))
    raise AssertionError(op)


def ref(op, n, kind, dtype=np.float64, **kw):
    """The oracle's answer for window `kind` ("a".."e") of length n under `op`: ("ok", result, margin) or
    ("raises", None, None).  Computed once per case and shared.  best_correlation also answers ("raises late", None,
    None): the first round found a period and a later one none, because every fold sum of the residual is exactly zero.
    A float64 kernel that sums in the reference's order reproduces that and is held to it; float32 arithmetic on the same
    window leaves sums of 1e-8 instead, so for float32 input such a row may end either way."""
    key = (op, n, kind, np.dtype(dtype).name, tuple(sorted(kw.items())))
    if key not in _REF:
        x = windows(n, dtype)[KINDS.index(kind)].astype(np.float64)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            try:
                out, margin, _NOISY[key] = _call(op, x, kw)
                if op == "qo_find_periods":
                    tr = _QO_TRACE.pop(id(x))
                    real = [b > NOISE * tr[0][0] for b, _, _ in tr] if tr and tr[0][0] > 0 else []
                    _QO_CLEAR[key] = real.index(False) if False in real else len(real)
                margin = float(margin) if margin == margin else 0.0
                _REF[key] = ("ok", out, margin)
            except LateRaise:
                _REF[key] = ("raises late", None, None)
            except RAISES:
                _REF[key] = ("raises", None, None)
    return _REF[key]


def noisy(op, n, kind, dtype=np.float64, **kw):
    """Whether a round of the oracle's best_correlation / a selection of its qo_find_periods / a step-1 pick of its m_best
    for this case ran on the rounding noise of an exactly fitted window: its winning value is below NOISE of the first
    (m_best: of the largest) one, or it found nothing.
    With max_length <= 4 there are at most three candidate periods (one for best_correlation at N = 9 .. 11, whose
    range ends at max_length - 1) and num exhausts them; what the reference returns then -- the same period again, a
    dictionary entry of 0 rows -- hangs on whether a residual of 1e-17 is exactly zero, and the margin of such a pick
    (its lead over a runner-up of 0) says nothing.  These cases are left out of the period comparison beside the margin
    rule; the census pins them."""
    ref(op, n, kind, dtype, **kw)
    flag = _NOISY.get((op, n, kind, np.dtype(dtype).name, tuple(sorted(kw.items()))), False)
    return flag[1] if op == "m_best" and flag is not False else flag


def qo_real_picks(n, kind, dtype=np.float64, **kw):
    """How many selections of the oracle's qo_find_periods for this case come before the first one on rounding noise."""
    ref("qo_find_periods", n, kind, dtype, **kw)
    return _QO_CLEAR[("qo_find_periods", n, kind, np.dtype(dtype).name, tuple(sorted(kw.items())))]


def step1_gap(n, kind, dtype=np.float64, **kw):
    """The smallest relative lead of a step-1 winner of the oracle's m_best over its runner-up (1.0 where it raises).
    Near 0 the kernel may take the tied candidates in another order: a period picked again adds to its row, so even an
    equal final list can then carry other powers and bases."""
    ref("m_best", n, kind, dtype, **kw)
    return _NOISY.get(("m_best", n, kind, np.dtype(dtype).name, tuple(sorted(kw.items()))), (1.0, False))[0]


# the default parameter sets the census measures (the GPU tests add a second set per op)
CENSUS = {
    "m_best": dict(num=3),
    "m_best_gamma": dict(num=3, gamma=True),
    "small_to_large": dict(thresh=0.05),
    "best_correlation": dict(num=2),
    "best_frequency": dict(num=2),
    "qo_find_periods": dict(num=3, thresh=0.1),
}


def second_set(name, n):
    """The second parameter set of an op at length n as the GPU tests run it (None: not at this length)."""
    if name in ("m_best", "m_best_gamma"):
        return dict(num=3, min_length=1, max_length=n - 1, gamma=name == "m_best_gamma") if n >= 3 else None
    if name == "m_best_mid":  # the range up to N // 2: periods of 64 and more from N = 128, without the ties of N - 1
        return dict(num=3, min_length=2, max_length=n // 2) if n >= 6 else None
    if name == "small_to_large":
        return dict(thresh=0.02, n_periods=n - 1) if n >= 2 else None
    if name == "best_correlation":
        return dict(num=2, max_length=n, ratio=0.0)
    if name == "best_frequency":
        return dict(num=2, win_size=1 << n.bit_length())  # the next power of two above n
    return None


def census_ref(name, n, kind, dtype=np.float64, fn=ref):
    op = "m_best" if name == "m_best_gamma" else name
    kw = dict(CENSUS[name])
    if name == "qo_find_periods":
        kw.update(min_length=2, max_length=max(2, n // 3))
    return fn(op, n, kind, dtype, **kw)
