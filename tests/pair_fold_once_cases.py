"""Case table of the fold-once path of k_mbest_step1_pair (test_pair_fold_once_cpu.py, test_gpu_pair_fold_once.py): the
windows, and a restatement in numpy of what picks the path of a window-sweep behind the screen
(pyperiod_amd/csrc/ph_mbest.h, ph_pair.h):

  scan      the screened ("top") periods q in [p_scr, max_length] whose upper bound reaches the best lower bound are
            listed, with the unskipped divisors below p_scr of every such period, skipped or not;
  path      fold-once when the window is usable, the list did not overflow, it holds exactly one top period m, every
            other entry divides m, and m > kPairSmallP -- otherwise the staged phases ("fallback: ...");
  thinning  m stays alone when every listed divisor has T_d < E_m - |E_m| 1e-9 - band ssq; otherwise the window-sweep
            falls back to the staged phases, thinning included ("fallback: tie").

The restatement works on the EXACT values E_q = sum_j S_q[j]^2 / cnt_q[j] (fp64, the oracle's fold) in place of the float
screen.  A float value lies within pair_radius x ssq of E_q, so a top period is listed for certain when it is within 1e-9
(relative) of the largest, and left out for certain when it is further below it than the radii allow; `trace` REJECTS
(raises Ambiguous) a window in which a top period is neither -- the margin is MARGIN = 10 radii --, or in which the
thinning verdict is closer to its threshold than four times the bound on the fp64 rounding of T_d and E_m.  So the path
of every window-sweep of an admitted case is known without the float screen's rounding.

A case is a dict: name, n, num, min_length, max_length, gamma, and `windows`, a tuple of window kinds:
  sin:S            multi_sinusoid_window(S, n) (pyperiod_amd.synth)
  plant:a,b*amp    zero-mean random patterns tiled at the periods a, b, .. (amplitude after '*') + 1e-3 noise
  int:d            an integer pattern of period d and nothing else: every fold of it is exact in any order
  near:d:m:ratio   a random pattern of period d + eps x a pattern of period m (d | m) + 1e-6 noise, eps tuned by bisection
                   on the exact values so that (E_m - E_d) / E_m = ratio on the first sweep
  pair1e9:side     the two planted components of tests/test_gpu_pair.py (periods 61 and 67: the families of 305 and 268),
                   2e-10 (relative) to either side of the crossing of their exact norms: both are listed for certain
  noise:S          white noise, seed S
  zeros, nan       all 0.0; sin:3 with x[100] = NaN
  2^k              sin:4 times 2^k
"""

import zlib

import numpy as np

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_window

SEED = 20268
K_PAIR_SMALL_P = 256  # ph_pair.h kPairSmallP
K_PAIR_LIST_CAP = 96  # ph_pair.h kPairListCap
BLOCK = 1024  # threads of k_mbest_step1_pair: a period above it gives some threads two columns
MARGIN = 10.0  # radii between a top period that is "certainly not listed" and the largest value
U24 = 2.0 ** -24


class Ambiguous(Exception):
    """The path of a window-sweep would hang on the float screen's rounding (or on fp64 rounding at the thinning threshold)."""


def rows(n, p):
    return -(-n // p)


def pair_radius(n, q):
    """ph_pair.h pair_radius(ceil(N / q), q)."""
    return 1.5 * (2.0 * rows(n, q) + (q >> 6) + 32.0) * U24


def cover_slack(n):
    """ph_pair.h pair_cover_slack."""
    return max(9.094947017729282e-13, (2.0 * n + 32.0) * 2.220446049250313e-16)


def thin_band(n):
    """ph_pair.h pair_thin_band."""
    return 5.0 * cover_slack(n)


def usable(rsq):
    """ph_pair.h pair_usable."""
    return 0.0 < rsq < 1.79e308


def exact_value(work, q):
    """E_q = sum_j S_q[j]^2 / cnt_q[j] in fp64."""
    s = po.fold_sums(work, q)
    return float(np.sum(s * s / po.fold_counts(work.size, q)))


def divisors(m, lo, hi):
    """proper divisors of m in [lo, hi)"""
    return [d for d in range(max(lo, 1), min(hi, m)) if m % d == 0]


def screen_lo(lo, hi, gamma, cover=True):
    """period_hip.hip pair_screen_lo."""
    return max(lo, hi // 2 + 1) if cover and not gamma else lo


def sweep_path(work, skip, lo, hi, gamma):
    """The path of one window-sweep -> dict(path, listed, m).  Raises Ambiguous."""
    n = work.size
    with np.errstate(all="ignore"):
        rsq = float(np.sum(work * work))
    if not usable(rsq):
        return dict(path="exact_all", listed=None, m=0)
    p_scr = screen_lo(lo, hi, gamma)
    cover = p_scr > lo
    tops = list(range(p_scr, hi + 1))
    live = [q for q in tops if q not in skip]
    if not live:
        return dict(path="exact_all: every screened period skipped", listed=None, m=0)
    val = {q: exact_value(work, q) / (q if gamma else 1) for q in tops}
    rad = {q: pair_radius(n, q) * rsq / (q if gamma else 1) for q in tops}
    qmax = max(live, key=lambda q: val[q])
    vmax = val[qmax]
    slack = cover_slack(n) * rsq if cover else 0.0
    hit = []
    for q in tops:
        gap = vmax - val[q]
        if gap <= 1e-9 * abs(vmax) + slack:
            hit.append(q)
        elif gap < MARGIN * (rad[q] + rad[qmax]) + slack + 1e-9 * abs(vmax):
            raise Ambiguous(f"top period {q}: {gap / rsq:.3e} ssq below period {qmax}, radius {rad[q] / rsq:.3e}")
    listed = [q for q in hit if q not in skip]
    if cover:
        seen = set()
        for q in hit:
            for d in divisors(q, lo, p_scr):
                if d not in skip and d not in seen:
                    seen.add(d)
                    listed.append(d)
    if len(listed) > K_PAIR_LIST_CAP:
        return dict(path="fallback: list overflow", listed=listed, m=0)
    top_listed = [q for q in listed if q >= p_scr]  # (never empty: the best unskipped top period is always listed)
    if len(top_listed) > 1:
        return dict(path="fallback: two top periods", listed=listed, m=0)
    m = top_listed[0]
    if any(m % d for d in listed):
        return dict(path="fallback: divisors of a skipped top period listed", listed=listed, m=m)
    if m <= K_PAIR_SMALL_P:
        return dict(path="fallback: short winner", listed=listed, m=m)
    others = [d for d in listed if d != m]
    if others:
        e_m = exact_value(work, m)
        t_max = max(exact_value(work, d) for d in others)
        thr = e_m - abs(e_m) * 1e-9 - thin_band(n) * rsq * (1.0 + 1e-9)
        edge = 4.0 * cover_slack(n) * rsq
        if abs(t_max - thr) <= edge:
            raise Ambiguous(f"thinning: a divisor of {m} is {(t_max - thr) / rsq:.3e} ssq from the threshold")
        if t_max > thr:
            return dict(path="fallback: tie", listed=listed, m=m, lead=(e_m - t_max) / e_m)
    return dict(path="fold: m > block" if m > BLOCK else "fold: m <= block", listed=listed, m=m)


def trace(x, num, lo, hi, gamma=False, max_sweeps=200):
    """Step 1 of the oracle (Periods.py:494-537) sweep by sweep -> list of dict(path, m, winner, action, first)."""
    x = np.asarray(x, dtype=np.float64)
    work, periods, skip, repeats, out = x.copy(), [], set(), 0, []
    while len(periods) < num and len(out) < max_sweeps:
        rec = sweep_path(work, skip, lo, hi, gamma)
        with np.errstate(all="ignore"):
            v = po.sweep_norms(work, lo, hi, gamma)
        for s in skip:
            v[s - lo] = -1.0
        v = np.where(v == v, v, -1.0)
        if not v.max() > 0:  # the reference fails here (Periods.py:520/537); the kernels report status 1
            rec.update(winner=0, action=None, first=not out)
            out.append(rec)
            break
        top = lo + int(np.argmax(v))
        if rec["path"].startswith("fold") and top != rec["m"]:
            raise Ambiguous(f"fold-once at {rec['m']} but the oracle takes {top}")
        if top in periods and repeats < 10:
            action, repeats = 2, repeats + 1
        elif top in periods:
            action, repeats = 0, 0
            skip.add(top)
        else:
            action, repeats = 1, 0
            periods.append(top)
        rec.update(winner=top, action=action, first=not out)
        out.append(rec)
        work = work - po.project(work, top)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Windows
# ------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([SEED] + [zlib.crc32(str(k).encode()) for k in key])


def _pattern(rng, p, n):
    pat = rng.standard_normal(p)
    return (pat - pat.mean())[np.arange(n) % p]


def _bisect(f, lo, hi, steps=200):
    """f increasing, f(lo) < 0 < f(hi)"""
    assert f(lo) < 0 < f(hi)
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
    return lo, hi


def near_tie(n, d, m, ratio):
    rng = _rng("near", n, d, m)
    a, b, noise = _pattern(rng, d, n), _pattern(rng, m, n), 1e-6 * rng.standard_normal(n)

    def lead(eps):
        x = a + eps * b + noise
        e_m = exact_value(x, m)
        return (e_m - exact_value(x, d)) / e_m - ratio

    lo, hi = _bisect(lead, 0.0, 1e-2)
    return a + hi * b + noise


def pair_planted(n, b):
    """tests/test_gpu_pair.py::_planted: components of period 61 and 67 (amplitude b) + 1e-3 noise."""
    rng = np.random.default_rng(3)
    t = np.arange(n)
    return rng.standard_normal(61)[t % 61] + b * rng.standard_normal(67)[t % 67] + 1e-3 * rng.standard_normal(n)


def pair_crossing(n):
    """The amplitudes just below and just above the crossing of the exact values of the two families within [2, n // 3]."""

    def gap(b):
        x = pair_planted(n, b)
        return max(exact_value(x, k * 67) for k in range(1, n // 3 // 67 + 1)) - max(exact_value(x, k * 61) for k in range(1, n // 3 // 61 + 1))

    return _bisect(gap, 0.5, 2.0, 60)


def pair_1e9(n, side):
    lo, hi = pair_crossing(n)
    return pair_planted(n, lo * (1 - 2e-10) if side == "below" else hi * (1 + 2e-10))


def window(kind, n):
    if kind.startswith("sin:"):
        return multi_sinusoid_window(int(kind[4:]), n)
    if kind.startswith("plant:"):
        rng = _rng(kind, n)
        x = 1e-3 * rng.standard_normal(n)
        for item in kind[6:].split(","):
            p, _, amp = item.partition("*")
            x += float(amp or 1.0) * _pattern(rng, int(p), n)
        return x
    if kind.startswith("int:"):
        d = int(kind[4:])
        return _rng(kind, n).integers(-9, 10, d)[np.arange(n) % d].astype(np.float64)
    if kind.startswith("near:"):
        d, m, ratio = kind[5:].split(":")
        return near_tie(n, int(d), int(m), float(ratio))
    if kind.startswith("pair1e9:"):
        return pair_1e9(n, kind[8:])
    if kind.startswith("noise:"):
        return np.random.default_rng(int(kind[6:])).standard_normal(n)
    if kind == "zeros":
        return np.zeros(n)
    if kind == "nan":
        x = multi_sinusoid_window(3, n)
        x[100] = np.nan
        return x
    if kind.startswith("2^"):
        return multi_sinusoid_window(4, n) * 2.0 ** int(kind[2:])
    raise AssertionError(kind)


def _case(name, n, num, windows, max_length=None, min_length=2, gamma=False):
    return dict(name=name, n=n, num=num, windows=tuple(windows), max_length=n // 3 if max_length is None else max_length,
                min_length=min_length, gamma=gamma)


CASES = (
    # N = 1024, max_length = 341: top periods 171 ... 341, R = 4 ... 6, both sides of kPairSmallP
    _case("n1024_341", 1024, 4, ("sin:1", "plant:300,190*0.7", "near:150:300:5e-10", "near:150:300:2e-9", "pair1e9:below", "pair1e9:above",
                                 "plant:260,250*0.8,130*0.5")),
    _case("n1024_341_degenerate", 1024, 3, ("zeros", "sin:2", "nan", "2^500", "2^-500")),
    _case("n1024_341_gamma", 1024, 3, ("plant:300,7*0.2", "sin:1", "plant:5,290*3"), gamma=True),
    # N = 1024, max_length = 700: R = 2; the integer window of period 256 ties 512 with 256 exactly
    _case("n1024_700", 1024, 3, ("int:256", "plant:600,380*0.7", "sin:5"), max_length=700),
    # white noise of 97 samples, periods 5 ... 20, twelve rows (tests/test_gpu_cover.py): present periods win again and again
    # until one is skipped; a skipped top period that still reaches the bound lists its divisors next to another top period
    _case("n97_skip", 97, 12, ("noise:54", "noise:88", "noise:54"), min_length=5, max_length=20),
    # the same with long periods: white noise of 500 samples, periods 150 ... 312 (two rows at the top), fourteen rows.  Period
    # 312 wins an eleventh time on the fold-once path and is skipped (action 0 there); two sweeps later it still reaches the
    # bound and lists its divisor 156 beside the top period 311 > kPairSmallP, which 156 does not divide: only the
    # kernel's divisibility test keeps that window-sweep off the fold-once path
    _case("n500_skip", 500, 14, ("noise:5", "zeros", "noise:5"), min_length=150, max_length=312),
    # N = 2246: shared passes of 3 ... 6 rows
    _case("n2246", 2246, 4, ("sin:7", "plant:700,410*0.6,130*0.4", "sin:8")),
    # N = 4096, default range: the only place a top period exceeds the block; seven windows
    _case("n4096", 4096, 3, ("sin:12", "plant:1200,900*0.7", "sin:9", "plant:1030,1300*0.8", "sin:16", "plant:690,1100*0.6", "sin:11")),
)
BY_NAME = {c["name"]: c for c in CASES}

_WIN, _TRACE = {}, {}


def windows(case):
    if case["name"] not in _WIN:
        x = np.stack([window(k, case["n"]) for k in case["windows"]])
        x.setflags(write=False)
        _WIN[case["name"]] = x
    return _WIN[case["name"]]


def traces(case):
    """One trace per window of the case (computed once and shared).  Raises Ambiguous for a case that is not admitted."""
    if case["name"] not in _TRACE:
        _TRACE[case["name"]] = [trace(x, case["num"], case["min_length"], case["max_length"], case["gamma"]) for x in windows(case)]
    return _TRACE[case["name"]]


def labels(case):
    """What the case reaches: the paths of its window-sweeps (with the source of a fold-once sweep) and the actions."""
    out = set()
    for tr in traces(case):
        for rec in tr:
            out.add(rec["path"])
            if rec["path"].startswith("fold"):
                out.add("fold: first sweep (source is the input)" if rec["first"] else "fold: later sweep (in place)")
                out.add("fold: no divisor listed" if len(rec["listed"]) == 1 else "fold: divisors thinned from the column sums")
            if rec["action"] is not None:
                out.add(f"action {rec['action']}")
            if rec["path"] == "fallback: tie":
                out.add("fallback: exact tie" if rec["lead"] == 0.0 else "fallback: near tie")
    return out
