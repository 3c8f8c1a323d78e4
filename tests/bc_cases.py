"""Case table of the best_correlation census (test_bc_census_cpu.py, test_gpu_bc_census.py): the windows, the expected
answers with the trace of every round, and a restatement in Python of what picks the code path of a round in
k_best_correlation and k_best_correlation_pair (pyperiod_amd/csrc/ph_bc.h, ph_pair.h, period_hip.hip).  `classify` turns a
case and its rounds into the set of CLASSES labels it reaches; the CPU census asserts that the table as a whole reaches
every label, so the GPU test can say which paths it ran.

A case is a dict: name, n, num, max_length (None: N // 3), ratio, dtype, trunc, orth, kinds (one word per window), exact
(every sum of every compared round is exact in fp64 in any order: the GPU test holds such a case bit for bit and the
margin rule never excuses it), fixture (tags of tests/golden/best_correlation_edges.npz, the reference's own answer, one
per window or None) and `claims`, the labels its entry in the table is there for.  Its windows are seeded by its name
alone.  Window kinds:
  noise, plant:a,b,..   as in s2l_cases
  impulse:k             a single 1.0 at index k: round 0 has the value 1.0 at every period, the lowest must win
  neartie:a:g1:g2       1 + 2^-50 at a, 1 at a + g1, 1 - 2^-50 at a + g2 (g1, g2 coprime): the periods that divide g1 see
                        2 + 2^-50, those that divide g2 see 2, those that divide g2 - g1 see 2 - 2^-50, no period sees all
                        three, and every sum is exact: the lowest divisor of g1 wins over the lowest divisor of g2 by
                        2^-51 relative
  tie2:s                a noise window (seed s) with one sample moved so that the runner-up of round 0 wins by a relative
                        lead inside [1e-8, 1e-7]: see planted_near_tie
  collapse:p0           s2l_cases.collapse_parts: 2^36 x an integer pattern of period p0 + small integers
  zeros, const          all 0.0, all 0.75
  nan, pinf, ninf       the planted window of the case with x[17] = NaN / +Inf / -Inf
  nan_inf               x[17] = NaN and x[40] = +Inf;  allnan: every sample NaN
  2^k                   the planted window of the case times 2^k
"""

import math
import zlib
from fractions import Fraction

import numpy as np

from oracle import period_oracle as po
from s2l_cases import COLLAPSE_BIG, K_MAX_WAVES, K_PAD, LDS_LIMIT, TOL, TOL32, _plant, carve, collapse_parts, pick_scale, stale, usable  # noqa: F401
from short_windows_cases import CAP32, CAP64, MARGIN32, MARGIN64  # noqa: F401  (the project's margin rule)

SEED = 20263
# ph_bc.h:12 kCandCap; ph_pair.h:939 kPairListCap; ph_device.h:1182 kRedDoubles = 2 kMaxWaves; ph_bc.h:218-226 BP_WORDS,
# BP_DOUBLES; period_hip.hip:162-195 build_plan, :713-728 plan_best_correlation, :1759 the plan of [2, max_length - 1]
K_CAND_CAP, K_PAIR_LIST_CAP, BP_WORDS, BP_DOUBLES, K_PAIR_BLOCK = 256, 96, 8, 10, 1024
FLOAT_MAX = 1.7976931348623157e308  # ph_bc.h:102: the screen of the one-window kernel runs when sum|x| <= this

ENGINES = {  # name -> environment of ph_create
    "pair": {},
    "one": {"PH_BC_PAIR": 0},
    "one256": {"PH_BC_PAIR": 0, "PH_SWEEP_BLOCK": 256},
    "hbm": {"PH_BC_PAIR": 0, "PH_HBM_WINDOW": 1},
}


def pair_lds_bytes(N):
    """ph_bc.h:240-252 (bc_pair_carve)."""
    return (carve(N + K_PAD, 8) + carve(N + K_PAD, 8) + carve(2 * K_MAX_WAVES, 8) + carve(K_MAX_WAVES, 8) + carve(K_MAX_WAVES, 4) +
            carve(2 * K_PAIR_LIST_CAP, 4) + carve(BP_WORDS, 4) + carve(BP_DOUBLES, 8))


def plan_variant(dtype, general, N, max_length, env=()):
    """period_hip.hip:713-728: -> 'pair' / 'one'.  (Every window of this table fits the LDS; PH_HBM_WINDOW moves it.)"""
    env = dict(env)
    pair = (int(env.get("PH_BC_PAIR", 1)) != 0 and np.dtype(dtype) == np.float64 and not general and
            not int(env.get("PH_HBM_WINDOW", 0)) and 3 <= max_length <= N and pair_lds_bytes(N) <= LDS_LIMIT)
    return "pair" if pair else "one"


def build_plan(p_lo, p_hi, chains, max_m=4):
    """period_hip.hip:162-195 without the duo pairing and the interleaving: -> {period: pass type of the pass that produces
    it}, 'm = 0' (row-split pass of one period below 64), 'm = 1', 'm = 2', 'm = 4' (base p also yields 2p, 4p), 'chain'."""
    out, covered = {}, set()
    if chains:
        for L in range(min(p_hi, 64), p_lo - 1, -1):
            q = L
            while q >= p_lo and q >= 1 and q not in covered:
                covered.add(q)
                out[q] = "chain"
                if q & 1:
                    break
                q >>= 1
    for p in range(p_lo, p_hi + 1):
        if p < 64 and not chains:
            out[p] = "m = 0"
            continue
        if p in covered:
            continue
        m = min(4 if 4 * p <= p_hi else 2 if 2 * p <= p_hi else 1, max_m)
        d = 1
        while d <= m:
            covered.add(d * p)
            out[d * p] = f"m = {m}"
            d *= 2
    return out


# ------------------------------------------------------------------------------------------------------------------
# Windows
# ------------------------------------------------------------------------------------------------------------------
def _rng(name, w):
    return np.random.default_rng([SEED, zlib.crc32(name.encode()), w])


EPS = 2.0 ** -50
PLANTED = "3,7,40"
TIE2_N, TIE2_ML = 1024, 341
_TIE2 = {}


def planted_near_tie(seed):
    """-> (window, old winner, new winner, lead) or None.  Noise of seed `seed`; p1, p2 its top two periods by
    po.sweep_maxabs, neither a multiple of the other; one sample of p2's largest class that is outside p1's largest class
    moves so that p2 leads p1 by 3e-8 relative.  The lead is then measured again over ALL periods (the moved sample changes
    one class of every period): None unless p2 wins with a lead inside [1e-8, 1e-7]."""
    if seed not in _TIE2:
        x = np.random.default_rng([SEED, 7, seed]).standard_normal(TIE2_N)
        vals = po.sweep_maxabs(x, 2, TIE2_ML - 1)
        order = np.argsort(-vals, kind="stable")
        p1, p2 = int(order[0]) + 2, int(order[1]) + 2
        got = None
        if p1 % p2 and p2 % p1:
            s1 = int(np.argmax(np.abs(po.fold_sums(x, p1))))
            f2 = po.fold_sums(x, p2)
            s2 = int(np.argmax(np.abs(f2)))
            idx = [i for i in range(s2, TIE2_N, p2) if i % p1 != s1]
            if idx:
                y = x.copy()
                y[idx[0]] += math.copysign(vals[p1 - 2] * (1 + 3e-8) - vals[p2 - 2], f2[s2])
                new = po.sweep_maxabs(y, 2, TIE2_ML - 1)
                top = int(np.argmax(new)) + 2
                lead = float((new[top - 2] - np.max(np.delete(new, top - 2))) / new[top - 2])
                if top == p2 and 1e-8 <= lead <= 1e-7:
                    y.setflags(write=False)
                    got = (y, p1, p2, lead)
        _TIE2[seed] = got
    return _TIE2[seed]


def tie2_seeds(count=8):
    """The first `count` seeds planted_near_tie accepts, at least three with the new winner above the old one and three
    below."""
    up, down, s = [], [], 0
    while len(up) + len(down) < count or len(up) < 3 or len(down) < 3:
        r = planted_near_tie(s)
        if r is not None:
            side = up if r[2] > r[1] else down
            if len(side) < count - 3:
                side.append(s)
        s += 1
        assert s < 400
    return sorted(up + down)[:count]


def _window(case, w, kind):
    n, name = case["n"], case["seed"]
    rng = _rng(name, w)
    if kind == "noise":
        return rng.standard_normal(n)
    if kind.startswith("plant:"):
        return _plant(rng, n, kind[6:])
    if kind.startswith("impulse:"):
        x = np.zeros(n)
        x[int(kind[8:])] = 1.0
        return x
    if kind.startswith("neartie:"):
        a, g1, g2 = (int(v) for v in kind[8:].split(":"))
        x = np.zeros(n)
        x[a], x[a + g1], x[a + g2] = 1.0 + EPS, 1.0, 1.0 - EPS
        return x
    if kind.startswith("tie2:"):
        assert n == TIE2_N and max_length_of(case) == TIE2_ML
        return planted_near_tie(int(kind[5:]))[0].copy()
    if kind.startswith("collapse:"):
        big, small = collapse_parts(name, w, n, int(kind[9:]))
        return COLLAPSE_BIG * big.astype(np.float64) + small.astype(np.float64)
    if kind == "zeros":
        return np.zeros(n)
    if kind == "const":
        return np.full(n, 0.75)
    if kind == "allnan":
        return np.full(n, np.nan)
    base = _plant(_rng("degenerate", 0), n, PLANTED)  # one planted window for every degenerate case of a length
    if kind in ("nan", "pinf", "ninf", "nan_inf"):
        base[17] = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf, "nan_inf": np.nan}[kind]
        if kind == "nan_inf":
            base[40] = np.inf
        return base
    if kind.startswith("2^"):
        return base * 2.0 ** int(kind[2:])
    raise AssertionError(kind)


_WIN = {}


def windows(case):
    """(W, N) windows of the case in its dtype (float32: the float64 windows rounded)."""
    key = (case["seed"], case["n"], case["kinds"], np.dtype(case["dtype"]).name)
    if key not in _WIN:
        x = np.stack([_window(case, w, k) for w, k in enumerate(case["kinds"])]).astype(case["dtype"])
        x.setflags(write=False)
        _WIN[key] = x
    return _WIN[key]


# ------------------------------------------------------------------------------------------------------------------
# The table
# ------------------------------------------------------------------------------------------------------------------
def _case(name, n, kinds, num=3, max_length=None, ratio=0.01, dtype=np.float64, trunc=False, orth=False, exact=None, fixture=None,
          claims=(), seed=None, knife=False):
    kinds = tuple(kinds)
    return dict(name=name, seed=seed or name, n=n, kinds=kinds, num=num, max_length=max_length, ratio=ratio, dtype=dtype, trunc=trunc, orth=orth,
                exact=tuple(exact) if exact else (False,) * len(kinds), fixture=tuple(fixture) if fixture else (None,) * len(kinds),
                claims=tuple(claims), knife=knife)


HEALTHY = "plant:" + PLANTED
N_DEG, N_ML = 256, 130
ZEROS_REF = ("nan", "pinf", "ninf")  # one non-finite sample: the reference returns zeros
RAISES_REF = ("nan_inf", "allnan", "zeros", "const")
SCALED = ("2^510", "2^400", "2^-400", "2^-530")
DEGENERATE = ZEROS_REF + RAISES_REF + SCALED
IMPULSES = (("impulse_pair_98", 512, 98, 200), ("impulse_pair_99", 512, 99, 200), ("impulse_one_66", 1024, 66, 333),
            ("impulse_one_258", 1024, 258, 333), ("impulse_one_259", 1024, 259, 333))
# near ties: (name, a, g1, g2): the lowest divisor >= 2 of g1 wins over the lowest divisor of g2.  179, 101, 67 and 61 are
# prime; at max_length 341 period 179 has a pass of its own (m = 1), 101 yields 202 (m = 2), 67 yields 134 and 268 (m = 4),
# 61 is a chain member in the pair kernel and an m = 0 pass in the one-window kernel.
NEARTIES = (("neartie_179", 300, 179, 88), ("neartie_mirror", 300, 88, 179), ("neartie_m2", 300, 101, 88), ("neartie_m4", 300, 67, 88),
            ("neartie_short", 300, 61, 88))
KNIFE_SOURCES = (("plant:3,7,40", 600), ("plant:5,31,100", 600), ("plant:11,64", 512))
ML_EDGES = (2, 3, N_ML, N_ML + 5)


def _table():
    t = []
    t.append(_case("noise", 1024, ("noise", "noise", "noise"), claims=["listed, few survivors", "lone window", "round 0 from x",
                                                                       "later round from workspace"]))
    t.append(_case("planted", 1000, ("plant:3,7,40,100", "plant:5,31,64,200"), num=5, claims=["listed, few survivors", "plan: pair", "plan: one"]))
    for name, n, ml, k in IMPULSES:
        label = {98: "pair: listed == 96", 99: "pair: listed > 96", 66: "one: ncand <= 64", 258: "one: ncand 65..256", 259: "one: ncand > 256"}[ml]
        # round 0 removes 1 - sqrt(1 - 2 / N) of the norm: 0.00196 at N = 512, 0.00098 at N = 1024; the ratio is below it
        t.append(_case(name, n, (f"impulse:{k}", HEALTHY), num=2, max_length=ml, ratio=0.001 if n == 512 else 0.0005, exact=(True, False), fixture=(name, None),
                       claims=[label, "exact tie, lowest wins"] + (["pair on different paths"] if ml == 99 else [])))
    for name, a, g1, g2 in NEARTIES:
        t.append(_case(name, 1024, (f"neartie:{a}:{g1}:{g2}",), num=1, ratio=1e-4, exact=(True,), fixture=(name,), claims=["near tie of 2^-51"]))
    seeds = tie2_seeds()
    for i in range(0, len(seeds), 2):
        t.append(_case(f"tie2_{seeds[i]}_{seeds[i + 1]}", TIE2_N, (f"tie2:{seeds[i]}", f"tie2:{seeds[i + 1]}"), num=1, max_length=TIE2_ML, ratio=0.0,
                       claims=["planted near tie"]))
    for p0 in (2, 8, 64):
        t.append(_case(f"collapse_{p0}", 1024, (f"collapse:{p0}", "noise"), num=3, max_length=400, ratio=1e-13, claims=["stale, rescaled", "later round from workspace"]))
    for k in DEGENERATE:
        tag = "deg_" + k
        t.append(_case(f"{tag}_second", N_DEG, (HEALTHY, k), fixture=(None, tag)))
        t.append(_case(f"{tag}_first", N_DEG, (k, HEALTHY), fixture=(tag, None)))
    t.append(_case("deg_lone_nan", N_DEG, (HEALTHY, "noise", "nan"), fixture=(None, None, "deg_nan"), claims=["lone window", "non-finite, reference returns zeros"]))
    t.append(_case("deg_lone_const", N_DEG, ("pinf", "2^510", "const"), fixture=("deg_pinf", "deg_2^510", "deg_const"),
                   claims=["lone window", "status 1 in round k > 0", "image unusable in round 0", "image unusable in a later round"]))
    t.append(_case("deg_lone_zeros", N_DEG, ("zeros", "allnan", "zeros"), fixture=("deg_zeros", "deg_allnan", "deg_zeros"),
                   claims=["status 1 in round 0", "reference raises"]))
    for ml in ML_EDGES:
        kinds = ("plant:2,3,16", "plant:3,5,17", "plant:2,15,18")
        t.append(_case(f"max_length_{ml}", N_ML, kinds, max_length=ml, fixture=[f"ml{ml}_w{w}" for w in range(3)],
                       claims=[f"max_length == {'N' if ml == N_ML else 'N + 5' if ml > N_ML else ml}"]))
    # ratio 1e-9 below (kept) and above (rejected) the gain of round 0 of window 0; both sides run on the same windows.
    # 1e-9 is the margin bar itself; these cases are compared whatever it says (`knife`): the gain is two norms of sums
    # of squares, its rounding error 1e-14 of it
    for i, (kind, n) in enumerate(KNIFE_SOURCES):
        gain = rounds(_window(dict(n=n, seed=f"knife_{i}"), 0, kind), 1, n // 3, 0.0)[0][0]["gain"]
        for side, ratio in (("kept", gain * (1 - 1e-9)), ("rejected", gain * (1 + 1e-9))):
            t.append(_case(f"knife_{i}_{side}", n, (kind, "noise"), num=4, ratio=ratio, seed=f"knife_{i}", knife=True,
                           claims=["rejected pick"] if side == "rejected" else []))
    # the one-window kernel under trunc, orth and float32, each with an exact-tie window (one round: the means of a later
    # round are no dyadic numbers under trunc / orth)
    for name, kw in (("trunc", dict(trunc=True)), ("orth", dict(orth=True)), ("trunc_orth", dict(trunc=True, orth=True)), ("f32", dict(dtype=np.float32))):
        t.append(_case(f"{name}_planted", 600, ("plant:3,7,40,100", "plant:5,31,64"), num=4, max_length=150, claims=[name.split("_")[0] if name != "f32" else "float32"], **kw))
        t.append(_case(f"{name}_impulse", 1024, ("impulse:333", "impulse:70"), num=1, max_length=258, ratio=0.0005, exact=(True, True),
                       claims=["exact tie, lowest wins", "one: ncand 65..256"], **kw))
    # one NaN sample under float32 and trunc: the one-window kernel in its other instantiations
    t.append(_case("f32_nan", N_DEG, (HEALTHY, "nan"), dtype=np.float32, claims=["float32", "non-finite, reference returns zeros"]))
    t.append(_case("trunc_nan", N_DEG, ("nan", HEALTHY), trunc=True, claims=["trunc", "non-finite, reference returns zeros"]))
    return t


def max_length_of(case):
    return case["n"] // 3 if case["max_length"] is None else case["max_length"]


def general(case):
    return bool(case["trunc"] or case["orth"])


# ------------------------------------------------------------------------------------------------------------------
# The rounds of a window: the oracle's loop (oracle/period_oracle.py:best_correlation) with everything a label needs
# ------------------------------------------------------------------------------------------------------------------
def rounds(x, num, max_length, ratio, trunc=False, orth=False):
    """-> (rounds, raised).  One dict per round that found a period: p, best, lead (relative lead of the winner over the
    best other period; 0.0 for an exact tie), ties (periods with exactly the winner's value), gain, kept, rsq / rnorm /
    rmax / asum (sum of squares, periodic norm, largest magnitude and sum of magnitudes of the residual the round ran on),
    base.  `raised`: the
    round that found no period (the reference raises TypeError there), or None."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    with np.errstate(all="ignore"):
        og = po.periodic_norm(x)
        old = og
        work = x.copy()
        for i in range(num):
            vals = np.full(max(max_length - 2, 0), -1.0)
            for p in range(2, max_length):
                col = np.abs(po.fold_sums(work, p))
                col = col[col == col]
                vals[p - 2] = np.max(col) if col.size else -1.0
            if not vals.size or not np.max(vals) > 0:
                return out, i
            k = int(np.argmax(vals))  # the first, i.e. lowest, period among equals: the strict '>' of Periods.py:329
            rest = vals[vals < vals[k]]  # (the lead over the periods with exactly the same value is 0: `ties`)
            second = float(np.max(rest)) if rest.size else 0.0
            base = po.project(work, k + 2, trunc, orth)
            r = dict(p=k + 2, best=float(vals[k]), lead=float((vals[k] - max(second, 0.0)) / vals[k]) if np.isfinite(vals[k]) else 1.0,
                     ties=[int(q) + 2 for q in np.where(vals == vals[k])[0]], rsq=float(np.sum(work * work)), rnorm=float(po.periodic_norm(work)),
                     rmax=float(np.max(np.abs(work))), asum=float(np.sum(np.abs(work))), base=base, vals=vals)
            work = work - base
            this = po.periodic_norm(work)
            r["gain"] = float((old - this) / og)
            r["kept"] = bool(r["gain"] > ratio)
            r["after_rsq"] = float(np.sum(work * work))
            if r["kept"]:
                old = this
            out.append(r)
    return out, None


CASES = tuple(_table())
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

CLASSES = tuple(
    ["plan: pair", "plan: one"]
    + [f"winner from {m}" for m in ("m = 0", "m = 1", "m = 2", "m = 4", "chain")]
    + ["one: ncand <= 64", "one: ncand 65..256", "one: ncand > 256", "one: no screen, sum|x| not finite", "pair: listed == 96", "pair: listed > 96",
       "listed, few survivors"]
    + ["image unusable in round 0", "image unusable in a later round", "stale, rescaled", "round 0 from x", "later round from workspace"]
    + ["exact tie, lowest wins", "near tie of 2^-51", "planted near tie", "rejected pick", "status 1 in round 0", "status 1 in round k > 0",
       "lone window", "pair on different paths", "pair: one window at status 1, partner runs on", "non-finite, reference returns zeros",
       "reference raises"]
    + ["max_length == 2", "max_length == 3", "max_length == N", "max_length == N + 5", "trunc", "orth", "float32"]
)


# ------------------------------------------------------------------------------------------------------------------
# Expected answers
# ------------------------------------------------------------------------------------------------------------------
_REF = {}


def ref(case):
    """Per window of the case: dict(rounds, raised, periods, norms, bases, margin) from `rounds` on the float64 samples.
    margin: the smallest of every round's lead and |gain - ratio| (relative to the ratio where it is not 0)."""
    if case["name"] not in _REF:
        res = []
        for row in windows(case).astype(np.float64):
            rs, raised = rounds(row, case["num"], max_length_of(case), case["ratio"], case["trunc"], case["orth"])
            per, nr, bs = np.zeros(case["num"], np.uint32), np.zeros(case["num"]), np.zeros((case["num"], case["n"]))
            for i, r in enumerate(rs):
                if r["kept"]:
                    per[i], nr[i], bs[i] = r["p"], r["gain"], r["base"]
            finite = [r for r in rs if r["gain"] == r["gain"]]
            gaps = [abs(r["gain"] - case["ratio"]) / (abs(case["ratio"]) or 1.0) for r in finite]
            leads = [r["lead"] if len(r["ties"]) == 1 or not np.isfinite(r["best"]) else 0.0 for r in rs]
            res.append(dict(rounds=rs, raised=raised, periods=per, norms=nr, bases=bs, margin=float(min(leads + gaps + [1.0]))))
        _REF[case["name"]] = res
    return _REF[case["name"]]


def bar(case):
    return MARGIN64 if case["dtype"] == np.float64 else MARGIN32


def admitted(case, w):
    """Whether window w takes part in the same-period-list comparison: always when its sums are exact."""
    r = ref(case)[w]
    return case["exact"][w] or case["knife"] or r["margin"] >= bar(case) or not r["rounds"]


# ------------------------------------------------------------------------------------------------------------------
# classify
# ------------------------------------------------------------------------------------------------------------------
def one_ncand_exact(r, P):
    """ph_bc.h:103-124 on a round whose periods ALL have the same exact value: every upper bound reaches every lower
    bound, so all P periods are listed."""
    return P if len(r["ties"]) == P else None


def _window_labels(case, kind, r, exact):
    ml = max_length_of(case)
    P = max(ml - 2, 0)
    out = set()
    plans = {plan_variant(case["dtype"], general(case), case["n"], ml, env) for env in ENGINES.values()}
    out |= {"plan: " + p for p in plans}
    state_sc, unusable_later = None, False
    for i, rd in enumerate(r["rounds"]):
        for variant in plans:
            out.add("winner from " + build_plan(2, ml - 1, variant == "pair")[rd["p"]])
        out.add("round 0 from x" if i == 0 else "later round from workspace")
        if len(rd["ties"]) > 1 and rd["p"] == min(rd["ties"]) and exact:
            out.add("exact tie, lowest wins")
        n_all = one_ncand_exact(rd, P) if exact and i == 0 else None
        if n_all is not None:
            if "one" in plans:
                out.add("one: ncand <= 64" if n_all <= 64 else "one: ncand 65..256" if n_all <= K_CAND_CAP else "one: ncand > 256")
            if "pair" in plans and n_all in (K_PAIR_LIST_CAP, K_PAIR_LIST_CAP + 1):
                out.add("pair: listed == 96" if n_all == K_PAIR_LIST_CAP else "pair: listed > 96")
        if "one" in plans and not rd["asum"] <= FLOAT_MAX:
            out.add("one: no screen, sum|x| not finite")
        if not usable(rd["rsq"]):
            out.add("image unusable in round 0" if i == 0 else "image unusable in a later round")
        elif kind in ("noise",) or kind.startswith("plant:"):
            out.add("listed, few survivors")
        if i == 0:
            state_sc = pick_scale(rd["rsq"], case["n"])
        if stale(rd["after_rsq"], state_sc, case["n"]) and i + 1 < len(r["rounds"]):
            out.add("stale, rescaled")
            state_sc = pick_scale(rd["after_rsq"], case["n"])
        if not rd["kept"] and rd["gain"] == rd["gain"] and any(q["kept"] for q in r["rounds"][i + 1:]):
            out.add("rejected pick")
    if r["raised"] is not None:
        out.add("status 1 in round 0" if r["raised"] == 0 else "status 1 in round k > 0")
        out.add("reference raises")
    elif kind in ZEROS_REF:
        out.add("non-finite, reference returns zeros")
    if kind.startswith("neartie:"):
        out.add("near tie of 2^-51")
    if kind.startswith("tie2:"):
        out.add("planted near tie")
    return out


def exact_all_round0(case, w):
    """Whether round 0 of window w evaluates every period exactly in the pair kernel: the image is unusable, or (exact
    windows) more than kPairListCap periods are listed."""
    r = ref(case)[w]
    if not r["rounds"]:
        return None
    rd = r["rounds"][0]
    P = max_length_of(case) - 2
    return not usable(rd["rsq"]) or (case["exact"][w] and one_ncand_exact(rd, P) is not None and P > K_PAIR_LIST_CAP)


def classify(case):
    """The labels of CLASSES the case reaches, from its shape and the rounds of its windows."""
    ml = max_length_of(case)
    rs = ref(case)
    out = set()
    for w, (kind, r) in enumerate(zip(case["kinds"], rs)):
        out |= _window_labels(case, kind, r, case["exact"][w])
    if plan_variant(case["dtype"], general(case), case["n"], ml) == "pair":
        if len(rs) % 2:
            out.add("lone window")
        for a in range(0, len(rs) - 1, 2):
            e0, e1 = exact_all_round0(case, a), exact_all_round0(case, a + 1)
            if e0 is not None and e1 is not None and e0 != e1:
                out.add("pair on different paths")
            done = [r["raised"] if r["raised"] is not None else case["num"] for r in rs[a:a + 2]]
            if min(done) < case["num"] and max(done) > min(done):
                out.add("pair: one window at status 1, partner runs on")
    for v in ML_EDGES:
        if ml == v and case["n"] == N_ML:
            out.add(f"max_length == {'N' if v == N_ML else 'N + 5' if v > N_ML else v}")
    if case["trunc"]:
        out.add("trunc")
    if case["orth"]:
        out.add("orth")
    if case["dtype"] == np.float32:
        out.add("float32")
    return out


# ------------------------------------------------------------------------------------------------------------------
# Exactness proofs (Fraction arithmetic)
# ------------------------------------------------------------------------------------------------------------------
def sums_exact(work, max_length):
    """Whether every residue-class sum of every period in [2, max_length) is exact in fp64 in ANY order of summation:
    all samples are multiples of one power of two u, and the sum of their magnitudes is below 2^53 u."""
    fr = [Fraction(float(v)) for v in work if v != 0]
    if not fr:
        return True
    u = Fraction(1, max(f.denominator for f in fr))
    return all((f / u).denominator == 1 for f in fr) and sum(abs(f) for f in fr) / u < 2 ** 53


def exact_rounds(case, w):
    """For an exact window: per compared round, whether its residual passes sums_exact (so the winner and its ties are the
    same in any order of summation) and, under the plain projection, whether the oracle's base is the correctly rounded
    quotient of the exact class sum and the class count (Fraction arithmetic): a kernel that adds a class in any order and
    divides once gets the same bits."""
    res = []
    work = windows(case)[w].astype(np.float64)
    for rd in ref(case)[w]["rounds"]:
        ok = sums_exact(work, max_length_of(case))
        if not general(case):
            p = rd["p"]
            means = [float(sum((Fraction(float(v)) for v in work[j::p]), Fraction(0)) / len(work[j::p])) for j in range(min(p, len(work)))]
            ok = ok and all(float(v) == means[i % p] for i, v in enumerate(rd["base"]))
        res.append(ok)
        work = work - rd["base"]
    return res


# ------------------------------------------------------------------------------------------------------------------
# The fixture: what the reference itself returns (tests/golden/best_correlation_edges.npz, make_golden_bc.py)
# ------------------------------------------------------------------------------------------------------------------
def fixture_cases():
    """-> [(tag, window, dict(num, max_length, ratio))]: every (window, parameters) of the table that names a fixture tag."""
    out = {}
    for case in CASES:
        for w, tag in enumerate(case["fixture"]):
            if tag is not None:
                kw = dict(num=case["num"], max_length=max_length_of(case), ratio=case["ratio"])
                x = windows(case)[w].astype(np.float64)
                if tag in out:
                    assert out[tag][1] == kw and np.array_equal(out[tag][0], x, equal_nan=True), tag
                out[tag] = (x, kw)
    return [(tag, x, kw) for tag, (x, kw) in sorted(out.items())]


def tile_rows(singles, n):
    return np.stack([np.tile(s, n // len(s) + 1)[:n] for s in singles])


def load_fixture(path):
    """-> {tag: ('ok', periods, norms, bases) or ('raises', exception name)}."""
    z = np.load(path)
    out = {}
    for tag in (str(t) for t in z["tags"]):
        if f"{tag}_raises" in z.files:
            out[tag] = ("raises", str(z[f"{tag}_raises"]))
        else:
            per = z[f"{tag}_periods"]
            n = len(z[f"{tag}_x"])
            out[tag] = ("ok", per, z[f"{tag}_norms"], tile_rows([z[f"{tag}_base{i}"] for i in range(len(per))], n))
        out[tag] += (z[f"{tag}_x"],)
    return out
