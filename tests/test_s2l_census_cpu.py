"""The small_to_large census on the CPU: what tests/s2l_cases.py reaches, and what its expected values rest on.

k_small_to_large_pair and k_small_to_large (ph_s2l.h) pick the code of an event by integers and by the state of the
window: the split of split_row_means, where the means live, the trips of the flat loops, the copy path of the staging
buffer, which window owns that buffer, the sign of A in set_thresholds, the rescale predicate.  s2l_cases restates them;
`test_table_reaches_every_class` asserts that the table reaches every label of s2l_cases.CLASSES and that every case
reaches what its entry claims, and prints how many cases reach each label (-s).

The expected values of the GPU test are the fp64 oracle's.  `test_reference_headroom` evaluates the oracle's accepted
periods again in longdouble and holds the oracle's powers and bases to TOL / 100 = 1e-12 of it in the units of the GPU
bars (||r_k|| / ||x|| and max|r_k| of the residual before accept k), so that two orders lie between the reference's own
rounding and what the kernels are asked for.

Measured (this table, x86-64 longdouble): 52 cases (114 windows and the 2051 of the persistent case), 75 labels, 6 knife
edges; the oracle on all of them 5 s, this module 9 s; largest |oracle - longdouble| 1.8e-16 (powers) and 1.3e-15
(bases) of the units above, i.e. 1.3e-3 of TOL / 100; no case is left out by the margin rule (smallest margin 1.2e-5 for
float64 -- the absolute one of a thresh-0 case --, 2.1e-3 for float32).  Labels with one carrier: G = 1 by 2p > width
at 512 threads (N = 7968, p = 257: below that length 257 periods have fewer than 32 rows), the two-trip lengths 4097 and
4100, each n_periods edge, the batch larger than the chip, and `flag only through kappa_q`: a window whose float screen
value, restated here in float32, is 3.5e-6 short of the fp64 value while the thresholds give away 1.2e-6 on their own.
"""

import collections

import numpy as np

import s2l_cases as sc
from oracle import period_oracle as po


def test_table_reaches_every_class():
    count, carriers = collections.Counter(), collections.defaultdict(list)
    for case in sc.CASES:
        labels = sc.classify(case)
        missing = [c for c in case["claims"] if c not in labels]
        assert not missing, (case["name"], "does not reach what its entry claims", missing)
        for label in labels:
            count[label] += 1
            carriers[label].append(case["name"])
    for label in sc.CLASSES:
        print(f"{count[label]:3d}  {label}")
    print("also reached:", ", ".join(f"{label} ({count[label]})" for label in sorted(set(count) - set(sc.CLASSES))))
    missing = [label for label in sc.CLASSES if not count[label]]
    assert not missing, missing
    assert len(set(sc.CLASSES)) == len(sc.CLASSES)
    # no case that is the only carrier of a label is left out of the period comparison
    for label in sc.CLASSES:
        if len(carriers[label]) == 1:
            assert sc.admitted(sc.BY_NAME[carriers[label][0]]), (label, carriers[label])
    assert max(c["n"] for c in sc.CASES) <= 7968 and sum(1 for c in sc.CASES if c["n"] > 4100) == 2  # long_257, kappa_33


def test_margin_rule_caps():
    for dtype, cap in ((np.float64, sc.CAP64), (np.float32, sc.CAP32)):
        cases = [c for c in sc.CASES if c["dtype"] == dtype]
        out = [c["name"] for c in cases if not sc.admitted(c)]
        low = min(min(r["margin"] for r in sc.ref(c)) for c in cases)
        print(f"{np.dtype(dtype).name}: {len(out)} of {len(cases)} cases left out {out}, smallest margin {low:.2e}")
        assert len(cases) >= 3 and len(out) <= cap * len(cases), (np.dtype(dtype).name, out)
    # thresh == 0 has no relative margin: the smallest |imposed| is held to the same number
    zero = [c for c in sc.CASES if c["thresh"] == 0]
    assert len(zero) >= 4
    for c in zero:
        for r in sc.ref(c):
            assert r["margin"] == min(abs(e[1]) for e in r["events"]) >= sc.MARGIN64, c["name"]


def test_reference_headroom():
    worst = (0.0, 0.0, None)
    for case in sc.CASES:
        for w in range(len(sc.ref(case))):
            dp, db = sc.headroom(case, w)
            assert dp <= sc.TOL / 100 and db <= sc.TOL / 100, (case["name"], w, dp, db)
            if max(dp, db) > max(worst[:2]):
                worst = (dp, db, (case["name"], w))
    print(f"largest |oracle - longdouble|: powers {worst[0]:.2e}, bases {worst[1]:.2e} of the GPU units, at {worst[2]}")


def test_what_the_oracle_says_about_the_degenerate_windows():
    """Pinned here, expected of the kernels with status 0: no period for zeros, NaN, Inf and 2^510; [2] and then a
    residual of exactly zero for the constant window; the unscaled list at 2^+-400."""
    for kind in sc.DEGENERATE:
        for place, w in (("second", 1), ("first", 0)):
            case = sc.BY_NAME[f"degenerate_{kind}_{place}"]
            r = sc.ref(case)[w]
            if kind in ("zeros", "nan", "inf", "2^510"):
                assert r["periods"] == [] and all(e[1] != e[1] for e in r["events"]), (kind, place)
            elif kind == "const":
                assert r["periods"] == [2] and r["powers"][0] == 1.0 and all(e[3] == 0.0 for e in r["events"][1:]), (kind, place)
            else:
                x = sc.windows(case)[w]
                plain = sc.oracle_window(x * 2.0 ** -int(kind[2:]), case)
                assert r["periods"] == plain["periods"] and len(r["periods"]) >= 3, (kind, place)
                assert np.array_equal(r["powers"], plain["powers"])
            other = sc.ref(case)[1 - w]
            assert len(other["periods"]) >= 3  # the healthy neighbour has something to lose


def test_collapse_cases_are_exact():
    """The first accepted period of a collapse window is its p0, the oracle's base of it is the rational column means
    and its residual the rational residual, bit for bit (Fraction arithmetic): a kernel that sums the columns in any
    other order gets the same bits, and everything after the collapse starts from the same residual."""
    cases = [c for c in sc.CASES if c["name"].startswith("collapse_")]
    assert len(cases) == 5
    for case in cases:
        for w, kind in enumerate(case["kinds"]):
            if not kind.startswith("collapse:"):
                assert r_all(case, w)  # the noise neighbour accepts every period
                continue
            first, base_ok, resid_ok = sc.collapse_exact(case, w)
            assert first == int(kind[9:]) and base_ok and resid_ok, (case["name"], w, first, base_ok, resid_ok)
            r = sc.ref(case)[w]
            after = [e for e in r["events"] if e[0] > first]
            assert after[0][3] < 2.0 ** -30 * r["events"][0][3]  # the residual really collapses
            if case["thresh"] == 0.05:
                assert r["periods"] == [first]
            elif case["thresh"] > 0:
                assert {24, 100} < set(r["periods"]) and r["margin"] >= 1e-3 and len(r["periods"]) < 10, (case["name"], r["periods"])
            else:
                assert r["periods"] == list(range(2, 121))


def r_all(case, w):
    return sc.ref(case)[w]["periods"] == list(range(2, sc.n_periods_of(case) + 1))


def test_knife_edges():
    knives = sc.knife_cases()
    assert len(knives) == 6
    seen = set()
    for name, case, w, p, thresh, accepts in knives:
        r = sc.oracle_window(sc.windows(case)[w], case, thresh)
        print(name, thresh, r["periods"], f"margin {r['margin']:.1e}")
        assert (p in r["periods"]) == accepts and r["margin"] < 1e-11, (name, r["margin"])
        seen.add(sc.knife_class(case["n"], p))
    assert seen == set(sc.KNIFE_CLASSES)


def test_trace_changes_nothing():
    case = sc.BY_NAME["planted_lone"]
    for x in sc.windows(case):
        tr = {}
        a = po.small_to_large(x, 0.05)
        b = po.small_to_large(x, 0.05, trace=tr)
        assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))
        ev = tr["events"]
        assert [e[0] for e in ev] == list(range(2, len(x) // 2 + 1))
        assert [e[0] for e in ev if e[2]] == a[0] and [e[1] for e in ev if e[2]] == a[1]
        res = x.copy()
        for e in ev:  # norm and maximum of the residual the decision was taken on
            assert e[3] == po.periodic_norm(res) and e[4] == np.max(np.abs(res))
            if e[2]:
                res = res - a[2][a[0].index(e[0])]
        assert tr["min_margin"] == min(abs(e[1] - 0.05) / 0.05 for e in ev)


# ------------------------------------------------------------------------------------------------ restatements
def test_split_G_against_a_search():
    """The doubling loop stops at the first G that fails; the conditions are monotone in G, so the answer is the largest
    power of two up to 64 with G p <= width and rows >= 16 G, or 1 below 32 rows."""
    reached = set()
    for width in sc.WIDTHS:
        for n in (48, 300, 511, 512, 1023, 1024, 1100, 2047, 2048, 2049, 4093, 4096, 4100, 7968):
            for p in range(2, min(n, 600)):
                rows = -(-n // p)
                best = max([g for g in (2, 4, 8, 16, 32, 64) if g * p <= width and rows >= 16 * g], default=1)
                assert sc.split_G(n, p, width) == best, (width, n, p)
                reached.add((width, best))
    assert reached == {(w, g) for w in sc.WIDTHS for g in (1, 2, 4, 8, 16, 32, 64)}
    assert sc.split_G(4096, 4, 512) == 64 and sc.split_G(4092, 4, 512) == 32  # 1024 rows are needed
    assert sc.split_label(7968, 257, 512).endswith("2p > width") and sc.split_label(7967, 257, 512).endswith("rows < 32")
    assert [sc.combine_trips(g) for g in (1, 2, 8, 16, 32, 64)] == [0, 1, 1, 1, 2, 4]


def test_copy_scale_and_stale_edges():
    assert sc.copy_path(4096, 0) == "vector" and sc.copy_path(4096, 8) == "scalar" and sc.copy_path(4097, 0) == "scalar"
    assert sc.copy_path(4096, 4096 * 8 * 3) == "vector" and sc.copy_path(4097, 4097 * 8) == "scalar"
    assert sc.copy_whole_trips(4096, 512) and not sc.copy_whole_trips(4096, 1024) and not sc.copy_whole_trips(1100, 512)
    assert sc.flat_trips(4096, 512) == (1, False) and sc.flat_trips(4097, 512) == (2, False) and sc.flat_trips(300, 512) == (1, True)
    assert sc.flat_trips(2048, 256) == (1, False) and sc.flat_trips(2049, 256) == (2, False)
    for n in (48, 1100, 4096):
        for e in range(-1000, 1000, 7):
            for m in (1.0, 1.4142135, 1.9999999):
                rsq = n * m * 2.0 ** e
                s = sc.pick_scale(rsq, n)
                assert np.frexp(s)[0] == 0.5 and 0.7 <= np.sqrt(rsq / n) * s < 1.5, (n, e, m)
    assert sc.pick_scale(0.0, 64) == sc.pick_scale(np.inf, 64) == sc.pick_scale(np.nan, 64) == sc.pick_scale(1.8e308, 64) == 1.0
    n = 4096
    assert sc.stale(8.9e-13 * n, 1.0, n) and not sc.stale(9.0e-13 * n, 1.0, n) and not sc.stale(0.0, 1.0, n)
    assert sc.stale(n * 2.0 ** -42, 1.0, n) and not sc.stale(n * 2.0 ** -42, 4.0, n) and not sc.stale(np.nan, 1.0, n)
    assert sc.threshold_A(1.0, 1.0, 0.05, n) > 0 > sc.threshold_A(0.04, 1.0, 0.05, n)
    assert sc.threshold_A(1.0, 1.0, 1.0, n) > 0 and sc.threshold_A(0.0, 1.0, 0.0, n) > 0 and sc.threshold_A(0.0, 1.0, 1e-12, n) < 0
    assert [sc.means_store(p, True) for p in (256, 257, 512, 513)] == ["msm", "prt", "prt", "column loop"]
    assert [sc.means_store(p, False) for p in (256, 257, 512, 513)] == ["msm", "msm", "msm", "column loop"]


def test_plan_variant():
    f64, f32, E = np.float64, np.float32, sc.ENGINES
    assert sc.plan_variant(f64, False, 4096, 2048) == ("pair", 1024, "lds")
    assert sc.plan_variant(f64, False, 4096, 2048, E["pair512"]) == ("pair", 512, "lds")
    assert sc.plan_variant(f64, False, 4096, 2048, E["one"]) == ("one", 512, "lds")
    assert sc.plan_variant(f64, False, 4096, 2048, E["one256"]) == ("one", 256, "lds")
    assert sc.plan_variant(f64, False, 4096, 2048, {"PH_SWEEP_BLOCK": 256}) == ("one", 256, "lds")
    assert sc.plan_variant(f64, False, 4096, 2048, E["hbm"]) == ("one", 512, "hbm")
    assert sc.plan_variant(f32, False, 4096, 2048) == ("one", 512, "lds")
    assert sc.plan_variant(f64, True, 4096, 2048) == ("one", 512, "lds")
    assert sc.plan_variant(f64, False, 60, 59)[0] == "pair" and sc.plan_variant(f64, False, 60, 60)[0] == "one"
    assert sc.plan_variant(f64, False, 60, 2)[0] == "pair" and sc.plan_variant(f64, False, 60, 1)[0] == "one"
    # the pair kernel's two window-sized buffers stop fitting long before the one-window kernel's single one
    assert sc.pair_lds_bytes(9704) <= sc.LDS_LIMIT < sc.pair_lds_bytes(9705)
    assert sc.plan_variant(f64, False, 9704, 100)[0] == "pair" and sc.plan_variant(f64, False, 9705, 100) == ("one", 512, "lds") and sc.plan_variant(f64, False, 7968, 260)[0] == "pair"
    assert sc.plan_variant(f64, False, 20000, 100) == ("one", 512, "hbm")
    for case in sc.CASES:  # what the GPU test asserts of each engine through plan_info
        plans = {name: sc.plan_variant(case["dtype"], sc.general(case), case["n"], sc.n_periods_of(case), env) for name, env in E.items()}
        pairable = case["dtype"] == f64 and not sc.general(case) and sc.n_periods_of(case) < case["n"]
        assert (plans["pair"][0] == "pair") == pairable and (plans["pair512"][0] == "pair") == pairable, case["name"]
        assert all(plans[k][0] == "one" for k in sc.ONE_ENGINES) and plans["hbm"][2] == "hbm" and plans["one256"][1] == 256
    assert sc.resident_pairs(48, 1024, 256) == 512 and sc.resident_pairs(48, 512, 256) == 1024 and sc.resident_pairs(4096, 1024, 256) == 512
