"""The phases of k_mbest_step1_pair behind its screen passes, and the remainder-first order of the shared-load pass.

The survivor scan takes its radius from the host table (pair_radius at the row count of the period, a tighter bound than
the device's old estimate, so the survivor lists may shrink) and keeps a thread's entry in registers across the barrier,
the winner's geometry comes from the geometry table, and the row that already holds the winner is found by a ballot.
None of this may change a result: the pair kernel is run against the one-window fp64 kernel (PH_STEP1_PAIR=0), which
has none of these phases, on windows that take every branch of the bookkeeping --

  * seeded multi-sinusoid windows, windows of two components whose winners repeat (action 2), an all-zero window next
    to a live one, windows scaled by 2^300 and 2^-300, an odd number of windows (the last workgroup holds a single one);
  * N = 2246 and 2301, the smallest lengths at which the plan has shared passes of 3 ... 6 rows (tests/test_gpu_duo_edges.py),
    and N = 1024 with max_length = 250, where no period has a legal partner and the plan holds single passes only;
  * two candidates planted 1e-9 apart on both sides of their crossing (the construction of tests/test_gpu_pair.py);
  * a window in which a period wins again after ten repeats and is skipped (two planted periods in a range of eleven).

Periods, status, sweep counts and bases must be identical, powers must agree to 1e-13.

The shared-load pass folds the columns in front of the cut with the group of odd size FIRST (pair_duo_front in
pyperiod_amd/csrc/ph_pair.h), so that every group holding one of the first R - 1 columns stands at a compile-time
position.  `front()` restates that walk; the census asserts that every class (R, whole mod UA) occurs and that no peeled
group runs past `whole`, and the pass test bed (tools/micro/pair_pass_bench.hip, mode 3: the pass compiled as it is) folds
every legal base: both values of every pass must lie inside pair_radius x sum of squares.  At N = 2246 and 2301 the only
bases with six rows are q = 385 and q = 385 ... 396, all with whole = 5; N = 2309 is the smallest length at which the
class (6, 0) occurs as well, so it is taken along."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (2246, 2301)
CENSUS_LENGTHS = LENGTHS + (2309,)
TOL = 1e-10


# ---------------------------------------------------------------------------------------------- remainder-first order
def rows(n, p):
    return -(-n // p)


def legal(n, q):
    """The pairing rule of build_plan for a base q (its partner is q + 64)."""
    r = rows(n, q)
    return q >= 64 and q + 64 < n and 3 <= r <= 6 and -(-q // 64) > r and rows(n, q + 64) == r


def bases(n):
    return [q for q in range(64, n - 64) if legal(n, q)]


def front(n, q):
    """The groups of pair_duo_rows in front of the cut as (first column, width, columns without a square of q + 64,
    peeled?), and `whole`."""
    r = rows(n, q)
    ua = 4 if r <= 4 else 2
    cut = q - (r * q - n)
    last = -(-q // 64) - 1
    whole = min(cut >> 6, last)
    first = whole % ua or ua
    groups = [(0, first, min(r - 1, first), True)]
    c = first
    while c < r - 1:  # pair_duo_peel: unconditional, at compile-time positions
        groups.append((c, ua, min(r - 1 - c, ua), True))
        c += ua
    while c + ua <= whole:  # the main loop
        groups.append((c, ua, 0, False))
        c += ua
    return dict(R=r, UA=ua, whole=whole, groups=groups, end=c)


def test_every_class_of_the_front_occurs_and_no_peeled_group_runs_past_whole():
    seen = {}
    for n in CENSUS_LENGTHS:
        for q in bases(n):
            f = front(n, q)
            seen.setdefault((f["R"], f["whole"] % f["UA"]), []).append((n, q))
            assert f["whole"] >= f["R"] - 1, (n, q)
            for c0, width, nosq, peeled in f["groups"]:
                assert c0 + width <= f["whole"], (n, q, f)  # no group, peeled or not, runs past `whole`
                assert nosq == max(0, min(width, f["R"] - 1 - c0)), (n, q, f)  # exactly the columns in front of R - 1
                assert peeled or c0 >= f["R"] - 1, (n, q, f)  # the main loop squares every column
            assert f["end"] == f["whole"], (n, q, f)  # the main loop ends exactly at `whole`: no remainder behind it
            cols = [c for c0, width, _, _ in f["groups"] for c in range(c0, c0 + width)]
            assert cols == list(range(f["whole"])), (n, q)  # every column once, in order: the sums keep their order
    for key, where in sorted(seen.items()):
        print(f"R = {key[0]}, whole mod UA = {key[1]}: {len(where)} bases, e.g. {where[:2]}")
    want = {(r, m) for r in (3, 4, 5, 6) for m in range(4 if r <= 4 else 2)}
    assert set(seen) == want, sorted(want - set(seen))
    for n in LENGTHS:  # what the two smallest lengths hold on their own: everything but (6, 0)
        assert {k for k, where in seen.items() if any(w[0] == n for w in where)} == want - {(6, 0)}, n


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the pass test bed is compiled with hipcc"
    tmp = tmp_path_factory.mktemp("pair_phases")
    exe = str(tmp / "pair_pass_bench")
    subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I", os.path.join(ROOT, "pyperiod_amd", "csrc"),
         os.path.join(ROOT, "tools", "micro", "pair_pass_bench.hip"), "-o", exe],
        check=True, timeout=600, cwd=str(tmp))
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("n", CENSUS_LENGTHS)
def test_both_values_of_every_remainder_first_pass_stay_inside_the_radius(bench, n):
    qs = bases(n)
    assert qs and {rows(n, q) for q in qs} == {3, 4, 5, 6}
    out = subprocess.run([bench, "3", str(qs[0]), str(qs[-1] + 1), str(n)], check=True, timeout=300, capture_output=True, text=True).stdout
    print(out)
    m = re.search(r"(\d+) screen values against the fp64 fold: largest \|error\| / \(pair_radius x sum of squares\) = ([0-9.eE+-]+)", out)
    assert m, out
    assert int(m.group(1)) == 2 * 2 * len(qs)  # two windows, two periods per pass: exactly the legal bases
    assert f"N = {n}: every value inside its radius: yes" in out, out
    assert float(m.group(2)) <= 1.0, out


# ---------------------------------------------------------------------------------------------- pair kernel against one-window kernel
@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import PeriodEngine

    old = os.environ.get("PH_STEP1_PAIR")
    os.environ["PH_STEP1_PAIR"] = "0"
    single = PeriodEngine(0)
    os.environ["PH_STEP1_PAIR"] = "1"
    pair = PeriodEngine(0)
    if old is None:
        del os.environ["PH_STEP1_PAIR"]
    else:
        os.environ["PH_STEP1_PAIR"] = old
    yield single, pair
    single.close()
    pair.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def compare(single, pair, x, **kw):
    """Both kernels on the batch x; returns the pair kernel's outputs."""
    n = x.shape[1]
    assert pair.m_best_info(n, kw["num"], kw.get("max_length"), kw.get("min_length", 2)) == (2, 8)
    assert single.m_best_info(n, kw["num"], kw.get("max_length"), kw.get("min_length", 2))[0] == 1
    a = single.m_best(x, want_sweeps=True, **kw)
    b = pair.m_best(x, want_sweeps=True, **kw)
    ok = a[3] == 0
    scale = np.maximum(np.max(np.abs(a[1]), axis=1, keepdims=True), 1e-300)
    dpow = float(np.max(np.abs(a[1] - b[1])[ok] / np.broadcast_to(scale, a[1].shape)[ok])) if ok.any() else 0.0
    print(f"N = {n} {kw}: periods equal {np.array_equal(a[0], b[0])}, status {np.array_equal(a[3], b[3])}, sweeps "
          f"{np.array_equal(a[4], b[4])}, bases identical {np.array_equal(a[2][ok], b[2][ok])}, powers rel {dpow:.2e}, "
          f"sweeps {b[4].tolist()}")
    assert np.array_equal(a[0], b[0]), (n, kw)
    assert np.array_equal(a[3], b[3]), (n, kw)
    assert np.array_equal(a[4], b[4]), (n, kw)
    assert np.array_equal(a[2][ok], b[2][ok]), (n, kw)  # (the rows of a window whose step 1 failed are no contract)
    assert dpow <= 1e-13, (n, kw, dpow)  # each window against its own largest power
    return b


def two_periods(n, p, q, seed=5):
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(p)[t % p] + rng.standard_normal(q)[t % q] + 1e-6 * rng.standard_normal(n)


def batch(n, seed):
    """Seven windows (odd: the last workgroup holds one): multi-sinusoids, a zero window next to a live one, 2^+-300, and
    two windows whose two components take turns, so that a winner repeats (action 2): periods 181 and 191 (plain m_best:
    one repeat at num = 3, two at num = 10, by the oracle's sweep) and periods 7 and 11 (m_best_gamma: two or three)."""
    x = multi_sinusoid_batch(seed, 7, n)
    x[1] = 0.0
    x[2] *= 2.0 ** 300
    x[3] *= 2.0 ** -300
    x[4] = two_periods(n, 181, 191)
    x[5] = two_periods(n, 7, 11)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("gamma", (False, True))
@pytest.mark.parametrize("num", (3, 10))
def test_pair_kernel_equals_one_window_kernel_with_shared_passes(engines, n, gamma, num):
    single, pair = engines
    x = batch(n, 700 + n)
    b = compare(single, pair, x, num=num, gamma=gamma)
    assert b[3][1] == 1 and b[3][0] == 0 and b[3][6] == 0  # the zero window has no period, its neighbour is not disturbed
    assert b[3][4] == 0 and b[3][5] == 0 and b[4][5 if gamma else 4] > num  # a winner repeated: a row was accumulated (action 2)
    # exact power-of-two scaling leaves the decisions alone
    plain = pair.m_best(multi_sinusoid_batch(700 + n, 7, n)[2:4], num, gamma=gamma)
    assert np.array_equal(b[0][2:4], plain[0])
    want = po.m_best(x[0], num, gamma=gamma)
    assert np.array_equal(b[0][0], want[0])
    assert np.max(np.abs(b[1][0] - want[1])) <= TOL * np.max(np.abs(want[1]))


def _planted(n, p, q, b, seed=3):
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    sp = rng.standard_normal(p)[t % p]
    sq = rng.standard_normal(q)[t % q]
    return sp + b * sq + 1e-3 * rng.standard_normal(n)


@pytest.fixture(scope="module")
def crossing():
    """Amplitudes 1e-9 / 1e-8 (relative, in the norm) to either side of the crossing of the families of 61 and 67 within
    [2, 250] at N = 1024, found by bisection on the oracle as in tests/test_gpu_pair.py."""
    n, p, q, hi = 1024, 61, 67, 250

    def gap(b):
        v = po.sweep_norms(_planted(n, p, q, b), 2, hi)
        fam_p = max(v[k * p - 2] for k in range(1, hi // p + 1))
        fam_q = max(v[k * q - 2] for k in range(1, hi // q + 1))
        return fam_q - fam_p, max(fam_p, fam_q)

    lo_b, hi_b = 0.5, 2.0
    assert gap(lo_b)[0] < 0 < gap(hi_b)[0]
    for _ in range(60):
        mid = 0.5 * (lo_b + hi_b)
        if gap(mid)[0] < 0:
            lo_b = mid
        else:
            hi_b = mid
    amps = (lo_b * (1 - 2e-9), lo_b * (1 - 2e-8), hi_b * (1 + 2e-9), hi_b * (1 + 2e-8))
    for b in amps:
        g, top = gap(b)
        assert 1e-12 < abs(g) / top < 1e-6  # inside the float radius, far outside an fp64 tie
    return n, p, q, hi, amps


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", (False, True))
@pytest.mark.parametrize("num", (3, 10))
def test_pair_kernel_equals_one_window_kernel_with_single_passes_only(engines, crossing, gamma, num):
    single, pair = engines
    n, p, q, hi, amps = crossing
    assert not any(legal(n, c) and c + 64 <= hi for c in range(64, hi + 1))  # no period of the range has a partner
    x = np.concatenate([np.stack([_planted(n, p, q, b) for b in amps]), batch(n, 41)[:3]])  # 4 + live, zero, 2^300: seven windows
    b = compare(single, pair, x, num=num, gamma=gamma, max_length=hi)
    assert np.array_equal(b[3], [0, 0, 0, 0, 0, 1, 0])
    sides = set()
    for w in range(4):  # the planted windows follow the oracle on both sides of the crossing
        want = po.m_best(x[w], num, max_length=hi, gamma=gamma)
        assert np.array_equal(b[0][w], want[0]), (w, b[0][w], want[0])
        assert np.max(np.abs(b[1][w] - want[1])) <= TOL * np.max(np.abs(want[1]))
        sides.add(int(po.m_best(x[w], 1, max_length=hi)[0][0]) % p == 0)
    assert sides == {True, False}  # the winner really changes sides


def step1_events(x, num, lo, hi):
    """The branch every sweep of step 1 takes (Periods.py:518-535), restated with the oracle's sweep."""
    work, periods, skip, repeats, ev = x.copy(), [], set(), 0, []
    while len(periods) < num and len(ev) < 200:
        v = po.sweep_norms(work, lo, hi)
        for s in skip:
            v[s - lo] = -1.0
        top = lo + int(np.argmax(v))
        assert v[top - lo] > 0
        if top in periods and repeats < 10:
            ev.append("repeat")
            repeats += 1
        elif top in periods:
            ev.append("skip")
            skip.add(top)
            repeats = 0
        else:
            ev.append("new")
            periods.append(top)
            repeats = 0
        work = work - po.project(work, top)
    return ev, periods


@pytest.mark.gpu
@pytest.mark.parametrize("num", (3, 10))
def test_a_period_skipped_after_ten_repeats(engines, num):
    """Components of period 61 and 67 and eleven candidate periods, 60 ... 70: the two take turns until one of them has
    won ten times in a row of known periods, wins again, and is skipped."""
    single, pair = engines
    n, lo, hi = 1024, 60, 70
    planted = two_periods(n, 61, 67)
    ev, _ = step1_events(planted, num, lo, hi)
    assert ev.count("skip") >= 1 and ev.count("repeat") >= 10, ev
    x = np.stack([planted, multi_sinusoid_batch(8, 1, n)[0], planted[::-1].copy()])
    b = compare(single, pair, x, num=num, min_length=lo, max_length=hi)
    assert b[3][0] == 0 and b[4][0] == len(ev)  # as many sweeps as the restated loop
    want = po.m_best(planted, num, max_length=hi, min_length=lo)
    assert np.array_equal(b[0][0], want[0])
    assert np.max(np.abs(b[1][0] - want[1])) <= TOL * np.max(np.abs(want[1]))
