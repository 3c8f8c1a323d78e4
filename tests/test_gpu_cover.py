"""Plain m_best through the window-pair screen with the cover rule (ph_pair.h): only the periods in
(max_length // 2, max_length] are screened, a smaller period is evaluated only when one of its multiples survives.

Three engines -- the rule on (default), off (PH_PAIR_COVER=0: every period screened, the kernel as it was) and the
one-window fp64 kernel (PH_STEP1_PAIR=0) -- must give identical periods, status and sweep counts and bit-identical
bases, powers within 1e-13 of each other; against the oracle periods equal, powers and bases within 1e-10.
"""

import os
import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po
from pyperiod_amd.synth import multi_sinusoid_batch

pytestmark = pytest.mark.gpu
TOL = 1e-10  # against the oracle
KTOL = 1e-13  # powers, kernel against kernel (test_gpu_pair.py)


def _engine(**env):
    from pyperiod_amd import PeriodEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
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
    on = _engine(PH_STEP1_PAIR="1", PH_PAIR_COVER="1")
    off = _engine(PH_STEP1_PAIR="1", PH_PAIR_COVER="0")
    single = _engine(PH_STEP1_PAIR="0")
    assert on.m_best_info(4096, 10) == (2, 8) and off.m_best_info(4096, 10) == (2, 8) and single.m_best_info(4096, 10) == (1, 8)
    # the rule halves the screened range: 683 few-row singles instead of the mixed plan over 2..1365
    assert on.m_best_plan_info(4096, 10) == (683, 1364) and off.m_best_plan_info(4096, 10)[0] > 683
    yield on, off, single
    for e in (on, off, single):
        e.close()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _np(out):
    return [o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in out]


def _same(a, b, what):
    """periods, status, sweeps identical; bases bit for bit; powers within KTOL."""
    good = (a[3] == 0) & (b[3] == 0)
    print(what, "periods", np.array_equal(a[0], b[0]), "status", np.array_equal(a[3], b[3]), "sweeps", np.array_equal(a[4], b[4]),
          "bases", np.array_equal(a[2][good], b[2][good]), "powers rel", rel_err(b[1][good], a[1][good]) if good.any() else None)
    assert np.array_equal(a[0], b[0]), (what, np.nonzero((a[0] != b[0]).any(1))[0][:10])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), what
    ok = a[3] == 0  # (what a window whose step 1 failed leaves in its rows is no contract)
    assert np.array_equal(a[2][ok], b[2][ok]), what
    assert not ok.any() or rel_err(b[1][ok], a[1][ok]) < KTOL, what


def _three(engines, x, what, oracle_rows=(0,), **kw):
    on, off, single = engines
    a = _np(on.m_best(x, want_sweeps=True, **kw))
    b = _np(off.m_best(x, want_sweeps=True, **kw))
    c = _np(single.m_best(x, want_sweeps=True, **kw))
    _same(b, a, f"{what} on/off")
    _same(c, a, f"{what} on/single")
    xh = x.cpu().numpy() if hasattr(x, "cpu") else x
    okw = {k: v for k, v in kw.items() if k != "num"}
    for w in oracle_rows:
        try:
            want = po.m_best(xh[w], kw.get("num", 5), **okw)
        except TypeError:  # the reference runs out of candidates (Periods.py:520/537)
            assert a[3][w] != 0, (what, w)
            continue
        assert a[3][w] == 0 and np.array_equal(a[0][w].astype(np.int64), np.asarray(want[0]).astype(np.int64)), (what, w, a[0][w], want[0])
        assert rel_err(a[1][w], want[1]) < TOL and rel_err(a[2][w], want[2]) < TOL, (what, w)
    return a


def test_full_config2_batch(engines):
    import torch

    xh = multi_sinusoid_batch(0, 1024, 4096)
    x = torch.from_numpy(xh).cuda()
    _three(engines, x, "config 2, 1024 windows", oracle_rows=(0, 511, 1023), num=10)
    _three(engines, x[:1023], "config 2, 1023 windows", oracle_rows=(1022,), num=10)


def test_odd_batches_and_lengths(engines):
    for n, w, kw in (
        (4096, 7, dict(num=10)),
        (4096, 1, dict(num=6)),
        (1000, 5, dict(num=5, max_length=499, min_length=3)),
        (1000, 3, dict(num=4, max_length=900)),
        (97, 3, dict(num=3)),
        (240, 9, dict(num=12, max_length=60)),
        (6000, 3, dict(num=4)),
    ):
        _three(engines, multi_sinusoid_batch(50 + n, w, n), f"N={n} W={w} {kw}", **kw)


def test_period_ranges(engines):
    """Nothing to cover (min_length > max_length / 2), min_length = 1, odd and even max_length, max_length below 64,
    near N / 2 and near N - 1; short-period components in the data so that the winners ARE divisors of top periods."""
    rng = np.random.default_rng(11)
    n = 4096
    t = np.arange(n)
    x = np.stack([3.0 * rng.standard_normal(6)[t % 6] + 2.0 * rng.standard_normal(48)[t % 48] +
                  1.5 * rng.standard_normal(35)[t % 35] + 0.2 * rng.standard_normal(n) for _ in range(3)])
    for lo, hi in ((700, 1365), (683, 1365), (682, 1365), (1, 1365), (1, 2), (2, 1364), (2, 50), (7, 40), (2, 63), (2, 64),
                   (33, 100), (2, 2047), (2, 2048), (2, 2049), (2, 4094), (2, 4095), (1, 4095)):
        _three(engines, x, f"range {lo}..{hi}", num=4, min_length=lo, max_length=hi)


def test_noise_free_period_wins_through_the_divisor_list(engines):
    """A noise-free period-T window ties T with every multiple up to rounding; the winner must be T or a small
    multiple -- a divisor of the screened periods, never screened itself.  Which of the tied periods wins is decided
    by rounding, so the kernels are held to the structure, not to each other."""
    rng = np.random.default_rng(5)
    for n, T in ((3000, 75), (4096, 12), (4096, 35)):
        x = np.tile(rng.standard_normal(T), n // T + 1)[None, :n] + 0.0
        xb = np.concatenate([x, multi_sinusoid_batch(9, 1, n)])
        outs = [_np(e.m_best(xb, 3, want_sweeps=True)) for e in engines]
        for o in outs:
            assert o[0][0][0] % T == 0 and o[0][0][0] <= (n // 3) // 2, (n, T, o[0][0])
            assert np.array_equal(o[0][1], outs[0][0][1]) and np.array_equal(o[3], outs[0][3])
        want = po.m_best(xb[1], 3)
        assert np.array_equal(outs[0][0][1], want[0]) and rel_err(outs[0][2][1], want[2]) < TOL
    # with a little noise the tie is broken and the three kernels and the oracle agree on every pick
    x = np.tile(rng.standard_normal(12), 4096 // 12 + 1)[None, :4096] + 1e-3 * rng.standard_normal((2, 4096))
    _three(engines, x, "period 12 + 1e-3 noise", oracle_rows=(0, 1), num=3)


def _oracle_step1(x, num, lo, hi):
    """Step 1 of the oracle (Periods.py:494-537), one (skip set, winner) per sweep."""
    work, periods, skip, i, repeats, out = x.copy(), [0] * num, set(), 0, 0, []
    while i < num:
        top_norm, top_p, top_base = 0, 0, None
        for p in range(lo, hi + 1):
            base = po.project(work, p)
            nrm = po.periodic_norm(base)
            if nrm > top_norm and p not in skip:
                top_p, top_norm, top_base = p, nrm, base
        out.append((set(skip), top_p))
        if top_p in periods and repeats < 10:
            repeats += 1
        elif top_p in periods:
            skip.add(top_p)
            repeats = 0
        else:
            periods[i] = top_p
            i += 1
            repeats = 0
        work = work - top_base
    return out


def test_skipped_top_period_still_covers_its_divisors(engines):
    """White noise of 97 samples, periods 5 ... 20, twelve rows: the spaces overlap so much that present periods win
    again and again, after ten repeats a period is skipped (Periods.py:525-529), and in every one of these windows a
    top period (11 ... 20) is skipped while a divisor of it is still eligible and WINS a later sweep with a norm far
    above rounding (checked here on the oracle's own step 1): the kernel must find it through the skipped period."""
    n, lo, hi, num = 97, 5, 20, 12
    x = np.stack([np.random.default_rng(seed).standard_normal(n) for seed in range(5)])
    for w in range(5):
        sweeps = _oracle_step1(x[w], num, lo, hi)
        assert any(m > hi // 2 and win < m and m % win == 0 for skip, win in sweeps for m in skip), w
    a = _three(engines, x, "skipped top periods", oracle_rows=range(5), num=num, min_length=lo, max_length=hi)
    assert int(a[4].min()) >= num + 11  # every window went through a skip


def test_few_periods_and_more_rows_than_periods(engines):
    """As many rows as candidate periods, or more: periods are skipped until none is left (status 1), and with every
    top period skipped the kernel falls back to evaluating every period.  The last picks here are divisors of periods
    that have been removed already -- their norms are rounding noise, and which of them the ORACLE takes is decided by
    its own rounding -- so the three kernels are held to each other, not to the oracle."""
    rng = np.random.default_rng(3)
    n = 1000
    t = np.arange(n)
    x = np.stack([sum(rng.standard_normal(p)[t % p] for p in (3, 4, 5, 6, 7, 9, 10, 12)) + 0.3 * rng.standard_normal(n)
                  for _ in range(5)])
    for lo, hi, num in ((3, 7, 5), (3, 7, 6), (2, 9, 8), (2, 9, 9), (2, 12, 11), (5, 11, 7), (3, 6, 4), (3, 6, 5)):
        _three(engines, x, f"few periods {lo}..{hi} num={num}", oracle_rows=(), num=num, min_length=lo, max_length=hi)


def test_gamma_is_untouched_by_the_switch(engines):
    on, off, _ = engines
    for n, w, kw in ((4096, 5, dict(num=6)), (1000, 3, dict(num=4, max_length=900)), (240, 4, dict(num=5, max_length=60))):
        x = multi_sinusoid_batch(70 + n, w, n)
        a = _np(on.m_best(x, gamma=True, want_sweeps=True, **kw))
        b = _np(off.m_best(x, gamma=True, want_sweeps=True, **kw))
        for k in range(5):
            assert np.array_equal(a[k], b[k]), (n, k)
        want = po.m_best(x[0], kw["num"], max_length=kw.get("max_length"), gamma=True)
        assert np.array_equal(a[0][0], want[0]) and rel_err(a[1][0], want[1]) < TOL and rel_err(a[2][0], want[2]) < TOL
    # m_best and m_best_gamma in alternation on one context: each gets its own plan
    x = multi_sinusoid_batch(3, 4, 4096)
    first = [_np(on.m_best(x, 5, gamma=g, want_sweeps=True)) for g in (False, True)]
    for _ in range(2):
        for g in (False, True):
            again = _np(on.m_best(x, 5, gamma=g, want_sweeps=True))
            for k in range(5):
                assert np.array_equal(again[k], first[int(g)][k]), (g, k)


def test_degenerate_and_extreme_scale_windows(engines):
    on, off, single = engines
    n = 2048
    base = multi_sinusoid_batch(70, 7, n)
    xb = base.copy()
    xb[1] = 0.0  # no positive norm: status 1
    xb[2] *= 2.0 ** 600  # squares overflow a double: not screened, every period exactly
    xb[3] *= 2.0 ** -500
    xb[4] *= 2.0 ** 500
    xb[5, 100] = np.nan
    a = _np(on.m_best(xb, 5, want_sweeps=True))
    b = _np(off.m_best(xb, 5, want_sweeps=True))
    c = _np(single.m_best(xb, 5, want_sweeps=True))
    for o in (b, c):
        assert np.array_equal(a[3], o[3]) and np.array_equal(a[4], o[4])
        assert np.array_equal(a[0], o[0])
        for w in (0, 3, 4, 6):
            assert np.array_equal(a[2][w], o[2][w]) and rel_err(o[1][w], a[1][w]) < KTOL, w
    assert a[3][1] == 1 and a[3][0] == 0
    for w in (0, 3, 4, 6):
        want = po.m_best(xb[w], 5)
        assert np.array_equal(a[0][w], want[0]) and rel_err(a[1][w], want[1]) < TOL and rel_err(a[2][w], want[2]) < TOL
    # exact power-of-two scaling leaves the period list alone
    assert np.array_equal(a[0][3], on.m_best(base[3:4], 5)[0][0]) and np.array_equal(a[0][4], on.m_best(base[4:5], 5)[0][0])
