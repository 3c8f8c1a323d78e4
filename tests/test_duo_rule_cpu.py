"""The shared-load pass of the window-pair screen (pair_pass_duo in pyperiod_amd/csrc/ph_pair.h), pinned on the CPU.

A wavefront that folds period q holds a[r][c] = x[64 c + lane + r q]; the fold of q + 64 is the sum of the same values
one column further per row, S_{q+64}[64 c + lane] = sum_r a[r][c + r].  The host pairs q with q + 64 when both have the
same row count R = ceil(N / q), 3 <= R <= 6, and q >= 64.  Checked here, on integer-valued data (so every sum is exact), for every
legal pair in (floor(N / 3) / 2, floor(N / 3)]:
  * the column-shifted sums under the load rule (row r, column c is read only while 64 c + r q < N) are the fold of q + 64,
    and the plain column sums the fold of q;
  * no index >= N + 64 is read (the window is followed by zeroed elements; the largest index read is N + 62);
  * the cut identity nfull(q + 64) = nfull(q) - 64 (R - 1): both periods cross their cut in the same column and lane;
  * a model of the pass as the kernel walks it (groups of columns, R - 1 pending sums, the tail behind the last column
    of q) puts every residue of both periods exactly once on its side of the cut, with the right sum and with exactly
    the loads the rule allows.  The host plans the pass only where q has more chunk columns than rows (q > 64 R).
N = 1000 is the hard small case for the rule: 4 chunk columns but 6 rows."""
import numpy as np
import pytest

SIZES = (1000, 1200, 1536, 4095, 4096, 4097)
PAD = 256  # kPad of ph_device.h


def rows_of(n, q):
    return -(-n // q)


def legal_bases(n):
    """Bases q of a shared-load pass with both periods in (floor(n / 3) / 2, floor(n / 3)]."""
    hi = n // 3
    lo = hi // 2 + 1
    return [q for q in range(max(lo, 64), hi - 63) if 3 <= rows_of(n, q) <= 6 and rows_of(n, q) == rows_of(n, q + 64)]


def fold(x, n, p):
    s = np.zeros(p, dtype=np.int64)
    for j in range(p):
        s[j] = x[j:n:p].sum()
    return s


def window(n, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(n + PAD, dtype=np.int64)
    x[:n] = rng.integers(-1000, 1000, size=n)
    return x


def shifted_sums(x, n, q):
    """The rule of the issue, column by column: -> (S_q, S_{q+64}, largest index read, wavefront loads)."""
    R = rows_of(n, q)
    ncb = -(-q // 64)
    ncol = ncb + R
    a = np.zeros((R, ncol, 64), dtype=np.int64)
    top, loads = -1, 0
    for r in range(R):
        for c in range(ncol):
            if 64 * c + r * q < n and r >= c - ncb:
                a[r, c] = x[64 * c + r * q: 64 * c + r * q + 64]
                top = max(top, 64 * c + r * q + 63)
                loads += 1
    base = a[:, :ncb].sum(axis=0).reshape(-1)[:q]
    partner = np.zeros((ncb + 1, 64), dtype=np.int64)
    for c in range(ncb + 1):
        for r in range(R):
            partner[c] += a[r, c + r] if c + r < ncol else 0
    return base, partner.reshape(-1)[:q + 64], top, loads


def planned_bases(n):
    """The legal bases the host plan pairs: the pass is built for more chunk columns than rows (q > 64 R)."""
    return [q for q in legal_bases(n) if -(-q // 64) > rows_of(n, q)]


def kernel_walk(x, n, q):
    """pair_duo_rows step by step: -> per-residue sums of (sa, sb, pa, pb), split at the cut; largest index; loads."""
    R = rows_of(n, q)
    cut = n - (R - 1) * q
    ncb = -(-q // 64)
    last = ncb - 1
    assert ncb > R
    lane = np.arange(64)
    pend = [np.zeros(64, dtype=np.int64) for _ in range(R - 1)]
    acc = {k: {} for k in ("sa", "sb", "pa", "pb")}  # residue -> sum
    st = {"top": -1, "loads": 0}

    def load(off):
        st["top"] = max(st["top"], off + 63)
        st["loads"] += 1
        return x[off: off + 64].copy()

    def put(name, js, vals, keep=None):
        for k in np.nonzero(np.ones(64, bool) if keep is None else keep)[0]:
            assert int(js[k]) not in acc[name]
            acc[name][int(js[k])] = int(vals[k])

    def group(c, nr, u_cols, lanes=False):
        """pair_duo_group<R, nr, u_cols, PRO, lanes>; PRO (a wave-uniform 0 for the unfinished sum) is modelled as 'no put'"""
        for u in range(u_cols):
            col = c + u
            v = [load(64 * col + r * q) for r in range(nr)]
            t = sum(v)
            d = pend[R - 2] + (v[R - 1] if nr == R else 0)
            j = 64 * col + lane
            jp = j - 64 * (R - 1)
            on = col >= R - 1
            if lanes and nr == R:
                full = j < cut
                put("sa", j, t, full)
                put("sb", j, t, ~full & (j < q))
                if on:
                    put("pa", jp, d, full)
                    put("pb", jp, d, ~full)
            elif lanes:
                put("sb", j, t, j < q)
                if on:
                    put("pb", jp, d)
            else:
                put("sa" if nr == R else "sb", j, t)
                if on:
                    put("pa" if nr == R else "pb", jp, d)
            for k in range(R - 2, 0, -1):
                pend[k] = pend[k - 1] + v[k]
            pend[0] = v[0].copy()

    ua = 4 if R <= 4 else 2
    ub = 4 if R <= 4 else 3 if R == 5 else 2
    c = 0
    whole = min(cut >> 6, last)
    while c + ua <= whole:
        group(c, R, ua)
        c += ua
    while c < whole:
        group(c, R, 1)
        c += 1
    if c < last and 64 * c < cut:
        group(c, R, 1, lanes=True)
        c += 1
    while c + ub <= last:
        group(c, R - 1, ub)
        c += ub
    while c < last:
        group(c, R - 1, 1)
        c += 1
    group(last, R if 64 * last < cut else R - 1, 1, lanes=True)
    # pair_duo_tail
    v = {}
    for t in range(R - 2):
        for r in range(t, R - 2):
            v[r, t] = load(64 * (ncb + t) + r * q)
    for t in range(R - 1):
        off = 64 * (ncb + t) + (R - 2) * q
        v[R - 2, t] = load(off) if off < n else np.zeros(64, dtype=np.int64)
    for t in range(R - 1):
        put("pb", 64 * (ncb + t - (R - 1)) + lane, pend[R - 2])
        for k in range(R - 2, 0, -1):
            pend[k] = pend[k - 1] + v[k, t] if k >= t else pend[k - 1]
        if t == 0:
            pend[0] = v[0, 0]
    put("pb", 64 * ncb + lane, pend[R - 2], 64 * (ncb - 1) + lane < q)
    return acc, st["top"], st["loads"]


@pytest.mark.parametrize("n", SIZES)
def test_shifted_columns_are_the_fold_of_the_partner(n):
    x = window(n, n)
    bases = legal_bases(n)
    assert bases, n
    worst = -1
    for q in bases:
        R = rows_of(n, q)
        assert rows_of(n, q + 64) == R and 3 <= R <= 6 and q >= 64
        # cut identity: nfull(p) = n - (R - 1) p
        assert (n - (R - 1) * (q + 64)) == (n - (R - 1) * q) - 64 * (R - 1) >= 1
        base, partner, top, _ = shifted_sums(x, n, q)
        assert np.array_equal(base, fold(x, n, q)), q
        assert np.array_equal(partner, fold(x, n, q + 64)), q
        assert top < n + 64, (q, top)
        worst = max(worst, top)
    assert worst <= n + 62


@pytest.mark.parametrize("n", SIZES)
def test_the_walk_of_the_kernel_reads_what_the_rule_allows_and_sums_the_same(n):
    x = window(n, 7 * n + 1)
    assert planned_bases(n) or n == 1000
    for q in planned_bases(n):
        R = rows_of(n, q)
        cut = n - (R - 1) * q
        acc, top, loads = kernel_walk(x, n, q)
        _, _, top_rule, loads_rule = shifted_sums(x, n, q)
        assert loads == loads_rule and top == top_rule and top < n + 64, q
        sq, sp = fold(x, n, q), fold(x, n, q + 64)
        # every residue exactly once, on the side of the cut its sample count puts it
        assert sorted(acc["sa"]) == list(range(cut)) and sorted(acc["sb"]) == list(range(cut, q)), q
        cut_p = cut - 64 * (R - 1)
        assert sorted(acc["pa"]) == list(range(cut_p)) and sorted(acc["pb"]) == list(range(cut_p, q + 64)), q
        assert all(acc["sa"][j] == sq[j] for j in acc["sa"]) and all(acc["sb"][j] == sq[j] for j in acc["sb"]), q
        assert all(acc["pa"][j] == sp[j] for j in acc["pa"]) and all(acc["pb"][j] == sp[j] for j in acc["pb"]), q


def test_no_pair_at_600():
    assert legal_bases(600) == []


def test_plan_counts_at_4096():
    """The greedy pairing of the host plan (ascending, inside a row class) over (682, 1365]: 290 shared passes and 103
    singles, 0.633 of the loads of 683 single passes."""
    n, lo, hi = 4096, 683, 1365
    covered, duo, single = set(), [], []
    for p in range(lo, hi + 1):
        if p in covered:
            continue
        R = rows_of(n, p)
        if p + 64 <= hi and 3 <= R <= 6 and rows_of(n, p + 64) == R:
            covered.add(p + 64)
            duo.append(p)
        else:
            single.append(p)
    assert (len(duo), len(single)) == (290, 103)

    def single_loads(p):
        R = rows_of(n, p)
        cut = n - (R - 1) * p
        acols = min(p, (cut + 63) & ~63)
        return -(-cut // 64) * R + -(-(p - acols) // 64) * (R - 1)

    x = np.zeros(n + PAD, dtype=np.int64)
    before = sum(single_loads(p) for p in range(lo, hi + 1))
    after = sum(shifted_sums(x, n, q)[3] for q in duo) + sum(single_loads(p) for p in single)
    assert before == 45281
    assert after <= 0.65 * before
    print(f"wavefront loads per window pair and sweep: {before} -> {after} ({after / before:.3f} x)")
