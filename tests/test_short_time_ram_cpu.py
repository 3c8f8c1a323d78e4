"""ShortTime.decompose_ramanujan without a GPU: the numpy restatement of the capped selection rule
(``select_ref``) that tests/test_gpu_short_time_ram.py holds k_ram_select_ref to, the planted norm table of that test
and a census of the paths it reaches, the host-route restatement of the whole pipeline on the test recording, the new
C-ABI symbol with its refusals, and the argument errors of decompose_ramanujan.

The rule (include/periodhip.h, ph_ramanujan_select): m = ref, or |max| of the row as numpy.max sees it; the candidates
are the q with norms[q] / m > thresh; `over` counts them; when there are more than pcap, q is kept iff fewer than pcap
candidates q' have norms[q'] > norms[q], or norms[q'] == norms[q] and q' < q; the kept periods are listed ascending."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_get_periods_cpu import closed_form
from test_short_time_cpu import frames_ref, sqrt_hann

THRESH = 0.25  # of the planted table: bigs lie in [0.5, 1] x level, smalls in [0, 0.1] x level
Q_HIS = (1, 62, 63, 64, 65, 127, 128, 129, 200)
PCAPS = (1, 2, 7, 64)
COND_CUT = 1e7  # tests/test_gpu_ram_fit.py


# ------------------------------------------------------------------ the rule
def select_ref(norms, thresh, ref=None, pcap=64):
    """One row -> (periods (pcap) int32, count, over), written from the rule."""
    norms = np.asarray(norms, dtype=np.float64)
    if ref is None:
        m = np.abs(np.nan if np.isnan(norms).any() else np.max(norms))
    else:
        m = np.float64(ref)
    with np.errstate(all="ignore"):
        cand = np.flatnonzero(norms / m > thresh)
    over = cand.size
    if over > pcap:
        v = norms[cand]
        # beaten[i] = how many candidates come before candidate i
        beaten = ((v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (cand[None, :] < cand[:, None]))).sum(axis=1)
        cand = cand[beaten < pcap]
    per = np.zeros(pcap, dtype=np.int32)
    per[: cand.size] = cand
    return per, int(cand.size), int(over)


def select_ref_batch(norms, thresh, ref=None, pcap=64):
    """(W, q_hi + 1) -> periods (W, pcap) int32, counts (W) int32, over (W) int32; `ref` None or W levels."""
    rows = [select_ref(r, thresh, None if ref is None else ref[w], pcap) for w, r in enumerate(norms)]
    return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.int32))


# ------------------------------------------------------------------ the planted table
def planted(q_hi, pcap, with_ref):
    """-> (norms (W, q_hi + 1), ref (W) or None, labels): the rows tests/test_gpu_short_time_ram.py gives the kernel at
    THRESH.  Without `ref` every row's level is its own maximum; with it the level is planted beside the row."""
    n = q_hi + 1
    rng = np.random.default_rng(1000 * q_hi + 10 * pcap + int(with_ref))
    rows, refs, labels = [], [], []

    def add(label, row, ref=1.0):
        rows.append(np.asarray(row, dtype=np.float64))
        refs.append(ref)
        labels.append(label)

    def smalls():
        return rng.uniform(0.0, 0.1, n)

    def bigs(k):
        """k distinct values in [0.5, 1), the largest replaced by 1.0 (the row's own maximum)."""
        v = 0.5 + rng.permutation(4096)[:k] / 8192.0
        if k:
            v[np.argmax(v)] = 1.0
        return v

    for k in (pcap - 1, pcap, pcap + 1, n):  # over = k where the row is long enough
        k = min(max(k, 0), n)
        row = smalls()
        row[rng.permutation(n)[:k]] = bigs(k)
        add(f"over={k}", row)
    # a tie straddling the cut at the first, a middle and the last lane of a stride: `keep` of the tied entries fit
    for stride in sorted({0, (n - 1) // 64}):
        lanes = sorted({min(64 * stride + l, n - 1) for l in (0, 31, 63)})
        for keep in (1, 2):
            above = pcap - keep
            free = np.setdiff1d(np.arange(n), lanes)
            if above < 0 or above > free.size or keep >= len(lanes):
                continue
            row = smalls()
            row[lanes] = 0.625
            row[rng.permutation(free)[:above]] = 0.75 + rng.permutation(1024)[:above] / 8192.0
            add(f"tie stride {stride} keep {keep}", row, 1.0)
    add("all equal", np.full(n, 3.0), 3.0)
    add("last mantissa bit", 1.0 + rng.permutation(n) * 2.0**-52, 1.0)
    add("exponent only", 2.0 ** -rng.permutation(n).astype(np.float64), 2.0**-300)
    add("denormals", (1 + rng.permutation(n)) * 5e-324, 5e-324)
    row = smalls()
    row[rng.permutation(n)[: min(n, pcap + 2)]] = bigs(min(n, pcap + 2))
    row[rng.integers(n)] = np.inf
    add("+inf", row)
    row = smalls()
    row[rng.permutation(n)[: min(n, pcap + 2)]] = bigs(min(n, pcap + 2))
    neg = rng.permutation(n)[: max(1, n // 3)]
    row[neg] = np.where(np.arange(neg.size) % 2 == 0, -0.0, -5.0)
    add("-0.0 and negative", row)
    row = smalls()
    row[rng.permutation(n)[: min(n, pcap + 2)]] = bigs(min(n, pcap + 2))
    row[rng.integers(n)] = np.nan
    add("one NaN", row)
    add("zero row", np.zeros(n), 0.0)
    if with_ref:
        row = smalls()
        row[rng.permutation(n)[: min(n, pcap + 1)]] = bigs(min(n, pcap + 1))
        add("ref NaN", row, np.nan)
    norms = np.stack(rows)
    assert norms.shape[0] <= 32
    return norms, (np.array(refs) if with_ref else None), labels


# ------------------------------------------------------------------ the recording and its host route
R_N, R_HOP, R_QHI, R_L = 96, 24, 32, 420
R_P7, R_P12, R_ZERO, R_QUIET, R_BURST = (0, 130), (130, 220), (220, 336), (336, 372), (372, 420)
R_GAIN = {7: 4.0, 12: 1.0}  # the period-12 pattern is mostly period 2, whose norm is large: the period-7 pattern is raised to its level
R_SEED = 2  # (the first seed tried; the census below holds its share of ill-conditioned frames)


def recording():
    """A period-7 pattern, then a period-12 pattern, exact zeros, 1e-3 noise and a burst of unit noise."""
    rng = np.random.default_rng(R_SEED)
    x = np.zeros(R_L)
    for (lo, hi), p in ((R_P7, 7), (R_P12, 12)):
        wave = rng.integers(-8, 9, p) / 4.0
        x[lo:hi] = R_GAIN[p] * np.tile(wave - wave.mean(), R_L // p + 1)[lo:hi]
    x[R_QUIET[0] : R_QUIET[1]] = 1e-3 * rng.standard_normal(R_QUIET[1] - R_QUIET[0])
    x[R_BURST[0] : R_BURST[1]] = 4.0 * rng.standard_normal(R_BURST[1] - R_BURST[0])
    return x


def reference_level(norms, reference):
    """None for "frame"; W copies of the largest finite row maximum for "recording" (NaN when no row has a finite
    positive one); W copies of an absolute level."""
    W = norms.shape[0]
    if reference == "frame":
        return None
    if reference == "recording":
        rmax = np.array([np.nan if np.isnan(r).any() else r.max() for r in norms])
        rmax = rmax[np.isfinite(rmax)]
        level = rmax.max() if rmax.size and rmax.max() > 0 else np.nan
        return np.full(W, level)
    return np.full(W, float(reference))


def oracle_norms(frames, q_lo, q_hi):
    from oracle import period_oracle as po

    return np.stack([po.ramanujan_norms_folded(f.astype(np.float64), q_lo, q_hi) for f in frames])


def oracle_fit(frame, periods):
    """-> (keys, rows, weights) of the oracle's dictionary fit, or None when its matrix is singular."""
    from oracle import period_oracle as po

    a, dims = po.qo_get_subspaces(periods, frame.size)
    try:
        w, _ = po.qo_solve_quadratic(frame.astype(np.float64), a)
    except np.linalg.LinAlgError:
        return None
    return [int(q) for q in dims], [int(r) for r in dims.values()], w


def oracle_cond(n, periods):
    from oracle import period_oracle as po

    a, _ = po.qo_get_subspaces(periods, n)
    return np.linalg.cond(a @ a.T) if a.shape[0] <= n else np.inf


def oracle_waves(keys, rows, weights):
    return closed_form(keys, rows, weights)


def host_route(x, window, thresh, reference, max_periods, dtype=np.float64, norms_fn=oracle_norms, fit_fn=oracle_fit,
               waves_fn=oracle_waves, tracks=None, max_tracks=8, min_length=2):
    """What a user does without decompose_ramanujan, on the test recording's geometry: numpy frames -> norms ->
    select_ref -> a dictionary fit per frame -> one waveform per period -> np.add.at.  -> dict of the fields of
    ShortTimeRamanujan and `seg`, `cond` (of the oracle's dictionary; 0 for a frame without a list)."""
    from pyperiod_amd import ShortTime

    L = x.shape[0]
    W = ShortTime(R_N, R_HOP).frame_count(L)
    frames = frames_ref(x, R_N, R_HOP, W, window, dtype)
    norms = norms_fn(frames, min_length, R_QHI)
    ref = reference_level(norms, reference)
    lists, counts, over = select_ref_batch(norms, thresh, ref, max_periods)
    status = np.where(counts == 0, 2, 0).astype(np.int8)
    per, cnt = np.zeros((W, max_periods), np.int32), np.zeros(W, np.int32)
    powers, cond, segs = np.zeros((W, max_periods)), np.zeros(W), [np.zeros(0)] * W
    for f in np.flatnonzero(counts):
        lst = lists[f, : counts[f]].astype(np.int64)
        cond[f] = oracle_cond(R_N, lst)
        fit = fit_fn(frames[f], lst)
        if fit is None:
            status[f] = 3
            continue
        keys, rows, weights = fit
        assert keys == lst.tolist()
        segs[f] = np.asarray(waves_fn(keys, rows, weights), dtype=np.float64)
        cnt[f] = len(keys)
        per[f, : cnt[f]] = keys
        ends = np.cumsum(keys)
        powers[f, : cnt[f]] = [np.mean(segs[f][e - p : e] ** 2) for p, e in zip(keys, ends)]
    ccap = max(1, max(s.size for s in segs))
    seg = np.zeros((W, ccap))
    for f in range(W):
        seg[f, : segs[f].size] = segs[f]
    groups = [(p,) for p in ShortTime.rank_periods(per, powers, cnt, max_tracks)] if tracks is None else tracks
    T = len(groups)
    masks = np.zeros((T + 2, W), np.uint64)
    masks[: T + 1] = ShortTime.track_masks(per, cnt, groups)
    masks[T + 1] = (np.uint64(1) << cnt.astype(np.uint64)) - np.uint64(1)
    # the overlap-add: every block tiled to the frame, times the synthesis window, np.add.at in ascending f and a
    ws = np.ones(R_N) if window is None else window
    num, den = np.zeros((T + 2, L)), np.zeros(L)
    for f in range(W):
        idx = f * R_HOP + np.arange(R_N)
        ok = idx < L
        np.add.at(den, idx[ok], (ws * ws)[ok])
        off = 0
        for a in range(cnt[f]):
            p = int(per[f, a])
            term = ws * seg[f, off + np.arange(R_N) % p]
            off += p
            for t in np.flatnonzero((masks[:, f] >> np.uint64(a)) & np.uint64(1)):
                np.add.at(num[t], idx[ok], term[ok])
    routed = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    x64 = x.astype(np.float64)
    periodic = routed[T + 1]
    return dict(norms=norms, periods=per, counts=cnt, over=over, frame_status=status, powers=powers, seg=seg, cond=cond,
                track_periods=groups, tracks=routed[:T], other=routed[T], periodic=periodic, residual=x64 - periodic,
                masks=masks, frames=frames, lists=lists, list_counts=counts)


# ------------------------------------------------------------------ tests: the rule
def _windows():
    rng = np.random.default_rng(77)
    for n in (96, 192, 200):
        noise = rng.standard_normal(n)
        wave = rng.standard_normal(9)
        pattern = np.tile(wave - wave.mean(), n // 9 + 1)[:n] + 0.05 * rng.standard_normal(n)
        impulse = np.zeros(n)
        impulse[n // 2] = 1.0
        for name, x in (("noise", noise), ("pattern", pattern), ("impulse", impulse), ("zero", np.zeros(n))):
            yield f"{name}{n}", x


def test_select_ref_is_the_reference_rule_without_a_cap():
    from oracle import period_oracle as po

    selected = 0
    for name, x in _windows():
        norms = po.ramanujan_norms_folded(x)
        for thresh in (0.2, 0.05, 0.01):
            with np.errstate(all="ignore"):
                want = np.argwhere(norms / np.abs(np.max(norms)) > thresh).flatten()  # the reference's test_function
            for pcap in (want.size, want.size + 3, 64 + want.size):
                per, count, over = select_ref(norms, thresh, None, max(pcap, 1))
                assert count == over == want.size and per[:count].tolist() == want.tolist() and not per[count:].any(), name
            selected += want.size
    assert selected > 100


def test_select_ref_with_a_cap_is_a_stable_sort():
    from oracle import period_oracle as po

    capped = 0
    tables = [planted(q_hi, pcap, wr) + (pcap,) for q_hi in Q_HIS for pcap in PCAPS for wr in (False, True)]
    for name, x in _windows():
        norms = po.ramanujan_norms_folded(x)[None, :]
        tables += [(norms, None, [name], pcap) for pcap in (1, 3, 8)]
        tables += [(norms, np.array([norms.max() or 1.0]) * 2.0, [name], 5)]
    for norms, ref, labels, pcap in tables:
        for w, row in enumerate(norms):
            for thresh in (THRESH, 0.01):
                per, count, over = select_ref(row, thresh, None if ref is None else ref[w], pcap)
                m = np.float64(ref[w]) if ref is not None else np.abs(np.nan if np.isnan(row).any() else row.max())
                with np.errstate(all="ignore"):
                    q = np.flatnonzero(row / m > thresh)
                assert over == q.size and count == min(over, pcap)
                want = np.sort(q[np.lexsort((q, -row[q]))[:pcap]])
                assert per[:count].tolist() == want.tolist() and not per[count:].any(), (labels[w], pcap, thresh)
                assert np.all(np.diff(per[:count]) > 0)
                capped += over > pcap
    assert capped > 200


def test_planted_table_census():
    """Every path of the kernel is in the table the GPU test uses."""
    seen = set()
    for q_hi in Q_HIS:
        for pcap in PCAPS:
            for with_ref in (False, True):
                norms, ref, labels = planted(q_hi, pcap, with_ref)
                assert norms.shape == (len(labels), q_hi + 1)
                per, counts, over = select_ref_batch(norms, THRESH, ref, pcap)
                for w, label in enumerate(labels):
                    row = norms[w]
                    key = (pcap, with_ref)
                    if over[w] < pcap:
                        seen.add(("under", q_hi) + key)
                    if over[w] == pcap:
                        seen.add(("at", q_hi) + key)
                    if over[w] == pcap + 1:
                        seen.add(("one over", q_hi) + key)
                    if over[w] == q_hi + 1:
                        seen.add(("all", q_hi) + key)
                    if over[w] > pcap:
                        kept = per[w, : counts[w]]
                        m = ref[w] if with_ref else row.max()
                        cand = np.flatnonzero(row / m > THRESH)
                        cut = row[kept].min()
                        tied = cand[row[cand] == cut]
                        if tied.size > 1 and not np.isin(tied, kept).all():
                            seen.add(("tie", q_hi) + key)
                            assert np.isin(tied, kept).sum() >= 1
                            assert tied[np.isin(tied, kept)].max() < tied[~np.isin(tied, kept)].min()  # the smaller periods
                    if label == "all equal":
                        assert over[w] == q_hi + 1 and per[w, : counts[w]].tolist() == list(range(min(pcap, q_hi + 1)))
                        seen.add(("equal", q_hi) + key)
                    if label == "one NaN":
                        assert (over[w] == 0) == (not with_ref)
                        assert not np.isin(np.flatnonzero(np.isnan(row)), per[w, : counts[w]]).any() or counts[w] == 0
                        seen.add(("nan", q_hi) + key)
                    if label == "zero row":
                        assert over[w] == 0
                        seen.add(("zero", q_hi) + key)
                    if label == "ref NaN":
                        assert over[w] == 0
                    if label == "+inf":
                        assert (over[w] == 0) == (not with_ref)
                        if with_ref:
                            assert np.isin(np.flatnonzero(np.isinf(row)), per[w, : counts[w]]).all()
                    if label == "-0.0 and negative":
                        assert np.all(row[per[w, : counts[w]]] > 0)
                    if label == "denormals" and with_ref:
                        assert over[w] == q_hi + 1
    for q_hi in Q_HIS:
        for pcap in PCAPS:
            for with_ref in (False, True):
                for path in ("under", "all", "equal", "nan", "zero"):
                    assert (path, q_hi, pcap, with_ref) in seen, (path, q_hi, pcap, with_ref)
                if q_hi + 1 >= pcap:
                    assert ("at", q_hi, pcap, with_ref) in seen, (q_hi, pcap, with_ref)
                if q_hi + 1 > pcap:
                    assert ("one over", q_hi, pcap, with_ref) in seen, (q_hi, pcap, with_ref)
                if q_hi + 1 >= pcap + 3:
                    assert ("tie", q_hi, pcap, with_ref) in seen, (q_hi, pcap, with_ref)


# ------------------------------------------------------------------ tests: the host route on the recording
@pytest.fixture(scope="module")
def routes():
    x = recording()
    out = {}
    for wname, window in (("hann", sqrt_hann(R_N)), ("rect", None)):
        for dtype in (np.float64, np.float32):
            out[wname, np.dtype(dtype).name] = host_route(x, window, 0.2, "recording", 16, dtype)
    return x, out


def test_recording_census(routes):
    """What the GPU test relies on: the frames of every kind are there, at most 1 frame in 4 has a dictionary above
    the condition cut (the oracle alone), and no norm sits so close to its threshold that 1e-10 could move the list."""
    x, out = routes
    for key, r in out.items():
        W = r["counts"].size
        assert W == 15
        st = r["frame_status"]
        print(key, "counts", r["counts"].tolist(), "over", r["over"].tolist(), "status", st.tolist(),
              "cond", [f"{c:.1e}" for c in r["cond"]])
        zero = [f for f in range(W) if not r["frames"][f].any()]
        quiet = [f for f in range(W) if r["frames"][f].any() and np.abs(r["frames"][f]).max() < 0.01]
        assert zero and quiet and np.all(st[zero] == 2) and np.all(st[quiet] == 2)
        assert (st == 0).sum() >= 8
        hard = (r["cond"] > COND_CUT) | (st == 3)
        assert 4 * hard.sum() <= W, (key, r["cond"])
        level = reference_level(r["norms"], "recording")[0]
        margin = np.abs(r["norms"] / level - 0.2)
        assert margin.min() > 1e-6
        # under "frame" the quiet frames select, the zero frames do not
        fr = host_route(x, None if key[0] == "rect" else sqrt_hann(R_N), 0.2, "frame", 16, np.dtype(key[1]))
        assert np.all(fr["list_counts"][quiet] > 0) and np.all(fr["list_counts"][zero] == 0)
        # thresh 0.01, four periods: capped frames, every list at most 4
        cp = host_route(x, None if key[0] == "rect" else sqrt_hann(R_N), 0.01, "recording", 4, np.dtype(key[1]))
        assert (cp["over"] > cp["list_counts"]).sum() >= 3 and cp["list_counts"].max() == 4
        hard = (cp["cond"] > COND_CUT) | (cp["frame_status"] == 3)
        assert 4 * hard.sum() <= W, (key, "capped", cp["cond"])


def test_host_route_restatement(routes):
    x, out = routes
    for key, r in out.items():
        T = len(r["track_periods"])
        assert T >= 2 and (7,) in r["track_periods"] and (12,) in r["track_periods"]
        total = r["tracks"].sum(axis=0) + r["other"]
        assert np.max(np.abs(total - r["periodic"])) <= 1e-12
        # residual is float64(signal) - periodic, to the bit; adding the periodic part back rounds once more (about
        # 50 of the 420 sums differ from the signal by one ulp here), so the round trip is held to that one rounding
        assert np.array_equal(r["residual"], x - r["periodic"])
        back = np.abs(r["periodic"] + r["residual"] - x)
        assert np.all(back <= 2.0**-52 * np.maximum(np.abs(x), np.abs(r["periodic"])))
        # without a window the planted pattern comes back where the frames hear it alone (the first two frames)
        if key[0] == "rect":
            assert np.max(np.abs(r["residual"][: 2 * R_HOP])) <= (1e-9 if key[1] == "float64" else 1e-5)
        # nothing periodic under the zero stretch's own frames
        assert np.all(r["periodic"][R_ZERO[0] + R_N : R_ZERO[1] - R_N] == 0.0)


# ------------------------------------------------------------------ tests: surface and refusals
def test_symbol_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    assert "k_ram_select_ref" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint ph_ramanujan_select\s*\(([^;]*)\);", text)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and len(_ffi.SIGNATURES["ph_ramanujan_select"]) == 11
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for arg, have in zip(args, _ffi.SIGNATURES["ph_ramanujan_select"]):
        want = ctypes.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]]
        assert have is want, arg


def test_entry_point_rejects_bad_arguments_without_gpu():
    """Every refusal comes before the first HIP call and before the context is looked at: a block of zeros stands in
    for the context, and the arrays are never read."""
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    ctx = ctypes.addressof((ctypes.c_char * 4096)())
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    good = dict(ctx=ctx, norms=buf, W=4, q_hi=7, thresh=0.2, ref=buf, pcap=4, flags=0, periods=buf, counts=buf, over=buf)

    def call(**change):
        a = dict(good, **change)
        return lib.ph_ramanujan_select(a["ctx"], a["norms"], a["W"], a["q_hi"], a["thresh"], a["ref"], a["pcap"], a["flags"],
                                       a["periods"], a["counts"], a["over"])

    for dev in (0, _ffi.PH_FLAG_DEVICE):
        assert call(ctx=None, flags=dev) == E and b"ctx" in lib.ph_last_error()
        for name in ("norms", "periods", "counts", "over"):
            assert call(flags=dev, **{name: None}) == E, name
            assert b"NULL" in lib.ph_last_error()
        for v in (0, -1, 1 << 40):
            assert call(flags=dev, W=v) == E and b"W=" in lib.ph_last_error()
        for v in (0, -1, 30030, 0x10000, 2**31 - 1):
            assert call(flags=dev, q_hi=v) == E and b"q_hi" in lib.ph_last_error(), v
        for v in (0, -1, (1 << 20) + 1):
            assert call(flags=dev, pcap=v) == E and b"pcap" in lib.ph_last_error()
        for v in (0.0, -0.5, float("nan")):
            assert call(flags=dev, thresh=v) == E and b"thresh" in lib.ph_last_error()


def test_result_type():
    import pyperiod_amd
    from pyperiod_amd import ShortTimeRamanujan, ShortTimeTracks

    assert ShortTimeRamanujan._fields == ShortTimeTracks._fields + ("norms", "over", "frame_status")
    assert "ShortTimeRamanujan" in pyperiod_amd.__all__


def test_decompose_ramanujan_validates_before_touching_the_gpu(monkeypatch):
    import sys

    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)
    st = ShortTime(96, 24)
    x = np.zeros(300)
    for bad in (0, 0.0, -0.2, float("nan"), None, "0.2", True):
        with pytest.raises(ValueError):
            st.decompose_ramanujan(x, thresh=bad)
    for bad in (0, 65, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            st.decompose_ramanujan(x, max_periods=bad)
    for bad in ("loudest", "", None, 0, 0.0, -1.0, float("inf"), float("nan"), True, [1.0]):
        with pytest.raises(ValueError):
            st.decompose_ramanujan(x, reference=bad)
    for bad in ([], [0], [12, (17, 12)], [()], 12, [1.5], "12"):
        with pytest.raises(ValueError):
            st.decompose_ramanujan(x, tracks=bad)
    with pytest.raises(ValueError):
        st.decompose_ramanujan(x, max_tracks=-1)
    with pytest.raises(ValueError):
        st.decompose_ramanujan(x, max_rows=0)
    with pytest.raises(ValueError):
        st.decompose_ramanujan(x, max_length=0)
    with pytest.raises(ValueError):
        st.decompose_ramanujan(x, min_length=0)
    with pytest.raises(TypeError):  # the analysis window and the basis are not arguments
        st.decompose_ramanujan(x, window=np.ones(96))
    with pytest.raises(TypeError):
        st.decompose_ramanujan(x, basis_type="ramanujan")
    # every argument in order reaches the engine
    with pytest.raises(AssertionError, match="the GPU was touched"):
        st.decompose_ramanujan(x, 0.2, 2, None, "recording", 16, None, 8, 2048)
    with pytest.raises(AssertionError, match="the GPU was touched"):
        st.decompose_ramanujan(x, reference=np.float64(3.5), max_periods=np.int64(64), tracks=[7, (12, 24)])


def test_engine_binding_checks_its_side_arrays():
    import torch

    from test_short_time_cpu import cpu_engine

    eng, Reached = cpu_engine()
    norms = torch.zeros((4, 9), dtype=torch.float64)
    with pytest.raises(Reached):
        eng.ramanujan_select(norms, 0.2)
    with pytest.raises(Reached):
        eng.ramanujan_select(norms, 0.2, torch.ones(4, dtype=torch.float64), 16)
    with pytest.raises(TypeError, match="on the device of"):
        eng.ramanujan_select(norms, 0.2, np.ones(4))
    with pytest.raises(TypeError, match="on the device of"):
        eng.ramanujan_select(norms, 0.2, torch.ones(4, dtype=torch.float32))
    with pytest.raises(ValueError):
        eng.ramanujan_select(norms, 0.2, torch.ones(5, dtype=torch.float64))
    with pytest.raises(TypeError):
        eng.ramanujan_select(norms.to(torch.float32), 0.2)
