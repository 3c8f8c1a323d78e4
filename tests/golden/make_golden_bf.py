#!/usr/bin/env python3
"""Generate tests/golden/best_frequency_edges.npz: the *reference* Periods.best_frequency at the edges of its
spectrum step -- round-half-even of 2 * win_size / k, zero padding and truncation of the rfft, the Nyquist bin, the
trunc / orth flags, a period beyond the window, windows the reference raises on -- and Periods.best_correlation under
the flags, with an explicit max_length and with picks that `ratio` rejects.  Same reference setup and shims as
make_golden.py (build container only; the .npz travels, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bf.py

Every case is also run through oracle.period_oracle, which must agree with the reference.  For best_frequency every
round's pick must be clear of its runner-up on the reference's own spectrum (runner-up / peak <= 1 - 1e-6: no stored
case depends on a tie that rounding could flip) and no round may repeat an earlier period (its base would be rounding
noise).  The worst margin of every case is printed.

Every projection is p-periodic, so a base is stored as its first min(p, N) samples; the generator checks that tiling
them gives the reference's row bit for bit.  Only data (inputs + the reference's outputs) is stored; no reference
source.  The archive is written with fixed member timestamps: a second run reproduces it byte for byte.
"""

import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import load_reference  # noqa: E402

from oracle import period_oracle as po  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

MARGIN = 1e-6  # least relative lead of a spectral peak over its runner-up
TOL = 1e-10
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def tones(seed, n, L, parts, noise=0.05):
    """sum_i a_i cos(2 pi k_i t / L + phase_i) + noise * white: tones at bins k_i of the length-L transform."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = noise * rng.standard_normal(n)
    for k, a in parts:
        x += a * np.cos(2.0 * np.pi * k * t / L + rng.uniform(0.2, 1.2))
    return x


def bf_cases():
    """(tag, window, win_size, num, flag combinations).  The comment of a case names 2 L / k of its main tone.  `num`
    stops before the round that would pick an earlier period again (a tone whose 2 L / k is no integer survives its own
    projection)."""
    flags_x = tones(30, 1200, 1200, [(89, 1.0), (38, 0.6), (160, 0.35)])  # p = 27, 63, 15: all composite, all <= N / 4
    return [
        # round-half-even, up: 187.5 -> 188, 37.5 -> 38
        ("half_up_k16", tones(1, 1500, 1500, [(16, 1.0), (125, 0.4)]), 1500, 3, FLAGS[:1]),
        ("half_up_k80", tones(2, 1500, 1500, [(80, 1.0), (125, 0.4)]), 1500, 1, FLAGS[:1]),
        # round-half-even, down: 62.5 -> 62 (twice)
        ("half_dn_k48", tones(3, 1500, 1500, [(48, 1.0), (125, 0.4)]), 1500, 1, FLAGS[:1]),
        ("half_dn_k32", tones(4, 1000, 1000, [(32, 1.0), (125, 0.4)]), 1000, 3, FLAGS[:1]),
        # zero padding: 12.5 -> 12; a power of two (FFT) and another length (chirp)
        ("pad_k240", tones(5, 1200, 1500, [(240, 1.0)]), 1500, 1, FLAGS[:1]),
        ("pad_fft", tones(6, 700, 1024, [(128, 1.0), (64, 0.5), (32, 0.3)]), 1024, 3, FLAGS[:1]),
        ("pad_chirp", tones(7, 700, 1000, [(125, 1.0), (100, 0.5), (50, 0.3)]), 1000, 2, FLAGS[:1]),
        # truncation (the reference warns): 7.5 -> 8
        ("cut_k400", tones(8, 2000, 1500, [(400, 1.0)]), 1500, 1, FLAGS[:1]),
        ("cut_fft", tones(9, 1500, 1024, [(128, 1.0), (64, 0.5), (32, 0.3)]), 1024, 3, FLAGS[:1]),
        # the Nyquist bin: p = 4
        ("nyquist", tones(10, 1024, 1024, [(512, 1.0), (128, 0.4), (64, 0.25)]), 1024, 3, FLAGS[:1]),
        # one window under every flag combination
        ("flags", flags_x, 1200, 3, FLAGS),
        # p > N: k = 1 -> p = 1800, the base is the window itself
        ("p_gt_n", tones(11, 900, 900, [(1, 1.0)]), 900, 1, FLAGS[:1]),
        # two ordinary windows of the same length as the raising ones (the mixed batch of the GPU test)
        ("live_a", tones(12, 900, 900, [(100, 1.0), (60, 0.5), (36, 0.3)]), 900, 3, FLAGS[:1]),
        ("live_b", tones(13, 900, 900, [(36, 1.0), (100, 0.6), (60, 0.35)]), 900, 3, FLAGS[:1]),
    ]


def raise_cases():
    """Windows on which the reference raises OverflowError in round 0 (2 * win_size / 0)."""
    nan = tones(22, 900, 900, [(100, 1.0)])
    nan[417] = np.nan
    return [
        ("offset", tones(20, 900, 900, [(100, 1.0)]) + 50.0),
        ("zero", np.zeros(900)),
        ("nan", nan),
    ]


def tile_rows(singles, n):
    """Rows of length n from their first periods: how the tests rebuild the stored bases."""
    return np.stack([np.tile(s, n // len(s) + 1)[:n] for s in singles])


def check_bf(tag, x, L, num, per, bases):
    """Margins of every round on the reference's spectrum; -> worst runner-up / peak."""
    work = x.copy()
    worst = 0.0
    for i in range(num):
        mags = np.abs(np.fft.rfft(work, L))
        k = int(np.argmax(mags))
        top = mags[k]
        rest = np.delete(mags, k)
        ratio = float(np.max(rest) / top)
        assert ratio <= 1.0 - MARGIN, (tag, i, ratio)
        assert int(np.round(2 * L / k)) == int(per[i]), (tag, i, k, per[i])
        worst = max(worst, ratio)
        work = work - bases[i]
    assert len(set(int(p) for p in per)) == num, (tag, per)  # no repeated pick
    return worst


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w") as fid:
                np.lib.format.write_array(fid, np.asanyarray(arrays[key]), allow_pickle=False)


def main():
    warnings.simplefilter("ignore")  # win_size < N, 0 / 0 columns of p > N, 2 L / 0
    per_mod, _, _ = load_reference()
    Periods = per_mod.Periods
    out = {}

    # ---------------------------------------------------------------- best_frequency
    tags = []
    for name, x, L, num, flagset in bf_cases():
        out[f"{name}_x"] = x
        n = len(x)
        seen = []
        for trunc, orth in flagset:
            tag = name if len(flagset) == 1 else f"{name}_t{int(trunc)}_o{int(orth)}"
            per, pw, bs = Periods(trunc, orth).best_frequency(x, win_size=L, num=num)
            worst = check_bf(tag, x, L, num, per, bs)
            oper, opw, obs = po.best_frequency(x, L, num, trunc, orth)
            assert np.array_equal(oper, per), (tag, oper, per)
            assert np.max(np.abs(opw - pw)) <= TOL * np.max(np.abs(pw)), tag
            assert np.max(np.abs(obs - bs)) <= TOL * np.max(np.abs(bs)), tag
            singles = [bs[i, : min(int(per[i]), n)] for i in range(num)]
            assert np.array_equal(tile_rows(singles, n), bs), tag
            out[f"{tag}_kw"] = np.array([L, num, trunc, orth], dtype=np.int64)
            out[f"{tag}_periods"], out[f"{tag}_powers"] = per, pw
            for i, s in enumerate(singles):
                out[f"{tag}_base{i}"] = s
            out[f"{tag}_src"] = np.array(name)
            tags.append(tag)
            seen.append(bs)
            print(f"bf {tag}: N={n} L={L} periods {per.tolist()} worst runner-up/peak {worst:.6f}")
        if len(flagset) > 1:  # the flags change the result: plain != trunc, plain != orth, orth removes something
            scale = np.max(np.abs(seen[0]))
            for other in seen[1:]:
                assert np.max(np.abs(other - seen[0])) > 1e-6 * scale, name
    out["bf_tags"] = np.array(tags)

    # the reference runs out of spectrum in round 1 of the k = 1 window: the residual is exactly zero
    try:
        Periods().best_frequency(out["p_gt_n_x"], win_size=900, num=2)
        raised = False
    except OverflowError:
        raised = True
    assert raised
    out["p_gt_n_raises_num2"] = np.array(raised)
    with np.testing.assert_raises(OverflowError):
        po.best_frequency(out["p_gt_n_x"], 900, 2)

    rtags = []
    for name, x in raise_cases():
        for fn in (lambda: Periods().best_frequency(x, win_size=None, num=3), lambda: po.best_frequency(x, None, 3)):
            try:
                fn()
                raised = False
            except OverflowError:
                raised = True
            assert raised, name
        out[f"{name}_x"] = x
        rtags.append(name)
        print(f"bf {name}: the reference raises OverflowError")
    out["bf_raise_tags"] = np.array(rtags)

    # ---------------------------------------------------------------- best_correlation
    ctags = []
    xc = multi_sinusoid_window(8, 600)
    out["bc_flags_x"] = xc
    bc = [(f"bc_flags_t{int(t)}_o{int(o)}", xc, dict(num=4, max_length=150, ratio=0.01), t, o) for t, o in FLAGS[1:]]
    xr = multi_sinusoid_window(9, 600)
    out["bc_ratio_x"] = xr
    bc.append(("bc_ratio", xr, dict(num=5, max_length=150, ratio=0.12), False, False))
    for tag, x, kw, trunc, orth in bc:
        per, nr, bs = Periods(trunc, orth).best_correlation(x, **kw)
        oper, onr, obs = po.best_correlation(x, trunc=trunc, orth=orth, **kw)
        assert np.array_equal(oper, per), (tag, oper, per)
        assert np.max(np.abs(onr - nr)) <= TOL * np.max(np.abs(nr)), tag
        assert np.max(np.abs(obs - bs)) <= TOL * np.max(np.abs(bs)), tag
        n = len(x)
        singles = [bs[i, : max(int(per[i]), 1)] for i in range(kw["num"])]
        assert np.array_equal(tile_rows(singles, n), bs), tag
        if tag == "bc_ratio":
            # a rejected pick leaves its row zero although the residual was reduced (Periods.py:340-347): a later
            # accepted pick exists, and the plain greedy loop without the ratio test would have kept the row
            zero = np.where(per == 0)[0]
            assert zero.size >= 1 and np.any(per[zero[0] + 1:] != 0), (tag, per)
            assert not bs[zero].any() and not nr[zero].any()
            loose = Periods().best_correlation(x, num=kw["num"], max_length=kw["max_length"], ratio=-1.0)
            assert np.all(loose[0] != 0)
        out[f"{tag}_kw"] = np.array([kw["num"], kw["max_length"], kw["ratio"], trunc, orth], dtype=np.float64)
        out[f"{tag}_periods"], out[f"{tag}_norms"] = per, nr
        for i, s in enumerate(singles):
            out[f"{tag}_base{i}"] = s
        ctags.append(tag)
        print(f"bc {tag}: periods {per.tolist()} norms {np.round(nr, 4).tolist()}")
    out["bc_tags"] = np.array(ctags)

    path = os.path.join(HERE, "best_frequency_edges.npz")
    save_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
