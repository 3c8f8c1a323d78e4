#!/usr/bin/env python3
"""Generate tests/golden/qo_window_keep.npz: the *reference* QOPeriods.find_periods under an analysis window
(``_window`` set) in the two settings that qo_window.npz and qo_orth.npz do not hold -- fixed weights
(update_weights=False: _dont_update_weights hands the window to solve_quadratic, QOPeriods.py:707-709) and orthogonal
(Muresan-Parks) selection with re-solved weights (_update_weights under the window, :640-642).  Same reference setup as
make_golden.py (``load_reference``, ``make_qo``); build container only: the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qo_window_keep.py

Signals are multi_sinusoid_window(seed, N), num = 4, min_length = 2.

K groups: the reference's own find_periods(update_weights=False), through the uint32 -> int64 shim of
make_golden_qo_edges.py.

  group   N     max_length  thresh  window               trunc   rows
  KA      36    12          0.05    np.hanning           False   6
  KB      600   100         0.05    np.hanning           False   6
  KC      600   100         0.05    np.hanning           True    6     (the seeds of KB)
  KD      1024  128         0.05    np.hamming           False   6
  KE      600   100         0.3     np.hanning           False   6     (mixed fate: some rows are stopped by the test)
  KF      600   100         0.05    np.hanning(N) - 0.2  False   6     (negative at the ends)

Per K row ("<group><w>_*"): seed, periods, norms, dictionary keys and values, weights, residual, ``blocks`` = the
(period, keep) of every _dont_update_weights call (the dictionary collapses repeated periods), the relative gap between
the best and second-best gamma norm of every round (taken off periodic_norm as the reference calls it), and ``minden`` =
the smallest |sum of the window over a fitted residue class| / samples of the class.  A seed with a gap below 1e-6 or
minden below 1e-3 is replaced by the next seed.

O groups: the loop of make_golden_qo_orth.run with ``qo._window = win``.

  OB      600   100         0.05    np.hanning           False   6
  OC      600   100         0.05    np.hanning           True    6     (the seeds of OB)
  OE      600   100         first of 0.3, 0.45, 0.6, 0.75 with both fates in 6 rows ("OE_kw")

Per O row: the fields of qo_orth.npz; cond is that of the windowed Gram matrix (A * win) A^T.  A seed with a gap below
1e-6, a block without rows or cond > 1e7 is replaced by the next seed.  Only data (inputs + what the reference's
functions returned) is stored; no reference source.
"""

import contextlib
import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference, make_qo  # noqa: E402

sys.path.insert(0, ROOT)
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

WINDOWS = {"hanning": np.hanning, "hamming": np.hamming, "hanning_m02": lambda n: np.hanning(n) - 0.2}
WINDOW_CODES = {"hanning": 0, "hamming": 1, "hanning_m02": 2}
K_GROUPS = {  # tag: (N, max_length, thresh, window, trunc)
    "KA": (36, 12, 0.05, "hanning", False),
    "KB": (600, 100, 0.05, "hanning", False),
    "KC": (600, 100, 0.05, "hanning", True),
    "KD": (1024, 128, 0.05, "hamming", False),
    "KE": (600, 100, 0.3, "hanning", False),
    "KF": (600, 100, 0.05, "hanning_m02", False),
}
O_GROUPS = {"OB": (600, 100, 0.05, "hanning", False), "OC": (600, 100, 0.05, "hanning", True)}
OE_THRESH = (0.3, 0.45, 0.6, 0.75)
NUM, MIN_LENGTH, ROWS = 4, 2, 6
GAP = 1e-6
MINDEN = 1e-3
COND_CUT = 1e7


def run_keep(qo, x, win, max_length, thresh, trunc):
    """The reference's find_periods(update_weights=False) under `win` -> dict of the row, or why the seed is not used."""
    n = x.size
    qo._window = win
    qo._trunc_to_integer_multiple = trunc
    seen, blocks, dens = [], [], []
    norm, fixed = qo.periodic_norm, qo._dont_update_weights

    def norm_and_keep(*a, **k):
        seen.append(float(norm(*a, **k)))
        return seen[-1]

    def fixed_and_keep(data, nn, nonzero, *a):
        got = fixed(data, nn, np.asarray(nonzero, dtype=np.int64), *a)
        p = int(nonzero[-1])
        keep = int(got[1][str(p)])
        blocks.append((p, keep))
        for j in range(keep if keep else p):
            dens.append(abs(float(np.sum(win[j::p]))) / win[j::p].size)
        return got

    qo.periodic_norm, qo._dont_update_weights = norm_and_keep, fixed_and_keep
    try:
        with contextlib.redirect_stdout(io.StringIO()):  # QOPeriods.py:488,693,700 print unconditionally
            bases, res = qo.find_periods(x, num=NUM, thresh=thresh, min_length=MIN_LENGTH, max_length=max_length,
                                         update_weights=False)
    finally:
        del qo.periodic_norm, qo._dont_update_weights  # (instance attributes: the class's methods show again)
        qo._window = False
    n_cand = max_length - MIN_LENGTH + 1
    assert len(seen) % n_cand == 0
    rounds = np.array(seen).reshape(-1, n_cand)
    top = np.sort(rounds, axis=1)[:, ::-1]
    gaps = (top[:, 0] - top[:, 1]) / top[:, 0]
    if gaps.min() < GAP:
        return f"smallest gap {gaps.min():.2e}"
    if min(dens) < MINDEN:
        return f"smallest |den| / count {min(dens):.2e}"
    dims = bases["basis_dictionary"]
    for name, v in (("norms", bases["norms"]), ("weights", bases["weights"]), ("residual", res)):
        assert np.all(np.isfinite(np.asarray(v, dtype=np.float64))), name
    assert np.asarray(bases["subspaces"]).shape == (sum(k if k else p for p, k in blocks), n)
    return dict(periods=np.asarray(bases["periods"], dtype=np.int64), norms=np.asarray(bases["norms"], dtype=np.float64),
                dict_keys=np.array([int(q) for q in dims.keys()]), dict_vals=np.array([int(v) for v in dims.values()]),
                weights=np.asarray(bases["weights"], dtype=np.float64), residual=np.asarray(res, dtype=np.float64),
                blocks=np.array(blocks, dtype=np.int64).reshape(-1, 2), gaps=gaps, minden=np.float64(min(dens)))


def run_orth(qo, rms, x, win, max_length, thresh, trunc):
    """make_golden_qo_orth.run with the fit under `win` -> dict of the row, or why the seed is not used."""
    n = x.size
    qo._window = win
    qo._trunc_to_integer_multiple = trunc
    res = x.copy()
    periods, norms, gaps = [], [], []
    fit = None
    pows0 = None
    n_report = None
    try:
        for i in range(NUM):
            if i > 0 and not (rms(fit[3]) > rms(x) * thresh):
                n_report = len(periods) - 1
                break
            with contextlib.redirect_stdout(io.StringIO()):
                pows = np.asarray(qo.get_best_period_orthogonal(res, max_length, normalize=True, return_powers=True), dtype=np.float64)
            if i == 0:
                pows0 = pows.copy()
            p = int(np.argmax(pows))
            p = p if p > 0 else 1
            top = np.sort(pows)[::-1]
            gaps.append((top[0] - top[1]) / top[0] if top[0] > 0 else 0.0)
            base = qo.project(res, p, trunc, True)
            norms.append(float(qo.periodic_norm(base, p)))
            periods.append(p)
            with contextlib.redirect_stdout(io.StringIO()):
                fit = qo._update_weights(x, n, np.array(periods))
            if any(int(v) == 0 for v in fit[1].values()):
                return "a block without rows"
            res = x - fit[3]
    finally:
        qo._window = False
    if n_report is None:
        n_report = len(periods)
    if min(gaps) < GAP:
        return f"smallest gap {min(gaps):.2e}"
    a = np.asarray(fit[0], dtype=np.float64)
    cond = float(np.linalg.cond((a * win) @ a.T))
    if cond > COND_CUT:
        return f"cond {cond:.3g}"
    return dict(periods=np.array(periods[:n_report], dtype=np.int64), norms=np.array(norms[:n_report]),
                dict_keys=np.array([int(q) for q in fit[1].keys()]), dict_vals=np.array([int(v) for v in fit[1].values()]),
                weights=np.asarray(fit[2], dtype=np.float64), residual=np.asarray(res, dtype=np.float64),
                gaps=np.array(gaps), cond=np.float64(cond), pows0=pows0)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def collect(out, tags, runner, describe):
    """ROWS rows per tag from the same seeds: a seed is used when `runner(tag, x)` returns a row for every tag."""
    seed, w = 0, 0
    while w < ROWS:
        got = {tag: runner(tag, seed) for tag in tags}
        seed += 1
        bad = [f"{tag}: {g}" for tag, g in got.items() if isinstance(g, str)]
        if bad:
            print(f"{'/'.join(tags)}: seed {seed - 1} skipped, {'; '.join(bad)}")
            continue
        for tag, g in got.items():
            for k, v in g.items():
                out[f"{tag}{w}_{k}"] = v
            out[f"{tag}{w}_seed"] = np.int64(seed - 1)
            print(f"{tag}{w}: seed {seed - 1} {describe(g)}", flush=True)
        w += 1


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    rms = qo_mod.rms
    out = {}

    def k_runner(tag, seed):
        n, max_length, thresh, wname, trunc = K_GROUPS[tag]
        return run_keep(qo, multi_sinusoid_window(seed, n), WINDOWS[wname](n), max_length, thresh, trunc)

    def k_describe(g):
        return f"periods {g['periods']} blocks {g['blocks'].tolist()} min gap {g['gaps'].min():.2e} minden {g['minden']:.3g}"

    for tags in (("KA",), ("KB", "KC"), ("KD",), ("KE",), ("KF",)):
        collect(out, tags, k_runner, k_describe)
    for tag, (n, max_length, thresh, wname, trunc) in K_GROUPS.items():
        out[f"{tag}_kw"] = np.array([n, NUM, thresh, MIN_LENGTH, max_length, int(trunc), WINDOW_CODES[wname]], dtype=np.float64)
    # the mixed-fate group holds rows of both kinds; some stored row meets the keep == 0 quirk
    stopped = [out[f"KE{w}_periods"].size < out[f"KE{w}_blocks"].shape[0] for w in range(ROWS)]
    assert any(stopped) and not all(stopped), stopped
    assert any((out[f"{tag}{w}_blocks"][:, 1] == 0).any() for tag in K_GROUPS for w in range(ROWS))

    def o_runner(groups):
        def runner(tag, seed):
            n, max_length, thresh, wname, trunc = groups[tag]
            return run_orth(qo, rms, multi_sinusoid_window(seed, n), WINDOWS[wname](n), max_length, thresh, trunc)
        return runner

    def o_describe(g):
        return (f"periods {g['periods']} dict {dict(zip(g['dict_keys'].tolist(), g['dict_vals'].tolist()))} cond {g['cond']:.3g} "
                f"min gap {g['gaps'].min():.2e}")

    collect(out, ("OB", "OC"), o_runner(O_GROUPS), o_describe)
    for thresh in OE_THRESH:
        trial = {}
        collect(trial, ("OE",), o_runner({"OE": (600, 100, thresh, "hanning", False)}), o_describe)
        full = [trial[f"OE{w}_periods"].size == trial[f"OE{w}_dict_keys"].size for w in range(ROWS)]
        if any(full) and not all(full):
            out.update(trial)
            O_GROUPS["OE"] = (600, 100, thresh, "hanning", False)
            break
    assert "OE" in O_GROUPS
    for tag, (n, max_length, thresh, wname, trunc) in O_GROUPS.items():
        out[f"{tag}_kw"] = np.array([n, NUM, thresh, max_length, int(trunc), WINDOW_CODES[wname]], dtype=np.float64)
    path = os.path.join(HERE, "qo_window_keep.npz")
    save_npz(path, out)
    print(os.path.getsize(path), "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "qo_window_keep.npz")
    assert os.path.getsize(path) < largest


if __name__ == "__main__":
    main()
