#!/usr/bin/env python3
"""Generate tests/golden/qo_orth.npz: QOPeriods.find_periods under orthogonal (Muresan-Parks) selection, driven from the
*reference's* own pieces in the loop its commented-out lines intend (QOPeriods.py:435-448 -- as written the branch
dies, ``best_base`` is never assigned).  Same reference setup as make_golden.py (``load_reference``, ``make_qo``); build
container only: the .npz travels, the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qo_orth.py

Per round: ``get_best_period_orthogonal(res, max_length, normalize=True, return_powers=True)``, argmax with 0 -> 1
(:1227-1232), ``project(res, p, trunc, True)``, ``periodic_norm(base, p)``, ``_update_weights(data, N, periods)`` and,
from the second round on, the default test function ``rms(reconstruction) > rms(data) * thresh`` first; a row the test
stops reports its last fit with one period fewer (:560-594).  Signals are multi_sinusoid_window(seed, N), num = 4.

  group   N     max_length  thresh  trunc   rows
  A       36    12          0.05    False   8
  B       600   100         0.05    False   8
  C       600   100         0.05    True    8
  D       1024  128         0.05    False   8
  E       600   100         0.6     False   8     (mixed fate: some rows run all rounds, some stop after the first fit)

Per row ("<group><w>_*"): seed, periods, norms, dictionary keys and values, weights, residual, the relative gap between
the best and second-best power of every round, cond of the last Gram matrix, the round-0 power vector.  A seed with a gap
below 1e-6, a block without rows or cond > 1e7 is replaced by the next seed.  Only data (inputs + what the reference's
functions returned) is stored; no reference source.
"""

import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, load_reference, make_qo  # noqa: E402

sys.path.insert(0, ROOT)
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402

GROUPS = {  # tag: (N, max_length, thresh, trunc)
    "A": (36, 12, 0.05, False),
    "B": (600, 100, 0.05, False),
    "C": (600, 100, 0.05, True),
    "D": (1024, 128, 0.05, False),
    "E": (600, 100, 0.6, False),
}
NUM, ROWS = 4, 8
GAP = 1e-6
COND_CUT = 1e7


def run(qo, rms, x, max_length, thresh, trunc):
    """-> dict of the row, or a string saying why the seed is not used."""
    n = x.size
    res = x.copy()
    periods, norms, gaps = [], [], []
    fit = None
    pows0 = None
    n_report = None
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
    if n_report is None:
        n_report = len(periods)
    if min(gaps) < GAP:
        return f"smallest gap {min(gaps):.2e}"
    a = np.asarray(fit[0], dtype=np.float64)
    cond = float(np.linalg.cond(a @ a.T))
    if cond > COND_CUT:
        return f"cond {cond:.3g}"
    return dict(periods=np.array(periods[:n_report], dtype=np.int64), norms=np.array(norms[:n_report]),
                dict_keys=np.array([int(q) for q in fit[1].keys()]), dict_vals=np.array([int(v) for v in fit[1].values()]),
                weights=np.asarray(fit[2], dtype=np.float64), residual=np.asarray(res, dtype=np.float64),
                gaps=np.array(gaps), cond=np.float64(cond), pows0=pows0)


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    rms = qo_mod.rms
    out = {}
    for tag, (n, max_length, thresh, trunc) in GROUPS.items():
        qo._trunc_to_integer_multiple = trunc
        seed, w = 0, 0
        while w < ROWS:
            got = run(qo, rms, multi_sinusoid_window(seed, n), max_length, thresh, trunc)
            seed += 1
            if isinstance(got, str):
                print(f"{tag}: seed {seed - 1} skipped, {got}")
                continue
            for k, v in got.items():
                out[f"{tag}{w}_{k}"] = v
            out[f"{tag}{w}_seed"] = np.int64(seed - 1)
            print(f"{tag}{w}: seed {seed - 1} periods {got['periods']} dict {dict(zip(got['dict_keys'], got['dict_vals']))} "
                  f"cond {got['cond']:.3g} min gap {got['gaps'].min():.2e}", flush=True)
            w += 1
        out[f"{tag}_kw"] = np.array([n, NUM, thresh, max_length, int(trunc)], dtype=np.float64)
    # the mixed-fate group holds rows of both kinds
    full = [out[f"E{w}_periods"].size == out[f"E{w}_dict_keys"].size for w in range(ROWS)]
    assert any(full) and not all(full), full
    # trunc changes norms, not periods
    for w in range(ROWS):
        assert out[f"B{w}_seed"] == out[f"C{w}_seed"] and np.array_equal(out[f"B{w}_periods"], out[f"C{w}_periods"])
    assert any(not np.array_equal(out[f"B{w}_norms"], out[f"C{w}_norms"]) for w in range(ROWS))
    path = os.path.join(HERE, "qo_orth.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "qo_orth.npz")
    assert os.path.getsize(path) < largest


if __name__ == "__main__":
    main()
