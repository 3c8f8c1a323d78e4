#!/usr/bin/env python3
"""Generate tests/golden/best_correlation_edges.npz: the *reference* Periods.best_correlation on the windows of
tests/bc_cases.py that name a fixture tag -- one NaN, +Inf or -Inf sample, NaN and Inf together, all NaN, zeros, a
constant, the planted window times 2^510, 2^400, 2^-400 and 2^-530, the impulse and near-tie windows (exact ties and
leads of 2^-51), and max_length at 2, 3, N and N + 5.  Same reference setup and shims as make_golden.py (build container
only; the .npz travels, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bc.py

Per case the file holds the window, the parameters, and either the reference's periods, norms and bases or the name of
the exception it raises.  oracle.period_oracle.best_correlation must agree with every stored case: the same exception,
or the same periods exactly and values within 1e-10 of the row's largest magnitude.  A base is stored as its first
min(p, N) samples (one sample for an all-zero row); the generator checks that tiling them gives the reference's row bit
for bit.  Only data is stored; the archive is written with fixed member timestamps, so a second run reproduces it byte
for byte.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import load_reference  # noqa: E402
from make_golden_bf import save_npz, tile_rows  # noqa: E402

import bc_cases as bc  # noqa: E402
from oracle import period_oracle as po  # noqa: E402

TOL = 1e-10
RAISES = (TypeError, ValueError, OverflowError, ZeroDivisionError, IndexError)


def run(fn):
    try:
        return ("ok",) + tuple(fn())
    except RAISES as e:
        return ("raises", type(e).__name__)


def main():
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    per_mod, _, _ = load_reference()
    Periods = per_mod.Periods
    out, tags = {}, []
    for tag, x, kw in bc.fixture_cases():
        n = len(x)
        got = run(lambda: Periods().best_correlation(x.copy(), **kw))
        mine = run(lambda: po.best_correlation(x.copy(), **kw))
        assert got[0] == mine[0], (tag, got[:2], mine[:2])
        out[f"{tag}_x"] = x
        out[f"{tag}_kw"] = np.array([kw["num"], kw["max_length"], kw["ratio"]], dtype=np.float64)
        if got[0] == "raises":
            assert got[1] == mine[1], (tag, got, mine)
            out[f"{tag}_raises"] = np.array(got[1])
            print(f"{tag}: N={n} {kw} the reference raises {got[1]}")
        else:
            _, per, nr, bs = got
            _, oper, onr, obs = mine
            assert np.array_equal(oper, per), (tag, oper, per)
            assert np.all(np.isfinite(nr)) and np.all(np.isfinite(bs)), tag
            assert np.max(np.abs(onr - nr)) <= TOL * np.max(np.abs(nr), initial=0.0), tag
            assert np.max(np.abs(obs - bs)) <= TOL * np.max(np.abs(bs), initial=0.0), tag
            singles = [bs[i, : max(min(int(per[i]), n), 1)] for i in range(kw["num"])]
            assert np.array_equal(tile_rows(singles, n), bs), tag
            out[f"{tag}_periods"], out[f"{tag}_norms"] = per, nr
            for i, s in enumerate(singles):
                out[f"{tag}_base{i}"] = s
            print(f"{tag}: N={n} {kw} periods {per.tolist()} norms {np.round(nr, 6).tolist()}")
        tags.append(tag)
    out["tags"] = np.array(tags)
    path = os.path.join(HERE, "best_correlation_edges.npz")
    save_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.0f} kB, {len(tags)} cases")


if __name__ == "__main__":
    main()
