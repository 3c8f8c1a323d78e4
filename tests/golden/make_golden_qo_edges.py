#!/usr/bin/env python3
"""Generate tests/golden/qoperiods_edges.npz: the *reference* QOPeriods.find_periods (plain branch) at the edges of
the device loops -- the fixed-weight quirks, dictionaries of 16, 17, 40 and 70 blocks, short windows and float32
input.  Same reference setup and shims as make_golden.py (build container only; the .npz travels, the reference
does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qo_edges.py

Every case is also run through oracle.period_oracle.qo_find_periods, which must agree with the reference, pick
its periods by a clear margin at every iteration (no near-tie that rounding could flip) and stay finite.
One shim on top of make_golden.py's: the reference's find_periods hands _dont_update_weights its uint32 period
array (QOPeriods.py:383,484), and Pp_column's ``(i - s) % p`` (:1001) overflows on it under numpy 2.  The harness
binds an instance-level _dont_update_weights that calls the reference's own method with the same periods as int64;
the arithmetic is the reference's.

Only data (inputs + the reference's outputs) is stored; no reference source.
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

sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import period_oracle as po  # noqa: E402
from pyperiod_amd._factors import phi  # noqa: E402
from pyperiod_amd.QOPeriods import ramanujan_sum  # noqa: E402
from pyperiod_amd.synth import multi_sinusoid_window  # noqa: E402
from test_qo_batch_cpu import keep_quirk_rows  # noqa: E402

# least relative gap between the best and second-best gamma norm (float32: the reference selects on float32 sums)
MARGIN = {np.float64: 1e-9, np.float32: 1e-5}


def white(seed, n):
    return np.random.default_rng(seed).standard_normal(n)


def ladder(seed, n, r=0.97, sigma=0.01):
    """One exact-period component (a Ramanujan sum) for every period 2..80, weighted so that the greedy loop takes
    them roughly in ascending order: 70 selections that each add rows, where white noise runs out of new rows after
    about 47 blocks of periods <= 80 and then selects at rounding level."""
    t = np.arange(n)
    x = sigma * white(seed, n)
    for q in range(2, 81):
        c = ramanujan_sum(q).astype(np.float64)
        x += r**q * np.sqrt(q / phi(q)) * c[t % q] / np.sqrt(phi(q))
    return x


def blocks_kw(num):
    return dict(num=num, thresh=0.0, min_length=2, max_length=80)


# (tag, input, find_periods keywords, trunc, update_weights)
def cases():
    qa, qb = keep_quirk_rows(900)
    out = []
    for trunc in (False, True):
        t = "t" if trunc else "p"
        out += [
            (f"keep_a_{t}", qa, dict(num=4, thresh=1e-3, min_length=2, max_length=300), trunc, False),
            (f"keep_b_{t}", qb, dict(num=5, thresh=0.1, min_length=2, max_length=300), trunc, False),
            (f"keep_m1537_{t}", multi_sinusoid_window(5, 1537), dict(num=6, thresh=0.02, min_length=2, max_length=200),
             trunc, False),
            (f"keep_m1000_{t}", multi_sinusoid_window(9, 1000), dict(num=5, thresh=0.05, min_length=2, max_length=120),
             trunc, False),
            # trunc selects other periods than plain here (a repeat of 17; 82, 73, 86 instead of 83, 74, 67)
            (f"keep_d301_{t}", multi_sinusoid_window(41, 301), dict(num=5, thresh=0.05, min_length=2, max_length=150),
             trunc, False),
            (f"keep_d777_{t}", multi_sinusoid_window(45, 777), dict(num=5, thresh=0.05, min_length=2, max_length=388),
             trunc, False),
        ]
    x = white(16, 4000)
    out += [
        ("blocks16", x, blocks_kw(16), False, True),
        ("blocks17", x, blocks_kw(17), False, True),
        ("blocks40", x, blocks_kw(40), False, True),
        ("blocks40_t", x, blocks_kw(40), True, True),
        ("blocks70", ladder(70, 4000), blocks_kw(70), False, True),
        ("blocks70_k", x, blocks_kw(70), False, False),
    ]
    for n, seed in ((24, 31), (65, 32), (127, 33)):
        s = multi_sinusoid_window(seed, n) if n > 24 else np.sin(2 * np.pi * np.arange(24) / 5.0) + 0.3 * white(seed, 24)
        hi = (3 * n) // 4
        out += [
            (f"small{n}", s, dict(num=3, thresh=0.05, min_length=2, max_length=None), False, True),
            (f"small{n}_t", s, dict(num=3, thresh=0.05, min_length=2, max_length=hi), True, True),
            (f"small{n}_kt", s, dict(num=4, thresh=0.05, min_length=2, max_length=hi), True, False),
        ]
    f = multi_sinusoid_window(21, 2048, dtype=np.float32)
    kw = dict(num=5, thresh=0.05, min_length=2, max_length=300)
    out += [
        ("f32_k", f, kw, False, False),
        ("f32_kt", f, kw, True, False),
        ("f32_t", f, kw, True, True),
    ]
    return out


def main():
    warnings.simplefilter("ignore")
    per_mod, ram_mod, qo_mod = load_reference()
    qo = make_qo(qo_mod.QOPeriods, per_mod.Periods)
    fixed = qo._dont_update_weights
    qo._dont_update_weights = lambda data, n, nonzero, *a: fixed(data, n, np.asarray(nonzero, dtype=np.int64), *a)
    out = {}
    tags = []
    for tag, sig, kw, trunc, uw in cases():
        qo._trunc_to_integer_multiple = trunc
        with contextlib.redirect_stdout(io.StringIO()):  # QOPeriods.py:488,688,703 print unconditionally
            res_out, res = qo.find_periods(sig, update_weights=uw, **kw)
        periods = np.asarray(res_out["periods"])
        keys = np.array([int(k) for k in res_out["basis_dictionary"].keys()])
        vals = np.array([int(v) for v in res_out["basis_dictionary"].values()])
        for name, v in (("norms", res_out["norms"]), ("weights", res_out["weights"]), ("residual", res)):
            assert np.all(np.isfinite(np.asarray(v, dtype=np.float64))), (tag, name)
        # the oracle agrees, and every selection is clear of its runner-up
        trace = []
        o, ores = po.qo_find_periods(sig.astype(np.float64), trunc=trunc, update_weights=uw, trace=trace, **kw)
        assert np.array_equal(o["periods"], periods), (tag, o["periods"], periods)
        assert [int(k) for k in o["basis_dictionary"]] == list(keys) and list(o["basis_dictionary"].values()) == list(vals), tag
        tol = 1e-8 if sig.dtype == np.float64 else 1e-4
        scale = np.max(np.abs(res_out["weights"]))
        assert np.max(np.abs(o["weights"] - res_out["weights"])) <= tol * scale, tag
        assert np.max(np.abs(ores - res)) <= tol * np.max(np.abs(res)), tag
        for best, second, p in trace:
            assert best - second >= MARGIN[sig.dtype.type] * best, (tag, p, best, second)
            assert best >= 1e-6 * trace[0][0], (tag, p, best)  # a selection above rounding level
        # a re-solved dictionary never takes a period again or a divisor of an earlier one: that block would keep 0
        # rows, Pp would hand it all p rows and the Gram matrix would be singular (whether solve raises is rounding)
        picked = [p for _, _, p in trace]
        assert not uw or all(all(q % p for q in picked[:i]) for i, p in enumerate(picked)), (tag, picked)
        out[f"{tag}_x"] = sig
        ml = -1 if kw["max_length"] is None else kw["max_length"]
        out[f"{tag}_kw"] = np.array([kw["num"], kw["thresh"], kw["min_length"], ml, trunc, uw], dtype=np.float64)
        out[f"{tag}_periods"] = periods
        out[f"{tag}_norms"] = np.asarray(res_out["norms"], dtype=np.float64)
        out[f"{tag}_weights"] = np.asarray(res_out["weights"], dtype=np.float64)
        out[f"{tag}_dict_keys"] = keys
        out[f"{tag}_dict_vals"] = vals
        out[f"{tag}_residual"] = np.asarray(res)
        out[f"{tag}_rows"] = np.array(res_out["subspaces"].shape[0])
        tags.append(tag)
        print(tag, len(periods), "periods", int(out[f"{tag}_rows"]), "rows", periods[:8], vals[:8])
    out["tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "qoperiods_edges.npz"), **out)


if __name__ == "__main__":
    main()
