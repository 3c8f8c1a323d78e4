"""Child process of tests/test_gpu_duo_edges_mbest.py: m_best(num=4) on a few windows at the window lengths of the
edge-shape test, with whatever PH_* switches the parent set in the environment (they are read when the library is
loaded, hence one process per setting).  Writes every output into one .npz.

  python tests/duo_edges_job.py <out.npz>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = (2246, 2301)
W = 7  # odd: one workgroup has a missing partner
NUM = 4


def configs(n):
    """(name, keyword arguments of m_best): the default range (periods up to N / 3: rows 4 ... 6 among the screened ones)
    and one that reaches three-row periods."""
    return (("default", {}), ("three_rows", dict(min_length=2, max_length=n // 2 - 1)))


def planted(n, hi):
    """Bases of shared-load passes inside the screened range (hi / 2, hi] that meet edge shapes: from the census of
    test_gpu_duo_edges (cut in the last column, cut on a column boundary, no full group in front of the cut, six rows)."""
    from test_gpu_duo_edges import bases, shape

    picks = {}
    for q in bases(n):
        if q <= hi // 2 or q + 64 > hi:
            continue
        s = shape(n, q)
        for name, hit in (("cut_in_last", s["cut_in_last"]), ("boundary", s["cut"] % 64 == 0), ("no_full_group", s["whole"] < s["UA"]),
                          ("six_rows", s["R"] == 6), ("three_rows", s["R"] == 3)):
            if hit and name not in picks:
                picks[name] = q
    return sorted(set(picks.values()))


def windows(n, hi):
    from pyperiod_amd.synth import multi_sinusoid_batch

    rng = np.random.default_rng(n + hi)
    t = np.arange(n)
    x = multi_sinusoid_batch(500 + n, W, n)
    for w, q in zip(range(W - 1, 0, -1), planted(n, hi)):  # the last windows carry a base and its partner, the partner stronger
        x[w] = 2.0 * rng.standard_normal(q)[t % q] + 3.0 * rng.standard_normal(q + 64)[t % (q + 64)] + 0.05 * rng.standard_normal(n)
    return x


def main(out):
    from pyperiod_amd import PeriodEngine

    e = PeriodEngine(0)
    res = {}
    for n in LENGTHS:
        for name, kw in configs(n):
            hi = kw.get("max_length", n // 3)
            x = windows(n, hi)
            r = e.m_best(x, NUM, want_sweeps=True, **kw)
            for key, val in zip(("periods", "powers", "bases", "status", "sweeps"), r):
                res[f"{n}_{name}_{key}"] = val.cpu().numpy() if hasattr(val, "cpu") else np.asarray(val)
            res[f"{n}_{name}_info"] = np.asarray(e.m_best_screen_info(n, NUM, **kw))
            res[f"{n}_{name}_kernel"] = np.asarray(e.m_best_info(n, NUM, **kw))
    e.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
