"""The CPU oracle's best_frequency and best_correlation against the reference at the edges that
tests/golden/best_frequency_edges.npz records (tests/golden/make_golden_bf.py): win_size != N (zero padding and
truncation of the rfft), round-half-even of 2 * win_size / k, the Nyquist bin, the trunc / orth flags, a period
beyond the window, the windows the reference raises on; best_correlation under the flags with an explicit max_length
and with picks that `ratio` rejects.  No GPU: this ties the oracle, which the GPU tests are judged by, to the
reference on these branches.
"""

import warnings

import numpy as np
import pytest

from conftest import rel_err
from oracle import period_oracle as po

TOL = 1e-10
NAME = "best_frequency_edges"


def bf_case(g, tag):
    """-> (window, win_size, num, trunc, orth, periods, powers, bases) of a stored best_frequency case."""
    x = g[str(g[f"{tag}_src"]) + "_x"]
    L, num, trunc, orth = (int(v) for v in g[f"{tag}_kw"])
    bases = tile_rows([g[f"{tag}_base{i}"] for i in range(num)], len(x))
    return x, L, num, bool(trunc), bool(orth), g[f"{tag}_periods"], g[f"{tag}_powers"], bases


def tile_rows(singles, n):
    """Rows of length n from their stored first periods (every projection is p-periodic)."""
    return np.stack([np.tile(s, n // len(s) + 1)[:n] for s in singles])


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def test_fixture_holds_the_cases_the_tests_rely_on(golden):
    g = golden(NAME)
    tags = [str(t) for t in g["bf_tags"]]
    want = {"half_up_k16": 188, "half_up_k80": 38, "half_dn_k48": 62, "half_dn_k32": 62, "pad_k240": 12, "cut_k400": 8,
            "nyquist": 4, "p_gt_n": 1800}
    for tag, p in want.items():
        assert tag in tags and int(g[f"{tag}_periods"][0]) == p, tag
    for tag in ("pad_fft", "pad_chirp", "cut_fft", "live_a", "live_b"):
        assert tag in tags
    for t, o in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert f"flags_t{t}_o{o}" in tags
    assert bool(g["p_gt_n_raises_num2"])
    assert [str(t) for t in g["bf_raise_tags"]] == ["offset", "zero", "nan"]
    assert len(g["bc_tags"]) == 4


def test_oracle_best_frequency_matches_reference_at_the_edges(golden):
    g = golden(NAME)
    for tag in (str(t) for t in g["bf_tags"]):
        x, L, num, trunc, orth, per, pw, bs = bf_case(g, tag)
        got = po.best_frequency(x, L, num, trunc, orth)
        assert np.array_equal(got[0], per), (tag, got[0], per)
        assert rel_err(got[1], pw) < TOL and rel_err(got[2], bs) < TOL, tag
        if L == len(x):  # win_size=None is the window's own length
            again = po.best_frequency(x, None, num, trunc, orth)
            assert np.array_equal(again[0], per) and np.array_equal(again[2], got[2]), tag


def test_oracle_best_frequency_raises_where_the_reference_does(golden):
    g = golden(NAME)
    for tag in (str(t) for t in g["bf_raise_tags"]):
        with pytest.raises(OverflowError):
            po.best_frequency(g[f"{tag}_x"], None, 3)
    # the k = 1 window is its own base at p = 2 N: the residual is exactly zero and round 1 divides by bin 0
    assert bool(g["p_gt_n_raises_num2"])
    with pytest.raises(OverflowError):
        po.best_frequency(g["p_gt_n_x"], 900, 2)


def bc_case(g, tag):
    """-> (window, num, max_length, ratio, trunc, orth, periods, norms, bases) of a stored best_correlation case."""
    num, max_length, ratio, trunc, orth = g[f"{tag}_kw"]
    x = g["bc_ratio_x"] if tag == "bc_ratio" else g["bc_flags_x"]
    bases = tile_rows([g[f"{tag}_base{i}"] for i in range(int(num))], len(x))
    return (x, int(num), int(max_length), float(ratio), bool(trunc), bool(orth), g[f"{tag}_periods"], g[f"{tag}_norms"],
            bases)


def test_oracle_best_correlation_matches_reference_under_flags_and_ratio(golden):
    g = golden(NAME)
    for tag in (str(t) for t in g["bc_tags"]):
        x, num, max_length, ratio, trunc, orth, per, nr, bs = bc_case(g, tag)
        got = po.best_correlation(x, num, max_length, ratio, trunc, orth)
        assert np.array_equal(got[0], per), (tag, got[0], per)
        assert rel_err(got[1], nr) < TOL and rel_err(got[2], bs) < TOL, tag
    per = g["bc_ratio_periods"]
    zero = np.where(per == 0)[0]
    assert zero.size and np.any(per[zero[0] + 1:] != 0)  # a rejected pick with an accepted one after it
