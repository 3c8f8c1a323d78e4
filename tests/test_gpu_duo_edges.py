"""Every edge shape of the shared-load pass (pair_pass_duo in pyperiod_amd/csrc/ph_pair.h), value by value, at small N.

The pass folds q and q + 64 from one set of LDS reads.  Away from its main groups it has: the column that holds the cut
of the period and the last column of q, whose lanes are classified under lane masks from the scalar unit; remainder
groups of one to three columns on either side of the cut; the first R - 1 columns, where no sum of q + 64 is complete
(peeled at fixed positions when a full group exists, a wave-uniform 0 / 1 factor otherwise); and the tail columns, whose
last row lies inside the window or behind it.  `shape()` derives, from the rule of the host plan (build_plan in
period_hip.hip) and the geometry of the pass, which of these a base q meets; the test asserts that every listed case
occurs at the window lengths below, then runs the pass test bed (tools/micro/pair_pass_bench.hip, mode 3: the pass
compiled as it is) over every legal base and compares both values of each pass and window with the fp64 fold of the same
float samples: |screen - exact| <= pair_radius(rows, period) x sum of squares, the bound k_mbest_step1_pair prunes with
and tests/test_gpu_duo_screen.py uses at N = 4096.

Window lengths: a pair with six rows needs q > 384 and ceil(N / (q + 64)) = 6, i.e. N > 5 (385 + 64) = 2245; N = 2246
is the smallest length at which R = 3 ... 6 all have legal pairs (asserted below), 2301 is an odd one next to it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (2246, 2301)


def rows(n, p):
    return -(-n // p)


def legal(n, q):
    """The pairing rule of build_plan for a base q (its partner is q + 64)."""
    r = rows(n, q)
    return q >= 64 and q + 64 < n and 3 <= r <= 6 and -(-q // 64) > r and rows(n, q + 64) == r


def shape(n, q):
    """The path of base q through pair_duo_rows, as a dict of the quantities the cases below are stated in."""
    r = rows(n, q)
    ua = 4 if r <= 4 else 2
    ub = 4 if r <= 4 else 3 if r == 5 else 2
    cut = q - (r * q - n)  # nfull: residues below it own r samples
    assert 1 <= cut <= q
    ncb = -(-q // 64)
    last = ncb - 1
    whole = min(cut >> 6, last)
    front_groups, front_rem = divmod(whole, ua)
    cut_column = whole < last and 64 * whole < cut
    c = whole + (1 if cut_column else 0)
    behind_rem = (last - c) % ub
    tail_rows = sum(1 for t in range(r - 1) if 64 * (ncb + t) + (r - 2) * q < n)  # tail columns whose last row is inside the window
    return dict(R=r, UA=ua, UB=ub, cut=cut, last=last, whole=whole, front_groups=front_groups, front_rem=front_rem,
                cut_column=cut_column, cut_in_last=64 * last < cut, behind_from=c, behind_rem=behind_rem, tail_rows=tail_rows)


CASES = {
    "three rows": lambda s: s["R"] == 3,
    "four rows": lambda s: s["R"] == 4,
    "five rows": lambda s: s["R"] == 5,
    "six rows": lambda s: s["R"] == 6,
    "cut on a column boundary (first lane behind it is lane 0)": lambda s: s["cut"] % 64 == 0,
    "cut column with lane 0 alone in front of the cut": lambda s: s["cut_column"] and s["cut"] % 64 == 1,
    "cut column with lane 63 alone behind the cut": lambda s: s["cut_column"] and s["cut"] % 64 == 63,
    "cut in the last column of q": lambda s: s["cut_in_last"],
    "cut at q (no short residue)": lambda s: s["cut_in_last"] and s["cut"] == s["q"],
    "cut in the first column the rule allows (column R - 1)": lambda s: s["cut_column"] and s["cut"] >> 6 == s["R"] - 1,
    "no cut column": lambda s: not s["cut_column"],
    "no cut column, cut in front of the last column": lambda s: not s["cut_column"] and not s["cut_in_last"],
    "front remainder 0": lambda s: s["front_rem"] == 0 and s["front_groups"] > 0,
    "front remainder 1": lambda s: s["front_rem"] == 1,
    "front remainder 2": lambda s: s["front_rem"] == 2,
    "front remainder 3": lambda s: s["front_rem"] == 3,
    "front remainder behind a full group": lambda s: s["front_rem"] > 0 and s["front_groups"] > 0,
    "front remainder of five or six rows behind the peeled groups": lambda s: s["R"] >= 5 and s["front_rem"] == 1 and s["whole"] > s["R"] - 1,
    "front remainder of five or six rows in front of column R - 1": lambda s: s["R"] >= 5 and s["front_rem"] == 1 and 0 < s["front_groups"] and s["whole"] - 1 < s["R"] - 1,
    "no full group in front of the cut (whole < UA)": lambda s: s["whole"] < s["UA"],
    "no full group, remainder 3": lambda s: s["whole"] == 3 and s["UA"] == 4,
    "no full group, remainder 2": lambda s: s["whole"] == 2 and s["UA"] == 4,
    "behind remainder 0": lambda s: s["behind_rem"] == 0,
    "behind remainder 1": lambda s: s["behind_rem"] == 1,
    "behind remainder 2": lambda s: s["behind_rem"] == 2,
    "behind remainder 3": lambda s: s["behind_rem"] == 3,
    "behind remainder 2 at five rows": lambda s: s["R"] == 5 and s["behind_rem"] == 2,
    "nothing behind the cut but the last column": lambda s: s["behind_from"] == s["last"],
    "tail: last row present in every column": lambda s: s["tail_rows"] == s["R"] - 1,
    "q a multiple of 64 (every lane of the last column is a residue of q)": lambda s: s["q"] % 64 == 0,
    "last column with one residue of q": lambda s: s["q"] % 64 == 1,
}

# Shapes that the pairing rule excludes.  The partner q + 64 has R rows as well, so (R - 1) (q + 64) < N and
#   cut = nfull(q) = N - (R - 1) q > 64 (R - 1):
# the cut never lies in the first R - 1 columns (in particular not in the first one, and at least R - 1 whole columns
# stand in front of it), nothing behind the cut lies in front of column R - 1, and row R - 2 of tail column t, whose
# first index is 64 (ncb + t) + (R - 2) q, lies inside the window for every t <= R - 2, because
#   64 ncb - q + 64 t <= 63 + 64 (R - 2) < 64 (R - 1) < cut = N - (R - 1) q.
# They are listed so that the census states it instead of passing over them: none may occur at any length tried.
EXCLUDED = {
    "cut in the first column": lambda s: s["cut"] < 64,
    "cut in front of column R - 1": lambda s: s["cut"] <= 64 * (s["R"] - 1),
    "fewer than R - 1 whole columns in front of the cut": lambda s: s["whole"] < s["R"] - 1,
    "behind the cut starts in front of column R - 1": lambda s: s["behind_from"] < s["R"] - 1,
    "tail: last row absent in some column": lambda s: s["tail_rows"] < s["R"] - 1,
}


def bases(n):
    return [q for q in range(64, n - 64) if legal(n, q)]


def census():
    seen = {name: [] for name in CASES}
    for n in LENGTHS:
        for q in bases(n):
            s = shape(n, q)
            s["q"] = q
            for name, hit in CASES.items():
                if hit(s):
                    seen[name].append((n, q))
    return seen


def test_the_smallest_length_with_all_row_classes():
    def classes(n):
        return {rows(n, q) for q in bases(n)}

    assert classes(LENGTHS[0]) == {3, 4, 5, 6}
    assert all(6 not in classes(n) for n in range(1024, LENGTHS[0]))
    assert LENGTHS[1] % 2 == 1 and classes(LENGTHS[1]) == {3, 4, 5, 6}


def test_every_edge_case_occurs():
    seen = census()
    for name, where in seen.items():
        print(f"{name}: {len(where)} passes, e.g. {where[:3]}")
    missing = [name for name, where in seen.items() if not where]
    assert not missing, missing


def test_shapes_the_pairing_rule_excludes():
    for n in LENGTHS + (1024, 2048, 2049, 4095, 4096, 4097):
        for q in bases(n):
            s = shape(n, q)
            s["q"] = q
            hit = [name for name, test in EXCLUDED.items() if test(s)]
            assert not hit, (n, q, hit)


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the pass test bed is compiled with hipcc"
    tmp = tmp_path_factory.mktemp("duo_edges")
    exe = str(tmp / "pair_pass_bench")
    subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I", os.path.join(ROOT, "pyperiod_amd", "csrc"),
         os.path.join(ROOT, "tools", "micro", "pair_pass_bench.hip"), "-o", exe],
        check=True, timeout=600, cwd=str(tmp))
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_both_values_of_every_edge_pass_stay_inside_the_radius(bench, n):
    qs = bases(n)
    assert qs and {rows(n, q) for q in qs} == {3, 4, 5, 6}
    lo, hi = qs[0], qs[-1] + 1
    out = subprocess.run([bench, "3", str(lo), str(hi), str(n)], check=True, timeout=300, capture_output=True, text=True).stdout
    print(out)
    m = re.search(r"(\d+) screen values against the fp64 fold: largest \|error\| / \(pair_radius x sum of squares\) = ([0-9.eE+-]+)", out)
    assert m, out
    assert int(m.group(1)) == 2 * 2 * len(qs)  # two windows, two periods per pass: the test bed folds exactly the legal bases
    assert f"N = {n}: every value inside its radius: yes" in out, out
    assert float(m.group(2)) <= 1.0, out
