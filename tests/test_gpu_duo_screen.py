"""The shared-load pass of the window-pair screen against its rigorous radius, value by value.

The pass test bed (tools/micro/pair_pass_bench.hip, mode 3: pair_pass_duo of pyperiod_amd/csrc/ph_pair.h compiled as it
is) folds one window pair at N = 4096 for every base q in [683, 1302) whose partner q + 64 has the same row count -- the
row classes 6, 5 and 4 of the m_best screen, every position of the cut -- and compares BOTH values of each pass, period
q and period q + 64, with the fp64 fold of the same float samples: |screen - exact| must stay below
pair_radius(rows, period) x sum of squares, the bound k_mbest_step1_pair prunes with."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LO, HI = 4096, 683, 1302


def _rows(p):
    return -(-N // p)


@pytest.mark.gpu
def test_both_values_of_every_shared_pass_stay_inside_the_radius(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "pair_pass_bench")
    subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I", os.path.join(ROOT, "pyperiod_amd", "csrc"),
         os.path.join(ROOT, "tools", "micro", "pair_pass_bench.hip"), "-o", exe],
        check=True, timeout=600, cwd=str(tmp_path))
    # the pairing rule: same row count, 3 ... 6 rows, more chunk columns than rows
    bases = [q for q in range(LO, HI) if 3 <= _rows(q) <= 6 and _rows(q + 64) == _rows(q) and -(-q // 64) > _rows(q)]
    assert len(bases) == 491 and {_rows(q) for q in bases} == {4, 5, 6}
    out = subprocess.run([exe, "3", str(LO), str(HI)], check=True, timeout=300, capture_output=True, text=True).stdout
    print(out)
    m = re.search(r"(\d+) screen values against the fp64 fold: largest \|error\| / \(pair_radius x sum of squares\) = ([0-9.eE+-]+)", out)
    assert m, out
    assert int(m.group(1)) == 2 * 2 * len(bases)  # two windows, two periods per pass
    assert float(m.group(2)) < 1.0, out
    assert re.search(r"shared-load pass \(q, q \+ 64\): .* ns per pass per CU", out), out
