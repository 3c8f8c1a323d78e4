"""m_best at the window lengths of the edge-shape test (tests/test_gpu_duo_edges.py), through three step-1 kernels:
the window-pair screen with shared-load passes (default), with one pass per period (PH_PAIR_DUO=0) and the one-window
fp64 kernel (PH_STEP1_PAIR=0).  Period lists, status, sweep counts and bases must be identical across the three and the
powers equal to 1e-13, what tests/test_gpu_duo.py asserts at its shapes.  The switches are read when the library is
loaded, so every setting runs in a fresh child process (tests/duo_edges_job.py); the three run side by side.  Some
windows carry components planted at a base and its partner of passes that meet edge shapes, so that values from those
passes decide."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
from duo_edges_job import LENGTHS, NUM, W, configs, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTOL = 1e-13  # powers, kernel against kernel (test_gpu_duo.py)
SETTINGS = {
    "duo": dict(PH_STEP1_PAIR="1", PH_PAIR_DUO="1"),
    "off": dict(PH_STEP1_PAIR="1", PH_PAIR_DUO="0"),
    "one_window": dict(PH_STEP1_PAIR="0"),
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    import __graft_entry__ as ge

    ge.build()
    tmp = tmp_path_factory.mktemp("duo_edges_mbest")
    procs = {}
    for name, env in SETTINGS.items():
        out = str(tmp / f"{name}.npz")
        procs[name] = (subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "duo_edges_job.py"), out],
                                        env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
    res = {}
    for name, (proc, out) in procs.items():
        try:
            log, _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for p, _ in procs.values():
                p.kill()
            raise
        assert proc.returncode == 0, (name, proc.returncode, log[-3000:])
        res[name] = dict(np.load(out))
    return res


@pytest.mark.gpu
def test_the_three_settings_ran_three_different_plans(results):
    for n in LENGTHS:
        for cfg, kw in configs(n):
            duo, off, one = (results[s][f"{n}_{cfg}_info"] for s in ("duo", "off", "one_window"))
            print(n, cfg, "entries / periods / LDS elements: duo", duo.tolist(), "off", off.tolist(), "kernels",
                  [results[s][f"{n}_{cfg}_kernel"].tolist() for s in SETTINGS])
            assert results["duo"][f"{n}_{cfg}_kernel"][0] == 2 and results["off"][f"{n}_{cfg}_kernel"][0] == 2
            assert results["one_window"][f"{n}_{cfg}_kernel"][0] == 1
            assert duo[1] == off[1] and duo[0] < off[0] and duo[2] < off[2]  # same periods from fewer passes and loads
            hi = kw.get("max_length", n // 3)
            assert len(planted(n, hi)) >= 3, (n, cfg, planted(n, hi))


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cfg", ["default", "three_rows"])
def test_identical_across_the_three_kernels(results, n, cfg):
    a = {k: results["duo"][f"{n}_{cfg}_{k}"] for k in ("periods", "powers", "bases", "status", "sweeps")}
    assert a["periods"].shape == (W, NUM) and (a["status"] == 0).all(), a["status"]
    for other in ("off", "one_window"):
        b = {k: results[other][f"{n}_{cfg}_{k}"] for k in a}
        print(n, cfg, other, "periods", np.array_equal(a["periods"], b["periods"]), "sweeps", np.array_equal(a["sweeps"], b["sweeps"]),
              "bases", np.array_equal(a["bases"], b["bases"]), "powers rel", rel_err(b["powers"], a["powers"]))
        assert np.array_equal(a["periods"], b["periods"]), (other, np.nonzero((a["periods"] != b["periods"]).any(1))[0])
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["sweeps"], b["sweeps"]), other
        assert np.array_equal(a["bases"], b["bases"]), other
        assert rel_err(b["powers"], a["powers"]) < KTOL, other
    hi = n // 3 if cfg == "default" else n // 2 - 1
    for w, q in zip(range(W - 1, 0, -1), planted(n, hi)):  # the planted pair is found, from both outputs of its pass
        assert {q, q + 64} <= set(a["periods"][w].tolist()), (w, q, a["periods"][w])
