"""bench.py's command line: the N > 1 line must never describe a one-GPU job."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_mismatch_with_world_size_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout)
    assert '"n_gpus"' not in r.stdout  # no bench line was printed


def test_launcher_relays_failure_of_its_ranks():
    """Without WORLD_SIZE, --gpus 2 starts two ranks itself; here they cannot run (no GPU in the CPU container, or
    an unknown backend), and the parent must come back non-zero instead of printing a 1-GPU line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--backend", "no-such-backend", "--no-cpu-baseline", "--no-c4"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert '"n_gpus": 1' not in r.stdout


def test_csrc_hash_guards_recorded_traffic():
    sys.path.insert(0, ROOT)
    import bench

    h = bench.csrc_hash()
    assert len(h) == 16 and h == bench.csrc_hash()
    val, why, ms = bench.load_recorded_traffic("no_such_kernel")
    assert val is None and ms is None


def test_steps_below_one_exits_nonzero():
    """The argument check ends the run at once (SystemExit with its message, nothing built, no line printed)."""
    for steps, warmup in (("0", "0"), ("1", "-1")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", steps, "--warmup", warmup],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "--steps must be >= 1 and --warmup >= 0" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
        assert r.stdout == ""


def test_dump_outputs_float64_fixed_sample(tmp_path):
    """--dump-outputs on arrays of m_best's shapes and dtypes (torch: uint32 periods as int32, int32 status / sweeps;
    and the same as numpy): every array as float64 .npy, the bases of the same seeded windows on every run, the files
    under the 64 MB cap."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    W, num, n = bench.WINDOWS_PER_GPU, bench.NUM_PERIODS, bench.N_SAMPLES
    g = torch.Generator().manual_seed(7)
    periods = torch.randint(2, n // 3 + 1, (W, num), dtype=torch.int32, generator=g)
    powers = torch.rand(W, num, dtype=torch.float64, generator=g)
    bases = torch.arange(W, dtype=torch.float64).view(W, 1, 1).expand(W, num, n)  # bases[w] == w, no 335 MB copy
    status = torch.zeros(W, dtype=torch.int32)
    sweeps = torch.randint(1, 20, (W,), dtype=torch.int32, generator=g)
    step = (periods, powers, bases, status, sweeps)
    totals = [bench.dump_outputs(str(tmp_path / "a"), *step), bench.dump_outputs(str(tmp_path / "b"), *step),
              bench.dump_outputs(str(tmp_path / "np"), *(t.numpy() for t in step))]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bases_sample.npy", "bases_sample_windows.npy", "n_sweeps.npy", "periods.npy", "powers.npy", "status.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert all(a.dtype == np.float64 for a in got.values())
    for d in ("b", "np"):
        for f in names:
            assert np.array_equal(got[f[:-4]], np.load(tmp_path / d / f)), (d, f)
    rows = got["bases_sample_windows"]
    assert rows.size == bench.DUMP_BASES_WINDOWS and len(set(rows.tolist())) == rows.size and rows.max() < W
    assert got["bases_sample"].shape == (rows.size, num, n)
    assert np.array_equal(got["bases_sample"], np.broadcast_to(rows.reshape(-1, 1, 1), (rows.size, num, n)))
    for k, t in zip(("periods", "powers", "status", "n_sweeps"), (periods, powers, status, sweeps)):
        assert got[k].shape == tuple(t.shape) and np.array_equal(got[k], t.numpy()), k
    on_disk = sum(os.path.getsize(tmp_path / "a" / f) for f in names)
    assert totals[0] == totals[1] == totals[2] == sum(a.nbytes for a in got.values())
    assert on_disk <= bench.DUMP_MAX_BYTES


def test_bench_uses_library_of_a_tree_it_cannot_write(tmp_path):
    """A build() that cannot take its lock file (a tree another user built) leaves bench with the library built there
    when it is up to date; a stale or missing library is still an error."""
    import time
    import types

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import bench

    ge.build()

    def build():
        raise PermissionError(13, "Permission denied")

    bench.build_library(types.SimpleNamespace(build=build, LIB=ge.LIB, DEPS=ge.DEPS))
    lib, src = tmp_path / "libperiod_hip.so", tmp_path / "period_hip.hip"
    with pytest.raises(PermissionError):
        bench.build_library(types.SimpleNamespace(build=build, LIB=str(lib), DEPS=ge.DEPS))
    lib.write_bytes(b"")
    src.write_text("")
    now = time.time()
    os.utime(lib, (now - 100, now - 100))
    os.utime(src, (now, now))
    with pytest.raises(PermissionError):
        bench.build_library(types.SimpleNamespace(build=build, LIB=str(lib), DEPS=[str(src)]))


@pytest.mark.gpu
def test_dump_is_what_the_timed_step_returns(tmp_path, monkeypatch, capsys):
    """bench.main() with --dump-outputs (in this process: nothing is spawned after HIP is up): the line reports the
    steps asked for, and the dump equals m_best on the same seeded windows, array for array, under the cap."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from pyperiod_amd import PeriodEngine
    from pyperiod_amd.synth import multi_sinusoid_batch

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-c3", "--no-c4",
                                      "--no-c5", "--dump-outputs", str(out)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and all(line["checks"].values()), line["checks"]
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= bench.DUMP_MAX_BYTES

    eng = PeriodEngine(0)
    x = torch.from_numpy(multi_sinusoid_batch(0, bench.WINDOWS_PER_GPU, bench.N_SAMPLES)).to(torch.device("cuda", eng.device))
    periods, powers, bases, status, sweeps = eng.m_best(x, bench.NUM_PERIODS, None, 2, False, want_sweeps=True)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    rows = got["bases_sample_windows"].astype(np.int64)
    want = {"periods": periods, "powers": powers, "status": status, "n_sweeps": sweeps, "bases_sample": bases[rows.tolist()]}
    for k, t in want.items():
        assert got[k].dtype == np.float64
        assert np.array_equal(got[k], t.cpu().numpy().astype(np.float64)), k
