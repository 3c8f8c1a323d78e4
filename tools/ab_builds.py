#!/usr/bin/env python3
"""A/B of two BUILDS of the library on one box in one visit: m_best step 1 of the config-2 batch under the library's
HIP events, the two builds in alternating rounds (the library is loaded once per process, so every round of a build is
a fresh child process that runs 10 timed calls after a warm-up).  Outputs of the two builds are compared.  The gain
counts only if the difference of the means exceeds three times the larger spread (max - min of the round means) of the
two builds -- the 3-spread rule of DESIGN 5.5.

  tools/ab_builds.py <other libperiod_hip.so> [--rounds 5] [--gamma] [--out DIR]

`other` is the build to compare against (e.g. the parent commit's library, built aside); the in-tree library is "new".
Every child runs under its own time limit and the script stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 10


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from pyperiod_amd import PeriodEngine
    from pyperiod_amd.synth import multi_sinusoid_batch

    x = torch.from_numpy(multi_sinusoid_batch(0, args.windows, args.n)).cuda()
    e = PeriodEngine(0)
    out = e.m_best(x, 10, None, 2, args.gamma, want_sweeps=True)
    torch.cuda.synchronize()
    e.profile(True)
    for _ in range(REPS):
        out = e.m_best(x, 10, None, 2, args.gamma, want_sweeps=True)
    torch.cuda.synchronize()
    prof = e.profile_read()
    e.profile(False)
    k1 = [ms for nm, ms in prof if nm == "k_mbest_step1"]
    k2 = [ms for nm, ms in prof if nm == "k_mbest_step2"]
    res = [o.cpu().numpy() for o in out]
    if args.dump:
        import hashlib

        good = np.ascontiguousarray(res[2][res[3] == 0])  # (what a window whose step 1 failed leaves in its rows is no contract)
        np.savez(args.dump, periods=res[0], powers=res[1], bases_sha=hashlib.sha256(good.tobytes()).hexdigest(), status=res[3], sweeps=res[4])
    print(json.dumps({"step1": float(np.mean(k1)), "step1_min": float(np.min(k1)), "step2": float(np.mean(k2)), "sweeps": int(res[4].sum())}))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gamma", action="store_true")
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.other and os.path.exists(args.other), "the library of the other build"
    import numpy as np

    import tempfile

    out_dir = args.out or tempfile.mkdtemp(prefix="ab_builds_")  # (only the children's output files for the comparison)
    os.makedirs(out_dir, exist_ok=True)
    times = {"other": [], "new": []}
    for rnd in range(args.rounds):
        for name in ("other", "new"):
            env = dict(os.environ)
            env.pop("PYPERIOD_AMD_LIB", None)
            if name == "other":
                env["PYPERIOD_AMD_LIB"] = os.path.abspath(args.other)
            cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--n", str(args.n),
                   "--dump", os.path.join(out_dir, f"{name}.npz")] + (["--gamma"] if args.gamma else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"round {rnd} {name}: child ended with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 1
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            times[name].append(rec)
            print(f"round {rnd} {name:5s} step1 {rec['step1']:.4f} ms (min {rec['step1_min']:.4f})  step2 {rec['step2']:.4f} ms  sweeps {rec['sweeps']}", flush=True)
    a, b = (np.load(os.path.join(out_dir, f"{name}.npz")) for name in ("other", "new"))
    ok = a["status"] == 0
    dpow = float(np.max(np.abs(a["powers"][ok] - b["powers"][ok]) / np.maximum(np.abs(a["powers"][ok]), 1e-300))) if ok.any() else 0.0
    print(f"outputs: periods identical {np.array_equal(a['periods'], b['periods'])}, status {np.array_equal(a['status'], b['status'])}, "
          f"sweeps {np.array_equal(a['sweeps'], b['sweeps'])}, bases bit-identical {str(a['bases_sha']) == str(b['bases_sha'])}, powers rel {dpow:.2e}")
    s = np.array([t["step1"] for t in times["other"]])
    d = np.array([t["step1"] for t in times["new"]])
    spread = max(s.max() - s.min(), d.max() - d.min())
    diff = s.mean() - d.mean()
    print(f"step 1: other {s.mean():.4f} ms (spread {s.max() - s.min():.4f}), new {d.mean():.4f} ms (spread {d.max() - d.min():.4f}): "
          f"{s.mean() / d.mean():.3f} x, difference {diff:.4f} ms = {diff / spread if spread > 0 else float('inf'):.1f} spreads "
          f"({'counts' if diff > 3 * spread else 'inside the noise'}); step 2 {np.mean([t['step2'] for t in times['other']]):.4f} / "
          f"{np.mean([t['step2'] for t in times['new']]):.4f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
