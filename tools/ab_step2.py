#!/usr/bin/env python3
"""A/B of BUILDS of the library on one box in one visit: k_mbest_step2 of the config-2 batch under the library's HIP
events, the builds in alternating rounds (the library is loaded once per process, so every round of a build is a fresh
child process that runs 10 timed calls after a warm-up).  The outputs of every build are compared with the first one's,
bit for bit.  A difference counts only if it exceeds three times the larger spread (max - min of the round means) of
the two builds -- the 3-spread rule of DESIGN 5.5.

  tools/ab_step2.py <parent libperiod_hip.so> [--build NAME=LIB ...] [--rounds 5] [--out DIR]

The parent's library (built aside) is "parent", the in-tree library is "new"; --build adds further libraries (the
candidates on the way to "new") and --env NAME=VAR=VALUE a run of the in-tree library with a switch set
(e.g. --env fallback=PH_STEP2_GEOM=0).  Every child runs under its own time limit and the script stops at the first
child that fails."""
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
    out = e.m_best(x, 10, None, 2, False, want_sweeps=True)
    torch.cuda.synchronize()
    e.profile(True)
    for _ in range(REPS):
        out = e.m_best(x, 10, None, 2, False, want_sweeps=True)
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
    print(json.dumps({"step1": float(np.mean(k1)), "step2": float(np.mean(k2)), "step2_min": float(np.min(k2)), "step2_max": float(np.max(k2))}))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("--build", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--env", action="append", default=[], metavar="NAME=VAR=VALUE")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.parent and os.path.exists(args.parent), "the library of the parent build"
    import tempfile

    import numpy as np

    builds = [("parent", os.path.abspath(args.parent), {})]
    for spec in args.build:
        name, lib = spec.split("=", 1)
        assert os.path.exists(lib), lib
        builds.append((name, os.path.abspath(lib), {}))
    for spec in args.env:
        name, var, value = spec.split("=", 2)
        builds.append((name, None, {var: value}))
    builds.append(("new", None, {}))
    out_dir = args.out or tempfile.mkdtemp(prefix="ab_step2_")  # (only the children's output files for the comparison)
    os.makedirs(out_dir, exist_ok=True)
    times = {name: [] for name, _, _ in builds}
    for rnd in range(args.rounds):
        for name, lib, extra in builds:
            env = dict(os.environ)
            env.pop("PYPERIOD_AMD_LIB", None)
            if lib:
                env["PYPERIOD_AMD_LIB"] = lib
            env.update(extra)
            cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--n", str(args.n),
                   "--dump", os.path.join(out_dir, f"{name}.npz")]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"round {rnd} {name}: child ended with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 1
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            times[name].append(rec)
            print(f"round {rnd} {name:8s} step2 {rec['step2']:.4f} ms (min {rec['step2_min']:.4f}, max {rec['step2_max']:.4f})  step1 {rec['step1']:.4f} ms", flush=True)
    a = np.load(os.path.join(out_dir, "parent.npz"))
    for name, _, _ in builds[1:]:
        b = np.load(os.path.join(out_dir, f"{name}.npz"))
        same = {k: bool(np.array_equal(a[k], b[k])) for k in ("periods", "powers", "status", "sweeps")}
        same["bases"] = str(a["bases_sha"]) == str(b["bases_sha"])
        print(f"outputs of {name} against parent, bit for bit: " + ", ".join(f"{k} {'identical' if v else 'DIFFERENT'}" for k, v in same.items()))
    s = np.array([t["step2"] for t in times["parent"]])
    for name, _, _ in builds[1:]:
        d = np.array([t["step2"] for t in times[name]])
        spread = max(s.max() - s.min(), d.max() - d.min())
        diff = s.mean() - d.mean()
        print(f"step 2: parent {s.mean():.4f} ms (spread {s.max() - s.min():.4f}), {name} {d.mean():.4f} ms (spread {d.max() - d.min():.4f}): "
              f"{s.mean() / d.mean():.3f} x, difference {diff:.4f} ms = {diff / spread if spread > 0 else float('inf'):.1f} spreads "
              f"({'counts' if abs(diff) > 3 * spread else 'inside the noise'}); step 1 {np.mean([t['step1'] for t in times['parent']]):.4f} / "
              f"{np.mean([t['step1'] for t in times[name]]):.4f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
