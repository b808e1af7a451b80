"""Aggregate throughput of the batched engine (include/dibs_hip.h, n_problems): problem-steps/s of B independent MarginalDiBS + BGe
problems in one engine, next to the standalone engine (B = 1) on the same box.

    python scripts/gpu_batch_bench.py [--steps K] [--warmup W] [--out FILE]

Every measurement runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the script.
Sizes: config 2 (d = 20, 32 particles) for B in {1, 2, 4, 8, 16, 32}; the headline (d = 50, 128 particles) for B in {1, 2, 4}.  S = 128,
Sa = 32, 100 observations per problem, Erdos-Renyi-2 linear-Gaussian data (a different data set and key per problem)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [("config2", 20, 32, (1, 2, 4, 8, 16, 32)), ("headline", 50, 128, (1, 2, 4))]


def one(d, M, B, steps, warmup, reps=3):
    sys.path.insert(0, ROOT)
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    from dibs_amd.target import make_linear_gaussian_equivalent_model
    xs = [np.asarray(make_linear_gaussian_equivalent_model(key=random.PRNGKey(p), n_vars=d, graph_prior_str="er", n_observations=100)[0].x,
                     np.float32) for p in range(B)]
    e = Engine(make_config(n_vars=d, n_particles=M, n_observations=100, n_problems=B))
    if B == 1:
        e.set_data(xs[0])
        e.init_particles(random.PRNGKey(0))
    else:
        for p, x in enumerate(xs):
            e.set_data_problem(p, x)
        e.init_particles_batch(np.stack([random.PRNGKey(p) for p in range(B)]))
    e.run(0, warmup)
    times = []
    t = warmup
    for _ in range(reps):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    e.close()
    el = sorted(times)[len(times) // 2]
    return dict(d=d, n_particles=M, B=B, steps=steps, us_per_step=1e6 * el / steps, problem_steps_per_s=B * steps / el,
                reps_s=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, type=int, metavar=("D", "M", "B"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(*a.one, a.steps, a.warmup)))
        return 0
    rows = []
    for name, d, M, Bs in SIZES:
        base = None
        for B in Bs:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(d), str(M), str(B), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                print(f"{name} B={B}: time limit", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"{name} B={B}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            row["size"] = name
            base = base or row["problem_steps_per_s"]
            row["vs_standalone"] = row["problem_steps_per_s"] / base
            rows.append(row)
            print(f"{name:9s} B={B:3d}  {row['us_per_step']:9.1f} us/step  {row['problem_steps_per_s']:10.0f} problem-steps/s  "
                  f"x{row['vs_standalone']:.2f}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(script="scripts/gpu_batch_bench.py", steps=a.steps, warmup=a.warmup, rows=rows), open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
