"""What the per-problem hyper-parameters of the batched engine cost and buy (include/dibs_hip.h, dibs_engine_set_problem_hparams), against
a checkout of the PARENT commit with its own library built, on one MI355X in one job:

    python scripts/gpu_sweep_bench.py --parent-root DIR [--steps K] [--warmup W] [--out FILE] [--single-path-out FILE]

  table_cost    B = 16 problems at config-2 size (d = 20, 32 particles) with uniform hyper-parameters: ms/step of this tree against the
                parent's, five alternating runs each.  Gate: this tree's median within the parent's [min, max] widened by (max - min) on
                either side.
  sweep_gain    a 16-point grid (4 alpha_linear x 4 h) on one data set at config-2 size: problem-steps/s of the sweep in ONE engine of this
                tree against the same 16 configurations one after another on the parent's standalone engine.  Gate: faster.
  single_path   bench.py --dump-outputs of the headline config and config 2 from both trees (np.array_equal per array), and ms_per_step of
                five alternating plain bench.py runs each.  Gate: this tree's median inside the parent's [min, max].

Every measurement is a child process of its own under a time limit, run with the tree it measures as working directory and import
root; the first one that fails or runs out of time ends the script.  A timed window is K steps behind W warm-up steps and ends in a
device synchronise (dibs_engine_run blocks); a figure is the median of three windows."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, M, B = 20, 32, 16
GRID = [(al, h) for al in (0.25, 0.5, 1.0, 2.0) for h in (2.0, 5.0, 10.0, 20.0)]


def _data(n, d):
    import numpy as np
    from dibs_amd import random
    from dibs_amd.target import make_linear_gaussian_equivalent_model
    return [np.asarray(make_linear_gaussian_equivalent_model(key=random.PRNGKey(p), n_vars=d, graph_prior_str="er", n_observations=100)[0].x,
                       np.float32) for p in range(n)]


def _timed(e, steps, warmup, reps=3):
    e.run(0, warmup)
    times, t = [], warmup
    for _ in range(reps):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    return sorted(times)[len(times) // 2], times


def one(what, root, steps, warmup):
    """a child: `what` measured with the package of the tree `root`"""
    sys.path.insert(0, root)
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    keys = np.stack([random.PRNGKey(p) for p in range(B)])
    if what == "uniform":      # the batch of sample_batch: every problem its own data, the configuration's hyper-parameters
        xs = _data(B, D)
        e = Engine(make_config(n_vars=D, n_particles=M, n_observations=100, n_problems=B))
        for p, x in enumerate(xs):
            e.set_data_problem(p, x)
        e.init_particles_batch(keys)
        el, times = _timed(e, steps, warmup)
        e.close()
        return dict(ms_per_step=1e3 * el / steps, problem_steps_per_s=B * steps / el, reps_s=times)
    x = _data(1, D)[0]
    if what == "sweep":        # the grid in one engine
        e = Engine(make_config(n_vars=D, n_particles=M, n_observations=100, n_problems=len(GRID)))
        for p, (al, h) in enumerate(GRID):
            e.set_data_problem(p, x)
            e.set_problem_hparams(p, alpha_linear=al, h_latent=h)
        e.init_particles_batch(np.stack([random.PRNGKey(0)] * len(GRID)))
        el, times = _timed(e, steps, warmup)
        z = e.get_state()["z"]
        e.close()
        return dict(ms_per_step=1e3 * el / steps, problem_steps_per_s=len(GRID) * steps / el, reps_s=times,
                    finite=bool(np.isfinite(z).all()))
    if what == "sequential":   # the grid point by point on the standalone engine
        total, per = 0.0, []
        for al, h in GRID:
            e = Engine(make_config(n_vars=D, n_particles=M, n_observations=100, alpha_linear=al, h_latent=h))
            e.set_data(x)
            e.init_particles(random.PRNGKey(0))
            el, _ = _timed(e, steps, warmup)
            e.close()
            total += el
            per.append(1e3 * el / steps)
        return dict(problem_steps_per_s=len(GRID) * steps / total, ms_per_step_each=per)
    raise SystemExit(f"unknown measurement {what}")


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(what, root, a):
    return _child(root, [os.path.abspath(__file__), "--one", what, "--root", root, "--steps", str(a.steps), "--warmup", str(a.warmup)], 600)


def _bench(root, config, a, dump=None):
    argv = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--config", config]
    return _child(root, argv + (["--dump-outputs", dump] if dump else []), 600)


def _same_dumps(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and len(fa) > 0 and all(np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))) for f in fa), fa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-path-out", default=None)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.root, a.steps, a.warmup)))
        return 0
    if not a.parent_root:
        ap.error("--parent-root is required")
    parent, ok = os.path.abspath(a.parent_root), True
    out = dict(script="scripts/gpu_sweep_bench.py", steps=a.steps, warmup=a.warmup, size=dict(d=D, n_particles=M, S=128, Sa=32))

    # 1. cost of the table
    ser = dict(parent=[], this=[])
    for _ in range(a.runs):
        ser["parent"].append(_measure("uniform", parent, a)["ms_per_step"])
        ser["this"].append(_measure("uniform", HERE, a)["ms_per_step"])
    lo, hi = min(ser["parent"]), max(ser["parent"])
    med = statistics.median(ser["this"])
    out["table_cost"] = dict(B=B, ms_per_step=ser, parent_min=lo, parent_max=hi, this_median=med, bound=[lo - (hi - lo), hi + (hi - lo)],
                             within=bool(lo - (hi - lo) <= med <= hi + (hi - lo)))
    ok &= out["table_cost"]["within"]
    print("table_cost", json.dumps(out["table_cost"]), flush=True)

    # 2. what the feature buys
    sw, sq = _measure("sweep", HERE, a), _measure("sequential", parent, a)
    out["sweep_gain"] = dict(grid=GRID, sweep=sw, sequential_parent=sq, ratio=sw["problem_steps_per_s"] / sq["problem_steps_per_s"],
                             faster=bool(sw["problem_steps_per_s"] > sq["problem_steps_per_s"] and sw["finite"]))
    ok &= out["sweep_gain"]["faster"]
    print("sweep_gain", json.dumps(out["sweep_gain"]), flush=True)

    # 3. the standalone path
    lines = ["Standalone path beside the per-problem hyper-parameters of the batched engine (scripts/gpu_sweep_bench.py; one MI355X, one job,",
             f"alternating runs; bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}):"]
    out["single_path"] = {}
    with tempfile.TemporaryDirectory() as td:
        for config in ("headline", "2"):
            dp, dt = os.path.join(td, f"p{config}"), os.path.join(td, f"t{config}")
            _bench(parent, config, a, dp)
            _bench(HERE, config, a, dt)
            same, files = _same_dumps(dp, dt)
            ms = dict(parent=[], this=[])
            for _ in range(a.runs):
                ms["parent"].append(_bench(parent, config, a)["ms_per_step"])
                ms["this"].append(_bench(HERE, config, a)["ms_per_step"])
            lo, hi, med = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["this"])
            row = dict(dump_files=files, dumps_equal=bool(same), ms_per_step=ms, parent_min=lo, parent_max=hi, this_median=med,
                       inside=bool(lo <= med <= hi))
            out["single_path"][config] = row
            ok &= row["dumps_equal"] and row["inside"]
            lines += [f"  config {config}:",
                      f"    --dump-outputs, parent vs this change: {', '.join(files)} np.array_equal: {same}",
                      "    ms_per_step parent:      " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"   (min {lo:.4f}, max {hi:.4f})",
                      "    ms_per_step this change: " + " ".join(f"{v:.4f}" for v in ms["this"]) + f"   (median {med:.4f}: "
                      + ("inside" if row["inside"] else "OUTSIDE") + " the parent's min-max)"]
            print("single_path", config, json.dumps(row), flush=True)
    for path, text in ((a.out, json.dumps(out, indent=1)), (a.single_path_out, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            open(path, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
