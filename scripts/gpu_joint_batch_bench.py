"""What per-chain data in the chains engine buys (include/dibs_hip.h, CHAINS ENGINE; dibs_amd.inference.sample_joint_batch), what the
per-chain pointers cost, and what the change costs the paths it does not touch, against a checkout of the PARENT commit with its own
library built, on one MI355X in one job:

    python scripts/gpu_joint_batch_bench.py --parent-root DIR [--steps K] [--warmup W] [--out FILE] [--single-path-out FILE]

  batch         per size (LinearGaussian d = 20 / 32 particles and config-3 size d = 50 / 128 particles; 100 observations, S = 128,
                Sa = 32) and B = 1, 4, 16, 32 DISTINCT data sets: problem-steps/s of
                  (a) sequential_parent  the B problems one after another on the parent's standalone engine,
                  (b) chains_shared      this tree's chains engine, C = B chains on ONE data set (dibs_engine_set_data),
                  (c) batch              this tree's chains engine, chain c on data set c (dibs_engine_set_data_problem).
                (B = 1: the standalone engine of the side's tree.)  Alternating runs, medians.  (c) / (a) is what the feature buys,
                (c) / (b) what the per-chain pointers cost.  No gate: the ratios are the result, whichever way they fall.
  single_path   bench.py --dump-outputs of the headline config and config 3 from both trees (np.array_equal per array), and ms_per_step of
                five alternating plain bench.py runs each; the shared-data chains engine at d = 20, C = 16 of both trees the same way (five
                alternating runs of ms_per_step).  Gate: this tree's median inside the parent's [min, max] widened by (max - min) on
                either side.

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
SIZES = {
    "lingauss_d20_m32": dict(d=20, M=32),
    "lingauss_config3": dict(d=50, M=128),
}
BATCHES = (1, 4, 16, 32)
N_OBS, S, SA = 100, 128, 32


def _data(size, seed):
    import numpy as np
    from dibs_amd import random
    from dibs_amd.target import make_linear_gaussian_model
    return np.asarray(make_linear_gaussian_model(key=random.PRNGKey(seed), n_vars=size["d"], graph_prior_str="er",
                                                 n_observations=N_OBS)[0].x, np.float32)


def _timed(e, steps, warmup, reps=3):
    e.run(0, warmup)
    times, t = [], warmup
    for _ in range(reps):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    return sorted(times)[len(times) // 2]


def one(what, name, root, steps, warmup, batches):
    """a child: every batch size of one size as `sequential` standalone runs, one `chains_shared` engine or one `batch` engine, with the
    package of the tree `root`"""
    sys.path.insert(0, root)
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    size = SIZES[name]
    xs = [_data(size, b) for b in range(max(batches))]
    kw = dict(n_vars=size["d"], n_particles=size["M"], n_observations=N_OBS, joint=True, likelihood="lingauss", n_grad_mc_samples=S,
              n_acyclicity_mc_samples=SA)
    out = {}
    for B in batches:
        if what != "sequential" and B > 1:
            e = Engine(make_config(n_chains=B, **kw))
            if what == "batch":
                for b in range(B):
                    e.set_data_problem(b, xs[b])
            else:
                e.set_data(xs[0])
            e.init_particles_batch(np.stack([random.PRNGKey(b) for b in range(B)]))
            el = _timed(e, steps, warmup)
            finite = bool(np.isfinite(e.get_state()["z"]).all())
            e.close()
        else:
            el, finite = 0.0, True
            for b in range(B):
                e = Engine(make_config(**kw))
                e.set_data(xs[b])
                e.init_particles(random.PRNGKey(b))
                el += _timed(e, steps, warmup)
                finite &= bool(np.isfinite(e.get_state()["z"]).all())
                e.close()
        out[str(B)] = dict(problem_steps_per_s=B * steps / el, ms_per_step=1e3 * el / steps, finite=finite)
    return out


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(what, name, root, a, batches=BATCHES):
    return _child(root, [os.path.abspath(__file__), "--one", what, "--size", name, "--root", root, "--steps", str(a.steps), "--warmup",
                         str(a.warmup), "--batches", ",".join(map(str, batches))], 600)


def _bench(root, config, a, dump=None):
    argv = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--config", config]
    return _child(root, argv + (["--dump-outputs", dump] if dump else []), 600)


def _same_dumps(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and len(fa) > 0 and all(np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))) for f in fa), fa


def _gate(ms):
    lo, hi, med = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["this"])
    bound = [lo - (hi - lo), hi + (hi - lo)]
    return dict(ms_per_step=ms, parent_min=lo, parent_max=hi, this_median=med, bound=bound, within=bool(bound[0] <= med <= bound[1]))


def _gate_lines(row):
    ms, b = row["ms_per_step"], row["bound"]
    return ["    ms_per_step parent:      " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"   (min {row['parent_min']:.4f}, max {row['parent_max']:.4f})",
            "    ms_per_step this change: " + " ".join(f"{v:.4f}" for v in ms["this"]) + f"   (median {row['this_median']:.4f}: "
            + ("inside" if row["within"] else "OUTSIDE") + f" the parent's min-max widened by its spread, [{b[0]:.4f}, {b[1]:.4f}])"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per side of the batch measurement")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--skip-single-path", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-path-out", default=None)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--size", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.size, a.root, a.steps, a.warmup, tuple(int(b) for b in a.batches.split(",")))))
        return 0
    if not a.parent_root:
        ap.error("--parent-root is required")
    parent, ok = os.path.abspath(a.parent_root), True
    out = dict(script="scripts/gpu_joint_batch_bench.py", steps=a.steps, warmup=a.warmup, runs=a.runs, n_observations=N_OBS, S=S, Sa=SA, sizes={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(out, indent=1))

    # 1. what the feature buys, and what the per-chain pointers cost
    for name in ([] if a.skip_batch else a.sizes.split(",")):
        sides = dict(sequential_parent=("sequential", parent), chains_shared=("chains_shared", HERE), batch=("batch", HERE))
        runs = {k: [] for k in sides}
        for _ in range(a.runs):
            for k, (what, root) in sides.items():
                runs[k].append(_measure(what, name, root, a))
        row = dict(SIZES[name])
        for B in BATCHES:
            vals = {k: [r[str(B)]["problem_steps_per_s"] for r in runs[k]] for k in sides}
            med = {k: statistics.median(v) for k, v in vals.items()}
            fin = all(r[str(B)]["finite"] for side in runs.values() for r in side)
            row[f"B={B}"] = dict(problem_steps_per_s=vals, median=med, batch_over_sequential_parent=med["batch"] / med["sequential_parent"],
                                 batch_over_chains_shared=med["batch"] / med["chains_shared"], finite=fin)
            ok &= fin
        out["sizes"][name] = row
        print("batch", name, json.dumps(row), flush=True)
        save()

    # 2. the paths the change does not touch
    if not a.skip_single_path:
        lines = ["Untouched paths beside per-chain data in the chains engine (scripts/gpu_joint_batch_bench.py; one MI355X, one job, alternating",
                 f"runs; bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}):"]
        out["single_path"] = {}
        with tempfile.TemporaryDirectory() as td:
            for config in ("headline", "3"):
                dp, dt = os.path.join(td, f"p{config}"), os.path.join(td, f"t{config}")
                _bench(parent, config, a, dp)
                _bench(HERE, config, a, dt)
                same, files = _same_dumps(dp, dt)
                ms = dict(parent=[], this=[])
                for _ in range(a.bench_runs):
                    ms["parent"].append(_bench(parent, config, a)["ms_per_step"])
                    ms["this"].append(_bench(HERE, config, a)["ms_per_step"])
                row = dict(dump_files=files, dumps_equal=bool(same), **_gate(ms))
                out["single_path"][config] = row
                ok &= row["dumps_equal"] and row["within"]
                lines += [f"  config {config}:", f"    --dump-outputs, parent vs this change: {', '.join(files)} np.array_equal: {same}"] + _gate_lines(row)
                print("single_path", config, json.dumps(row), flush=True)
        # the shared-data chains engine (dibs_engine_set_data), LinearGaussian d = 20, 32 particles, C = 16: both trees have it
        ms = dict(parent=[], this=[])
        for _ in range(a.bench_runs):
            ms["parent"].append(_measure("chains_shared", "lingauss_d20_m32", parent, a, (16,))["16"]["ms_per_step"])
            ms["this"].append(_measure("chains_shared", "lingauss_d20_m32", HERE, a, (16,))["16"]["ms_per_step"])
        row = _gate(ms)
        out["single_path"]["chains_shared_d20_C16"] = row
        ok &= row["within"]
        lines += [f"  shared-data chains engine, LinearGaussian d = 20, 32 particles, C = 16 ({a.steps} steps behind {a.warmup}, median of 3 windows):"]
        lines += _gate_lines(row)
        print("single_path chains_shared_d20_C16", json.dumps(row), flush=True)
        if a.single_path_out:
            os.makedirs(os.path.dirname(os.path.abspath(a.single_path_out)), exist_ok=True)
            open(a.single_path_out, "w").write("\n".join(lines) + "\n")
    save()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
