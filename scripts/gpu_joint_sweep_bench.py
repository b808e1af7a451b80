"""What per-chain hyper-parameters in the chains engine buy (include/dibs_hip.h, PER-CHAIN HYPER-PARAMETERS;
dibs_amd.inference.sample_joint_sweep), what the table tier costs, and what the change costs the paths it does not touch, against a
checkout of the PARENT commit with its own library built, on one MI355X in one job:

    python scripts/gpu_joint_sweep_bench.py --parent-root DIR [--steps K] [--warmup W] [--out FILE] [--single-path-out FILE]

  sweep         per size (LinearGaussian d = 20 / 32 particles and config-3 size d = 50 / 128 particles; 100 observations, S = 128,
                Sa = 32) and B = 4, 16, 32 grid points of alpha_linear x h_latent on ONE data set: problem-steps/s of
                  (a) sequential_parent  the B grid points one after another on the parent's standalone engine,
                  (b) batch_uniform      this tree's chains engine with per-chain data and the configuration's values in every chain
                                         (the path of sample_joint_batch: the parent's launches),
                  (c) sweep              this tree's chains engine, chain c at grid point c (dibs_engine_set_chain_hparams),
                  (d) tier_only          the same engine with chain c's alpha_linear = the configuration's x (1 + c 1e-6): the table tier
                                         on, the work of (b) -- a larger alpha makes harder graphs and a dearer gradient kernel, so
                                         (c) / (b) mixes the tier's cost with the grid's.
                Alternating runs, medians.  (c) / (a) is what the feature buys, (d) / (b) what the table tier costs; with --timers the
                per-kernel timers of (b), (c), (d) and the parent's (b) at B = 16 say which kernel carries a difference.  No gate: the
                ratios are the result.
  single_path   bench.py --dump-outputs of the headline config and config 3 from both trees (np.array_equal per array), and ms_per_step of
                five alternating plain bench.py runs each; the shared-data chains engine at d = 20, C = 16 and the per-chain-data chains
                engine at d = 20, B = 16 (whose _chains kernels this change edits) of both trees the same way.  Gate: this tree's median
                inside the parent's [min, max] widened by (max - min) on either side.

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
BATCHES = (4, 16, 32)
N_OBS, S, SA = 100, 128, 32
ALPHAS = (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
HS = (2.0, 3.0, 5.0, 8.0)


def grid(B):
    """B points of the alpha_linear x h_latent grid (4 x 4 at B = 16; the first / all eight alphas at 4 / 32)"""
    na = B // len(HS) if B >= len(HS) else 1
    pts = [(al, h) for al in ALPHAS[:na] for h in HS]
    return pts[:B]


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


def one(what, name, root, steps, warmup, batches, timers=False):
    """a child: every batch size of one size as `sequential` standalone runs at the grid points, one `chains_shared` engine (one data
    set, dibs_engine_set_data), one `batch_uniform` engine (per-chain data, shared values), one `sweep` or one `tier_only` engine, with
    the package of the tree `root`"""
    sys.path.insert(0, root)
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    size = SIZES[name]
    x = _data(size, 0)
    kw = dict(n_vars=size["d"], n_particles=size["M"], n_observations=N_OBS, joint=True, likelihood="lingauss", n_grad_mc_samples=S,
              n_acyclicity_mc_samples=SA)
    out = {}
    for B in batches:
        pts = grid(B)
        if what != "sequential":
            e = Engine(make_config(n_chains=B, **kw))
            if what == "chains_shared":
                e.set_data(x)
            else:
                for b in range(B):
                    e.set_data_problem(b, x)
                    if what == "sweep":
                        e.set_chain_hparams(b, alpha_linear=pts[b][0], h_latent=pts[b][1])
                    elif what == "tier_only":
                        e.set_chain_hparams(b, alpha_linear=e.cfg.alpha_linear * (1.0 + b * 1e-6))
            e.init_particles_batch(np.stack([random.PRNGKey(b) for b in range(B)]))
            el = _timed(e, steps, warmup)
            finite = bool(np.isfinite(e.get_state()["z"]).all())
            row = {}
            if timers:   # (a profiled window of its own, behind the timed ones: per-kernel event timers)
                e.set_profiling(True)
                e.reset_timers()
                e.run(warmup + 3 * steps, steps)
                row["kernel_us_per_step"] = {k: 1e3 * ms / steps for k, (ms, n) in e.timers().items()}
                e.set_profiling(False)
            e.close()
        else:
            el, finite, row = 0.0, True, {}
            for b in range(B):
                e = Engine(make_config(alpha_linear=pts[b][0], h_latent=pts[b][1], **kw))
                e.set_data(x)
                e.init_particles(random.PRNGKey(b))
                el += _timed(e, steps, warmup)
                finite &= bool(np.isfinite(e.get_state()["z"]).all())
                e.close()
        out[str(B)] = dict(problem_steps_per_s=B * steps / el, ms_per_step=1e3 * el / steps, finite=finite, **row)
    return out


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(what, name, root, a, batches=BATCHES, timers=False):
    return _child(root, [os.path.abspath(__file__), "--one", what, "--size", name, "--root", root, "--steps", str(a.steps), "--warmup",
                         str(a.warmup), "--batches", ",".join(map(str, batches))] + (["--timers"] if timers else []), 600)


def _measure_parent_batch(parent, a):
    """the parent's per-chain-data chains engine at d = 20, B = 16 through ITS bench script (this one does not exist there)"""
    argv = [os.path.join(parent, "scripts", "gpu_joint_batch_bench.py"), "--one", "batch", "--size", "lingauss_d20_m32", "--root", parent,
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--batches", "16"]
    return _child(parent, argv, 600)["16"]["ms_per_step"]


def _measure_this_batch(a):
    argv = [os.path.join(HERE, "scripts", "gpu_joint_batch_bench.py"), "--one", "batch", "--size", "lingauss_d20_m32", "--root", HERE,
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--batches", "16"]
    return _child(HERE, argv, 600)["16"]["ms_per_step"]


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
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per side of the sweep measurement")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--skip-single-path", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-path-out", default=None)
    ap.add_argument("--timers", action="store_true", help="also the per-kernel timers of batch_uniform and sweep at B = 16")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--size", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.size, a.root, a.steps, a.warmup, tuple(int(b) for b in a.batches.split(",")), a.timers)))
        return 0
    if not a.parent_root:
        ap.error("--parent-root is required")
    parent, ok = os.path.abspath(a.parent_root), True
    out = dict(script="scripts/gpu_joint_sweep_bench.py", steps=a.steps, warmup=a.warmup, runs=a.runs, n_observations=N_OBS, S=S, Sa=SA,
               grid=dict(alpha_linear=ALPHAS, h_latent=HS), sizes={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(out, indent=1))

    # 1. what the feature buys, and what the table tier costs
    for name in ([] if a.skip_sweep else a.sizes.split(",")):
        sides = dict(sequential_parent=("sequential", parent), batch_uniform=("batch_uniform", HERE), sweep=("sweep", HERE),
                     tier_only=("tier_only", HERE))
        runs = {k: [] for k in sides}
        for _ in range(a.runs):
            for k, (what, root) in sides.items():
                runs[k].append(_measure(what, name, root, a))
        row = dict(SIZES[name])
        for B in BATCHES:
            vals = {k: [r[str(B)]["problem_steps_per_s"] for r in runs[k]] for k in sides}
            med = {k: statistics.median(v) for k, v in vals.items()}
            fin = all(r[str(B)]["finite"] for side in runs.values() for r in side)
            row[f"B={B}"] = dict(problem_steps_per_s=vals, median=med, sweep_over_sequential_parent=med["sweep"] / med["sequential_parent"],
                                 sweep_over_batch_uniform=med["sweep"] / med["batch_uniform"],
                                 tier_only_over_batch_uniform=med["tier_only"] / med["batch_uniform"], finite=fin)
            ok &= fin
        if a.timers:
            row["kernel_us_per_step_B16"] = {k: _measure(sides[k][0], name, HERE, a, (16,), True)["16"]["kernel_us_per_step"]
                                             for k in ("batch_uniform", "sweep", "tier_only")}
            row["kernel_us_per_step_B16"]["batch_uniform_parent"] = _measure("batch_uniform", name, parent, a, (16,), True)["16"]["kernel_us_per_step"]
        out["sizes"][name] = row
        print("sweep", name, json.dumps(row), flush=True)
        save()

    # 2. the paths the change does not touch
    if not a.skip_single_path:
        lines = ["Untouched paths beside per-chain hyper-parameters in the chains engine (scripts/gpu_joint_sweep_bench.py; one MI355X, one job,",
                 f"alternating runs; bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}):"]
        out["single_path"] = {}

        def gate(key, title, row):
            nonlocal ok
            out["single_path"][key] = row
            ok &= row["within"]
            lines.extend([title] + _gate_lines(row))
            print("single_path", key, json.dumps(row), flush=True)
            save()

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
                ok &= row["dumps_equal"]
                lines += [f"  config {config}:", f"    --dump-outputs, parent vs this change: {', '.join(files)} np.array_equal: {same}"]
                gate(config, "    (five alternating runs)", row)
        # the shared-data chains engine (dibs_engine_set_data), LinearGaussian d = 20, 32 particles, C = 16: both trees have it
        ms = dict(parent=[], this=[])
        for _ in range(a.bench_runs):
            ms["parent"].append(_child(parent, [os.path.join(parent, "scripts", "gpu_joint_batch_bench.py"), "--one", "chains_shared", "--size",
                                                "lingauss_d20_m32", "--root", parent, "--steps", str(a.steps), "--warmup", str(a.warmup),
                                                "--batches", "16"], 600)["16"]["ms_per_step"])
            ms["this"].append(_measure("chains_shared", "lingauss_d20_m32", HERE, a, (16,))["16"]["ms_per_step"])
        gate("chains_shared_d20_C16", f"  shared-data chains engine, LinearGaussian d = 20, 32 particles, C = 16 ({a.steps} steps behind {a.warmup}, "
             "median of 3 windows):", _gate(ms))
        # per-chain data, shared values (sample_joint_batch's engine): the _chains kernels this change edits, on the parent's launches
        ms = dict(parent=[], this=[])
        for _ in range(a.bench_runs):
            ms["parent"].append(_measure_parent_batch(parent, a))
            ms["this"].append(_measure_this_batch(a))
        gate("joint_batch_d20_B16", "  per-chain data, shared values (the engine of sample_joint_batch), LinearGaussian d = 20, 32 particles, B = 16 "
             "distinct data sets:", _gate(ms))
        if a.single_path_out:
            os.makedirs(os.path.dirname(os.path.abspath(a.single_path_out)), exist_ok=True)
            open(a.single_path_out, "w").write("\n".join(lines) + "\n")
    save()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
