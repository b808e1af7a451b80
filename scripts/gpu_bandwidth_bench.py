"""What the median-rule kernel bandwidth costs (include/dibs_hip.h, MEDIAN-HEURISTIC KERNEL BANDWIDTH), and what
the change costs the paths that do not use it, on one MI355X in one job:

    python scripts/gpu_bandwidth_bench.py [--parent-root DIR] [--steps K] [--warmup W] [--out FILE] [--single-path-out FILE]

  cost          per size -- config-2 size (BGe, d = 20, 32 particles), the headline size (BGe, d = 50, 128 particles), config-3 size
                (LinearGaussian, d = 50, 128 particles) and a 16-chain LinearGaussian engine at d = 20 / 32 particles -- steps/s of THIS
                tree with the fixed rule against the median rule (every kernel of the model on the rule).  Alternating runs, medians.  No
                gate: the ratio is the result.  Then one run per side with per-kernel timing (dibs_engine_set_profiling(1): every kernel
                alone on the GPU): microseconds per step and kernel family, which says where the cost sits.
  single_path   with --parent-root (a checkout of the parent commit with its library built): bench.py --dump-outputs of the headline
                config and config 3 from both trees (np.array_equal per array), and ms_per_step of five alternating plain bench.py runs
                each.  Gate: this tree's median inside the parent's [min, max] widened by (max - min) on either side.

Every measurement is a child process of its own under a time limit; the first one that fails or runs out of time ends the script.  A
timed window is K steps behind W warm-up steps and ends in a device synchronise (dibs_engine_run blocks); a figure is the median of three
windows."""
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
    "bge_config2": dict(d=20, M=32, likelihood="bge", chains=0),
    "bge_headline": dict(d=50, M=128, likelihood="bge", chains=0),
    "lingauss_config3": dict(d=50, M=128, likelihood="lingauss", chains=0),
    "lingauss_d20_m32_16chains": dict(d=20, M=32, likelihood="lingauss", chains=16),
}
N_OBS, S, SA = 100, 128, 32


def _engine(size, rule):
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    from dibs_amd.target import make_linear_gaussian_equivalent_model, make_linear_gaussian_model
    joint = size["likelihood"] != "bge"
    f = make_linear_gaussian_model if joint else make_linear_gaussian_equivalent_model
    x = np.asarray(f(key=random.PRNGKey(0), n_vars=size["d"], graph_prior_str="er", n_observations=N_OBS)[0].x, np.float32)
    kw = dict(n_vars=size["d"], n_particles=size["M"], n_observations=N_OBS, joint=joint, likelihood=size["likelihood"],
              n_grad_mc_samples=S, n_acyclicity_mc_samples=SA, n_chains=size["chains"])
    if rule == "median":
        kw.update(h_latent="median", **(dict(h_theta="median") if joint else {}))
    e = Engine(make_config(**kw))
    e.set_data(x)
    if size["chains"]:
        e.init_particles_batch(np.stack([random.PRNGKey(c) for c in range(size["chains"])]))
    else:
        e.init_particles(random.PRNGKey(0))
    return e


def one(rule, name, steps, warmup, timers):
    """a child: one size on one rule; `timers`: a further window with per-kernel timing"""
    import numpy as np
    size = SIZES[name]
    e = _engine(size, rule)
    e.run(0, warmup)
    times, t = [], warmup
    for _ in range(3):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    el = sorted(times)[1]
    out = dict(steps_per_s=steps / el, ms_per_step=1e3 * el / steps, finite=bool(np.isfinite(e.get_state()["z"]).all()),
               bandwidth=[float(v) for v in e.read("BANDWIDTH").reshape(-1)[:2]])
    if timers:
        e.set_profiling(1)
        e.reset_timers()
        e.run(t, steps)
        out["us_per_step_by_kernel"] = {k: 1e3 * ms / steps for k, (ms, n) in e.timers().items()}
    e.close()
    return out


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(rule, name, a, timers=False):
    return _child(HERE, [os.path.abspath(__file__), "--one", rule, "--size", name, "--steps", str(a.steps), "--warmup", str(a.warmup)]
                  + (["--timers"] if timers else []), 600)


def _bench(root, config, a, dump=None):
    argv = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--config", config]
    return _child(root, argv + (["--dump-outputs", dump] if dump else []), 600)


def _same_dumps(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and len(fa) > 0 and all(np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))) for f in fa), fa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built (the single-path check)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per side")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-path-out", default=None)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--size", help=argparse.SUPPRESS)
    ap.add_argument("--timers", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        sys.path.insert(0, HERE)
        print(json.dumps(one(a.one, a.size, a.steps, a.warmup, a.timers)))
        return 0
    ok = True
    out = dict(script="scripts/gpu_bandwidth_bench.py", steps=a.steps, warmup=a.warmup, runs=a.runs, n_observations=N_OBS, S=S, Sa=SA, sizes={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(out, indent=1))

    # 1. what the rule costs
    for name in a.sizes.split(","):
        runs = dict(fixed=[], median=[])
        for _ in range(a.runs):
            for rule in runs:
                runs[rule].append(_measure(rule, name, a))
        row = dict(SIZES[name])
        for rule, rs in runs.items():
            row[rule] = dict(steps_per_s=[r["steps_per_s"] for r in rs], median_steps_per_s=statistics.median(r["steps_per_s"] for r in rs),
                             bandwidth=rs[-1]["bandwidth"])
            ok &= all(r["finite"] for r in rs)
        row["median_over_fixed"] = row["median"]["median_steps_per_s"] / row["fixed"]["median_steps_per_s"]
        row["us_per_step_added"] = 1e6 / row["median"]["median_steps_per_s"] - 1e6 / row["fixed"]["median_steps_per_s"]
        row["us_per_step_by_kernel"] = {rule: _measure(rule, name, a, timers=True)["us_per_step_by_kernel"] for rule in runs}
        out["sizes"][name] = row
        print("cost", name, json.dumps(row), flush=True)
        save()

    # 2. the paths that do not use the rule
    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        lines = ["Fixed-rule path beside the median-rule bandwidth (scripts/gpu_bandwidth_bench.py; one MI355X, one job, alternating runs;",
                 f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}):"]
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
                lo, hi, med = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["this"])
                bound = [lo - (hi - lo), hi + (hi - lo)]
                row = dict(dump_files=files, dumps_equal=bool(same), ms_per_step=ms, parent_min=lo, parent_max=hi, this_median=med, bound=bound,
                           within=bool(bound[0] <= med <= bound[1]))
                out["single_path"][config] = row
                ok &= row["dumps_equal"] and row["within"]
                lines += [f"  config {config}:",
                          f"    --dump-outputs, parent vs this change: {', '.join(files)} np.array_equal: {same}",
                          "    ms_per_step parent:      " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"   (min {lo:.4f}, max {hi:.4f})",
                          "    ms_per_step this change: " + " ".join(f"{v:.4f}" for v in ms["this"]) + f"   (median {med:.4f}: "
                          + ("inside" if row["within"] else "OUTSIDE") + f" the parent's min-max widened by its spread, [{bound[0]:.4f}, {bound[1]:.4f}])"]
                print("single_path", config, json.dumps(row), flush=True)
        if a.single_path_out:
            os.makedirs(os.path.dirname(os.path.abspath(a.single_path_out)), exist_ok=True)
            open(a.single_path_out, "w").write("\n".join(lines) + "\n")
    save()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
