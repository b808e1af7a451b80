"""What the chains engine buys (include/dibs_hip.h, n_chains; dibs_amd.inference.sample_chains) and what it costs the standalone path,
against a checkout of the PARENT commit with its own library built, on one MI355X in one job:

    python scripts/gpu_chains_bench.py --parent-root DIR [--steps K] [--warmup W] [--out FILE] [--single-path-out FILE]

  chains        per size (LinearGaussian d = 20 / 32 particles and config-3 size d = 50 / 128 particles, DenseNonlinearGaussian (5,)
                d = 20 / 32 particles) and C = 1, 4, 16, 32: chain-steps/s of ONE chains engine of this tree against the same C runs one after
                another on the parent's standalone engine (C = 1: this tree's standalone engine).  Alternating runs, medians.  No gate: the
                ratio is the result, whichever way it falls.
  single_path   bench.py --dump-outputs of the headline config and config 3 from both trees (np.array_equal per array), and ms_per_step of
                five alternating plain bench.py runs each.  Gate: this tree's median inside the parent's [min, max] widened by (max - min)
                on either side.

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
    "lingauss_d20_m32": dict(d=20, M=32, likelihood="lingauss"),
    "lingauss_config3": dict(d=50, M=128, likelihood="lingauss"),
    "densenn5_d20_m32": dict(d=20, M=32, likelihood="densenn"),
}
CHAINS = (1, 4, 16, 32)
N_OBS, S, SA = 100, 128, 32


def _data(size):
    import numpy as np
    from dibs_amd import random
    from dibs_amd.target import make_linear_gaussian_model, make_nonlinear_gaussian_model
    f = make_linear_gaussian_model if size["likelihood"] == "lingauss" else make_nonlinear_gaussian_model
    return np.asarray(f(key=random.PRNGKey(0), n_vars=size["d"], graph_prior_str="er", n_observations=N_OBS)[0].x, np.float32)


def _timed(e, steps, warmup, reps=3):
    e.run(0, warmup)
    times, t = [], warmup
    for _ in range(reps):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    return sorted(times)[len(times) // 2]


def one(what, name, root, steps, warmup):
    """a child: every chain count of one size, as one chains engine (`chains`) or as C standalone runs (`sequential`), with the package of
    the tree `root`"""
    sys.path.insert(0, root)
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    size = SIZES[name]
    x = _data(size)
    kw = dict(n_vars=size["d"], n_particles=size["M"], n_observations=N_OBS, joint=True, likelihood=size["likelihood"], nn_hidden=(5,),
              n_grad_mc_samples=S, n_acyclicity_mc_samples=SA)
    out = {}
    for C in CHAINS:
        if what == "chains" and C > 1:
            e = Engine(make_config(n_chains=C, **kw))
            e.set_data(x)
            e.init_particles_batch(np.stack([random.PRNGKey(c) for c in range(C)]))
            el = _timed(e, steps, warmup)
            finite = bool(np.isfinite(e.get_state()["z"]).all())
            e.close()
        else:
            el, finite = 0.0, True
            for c in range(C):
                e = Engine(make_config(**kw))
                e.set_data(x)
                e.init_particles(random.PRNGKey(c))
                el += _timed(e, steps, warmup)
                finite &= bool(np.isfinite(e.get_state()["z"]).all())
                e.close()
        out[str(C)] = dict(chain_steps_per_s=C * steps / el, ms_per_step=1e3 * el / steps, finite=finite)
    return out


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(what, name, root, a):
    return _child(root, [os.path.abspath(__file__), "--one", what, "--size", name, "--root", root, "--steps", str(a.steps), "--warmup",
                         str(a.warmup)], 600)


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per side of the chains measurement")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--skip-single-path", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-path-out", default=None)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--size", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.size, a.root, a.steps, a.warmup)))
        return 0
    if not a.parent_root:
        ap.error("--parent-root is required")
    parent, ok = os.path.abspath(a.parent_root), True
    out = dict(script="scripts/gpu_chains_bench.py", steps=a.steps, warmup=a.warmup, runs=a.runs, n_observations=N_OBS, S=S, Sa=SA, sizes={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(out, indent=1))

    # 1. what the feature buys
    for name in a.sizes.split(","):
        runs = dict(sequential_parent=[], chains=[])
        for _ in range(a.runs):
            runs["sequential_parent"].append(_measure("sequential", name, parent, a))
            runs["chains"].append(_measure("chains", name, HERE, a))
        row = dict(SIZES[name])
        for C in CHAINS:
            seq = [r[str(C)]["chain_steps_per_s"] for r in runs["sequential_parent"]]
            ch = [r[str(C)]["chain_steps_per_s"] for r in runs["chains"]]
            fin = all(r[str(C)]["finite"] for side in runs.values() for r in side)
            ms, mc = statistics.median(seq), statistics.median(ch)
            row[f"C={C}"] = dict(sequential_parent_chain_steps_per_s=seq, chains_chain_steps_per_s=ch, sequential_parent_median=ms,
                                 chains_median=mc, ratio=mc / ms, finite=fin)
            ok &= fin
        out["sizes"][name] = row
        print("chains", name, json.dumps(row), flush=True)
        save()

    # 2. the standalone path
    if not a.skip_single_path:
        lines = ["Standalone path beside the chains engine (scripts/gpu_chains_bench.py; one MI355X, one job, alternating runs;",
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
