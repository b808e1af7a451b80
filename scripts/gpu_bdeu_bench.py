"""What MarginalDiBS with the BDeu likelihood on discrete data costs (include/dibs_hip.h, BDEU), what the change
costs the paths that do not use it, and what the posterior looks like, on one MI355X in one job:

    python scripts/gpu_bdeu_bench.py [--parent-root DIR] [--out FILE] [--single-path-out FILE] [--posterior-out FILE]

  cost          per size -- config-2 size (d = 20, 32 particles, N = 100), the headline size (d = 50, 128 particles, N = 100) and
                d = 11, 32 particles, N = 1 000, all of arity 3 -- steps/s of the BDeu engine beside the BGe engine of the same sizes on
                Gaussian data.  Alternating runs, medians and ranges.  No gate: nobody had measured this kernel.  Then one run per side
                with per-kernel timing (dibs_engine_set_profiling(1): every kernel alone on the GPU): microseconds per step and kernel
                family; k_bdeu_nodes is reported in k_bge_chol's slot, "bge_big".
  high_bits     one scoring call whose parents' fields are the top bits of the key word: d = 30, arity 4, N = 1 024, columns 24 .. 29 the
                base-4 digits of a permutation of the rows (1 024 configurations in bits 48 .. 59); 128 graphs in which every node's
                parents are columns 24 .. 29, beside the same call with parents 0 .. 5 (random columns, low bits).  Milliseconds per
                dibs_score_graphs call (3 840 problems; host mask building and the copy of the result included), median of seven.
                A record: what the table's slot function costs where the old one clustered.
  single_path   with --parent-root (a checkout of the parent commit with its library built): bench.py --dump-outputs of the headline
                config and config 3 from both trees (np.array_equal per array), and ms_per_step of five alternating plain bench.py runs
                each.  Gate: this tree's median inside the parent's [min, max] widened by (max - min) on either side.
  posterior     with --posterior-out: three make_discrete_model problems (d = 10, arity 3, N = 500), 16 particles, 1 000 steps; the
                expected structural Hamming distance of get_mixture beside the empty graph's distance.  A record, not a gate.

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
    "config2_d20_m32_n100": dict(d=20, M=32, N=100),
    "headline_d50_m128_n100": dict(d=50, M=128, N=100),
    "d11_m32_n1000": dict(d=11, M=32, N=1000),
}
ARITY, S, SA = 3, 128, 32


def _engine(size, lik):
    import numpy as np
    from dibs_amd import random
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    from dibs_amd.target import make_discrete_model, make_linear_gaussian_equivalent_model
    kw = dict(n_vars=size["d"], n_particles=size["M"], n_observations=size["N"], n_grad_mc_samples=S, n_acyclicity_mc_samples=SA)
    if lik == "bdeu":
        data, _, lm = make_discrete_model(key=random.PRNGKey(0), n_vars=size["d"], arities=ARITY, n_observations=size["N"])
        e = Engine(make_config(likelihood="bdeu", **kw))
        e.set_arities(lm.arities)
    else:
        data = make_linear_gaussian_equivalent_model(key=random.PRNGKey(0), n_vars=size["d"], graph_prior_str="er", n_observations=size["N"])[0]
        e = Engine(make_config(**kw))
    e.set_data(np.asarray(data.x, np.float32))
    e.init_particles(random.PRNGKey(0))
    return e


def one(lik, name, steps, warmup, timers):
    """a child: one size with one likelihood; `timers`: a further window with per-kernel timing"""
    import numpy as np
    e = _engine(SIZES[name], lik)
    e.run(0, warmup)
    times, t = [], warmup
    for _ in range(3):
        t0 = time.perf_counter()
        e.run(t, steps)
        times.append(time.perf_counter() - t0)
        t += steps
    el = sorted(times)[1]
    out = dict(steps_per_s=steps / el, ms_per_step=1e3 * el / steps, finite=bool(np.isfinite(e.get_state()["z"]).all()))
    if timers:
        e.set_profiling(1)
        e.reset_timers()
        e.run(t, steps)
        out["us_per_step_by_kernel"] = {k: 1e3 * ms / steps for k, (ms, n) in e.timers().items()}
    e.close()
    return out


def high_bits():
    """a child: the scoring call on top-bit parents and on low-bit parents"""
    import numpy as np
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.models import BDeu
    d, N, n = 30, 1024, S
    rng = np.random.default_rng(0)
    x = rng.integers(0, 4, size=(N, d))
    digits = rng.permutation(N)
    for i in range(24, 30):
        x[:, i] = digits % 4
        digits = digits // 4
    x = x.astype(np.float32)
    lm = BDeu(n_vars=d, arities=4)
    out = {}
    for name, pa in (("parents_24_29", range(24, 30)), ("parents_0_5", range(0, 6))):
        g = np.zeros((d, d), np.int32)
        g[list(pa), :] = 1
        g[np.arange(d), np.arange(d)] = 0
        gs = np.ascontiguousarray(np.broadcast_to(g, (n, d, d)))
        score_graphs(lm, gs, None, x)                                  # (packs the rows, builds the engine)
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            v = score_graphs(lm, gs, None, x)
            times.append(1e3 * (time.perf_counter() - t0))
        out[name] = dict(ms_per_call=sorted(times)[3], min_ms=min(times), max_ms=max(times), problems=d * n, score=float(v[0]))
    return out


def posterior(seed, steps):
    """a child: one discrete problem; E-SHD of the mixture after `steps` steps beside the empty graph's SHD"""
    import numpy as np
    from dibs_amd import random
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.metrics import expected_shd
    from dibs_amd.target import make_discrete_model
    data, gm, lm = make_discrete_model(key=random.PRNGKey(seed), n_vars=10, arities=ARITY, n_observations=500)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    t0 = time.perf_counter()
    g = m.sample(key=random.PRNGKey(100 + seed), n_particles=16, steps=steps)
    el = time.perf_counter() - t0
    dist = m.get_mixture(g)
    return dict(seed=seed, true_edges=int(np.asarray(data.g).sum()), eshd_mixture=float(expected_shd(dist=dist, g=data.g)),
                shd_empty_graph=int(np.asarray(data.g).sum()), mean_edges_of_particles=float(g.sum(axis=(1, 2)).mean()), seconds=el)


def _child(root, argv, timeout):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _measure(lik, name, a, timers=False):
    return _child(HERE, [os.path.abspath(__file__), "--one", lik, "--size", name, "--steps", str(a.steps), "--warmup", str(a.warmup)]
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
    ap.add_argument("--posterior-out", default=None)
    ap.add_argument("--posterior-steps", type=int, default=1000)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--size", help=argparse.SUPPRESS)
    ap.add_argument("--posterior-seed", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--timers", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--high-bits", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        sys.path.insert(0, HERE)
        print(json.dumps(one(a.one, a.size, a.steps, a.warmup, a.timers)))
        return 0
    if a.high_bits:
        sys.path.insert(0, HERE)
        print(json.dumps(high_bits()))
        return 0
    if a.posterior_seed is not None:
        sys.path.insert(0, HERE)
        print(json.dumps(posterior(a.posterior_seed, a.posterior_steps)))
        return 0
    ok = True
    out = dict(script="scripts/gpu_bdeu_bench.py", steps=a.steps, warmup=a.warmup, runs=a.runs, arity=ARITY, S=S, Sa=SA, sizes={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(out, indent=1))

    # 1. what the new path costs
    for name in [n for n in a.sizes.split(",") if n]:
        runs = dict(bge=[], bdeu=[])
        for _ in range(a.runs):
            for lik in runs:
                runs[lik].append(_measure(lik, name, a))
        row = dict(SIZES[name])
        for lik, rs in runs.items():
            v = [r["steps_per_s"] for r in rs]
            row[lik] = dict(steps_per_s=v, median_steps_per_s=statistics.median(v), min_steps_per_s=min(v), max_steps_per_s=max(v))
            ok &= all(r["finite"] for r in rs)
        row["bdeu_over_bge"] = row["bdeu"]["median_steps_per_s"] / row["bge"]["median_steps_per_s"]
        row["us_per_step_by_kernel"] = {lik: _measure(lik, name, a, timers=True)["us_per_step_by_kernel"] for lik in runs}
        row["k_bdeu_nodes_us_per_step"] = row["us_per_step_by_kernel"]["bdeu"].get("bge_big")
        out["sizes"][name] = row
        print("cost", name, json.dumps(row), flush=True)
        save()

    out["high_bits"] = dict(d=30, arity=4, N=1024, graphs=S, **_child(HERE, [os.path.abspath(__file__), "--high-bits"], 600))
    print("high_bits", json.dumps(out["high_bits"]), flush=True)
    save()

    # 2. the posterior record
    if a.posterior_out:
        rows = [_child(HERE, [os.path.abspath(__file__), "--posterior-seed", str(seed), "--posterior-steps", str(a.posterior_steps)], 900)
                for seed in (0, 1, 2)]
        out["posterior"] = rows
        lines = [f"MarginalDiBS + BDeu on make_discrete_model problems (scripts/gpu_bdeu_bench.py; d = 10, arity 3, N = 500, 16 particles, "
                 f"{a.posterior_steps} steps, defaults otherwise).",
                 "E-SHD of get_mixture(sample()) against the ground-truth DAG, beside the SHD of the empty graph (= the true edge count).",
                 "A record, not a gate."]
        for r in rows:
            lines.append(f"  problem key {r['seed']}: true edges {r['true_edges']:2d}   E-SHD of the mixture {r['eshd_mixture']:6.2f}   SHD of the empty graph "
                         f"{r['shd_empty_graph']:2d}   mean edges per particle {r['mean_edges_of_particles']:.1f}   {r['seconds']:.1f} s")
        os.makedirs(os.path.dirname(os.path.abspath(a.posterior_out)), exist_ok=True)
        open(a.posterior_out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)
        save()

    # 3. the paths that do not use the new likelihood
    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        lines = ["BGe and joint paths beside the BDeu likelihood (scripts/gpu_bdeu_bench.py; one MI355X, one job, alternating runs;",
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
