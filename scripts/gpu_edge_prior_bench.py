"""What the edge-wise graph prior costs, and that the paths beside it are what they were.  One MI355X, one job:

    python scripts/gpu_edge_prior_bench.py [--parent-root DIR] [--out FILE]

table_cost   the headline workload of bench.py (MarginalDiBS + BGe, d = 50, 128 particles) with the Erdos-Renyi prior and with the
             edge-wise prior on a table that holds the Erdos-Renyi probability in every entry -- the same arithmetic, k_particle_grad against
             k_particle_grad_edge -- on THIS tree: `--runs` alternating child processes per side (an engine alone in its process takes the
             schedule of the headline), each the median ms/step of three windows of `--steps` steps behind `--warmup`; medians and ratio.
             No gate: the number is written down.
single_path  with --parent-root (a checkout of the parent commit with its library built): `bench.py --dump-outputs` of the headline config
             and of config 3 against the parent's, array for array, and ms_per_step of five alternating runs per side; the gate is this
             tree's median inside the parent's [min, max] widened by (max - min) on either side.  Exit status 1 if a dump differs or a
             median lies outside.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(prior, steps, warmup):
    sys.path.insert(0, HERE)
    import numpy as np
    import bench
    from dibs_amd import random
    from dibs_amd.engine import Engine
    from dibs_amd.models import ErdosReniDAGDistribution
    cfg, x, mask = bench.make_workload("headline", bench.CONFIGS["headline"]["M"])
    d = cfg.n_vars
    if prior == "edgewise":
        from dibs_amd._abi import PRIOR
        cfg.graph_prior = PRIOR["edgewise"]
    e = Engine(cfg)
    e.set_data(x, mask)
    if prior == "edgewise":
        e.set_edge_prior(np.full((d, d), ErdosReniDAGDistribution(d, cfg.graph_prior_edges_per_node).p))
    e.init_particles(random.PRNGKey(0))
    e.run(0, warmup)
    ms, t = [], warmup
    for _ in range(3):
        t0 = time.perf_counter()
        e.run(t, steps)
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
        t += steps
    z = e.get_state()["z"]
    e.close()
    print(json.dumps(dict(prior=prior, ms_per_step=statistics.median(ms), windows=ms, finite=bool(np.isfinite(z).all()),
                          z_sum=float(np.abs(z.astype(np.float64)).sum()))))


def _child(root, argv, timeout=600):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(argv)} in {root}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _bench(root, config, a, dump=None):
    argv = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--config", config]
    return _child(root, argv + (["--dump-outputs", dump] if dump else []))


def _same_dumps(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and len(fa) > 0 and all(np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))) for f in fa), fa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built (single_path)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "edge_prior_single_path_check.txt"))
    ap.add_argument("--one", choices=["er", "edgewise"])
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.steps, a.warmup)
    ok, lines = True, []

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        lines += ["Untouched paths beside the edge-wise graph prior (scripts/gpu_edge_prior_bench.py; one MI355X, one job, alternating runs;",
                  f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}):"]
        for config in ("headline", "3"):
            with tempfile.TemporaryDirectory() as dp, tempfile.TemporaryDirectory() as dt:
                _bench(parent, config, a, dp)
                _bench(HERE, config, a, dt)
                same, files = _same_dumps(dp, dt)
            ms = dict(parent=[], this=[])
            for _ in range(5):
                ms["parent"].append(_bench(parent, config, a)["ms_per_step"])
                ms["this"].append(_bench(HERE, config, a)["ms_per_step"])
            lo, hi, med = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["this"])
            bound = [lo - (hi - lo), hi + (hi - lo)]
            within = bound[0] <= med <= bound[1]
            ok = ok and same and within
            lines += [f"  config {config}:", f"    --dump-outputs, parent vs this change: {', '.join(files)} np.array_equal: {same}",
                      "    (five alternating runs)",
                      "    ms_per_step parent:      " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"   (min {lo:.4f}, max {hi:.4f})",
                      "    ms_per_step this change: " + " ".join(f"{v:.4f}" for v in ms["this"]) + f"   (median {med:.4f}: "
                      + ("inside" if within else "OUTSIDE") + f" the parent's min-max widened by its spread, [{bound[0]:.4f}, {bound[1]:.4f}])"]
            save()
    me = os.path.abspath(__file__)
    ms = dict(er=[], edgewise=[])
    sums = set()
    for _ in range(a.runs):
        for prior in ("er", "edgewise"):
            r = _child(HERE, [me, "--one", prior, "--steps", str(a.steps), "--warmup", str(a.warmup)])
            ms[prior].append(r["ms_per_step"])
            sums.add(r["z_sum"])
            ok = ok and r["finite"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines += [f"Cost of the table form: the headline workload (d = 50, 128 particles), {a.runs} alternating runs per side, each the median of three",
              f"windows of {a.steps} steps behind {a.warmup}; the edge-wise table holds the Erdos-Renyi probability in every entry:",
              "    ms_per_step Erdos-Renyi prior (k_particle_grad):      " + " ".join(f"{v:.4f}" for v in ms["er"]) + f"   (median {med['er']:.4f})",
              "    ms_per_step edge-wise prior (k_particle_grad_edge):   " + " ".join(f"{v:.4f}" for v in ms["edgewise"]) + f"   (median {med['edgewise']:.4f})",
              f"    edge-wise / Erdos-Renyi: {med['edgewise'] / med['er']:.4f}; final particles of all {2 * a.runs} runs equal: {len(sums) == 1}"]
    save()
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
