"""Float64 engine against the float32 engine on the same commit (include/dibs_hip.h, dibs_config.reserved_i[1] = 64): steps/s of
MarginalDiBS + BGe at BASELINE config 2 (d = 20, 32 particles) and the headline size (d = 50, 128 particles), bench.py's data and sizes,
after W untimed warm-up steps; the median of three timed chunks of K steps, then each kernel's time alone on the GPU over K more steps
(the engine's serialised profiling timers).  Writes profiles/f64_bench.json (--out).

    timeout -k 10 600 python scripts/gpu_f64_bench.py [--steps K] [--warmup W] [--only NAME] [--out PATH]

--only headline64 runs one case (for a rocprofv3 --kernel-trace --stats run of the f64 headline step) and writes nothing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench import CONFIGS, make_workload  # noqa: E402
from dibs_amd import random  # noqa: E402
from dibs_amd.engine import Engine  # noqa: E402

CASES = [("config2", "2", 32), ("config2", "2", 64), ("headline", "headline", 32), ("headline", "headline", 64)]


def run_case(cfg_name, prec, K, W):
    cfg, x, mask = make_workload(cfg_name, CONFIGS[cfg_name]["M"])
    cfg.reserved_i[1] = 0 if prec == 32 else 64
    eng = Engine(cfg)
    eng.set_data(np.asarray(x, np.float64) if prec == 64 else x, mask)
    eng.init_particles(random.PRNGKey(1))
    eng.run(0, W)
    times = []
    t = W
    for _ in range(3):
        t0 = time.perf_counter()
        eng.run(t, K)
        times.append(time.perf_counter() - t0)
        t += K
    # per-kernel times of the same kind of steps, each kernel alone on the GPU (dibs_engine_set_profiling(1): event pairs, the step
    # serialised), steps t .. t + K - 1 right after the timed ones
    eng.set_profiling(1)
    eng.reset_timers()
    eng.run(t, K)
    kern = {k: round(ms / K, 4) for k, (ms, n) in eng.timers().items()}
    kern["steps"] = f"t={t}..{t + K - 1}"
    eng.close()
    return K / float(np.median(times)), kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_bench.json"))
    a = ap.parse_args()
    res = {}
    for label, name, prec in CASES:
        key = f"{label}{prec}"
        if a.only and key != a.only:
            continue
        sps, kern = run_case(name, prec, a.steps, a.warmup)
        res[key] = dict(config=CONFIGS[name]["label"], precision=prec, steps_per_s=round(sps, 1), ms_per_step=round(1e3 / sps, 3),
                        kernel_ms_per_step_alone=kern)
        print(key, res[key], flush=True)
    if a.only:
        return
    for label in ("config2", "headline"):
        res[f"{label}_f64_over_f32_time"] = round(res[f"{label}32"]["steps_per_s"] / res[f"{label}64"]["steps_per_s"], 2)
    res["method"] = (f"one engine per case, {a.warmup} untimed steps, then three chunks of {a.steps} steps (dibs_engine_run, blocking); "
                     "median chunk time; float32 and float64 on the same commit and GPU")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
