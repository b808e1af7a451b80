"""Randomised differential test (GPU box): random configurations of the SVGD step -- sizes, latent dimension, priors, estimators,
optimizer, interventions, PRNG layout, step index, model family and its hyper-parameters -- one or two steps each on the HIP
engine (through the C ABI) against the f64 C oracle from the same f32-representable state.  Prints every configuration whose Z
deviates by more than the north_star tolerance (1e-4 relative to max |Z|; DenseNN 5e-4: relu' flips) or whose sampled graphs differ.

    python tests/tools/gpu_fuzz.py [n_trials] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dibs_amd._abi import make_config          # noqa: E402
from dibs_amd.engine import Engine             # noqa: E402
from oracle import prng                        # noqa: E402
from oracle.c_oracle import COracle            # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from large_states import clustered_sparse_state   # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def graphs_from_masks(masks, M, S, d):
    gm = masks.reshape(M, d, S, -1)
    gg = np.zeros((M, S, d, d), np.uint8)
    for i in range(d):
        gg[:, :, i, :] = ((gm[:, :, :, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1)
    return gg


def draw(rng):
    fam = rng.choice(["bge", "bge", "lingauss", "densenn"])
    d = int(rng.choice([2, 3, 5, 7, 12, 16, 17, 20, 31, 32, 33, 40, 48, 49, 50, 64, 65, 80]))
    if fam == "densenn":
        d = min(d, 20)
    M = int(rng.choice([1, 2, 3, 5, 8]))
    S = int(rng.choice([1, 2, 3, 8, 16, 33])) if d > 33 else int(rng.choice([1, 2, 5, 16, 64, 128]))
    Sa = int(rng.choice([1, 2, 3, 4, 8]))
    k = int(rng.choice([d, d, max(1, d // 2), 1, d + 3])) if d <= 50 else d
    N = int(rng.choice([1, 3, 20, 100, 130])) if fam != "densenn" else int(rng.choice([3, 20, 60, 140]))
    kw = dict(n_vars=d, n_particles=M, n_observations=N, n_dim=k, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa,
              graph_prior=str(rng.choice(["er", "sf", "uniform"])), edges_per_node=0.4 if d <= 3 else (1 if d <= 9 else 2),
              optimizer=str(rng.choice(["rmsprop", "rmsprop", "gd"])), rng_layout=str(rng.choice(["legacy", "legacy", "partitionable"])),
              tau=float(rng.choice([1.0, 1.0, 0.7])), beta_linear=float(rng.choice([1.0, 0.3])),
              logistic_minval_tiny=bool(rng.random() < 0.2))
    if fam == "bge":
        # (score_function_baseline stays 0: with b > 0 the reference's estimator carries a factor exp(-baseline) ~ exp(+350) on real data,
        #  inf in float32 for the reference and the device alike -- only the f64 oracle survives it)
        kw.update(grad_estimator_z="score", score_function_baseline=0.0,
                  bge_alpha_mu=float(rng.choice([1.0, 0.5])), alpha_linear=float(rng.choice([1.0, 0.05, 0.3])))
        if rng.random() < 0.25:
            kw["bge_alpha_lambd"] = d + 2 + float(rng.choice([1.0, 3.5]))
    else:
        kw.update(joint=True, likelihood=fam, grad_estimator_z=str(rng.choice(["reparam", "score"])),
                  alpha_linear=float(rng.choice([0.05, 0.2])))
        if fam == "lingauss":
            kw.update(lin_obs_noise=float(rng.choice([0.1, 0.5])), lin_sig_edge=float(rng.choice([1.0, 2.0])), lin_mean_edge=float(rng.choice([0.0, 0.3])))
        else:
            hidden = [(5,), (8,), (4, 3), (6, 6), (70,)][int(rng.integers(5))]
            kw.update(nn_hidden=hidden, nn_activation=str(rng.choice(["relu", "tanh", "sigmoid", "leakyrelu"])), nn_bias=bool(rng.random() < 0.7),
                      nn_obs_noise=float(rng.choice([0.1, 0.4])))
    if os.environ.get("FUZZ_BIG"):   # larger particle counts / sample counts / graphs: other block splits, tiers and queue sizes
        kw["n_particles"] = int(rng.choice([16, 24, 40, 64, 128]))
        kw["n_grad_mc_samples"] = int(rng.choice([32, 64, 128]))
        kw["n_acyclicity_mc_samples"] = int(rng.choice([8, 16, 32]))
        if fam != "densenn":
            kw["n_vars"] = d = int(rng.choice([20, 40, 50, 64, 70, 96, 112]))
            kw["n_dim"] = int(rng.choice([d, d, d // 2]))
            kw["edges_per_node"] = 2
            if "bge_alpha_lambd" in kw:
                kw["bge_alpha_lambd"] = d + 2 + 1.5
        kw["n_observations"] = N = int(rng.choice([20, 100, 130]))
    if os.environ.get("FUZZ_NN") and fam == "densenn":   # per-node MLPs on larger graphs (BASELINE config 5 is d = 100)
        kw["n_vars"] = d = int(rng.choice([30, 50, 64, 65, 80, 100]))
        kw["n_dim"] = d
        kw["n_particles"] = int(rng.choice([2, 4, 8]))
        kw["n_grad_mc_samples"] = int(rng.choice([2, 8, 16]))
        kw["n_observations"] = N = int(rng.choice([20, 100, 128, 140]))
        kw["edges_per_node"] = 2
    if os.environ.get("FUZZ_PARTICLES"):   # many particles, small graphs: kernel-matrix / phi block splits, LDS table limits
        kw["n_particles"] = int(rng.choice([200, 256, 500, 1024]))
        kw["n_vars"] = d = int(rng.choice([3, 5, 8, 12, 20]))
        kw["n_dim"] = int(rng.choice([d, 2]))
        kw["n_grad_mc_samples"] = int(rng.choice([2, 8, 16]))
        kw["n_acyclicity_mc_samples"] = int(rng.choice([2, 4]))
        kw["edges_per_node"] = 0.4 if d <= 3 else (1 if d <= 9 else 2)
        kw.pop("bge_alpha_lambd", None)
        kw["n_observations"] = N = int(rng.choice([20, 100]))
    if os.environ.get("FUZZ_WIDE"):   # 113 .. 256 variables: the global-memory paths (marginal BGe, score estimator); three / four mask words
        fam = "bge"
        for k_ in ("joint", "likelihood", "lin_obs_noise", "lin_sig_edge", "lin_mean_edge", "nn_hidden", "nn_activation", "nn_bias", "nn_obs_noise"):
            kw.pop(k_, None)
        kw["n_vars"] = d = int(rng.choice([113, 120, 127, 128, 129, 144, 160, 191, 192, 193, 224, 225, 241, 255, 256]))
        kw["n_dim"] = int(rng.choice([d, d, d // 2, 40]))
        kw["n_particles"] = int(rng.choice([1, 2, 3, 6]))
        kw["n_grad_mc_samples"] = int(rng.choice([2, 5, 8, 16]))
        kw["n_acyclicity_mc_samples"] = int(rng.choice([1, 2, 4]))
        kw["edges_per_node"] = 2
        kw["n_observations"] = N = int(rng.choice([2 * d, 3 * d, d + 50]))
        kw.update(grad_estimator_z="score", score_function_baseline=0.0, bge_alpha_mu=float(rng.choice([1.0, 0.5])),
                  alpha_linear=float(rng.choice([1.0, 0.05, 0.3])))
        kw.pop("bge_alpha_lambd", None)
    if os.environ.get("FUZZ_SCALE") and fam != "bge":
        kw["n_observations"] = N = int(rng.choice([N, 200, 333, 500]))
    interv = rng.random() < 0.3 and N > 1
    kw["has_interventions"] = bool(interv)
    t = int(rng.choice([0, 1, 2, 7, 30]))
    if d > 210:   # (the sparse state of main() is sparse through alpha = alpha_linear t: the step index at which alpha = 20)
        t = int(round(20.0 / kw["alpha_linear"]))
    return fam, kw, interv, t


def main():
    n_trials = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    co = COracle("f64")
    bad = 0
    t_begin = time.time()
    for trial in range(n_trials):
        fam, kw, interv, t = draw(rng)
        d, M, S, N = kw["n_vars"], kw["n_particles"], kw["n_grad_mc_samples"], kw["n_observations"]
        x = (rng.normal(size=(N, d)) @ (np.eye(d) + 0.3 * np.triu(rng.normal(size=(d, d)), 1))).astype(np.float32)
        if os.environ.get("FUZZ_SCALE"):   # badly scaled / shifted data, more observations than the LDS-resident kernels take
            x = (x * np.float32(rng.choice([1.0, 0.05, 8.0])) + np.float32(rng.choice([0.0, 0.0, 3.0]))).astype(np.float32)
        mask = (rng.random((N, d)) < 0.15).astype(np.int32) if interv else None
        if os.environ.get("FUZZ_VERBOSE"):
            print(f"[{trial}] start t={t} {fam} " + " ".join(f"{k_}={v}" for k_, v in kw.items() if k_ != "likelihood"), flush=True)
        try:
            cfg = make_config(**kw)
            eng = Engine(cfg)
        except Exception as e:  # a documented limit of the device lowering (reported, not counted)
            print(f"[{trial}] rejected: {type(e).__name__}: {str(e)[:90]}   {fam} d={d}")
            continue
        mean_obs = rng.normal(size=d).astype(np.float32) if (fam == "bge" and os.environ.get("FUZZ_SCALE") and rng.random() < 0.5) else None
        eng.set_data(x, mask, mean_obs)   # (BGe prior mean: linearGaussian.py:35-48)
        st = co.new_state(cfg, prng.PRNGKey(int(rng.integers(1 << 30))))
        # RMSprop from v = 0 moves EVERY coordinate by ~3.2 stepsize in the direction of sign(phi): coordinates whose phi is below the float32
        # noise of the sum get a coin flip (in the reference as well).  A trajectory starts at t = 0 with a clean prior gradient; a trial
        # that starts in the middle gets a unit second-moment estimate instead.
        st["v_z"] = np.ones_like(st["v_z"])
        if d > 210:
            # fresh particles have soft graphs around 1/2 and (I + G/d)^(d-1) ~ 1.5^d leaves float32 near d = 220: a trial would compare
            # infinities.  Sparse, neighbouring particles instead (tests/large_states.py; its own seeded generator: `rng` is not touched)
            st["z"] = clustered_sparse_state(st["z"], 0.6, 2.0, seed=trial)
        if st.get("v_theta") is not None:
            st["v_theta"] = np.ones_like(st["v_theta"])
        worst, note = 0.0, ""
        for step in (t, t + 1):
            if np.abs(st["z"]).max() > 1e15:
                # a plain gradient-descent step on phi ~ 1e20 (wide graphs: tr((I + G/d)^d) ~ 1.5^d) leaves Z where U V^T overflows float32;
                # only the f64 oracle can continue from there
                note += " (state beyond the float32 range: second step skipped)"
                break
            for name in ("z", "v_z", "baseline", "theta", "v_theta"):
                if st.get(name) is not None:
                    st[name] = st[name].astype(np.float32).astype(np.float64)
            sk = dict(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
            if st.get("theta") is not None:
                sk.update(theta=st["theta"], v_theta=st["v_theta"])
            eng.set_state(**sk)
            dbg = co.step(cfg, x, mask, st, step, debug=True, mean_obs=mean_obs)
            eng.run(step, 1)
            g = eng.get_state()
            e = rel(g["z"], st["z"])
            if st.get("theta") is not None:
                e = max(e, rel(g["theta"], st["theta"]))
            phi_rel = rel(eng.read("PHI_Z"), dbg["phi_z"])
            if 0.1 * float(np.abs(dbg["phi_z"]).max()) ** 2 > 1e37 and phi_rel < 1e-4:
                # n_vars >= 128: tr((I + G/d)^d) of dense soft graphs grows like 1.5^d and phi^2 leaves the float32 range in RMSprop's second
                # moment (for the reference's float32 arithmetic too): the comparison ends with phi
                e, note = min(e, 0.0), note + f" (phi up to {np.abs(dbg['phi_z']).max():.1e}, phi^2 beyond float32: phi compared, rel {phi_rel:.1e})"
            elif cfg.optimizer == 1 and np.abs(dbg["phi_z"]).max() > 50.0 and phi_rel < 2e-5:
                # RMSprop normalises every coordinate to a step of ~stepsize / sqrt(0.1): coordinates whose phi lies below the float32 noise
                # of the largest one (|phi|_max * 1e-6) move by a full step in a direction decided by rounding -- in the reference too.
                # The transform itself is compared instead.
                e, note = min(e, 0.0), note + f" (phi up to {np.abs(dbg['phi_z']).max():.1e}: phi compared, rel {phi_rel:.1e})"
            if np.abs(dbg["scores"]).max() * cfg.alpha_linear * max(step, 1) > 15.0:
                # soft graphs within float rounding of 0 / 1: g (1 - g) is rounding noise times matrix-power entries, for the reference's
                # float32 arithmetic as for the device's (plain gradient descent with a one-dimensional latent space gets there in 2 steps)
                e, note = min(e, 0.0), note + " (saturated: Z not compared)"
            if not np.isfinite(g["z"]).all():
                if np.abs(dbg["phi_z"]).max() > 1e33 or np.abs(dbg["w_acyc"]).max() > 1e33:
                    # matrix-power entries of (I + G/d)^(d-1) ~ 1.5^d / d beyond ~1e33 overflow in float32 products (d >= ~200): inf * 0 = NaN
                    # for the reference's float32 arithmetic as for the device's
                    e, note = min(e, 0.0), note + " (acyclicity term beyond the float32 range: not compared)"
                else:
                    e, note = float("inf"), note + " non-finite"
            # stage buffers are compared in EVERY trial, also where Z is not (saturation, Bernoulli boundary flips, phi-only comparisons):
            # the deterministic stages always, the estimator stages wherever their inputs are the oracle's
            stage = {"SCORES": (rel(eng.read("SCORES"), dbg["scores"]), 5e-6), "KXX": (rel(eng.read("KXX"), dbg["kxx"]), 2e-5)}
            same_s = None   # [M, S]: sampled graph identical to the oracle's (BGe; the other families draw no Bernoulli graphs for Z)
            if fam == "bge":
                # a Bernoulli draw flips where the uniform falls between the float32 and the float64 value of sigmoid(alpha s): a handful of
                # the M S d^2 bits at the larger sizes (for the reference's float32 arithmetic against the f64 oracle as well)
                gg = graphs_from_masks(eng.read("PARENT_MASKS"), kw["n_particles"], kw["n_grad_mc_samples"], kw["n_vars"])
                nflip = int((gg != dbg["g_samples"]).sum())
                same_s = (gg == dbg["g_samples"]).all(axis=(2, 3))
                # (a draw flips when its 23-bit uniform falls between the float32 and the float64 threshold, |p32 - p64| <~ 2^-24: about
                #  gg.size 2^-24 flips are expected; 2 + 8 x that many are excused -- 3 of 12.8 M draws, not round 5's 1e-5 of them)
                if nflip > 2 + int(8 * gg.size * 2.0 ** -23):
                    note += f" graphs-differ({nflip} of {gg.size})"
                elif nflip:
                    e, note = min(e, 0.0), note + f" ({nflip} Bernoulli boundary flips of {gg.size}: Z not compared)"
                # node scores of the samples whose graph is the oracle's, entry by entry, to the bound of test_marginal_bge_step_stages
                # (relative to the largest score: fp32 Cholesky pivots, the log-det error multiplied by (N + alpha_lambd - d + l) / 2)
                ns_d = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1)[same_s]   # device layout [m][j][s]
                ns_o = np.asarray(dbg["node_scores"], np.float64)[same_s]
                if ns_o.size and np.isfinite(ns_o).all():
                    stage["NODE_SCORES"] = (float(np.abs(ns_d - ns_o).max() / max(np.abs(ns_o).max(), 1e-300)),
                                            1e-4 if d <= 50 else (5e-4 if d <= 112 else 1e-3))
            lp_d, lp_o = eng.read("LOGPROBS_Z").reshape(M, S), np.asarray(dbg["logprobs_z"], np.float64).reshape(M, S)
            sel = np.ones((M, S), bool) if same_s is None else same_s
            if fam != "bge" and kw.get("grad_estimator_z") == "score" and np.isfinite(lp_o).all():
                # the joint models' score estimator draws hard graphs as well (threshold from the float32 sigmoid on the device, the float64 one in
                # the oracle) and those graphs cannot be read back: a handful of samples whose log-probability is off while all others agree to
                # 1e-3 of the largest are Bernoulli boundary flips, as above (seed 902 trial 6 of FUZZ_BIG: one of 5 120 samples, on every
                # device kernel and on round 4's library alike)
                off = np.abs(lp_d - lp_o) > 1e-3 * max(np.abs(lp_o).max(), 1e-300)
                if 0 < off.sum() <= 2 + int(8 * M * S * d * d * 2.0 ** -23):   # (expected threshold ties, as above -- an absolute handful, not a share of the samples)
                    sel = sel & ~off
                    e, note = min(e, 0.0), note + f" ({int(off.sum())} of {M * S} samples off in log-probability: Bernoulli boundary flips, Z not compared)"
            if sel.any() and np.isfinite(lp_o[sel]).all():
                # (a net for gross errors in trials whose Z is not compared: the suite holds 2e-5 on ordinary states; a state 30 steps into a
                #  badly scaled run -- phi ~ 1e10 -- showed 2.5e-4 with phi itself at 3e-6)
                stage["LOGPROBS_Z"] = (float(np.abs(lp_d - lp_o)[sel].max() / max(np.abs(lp_o[sel]).max(), 1e-300)), 1e-3)
            # (log-scores beyond 2^23: their float32 spacing exceeds 1, so the softmax weights over the samples are not determined in float32 --
            #  seed 911 trial 89: gradient descent blown up to |scores| ~ 1e6, log-scores ~ 1.5e9 equal to 1.4e-7, W_LIK 10 % apart)
            lp_resolved = np.isfinite(lp_o).all() and np.abs(lp_o).max() < 8.0e6
            if lp_resolved and (same_s is None or same_s.all()) and np.isfinite(dbg["w_lik"]).all() and np.abs(dbg["w_lik"]).max() > 0:
                # (softmax-weighted: a near-tie of two log-scores moves single entries by O(alpha); the RMS over the matrix catches a wrong kernel)
                wd, wo = eng.read("W_LIK").astype(np.float64).ravel(), np.asarray(dbg["w_lik"], np.float64).ravel()
                # (saturated graphs: every sample equals P, so W_lik = alpha (sum_s w_s - 1) P is rounding noise around 0 -- 1e-16 alpha in the
                #  f64 oracle, 6e-8 alpha in float32: the scale has a floor)
                a_t = abs(cfg.alpha_linear * step)
                stage["W_LIK"] = (float(np.sqrt(np.mean((wd - wo) ** 2)) / max(np.sqrt(np.mean(wo ** 2)), 1e-5 * max(a_t, 1.0))), 5e-2)
            for name, (err, lim) in stage.items():
                if not err <= lim:
                    e, note = max(e, 1.0), note + f" stage-differs({name} {err:.1e} > {lim:.0e})"
            if not (g["key"] == st["key"]).all():
                note += " key-differs"
            worst = max(worst, e)
        eng.close()
        tol = 5e-4 if fam == "densenn" else 1e-4
        flag = worst > tol or (note and "differ" in note) or "non-finite" in note
        if flag:
            bad += 1
        if flag or trial % 20 == 0:
            print(f"[{trial}] {'FAIL' if flag else 'ok  '} rel {worst:.2e}{note}  t={t} {fam} " + " ".join(f"{k_}={v}" for k_, v in kw.items() if k_ not in ("likelihood",)), flush=True)
    print(f"{n_trials} trials, {bad} outside tolerance, {time.time() - t_begin:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
