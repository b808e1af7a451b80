"""The softmax-weighted gradient kernels (k_lin_grad, k_ling_grad, k_nn_grad, k_nng_grad; kernels_joint.h: GradSplit) across the weight
range, on the constructed states of tests/weight_states.py: a chosen number of samples above the 2^-30 cut, samples below it and
underflowing ones interleaved with them, weights on either side of the cut.

Spread weights turn the 2e-5 of the LOGPROBS stage into per cents of a weight, which would hide the gradient kernel behind the
log-probability kernel.  So the reference takes the log-probabilities as given: w = float32(float64 softmax of the DEVICE's LOGPROBS),
membership w >= 2^-30, and the per-sample terms g_s of the autograd oracle (oracle.dibs_oracle.likelihood_sample_terms):
  kept sum      dev against sum_kept w_s g_s within the stage bounds of the step tests (conftest.stage_err): GRAD_THETA 5e-4, W_LIK 2e-3
  every sample  on the free edges' coordinates of GRAD_THETA and of the reparam W_LIK: |dev_e - ref_e| <= 5e-4 sum_kept w_s |g_se| -- the
                forward-error form of a sum with the project's constant.  These coordinates are fed by the low-weight samples alone, so
                a lost, doubled or misdealt sample shows.  (Z score: W = alpha (sum w G - P); the term -p_e swamps these coordinates,
                the kept-sum bound is what holds there.)
  the cut       |sum_dropped w_s g_s|_inf / |sum_all|_inf is printed per particle; <= 1e-6 on the ladder profiles is asserted by
                tests/test_weight_states_host.py on the reference alone.
The comparison with the C oracle's own step (its own log-probabilities) is asserted with the same bounds where one sample has all the
weight and printed elsewhere: its weights differ by the amplified LOGPROBS error wherever more than one sample counts."""
import numpy as np
import pytest

import weight_states as W
from conftest import rel_err, stage_err
from dibs_amd._abi import make_config

pytestmark = pytest.mark.gpu


def _run(b, monkeypatch, theta=None):
    from dibs_amd.engine import Engine
    if b["gram"]:
        monkeypatch.setenv("DIBS_LIN_GRAM", "1")   # (latched when the engine is created: tuning.h)
    eng = Engine(make_config(**b["cfg_kw"]))
    eng.set_data(b["x"], b["mask"])
    eng.set_state(**dict(W.fresh_state(b), **({} if theta is None else dict(theta=theta))))
    eng.run(b["t"], 1)
    M, S = b["M"], b["S"]
    out = dict(key=eng.get_state()["key"], lp_theta=eng.read("LOGPROBS_THETA").reshape(M, S), lp_z=eng.read("LOGPROBS_Z").reshape(M, S),
               theta=eng.read("GRAD_THETA").reshape(M, -1), z=eng.read("W_LIK").reshape(M, -1))
    eng.close()
    return out


@pytest.mark.parametrize("case", W.GRAD_CASES, ids=W.case_id)
def test_gradient_kernels_on_weight_profiles(c_oracle64, monkeypatch, case):
    b = W.build(case, c_oracle64)
    if b["M"] > 6:   # the case with more (particle, share) items than k_nn_grad has resident blocks (at most two per CU)
        import torch
        assert b["M"] * b["ns"] > 2 * torch.cuda.get_device_properties(0).multi_processor_count and b["M"] <= 255
    _check(b, _run(b, monkeypatch))


def _check(b, dev, skip=()):
    """every assertion of the module on the particles not in `skip`"""
    dbg, M, S, ns = b["dbg"], b["M"], b["S"], b["ns"]
    rows = [m for m in range(M) if m not in skip]
    # keys bit-exact; the sampled graphs with them: one differing free-edge bit moves a log-probability by a rung of the ladder
    assert np.array_equal(dev["key"], b["after"]["key"])
    assert rel_err(dev["lp_theta"][rows], dbg["logprobs_th"][rows]) < 2e-5
    assert rel_err(dev["lp_z"][rows], dbg["logprobs_z"][rows]) < 2e-5
    alpha = make_config(**b["cfg_kw"]).alpha_linear * b["t"]
    for name, lps, stage, tol in (("theta", dev["lp_theta"], "GRAD_THETA", 5e-4), ("z", dev["lp_z"], "W_LIK", 2e-3)):
        w = W.weights32(lps)
        ref = np.zeros_like(dev[name], dtype=np.float64)
        fc = W.free_coords(b, name)
        counts, shares, free_err = {}, [], []
        for m in rows:
            s = W.weighted_sums(b, name, m, w[m])
            ref[m, :s["kept"].size] = s["kept"]
            if name == "z" and b["est"] == "score":
                # the device subtracts P once, the reference sum_kept w times: alpha P sum_dropped w (1e-8 of the stage) is added back
                p = 1.0 / (1.0 + np.exp(-alpha * np.asarray(b["z"][m, :, :, 0], np.float64)))
                np.fill_diagonal(p, 0.0)
                ref[m] -= alpha * p.reshape(-1) * (1.0 - float(np.asarray(w[m], np.float64)[w[m] >= np.float32(W.CUT)].sum()))
            counts[m] = s["nnz"]
            shares.append(np.abs(s["dropped"]).max() / max(np.abs(s["kept"] + s["dropped"]).max(), 1e-300))
            prof = b["profile"][name][m]
            if prof["near"] == 0:   # (straddle and the margin-free profiles: membership is the device's, the count is not predicted)
                assert W.classify(s["nnz"], S, ns) == W.classify(prof["nnz"], S, ns) and s["nnz"] == prof["nnz"], (name, m, s["nnz"], prof)
                if b["t_th"][m] != "straddle":   # the cut, with the device's weights (the host test has it with the oracle's)
                    assert shares[-1] <= 1e-6, (name, m, shares[-1])
            if name == "theta" or b["est"] == "reparam":
                err = np.abs(dev[name][m, fc].astype(np.float64) - ref[m, fc])
                bound = 5e-4 * s["abs"][fc]
                free_err.append(float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0)
                assert (err <= bound).all(), (name, m, err, bound)
        print(f"\n  {b['id']} {name}: participation {list(counts.values())} | cut share {' '.join(f'{v:.1e}' for v in shares)}"
              + (f" | free-edge error / bound {' '.join(f'{v:.2f}' for v in free_err)}" if free_err else ""))
        for m in rows:
            stage_err(f"{stage}[{m}] kept sum", dev[name][m], ref[m], tol)
        # the C oracle's own step: asserted where one sample has all the weight (the weights are then 1 and 0 whatever the 2e-5 of the
        # log-probabilities), printed elsewhere -- a flat profile too has weights exp(log p), off by the ABSOLUTE error of log p
        full = np.asarray(dbg["grad_theta"] if name == "theta" else dbg["w_lik"]).reshape(M, -1)[:, :dev[name].shape[1]]
        for m in rows:
            if counts[m] == 1 and b["profile"][name][m]["near"] == 0 and b["t_th"][m] != "straddle":
                stage_err(f"{stage}[{m}] C oracle step", dev[name][m], full[m], tol)
            else:
                print(f"  {stage}[{m}] against the C oracle's own step (not asserted, {counts[m]} samples): {rel_err(dev[name][m], full[m]):.2e}")


@pytest.mark.parametrize("case", [c for c in W.GRAD_CASES if c["S"] == 64 and c["N"] == 40 and c["d"] == 8 or c["kernel"] == "k_nng_grad"], ids=W.case_id)
def test_non_finite_log_probabilities_propagate(c_oracle64, monkeypatch, case):
    """One particle has +inf in a parameter of an edge of G*: every sample's log-probability is non-finite, and so is the reference's
    gradient for that particle.  All four kernels take part with the ONE predicate !(w < GRAD_W_MIN) (kernels_joint.h), which a NaN weight
    passes: the particle's GRAD_THETA and W_LIK are non-finite -- never a silent zero -- and every other particle meets the bounds above.
    (d = 8 for k_lin_grad, k_ling_grad and k_nn_grad; the two-hidden-layer cases of k_nng_grad are the d = 12 ones of this module.)"""
    b = W.build(case, c_oracle64)
    d = b["d"]
    i, j = np.argwhere(np.asarray(b["g0"]) != 0)[0]
    theta = np.array(b["theta"], np.float32)
    H = 1 if b["model"] == "lingauss" else b["cfg_kw"]["nn_hidden"][0]
    theta[0, (i * d + j) if b["model"] == "lingauss" else (j * d + i) * H] = np.inf
    dev = _run(b, monkeypatch, theta=theta)
    assert not np.isfinite(dev["lp_theta"][0]).any() and not np.isfinite(dev["lp_z"][0]).any()
    for name in ("theta", "z"):
        assert not np.isfinite(dev[name][0]).all(), (name, dev[name][0])
        assert np.isfinite(dev[name][1:]).all(), name
    _check(b, dev, skip=(0,))
