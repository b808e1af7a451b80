"""The soft-graph BGe kernels (k_bge_soft_mf<NB, RL, 3>, k_bge_soft<RL, 2>, k_bge_soft<false, 4, true>, k_soft_combine;
dibs_amd/csrc/tu_bge_soft.hip) across the range of the parent weights, on the constructed states of tests/soft_states.py: saturated
backbones with a handful of free edges that carry the whole gradient, parents with p down to 1e-7 and below 1e-20, exact zeros and ones,
p near 1 everywhere, near-collinear children, one to five observations, a node without any.

One step through the C ABI per case (computed once per case and shared).  Compared with the float64 numpy reference of soft_states.py
(pinned to the autograd oracle by tests/test_soft_states_host.py):

  LOGPROBS_Z  per sample, max-norm relative to the largest: max(5e-5 below 50 variables / 3e-4 from 50 on, 4 x yardstick)
  W_LIK       against sum_s w_s dscore_s with w = softmax of the DEVICE's log-probabilities (as tests/test_gpu_grad_weights.py: the
              log-probability error stays out of the comparison of the sum): max-norm 2e-3, and entry by entry on the free / small / dense
              edges |dev_e - ref_e| <= max(C_SUM sum_s w_s |dscore_se|, 4 x yardstick of the entry class |ref_e|)
  exact       saturated: W_LIK has no non-zero entry; a node without observations: its column of W_LIK is 0; nothing non-finite anywhere,
              z and v_z after the step included.  (One documented exception, asserted as such: `dense` at 129 variables -- every edge
              of a complete digraph above 0.9 -- where phi^2 of the acyclicity term leaves float32 in RMSprop's second moment, for the
              reference's float32 arithmetic as for the engine (limits table): v_z is +inf exactly on the coordinates
              whose phi^2 overflows, z stays finite.  The float64 autograd oracle on that state: max |phi| = 2.1e37, phi^2 beyond
              float32 on 33 153 of the 33 282 coordinates.)

The yardstick is the float32 run of the reference against its float64 run on the same case, never device output (the rule of
tests/test_gpu_max_size.py, the factor 4 for the same reason: one draw of the rounding, another summation order).  Every comparison
prints yardstick, bound and device error (`pytest -s`); profiles/soft_bge_errors.txt keeps one run."""
import numpy as np
import pytest

import bge_states as bs
import soft_states as ss
from conftest import assert_update_parity, update_check
from dibs_amd._abi import make_config

pytestmark = pytest.mark.gpu

_RUNS = {}


def _next_key(b):
    """the loop-carry key after one marginal step: svgd.py:226-267 splits it for the likelihood and for the prior estimator"""
    from oracle import prng
    k = prng.split(b["key"], b["M"] + 1)[0]
    return prng.split(k, b["M"] + 1)[0]


def _run(b):
    """one engine step of a built case: LOGPROBS_Z [M, S], W_LIK [M, d, d], PHI_Z, the state after the step"""
    if b["id"] not in _RUNS:
        from dibs_amd.engine import Engine
        M, S, d = b["M"], b["S"], b["d"]
        eng = Engine(make_config(**b["cfg_kw"]))
        try:
            eng.set_data(b["x"], b["mask"])
            eng.set_state(**ss.fresh_state(b))
            eng.run(b["t"], 1)
            out = dict(lp=eng.read("LOGPROBS_Z").reshape(M, S).astype(np.float64), w=eng.read("W_LIK").reshape(M, d, d).astype(np.float64),
                       phi=eng.read("PHI_Z").copy(), state=eng.get_state())
        finally:
            eng.close()
        _RUNS[b["id"]] = out
    return _RUNS[b["id"]]


def test_every_path_of_the_launcher_is_run():
    """from the bookkeeping: NB 1 .. 4 with and without LDS-resident R, two rows per lane with both values of `rl`, the global-scratch kernel"""
    assert {ss.path_key(ss.soft_path(c["d"], c["interv"])) for c in ss.CASES} == ss.required_paths()


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_soft_kernels_on_profiles(case):
    b = ss.build(case)
    dev, d, M = _run(b), b["d"], b["M"]
    y = ss.yardstick(b)
    tag = f"soft-bge | {b['id']:34s} {b['path']['name']:26s}"
    for name in ("lp", "w", "phi"):
        assert np.isfinite(dev[name]).all(), name
    st = dev["state"]
    assert np.isfinite(st["z"]).all()
    # v_z = 0.1 phi^2 from v = 0.  Dense soft graphs beyond 128 variables: the acyclicity term's phi^2 leaves float32, for the reference's
    # float32 arithmetic as for the engine (limits table) -- there, and only there, v_z is inf exactly where phi^2 overflows
    phi2 = dev["phi"].astype(np.float64).reshape(st["v_z"].shape) ** 2
    fmax = float(np.finfo(np.float32).max)
    inf_v = ~np.isfinite(st["v_z"])
    assert (phi2[inf_v] > 0.999 * fmax).all() and inf_v[0.1 * phi2 > 1.001 * fmax].all() and not np.isnan(st["v_z"]).any()
    assert not inf_v.any() or (case["profile"] == "dense" and d > 128), "v_z must be finite"
    assert np.array_equal(st["key"], _next_key(b))
    # LOGPROBS_Z
    lp_ref = b["ref64"]["logprobs"]
    bound, err = max(ss.lp_floor(d), 4 * y["lp"]), ss.rel(dev["lp"], lp_ref)
    print(f"\n{tag} LOGPROBS_Z yardstick {y['lp']:.2e} bound {bound:.1e} device {err:.2e}" + ("   ABOVE THE BOUND" if not err < bound else ""))
    ok = [err < bound]
    # W_LIK with the device's own weights
    w = ss.softmax_weights(dev["lp"])
    W64, _, absw = ss.reference_sums(b, w)
    if np.abs(W64).max() > 1e-30:
        err = ss.rel(dev["w"], W64)
        print(f"{tag} W_LIK max-norm yardstick {y['w_max']:.2e} bound {ss.W_LIK_MAXNORM:.1e} device {err:.2e}" + ("   ABOVE THE BOUND" if not err < ss.W_LIK_MAXNORM else ""))
        ok.append(err < ss.W_LIK_MAXNORM)
    for k in ss.ENTRY_CLASSES:
        name = ss.CLASSES[k]
        sel = (b["cls"] == k) & (np.abs(W64) > 1e-30)
        if not sel.any():
            continue
        yk = y["entry"][name][1] if name in y["entry"] else 0.0
        e = np.abs(dev["w"] - W64)[sel]
        bnd = np.maximum(ss.C_SUM * absw[sel], 4 * yk * np.abs(W64[sel]))
        worst = int(np.argmax(e / bnd))
        print(f"{tag} W_LIK {name:5s} entries {int(sel.sum()):5d} yardstick {yk:.2e} (of the entry) | device worst |err| / |ref| {(e / np.abs(W64[sel])).max():.2e} "
              f"|err| / sum w |ds| {(e / absw[sel]).max():.2e} (floor {ss.C_SUM:.0e}) | worst err / bound {e[worst] / bnd[worst]:.3f}"
              + ("   ABOVE THE BOUND" if not (e <= bnd).all() else ""))
        ok.append(bool((e <= bnd).all()))
    assert all(ok), "a comparison is beyond its bound (see the lines printed above)"
    # exact properties
    if case["profile"] == "saturated":
        assert not dev["w"].any()
    if b["all_intervened"] is not None:
        assert not dev["w"][:, :, b["all_intervened"]].any(), "a node without observations has no gradient"
    assert not dev["w"][:, np.arange(d), np.arange(d)].any()


@pytest.mark.parametrize("case", [c for c in ss.CASES if c["profile"] == "saturated" and c["d"] in (17, 49, 65)], ids=ss.case_id)
def test_saturated_equals_the_hard_graph_kernels(case):
    """LOGPROBS_Z of the soft engine against the sum over the nodes of NODE_SCORES of a score-estimator engine on the same z: its sampled
    graphs are deterministic there and equal the limit graph (checked on PARENT_MASKS), as are the soft engine's (every p exactly 0 or 1:
    the device's arithmetic on the reference's draws, and W_LIK without a non-zero entry).  Bound: the sum of the two paths' own bounds
    (test_marginal_bge_reparam_estimator; LOGPROBS_Z of test_marginal_bge_step_stages, 2e-5)."""
    from dibs_amd.engine import Engine
    b = ss.build(case)
    d, M, S = b["d"], b["M"], b["S"]
    soft = _run(b)
    g = ss.limit_graph(b)
    assert np.array_equal(ss.device_p32(b), np.broadcast_to(g[:, None].astype(np.float32), (M, S, d, d))) and not soft["w"].any()
    eng = Engine(make_config(**dict(b["cfg_kw"], grad_estimator_z="score")))
    try:
        eng.set_data(b["x"], b["mask"])
        eng.set_state(**ss.fresh_state(b))
        eng.run(b["t"], 1)
        gg = bs.graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d)
        hard = eng.read("NODE_SCORES").reshape(M, d, S).sum(1)
    finally:
        eng.close()
    assert np.array_equal(gg, np.broadcast_to(g[:, None].astype(np.uint8), gg.shape)), "the score estimator's graphs are the limit graph"
    bound, err = ss.lp_floor(d) + 2e-5, ss.rel(soft["lp"], hard)
    print(f"\nsoft-bge | {b['id']:34s} soft LOGPROBS_Z against hard NODE_SCORES: bound {bound:.1e} device {err:.2e}; against the reference: "
          f"soft {ss.rel(soft['lp'], b['ref64']['logprobs']):.2e} hard {ss.rel(hard, b['ref64']['logprobs']):.2e}")
    assert err < bound


@pytest.mark.parametrize("case", [c for c in ss.CASES if c["profile"] == "mixed" and c["d"] <= 64 and c["S"] <= 4], ids=ss.case_id)
def test_whole_step_on_mixed_states(case):
    """the whole step against the autograd oracle's svgd_step with the step criterion of tests/conftest.py, as
    test_marginal_bge_reparam_estimator"""
    import torch
    from oracle import dibs_oracle as O
    b = ss.build(case)
    dev, M, d = _run(b), b["M"], b["d"]
    cfg = make_config(**b["cfg_kw"])
    ocfg = O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=b["S"], n_acyclicity_mc_samples=2,
                    alpha_linear=ss.ALPHA_LINEAR, prior=O.GraphPrior("er", b["cfg_kw"]["edges_per_node"]))
    z = torch.as_tensor(np.array(b["z"]))
    st = O.State(z=z, v_z=torch.zeros_like(z), key=b["key"].copy(), sf_baseline=torch.zeros(M, dtype=torch.float64),
                 latent_prior_std=float(1.0 / np.sqrt(np.float32(d))), t=b["t"])
    x = torch.as_tensor(np.asarray(b["x"], np.float64))
    it = torch.zeros_like(x) if b["mask"] is None else torch.as_tensor(np.asarray(b["mask"], np.float64))
    st2, aux = O.svgd_step(ocfg, st, x, it, b["t"], return_aux=True)
    assert (dev["state"]["key"] == st2.key).all()
    phi_o = aux["phi_z"].numpy()
    u = update_check(cfg, b["z"], np.zeros_like(b["z"]), dev["phi"].reshape(phi_o.shape), phi_o, dev["state"]["z"], st2.z.numpy())
    print(f"\nsoft-bge | {b['id']:34s} z update {u}")
    assert_update_parity(u, 0.9, b["id"])
