"""GPU parity tests (run on the MI355X box with `pytest -m gpu`): the HIP engine, called through the C ABI,
against the oracle on identical seeded inputs.

Tolerances (relative to the largest magnitude of the compared array, float32 arithmetic on the device):
  kernel stages 1e-5 (node scores / log-probs) .. 3e-4 (softmax-weighted W_lik, which amplifies fp32 noise of
  near-tied log-scores), single step on Z 1e-4 (the tolerance BASELINE.json's north_star states), sampled
  graphs / PRNG keys bit-exact."""
import os

import numpy as np
import pytest

from conftest import assert_update_parity, make_data, rel_err, stage_err, update_check
from dibs_amd._abi import make_config
from oracle import prng

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _engine(cfg, x, mask=None):
    from dibs_amd.engine import Engine
    eng = Engine(cfg)
    eng.set_data(x, mask)
    return eng


def _graphs_from_masks(masks, M, S, d):
    gm = masks.reshape(M, d, S, -1)  # [m][j][s][w]: bit i of word i // 64 = g[i, j]
    gg = np.zeros((M, S, d, d), np.uint8)
    for i in range(d):
        gg[:, :, i, :] = ((gm[:, :, :, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1)
    return gg


def _sync_states(eng, st):
    """start device and oracle from the same f32-representable state"""
    st["z"] = st["z"].astype(np.float32).astype(np.float64)
    st["v_z"] = st["v_z"].astype(np.float32).astype(np.float64)
    st["baseline"] = st["baseline"].astype(np.float32).astype(np.float64)
    kw = dict(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
    if st.get("theta") is not None:
        st["theta"] = st["theta"].astype(np.float32).astype(np.float64)
        st["v_theta"] = st["v_theta"].astype(np.float32).astype(np.float64)
        kw.update(theta=st["theta"], v_theta=st["v_theta"])
    eng.set_state(**kw)


def test_init_particles_matches_oracle(c_oracle64):
    for d, M, k in ((5, 4, 5), (20, 8, 20), (7, 3, 4)):
        cfg = make_config(n_vars=d, n_particles=M, n_observations=10, n_dim=k, edges_per_node=1)
        data, _, _ = make_data(d, n_obs=10)
        eng = _engine(cfg, data.x)
        eng.init_particles(prng.PRNGKey(1))
        g = eng.get_state()
        z0, _, key = c_oracle64.init_particles(cfg, prng.PRNGKey(1))
        assert (g["key"] == key).all()
        assert rel_err(g["z"], z0) < 1e-6
        assert not g["v_z"].any() and not g["baseline"].any()
        eng.close()


@pytest.mark.parametrize("d,M,S,Sa,prior,steps,layout", [
    (5, 4, 128, 32, "er", (0, 1, 5), "legacy"),
    (5, 3, 17, 5, "sf", (0, 2), "legacy"),          # odd S / Sa: unpaired Threefry path
    (20, 8, 128, 32, "er", (0, 3), "legacy"),
    (20, 4, 64, 16, "uniform", (1,), "legacy"),
    (50, 4, 128, 32, "er", (0, 2), "legacy"),
    (70, 2, 32, 8, "er", (1,), "legacy"),           # > 64 variables: two mask words, 80x80 MFMA tiles
    (112, 2, 16, 4, "er", (1,), "legacy"),          # engine maximum: 112x112 tiles; l = 35 .. 75 here, the one-problem-per-wave BGe tier ONLY (the other tiers at 65 .. 112 variables: test_gpu_bge_tiers.py)
    (96, 8, 64, 8, "er", (1,), "legacy"),           # thousands of queued problems at d > 80: only two waves of a factorisation block fit the
    (112, 6, 64, 4, "sf", (2,), "partitionable"),   # one-problem-per-wave tier, all four need quad index lists (LDS layout bug found by gpu_fuzz.py)
    (120, 2, 16, 4, "er", (1,), "legacy"),          # > 112: matrix powers through global memory, chunked edge scores, W through global memory
    (128, 3, 8, 4, "sf", (0, 2), "legacy"),         # two full mask words
    (130, 2, 8, 2, "er", (1,), "legacy"),           # three mask words: plain sampling loop, one factorisation per wave (k_bge_chol_wide)
    (200, 2, 8, 2, "er", (1,), "partitionable"),    # four mask words, complement form with up to 100 rows
    (3, 1, 4, 2, "uniform", (0, 1), "legacy"),      # smallest sensible problem, a single particle
    (20, 5, 32, 8, "er", (2,), "partitionable"),   # jax_threefry_partitionable=True streams (no call pairing)
    (5, 3, 16, 4, "sf", (0, 1), "partitionable"),
    (6, 272, 8, 4, "er", (0, 2), "legacy"),         # >= 256 particles: the SVGD transform as a GEMM (k_phi_gemm), ragged 128-particle tiles
])
def test_marginal_bge_step_stages(c_oracle64, d, M, S, Sa, prior, steps, layout):
    # (more observations than variables beyond d = 112: with N = 100 < d the matrix R = t I + X^T X is a rank-deficient Gram matrix plus a
    #  small ridge, and float32 pivots of such minors lose another digit -- the reference computes them in float32 as well)
    n_obs = 100 if d <= 112 else 3 * d
    data, _, _ = make_data(d, seed=0, n_obs=n_obs)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=n_obs, edges_per_node=1 if d <= 5 else 2, graph_prior=prior,
                      n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, rng_layout=layout)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(1))
    eng = _engine(cfg, data.x)
    for t in steps:
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        gg = _graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d)
        assert np.array_equal(gg, dbg["g_samples"]), "sampled graphs must be bit-identical"
        assert (g["key"] == st["key"]).all()
        assert rel_err(eng.read("SCORES"), dbg["scores"]) < 2e-6
        # fp32 Cholesky pivots: the log-det error is multiplied by (N + alpha_lambd - d + l) / 2 ~ 50-90
        ns = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1)  # device layout [m][j][s]
        assert rel_err(ns, dbg["node_scores"]) < (1e-4 if d <= 50 else (5e-4 if d <= 112 else 1e-3))
        assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < (2e-5 if d <= 112 else 5e-5)   # (measured 3.1e-5 at d = 128)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5
        assert rel_err(eng.read("GRAD_Z"), dbg["grad_z"]) < 1e-4
        assert rel_err(eng.read("KXX"), dbg["kxx"]) < 1e-5
        assert rel_err(eng.read("PHI_Z"), dbg["phi_z"]) < 1e-4
        if 0.1 * float(np.abs(dbg["phi_z"]).max()) ** 2 > 1e38:
            # tr((I + G/d)^d) of the dense soft graphs of the first steps grows like 1.5^d: beyond d ~ 128 phi^2 leaves the float32 range in
            # RMSprop's second moment from d = 128 on (for the reference's float32 arithmetic as for the device's; the f64 oracle does not overflow), so the
            # comparison ends with phi (the update at these sizes, on states where phi^2 stays inside float32: tests/test_gpu_max_size.py)
            assert d >= 128
            continue
        assert rel_err(g["v_z"], st["v_z"]) < 2e-4
        assert rel_err(g["z"], st["z"]) < 1e-4  # north_star tolerance on Z
    eng.close()


def test_marginal_bge_with_interventions(c_oracle64):
    d, M = 12, 4
    data, _, _ = make_data(d, seed=3)
    rng = np.random.default_rng(0)
    mask = (rng.random((100, d)) < 0.1).astype(np.int32)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, has_interventions=True)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(2))
    eng = _engine(cfg, data.x, mask)
    for t in (0, 2):
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, mask, st, t, debug=True)
        eng.run(t, 1)
        ns = eng.read("NODE_SCORES").reshape(M, d, 128).transpose(0, 2, 1)
        assert rel_err(ns, dbg["node_scores"]) < 1e-4
        assert rel_err(eng.get_state()["z"], st["z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("d,M,S,Sa,k,case", [
    (2, 1, 1, 1, 2, "minimal"),          # smallest legal problem: one particle, one sample, one chain (unpaired Threefry paths)
    (2, 3, 2, 2, 1, "k1"),               # latent dimension 1
    (9, 2, 8, 2, 4, "all_intervened"),   # node 3 is intervened in EVERY observation: N_j = 0, its BGe term is 0 (linearGaussian.py:118)
    (6, 2, 4, 2, 6, "one_observation"),  # a single observation
    (33, 2, 6, 2, 33, "d33"),            # one variable past two MFMA tiles; 64-bit masks half used
    (64, 1, 4, 2, 8, "d64"),             # mask word exactly full, n <= 32 via the complement form for every parent set
    (65, 1, 4, 2, 8, "d65"),             # first size with two mask words; its one-problem-per-wave tier holds l = 32 alone, which these 260 parent sets need not contain (test_gpu_bge_tiers.py constructs it)
])
def test_marginal_bge_edge_cases(c_oracle64, d, M, S, Sa, k, case):
    """Edge cases of the marginal step against the oracle: degenerate sizes, latent dimension != n_vars, a node without
    observational data, mask-word boundaries."""
    N = 1 if case == "one_observation" else 40
    rng = np.random.default_rng(5)
    x = rng.normal(size=(N, d)).astype(np.float32)
    mask = None
    if case == "all_intervened":
        mask = (rng.random((N, d)) < 0.1).astype(np.int32)
        mask[:, 3] = 1
    cfg = make_config(n_vars=d, n_particles=M, n_observations=N, n_dim=k, edges_per_node=0.4 if d == 2 else (1 if d <= 9 else 2),
                      n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, has_interventions=mask is not None)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(11))
    eng = _engine(cfg, x, mask)
    eng.init_particles(prng.PRNGKey(11))
    g0 = eng.get_state()
    assert (g0["key"] == st["key"]).all() and rel_err(g0["z"], st["z"]) < 1e-6
    for t in (0, 1, 4):
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, x, mask, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert np.array_equal(_graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d), dbg["g_samples"])
        assert (g["key"] == st["key"]).all()
        ns = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1)
        assert rel_err(ns, dbg["node_scores"]) < (1e-4 if d <= 50 else 5e-4)
        if case == "all_intervened":
            assert not ns[:, :, 3].any()
        assert rel_err(eng.read("W_LIK"), dbg["w_lik"]) < 2e-3 or np.abs(dbg["w_lik"]).max() == 0
        assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5 or np.abs(dbg["w_acyc"]).max() == 0
        assert rel_err(eng.read("KXX"), dbg["kxx"]) < 1e-5
        assert rel_err(g["z"], st["z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("d,Sa", [(33, 4), (34, 2), (40, 4), (47, 2), (48, 4), (49, 2), (52, 4), (63, 2), (64, 4), (50, 3)])
def test_acyclicity_kernel_sizes_33_to_64(c_oracle64, d, Sa):
    """k_acyc_hf (float products on the f16 matrix pipe with two block-scaled pieces per operand, kernels_acyc_f16.h) at every tile / exponent
    boundary of its range: d - 1 = 32 (squarings only), 63 (a "times M" step after every squaring), 47 / 48 / 49 (last row tile and
    last column tile empty, just filled, just started).  Sa = 3 takes the f32-MFMA kernel (chains cannot be paired): same tolerance.
    reference: graph_utils.py:8-28, dibs.py:557-601"""
    M, S = 2, 4
    data, _, _ = make_data(d, seed=2)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(5))
    eng = _engine(cfg, data.x)
    for t in (1, 6):   # alpha = alpha_linear t = t (MarginalDiBS: alpha_linear = 1): soft graphs away from 1/2
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
        eng.run(t, 1)
        assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5
        assert rel_err(eng.get_state()["z"], st["z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("d,Sa", [(65, 2), (72, 4), (80, 2), (81, 4), (96, 2), (97, 2), (100, 4), (111, 2), (112, 4), (100, 3)])
def test_acyclicity_kernel_sizes_65_to_112(c_oracle64, d, Sa):
    """k_acyc_hfw<5 / 6 / 7> (the two-piece f16 scheme with 5 .. 7 tiles and waves, kernels_acyc_f16.h) at the boundaries of its range:
    first / last size of every tile count, odd tile counts (the last k-step reads its second half from the zero page), d = 100 (BASELINE
    config 5).  Sa = 3 takes the f32-MFMA kernel (chains cannot be paired): same tolerance.  reference: graph_utils.py:8-28, dibs.py:557-601"""
    M, S = 2, 2
    data, _, _ = make_data(d, seed=2, n_obs=2 * d)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=2 * d, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(5))
    eng = _engine(cfg, data.x)
    for t in (1, 6):
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
        eng.run(t, 1)
        assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5
        assert rel_err(eng.read("PHI_Z"), dbg["phi_z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("d,Sa,t", [(64, 4, 20000), (64, 2, 200000), (50, 4, 20000), (80, 2, 20000), (80, 4, 400), (72, 2, 100000),
                                    (96, 2, 400), (100, 4, 20000), (112, 2, 400), (112, 4, 20000)])
def test_acyclicity_f16_pipe_worst_cases(c_oracle64, monkeypatch, d, Sa, t):
    """The two-piece f16 operands of k_acyc_hf / k_acyc_hfw (22 mantissa bits, truncation bias ~1e-7 per product level)
    where the bias is largest: the longest product chains of each kernel (d = 64: 63 = 111111b, a multiply after every squaring; d = 80,
    the last size on the f16 pipe) and hard soft graphs (alpha = alpha_linear t = t = 400 .. 200000: entries of the matrix either ~1/d or ~0, the
    few edges near 1/2 carry the whole gradient).
    Two comparisons.  (1) f16 pipe against the f32-MFMA kernel (DIBS_ACYC_F32=1) on the same inputs: the pipe's own contribution, bounded
    by 1e-7 (d - 1) (measured 1.2e-6 at d = 64; 4.1e-6 at d = 80 with k_acyc_hfw's first-order bias compensation, 1.3e-5 without;
    1.5e-7 (d - 1) from 81 variables on: 1.05e-5 at d = 96, 1.35e-5 at d = 112, where the f16 pipe is the CLOSER one to the oracle).  (2) both against the float64 oracle: at alpha >= 1000 ANY float32 evaluation of sigmoid(alpha (s + l)) --
    the reference's included -- carries up to alpha 2^-24 relative error per edge (measured: the f32 kernel 2.0e-4 at d = 50, t = 20000,
    the f16 pipe the same 2.0e-4: 0.17 alpha 2^-24), so the bound scales with alpha there: 0.2 alpha 2^-24.  (alpha_linear = 1 is
    make_config's default for MarginalDiBS; 0.05 is JointDiBS's.)  reference: graph_utils.py:8-28, dibs.py:557-601"""
    M, S = 2, 2
    data, _, _ = make_data(d, seed=2, n_obs=2 * d)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=2 * d, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(7))
    dbg = None
    out = {}
    for pipe in ("f16", "f32"):
        if pipe == "f32":
            monkeypatch.setenv("DIBS_ACYC_F32", "1")
        eng = _engine(cfg, data.x)
        _sync_states(eng, st)
        if dbg is None:
            snap = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
            dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
            st = snap
        eng.run(t, 1)
        out[pipe] = eng.read("W_ACYC").copy()
        eng.close()
    ref = np.asarray(dbg["w_acyc"])
    assert np.abs(ref).max() > 0, "vacuous: every edge saturated"
    alpha = cfg.alpha_linear * t
    assert cfg.alpha_linear == 1.0
    e16, e32, pipe_err = rel_err(out["f16"], ref), rel_err(out["f32"], ref), rel_err(out["f16"], out["f32"])
    print(f"d={d} Sa={Sa} alpha={alpha:g}: vs oracle f16 {e16:.2e} f32 {e32:.2e}; f16 vs f32 {pipe_err:.2e}; nonzero share {np.mean(ref != 0):.3f}")
    big = np.abs(out["f32"]) > 1e-3 * np.abs(out["f32"]).max()
    r = out["f16"][big].astype(np.float64) / out["f32"][big].astype(np.float64) - 1.0
    print(f"   ratio-1 over {big.sum()} entries: mean {r.mean():.3e} std {r.std():.3e} min {r.min():.3e} max {r.max():.3e}")
    # (beyond 80 variables the f32 kernel's own distance to the oracle is 6-9e-6: the difference of the two kernels carries both roundings)
    assert pipe_err < (1e-7 if d <= 80 else 1.5e-7) * (d - 1)
    assert e16 < max(1e-5, 0.2 * alpha * 2.0 ** -24) and e32 < max(1e-5, 0.2 * alpha * 2.0 ** -24)


@pytest.mark.parametrize("d,Sa", [(20, 4), (40, 4), (50, 4), (50, 3), (70, 2)])
def test_acyclicity_gradient_of_saturated_soft_graphs_is_zero(c_oracle64, d, Sa):
    """Once alpha * score leaves the range where float32 resolves sigmoid from 0 / 1 (every edge after the first few hundred steps of a
    run with alpha_linear = 1) the reference's soft graph is exactly 0 / 1 and g (1 - g) = 0 kills the acyclicity gradient of that edge
    whatever the matrix-power entry behind it.  The kernels draw g = u / (u + (1 - u) exp(-alpha s)) with an approximate reciprocal:
    the saturated case has to come out as exactly 1, not 1 +- 2^-24 (found by tests/tools/gpu_fuzz.py).  dibs.py:121-140, 557-601"""
    M = 2
    data, _, _ = make_data(d, seed=1)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=4, n_acyclicity_mc_samples=Sa, n_dim=1)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(3))
    st["z"] = np.sign(st["z"]) * (6.0 + np.abs(st["z"]))   # one latent dimension: |score| = |u_i v_j| >= 36, alpha |s| >= 720 at t = 20
    eng = _engine(cfg, data.x)
    _sync_states(eng, st)
    dbg = c_oracle64.step(cfg, data.x, None, st, 20, debug=True)
    eng.run(20, 1)
    assert np.abs(np.asarray(dbg["w_acyc"])).max() < 1e-30   # (double resolves sigmoid a little further out than float: ~1e-85, not 0)
    assert not eng.read("W_ACYC").any(), "saturated soft graphs must have an exactly zero acyclicity gradient"
    eng.close()


def test_score_function_baseline_and_gd_optimizer(c_oracle64):
    d, M = 8, 4
    data, _, _ = make_data(d, seed=1)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, score_function_baseline=0.05, optimizer="gd",
                      n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(4))
    eng = _engine(cfg, data.x)
    for t in (1, 2):
        _sync_states(eng, st)
        c_oracle64.step(cfg, data.x, None, st, t)
        eng.run(t, 1)
        g = eng.get_state()
        assert rel_err(g["baseline"], st["baseline"]) < 1e-5
        assert rel_err(g["z"], st["z"]) < 1e-4
    eng.close()


def test_golden_config1(c_oracle64):
    """BASELINE.json configs[0] against the committed fixture: autograd steps 1-5 from a common start, then the
    free-running 50-step trajectory with the step of first divergence reported."""
    gold = np.load(os.path.join(GOLD, "config1_marginal_bge_d5.npz"))
    cfg = make_config(n_vars=5, n_particles=4, n_observations=100, edges_per_node=1)
    eng = _engine(cfg, gold["x"])
    eng.init_particles(gold["key"])
    g = eng.get_state()
    assert (g["key"] == gold["key_after_init"]).all() and rel_err(g["z"], gold["z_init"]) < 1e-6
    first_div = None
    for t in range(50):
        eng.run(t, 1)
        if t + 1 in (1, 2, 5, 10, 20, 50):
            ref = gold["z_autograd_steps1to5"][t] if t + 1 <= 5 else gold[f"z_cport_step{t + 1}"]
            err = rel_err(eng.get_state()["z"], ref)
            if err > 1e-4 and first_div is None:
                first_div = t + 1
            if t + 1 <= 5:
                assert err < 1e-4, f"step {t + 1}: {err}"
    print("config1 free-running trajectory: first step with rel err > 1e-4:", first_div)
    assert (eng.get_state()["key"] == gold["key_after_50"]).all()
    assert first_div is None or first_div >= 10
    eng.close()


def test_chunking_is_transparent():
    """run(0, 6) == run(0, 2); run(2, 4): the loop carry lives entirely in the engine state (svgd.py:315)."""
    data, _, _ = make_data(10, seed=2)
    cfg = make_config(n_vars=10, n_particles=8, n_observations=100)
    a, b = _engine(cfg, data.x), _engine(cfg, data.x)
    a.init_particles(prng.PRNGKey(5))
    b.init_particles(prng.PRNGKey(5))
    a.run(0, 6)
    b.run(0, 2)
    st = b.get_state()
    b.set_state(**{k: v for k, v in st.items() if v is not None})  # checkpoint / resume round trip
    b.run(2, 4)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa["z"], sb["z"]) and np.array_equal(sa["v_z"], sb["v_z"]) and (sa["key"] == sb["key"]).all()
    a.close()
    b.close()


def test_headline_size_properties():
    """d=50, M=128 (BASELINE.json metric config): size-independent properties -- determinism, finite state,
    kernel-matrix symmetry / unit diagonal, and particle-sharding independence of the per-particle estimators."""
    from dibs_amd.engine import Engine
    data, _, _ = make_data(50, seed=0)
    cfg = make_config(n_vars=50, n_particles=128, n_observations=100)
    outs = []
    for rep in range(2):
        eng = _engine(cfg, data.x)
        eng.init_particles(prng.PRNGKey(1))
        eng.run(0, 3)
        outs.append((eng.get_state(), eng.read("KXX").reshape(128, 128), eng.read("GRAD_Z").reshape(128, -1)))
        eng.close()
    (s0, k0, g0), (s1, k1, g1) = outs
    assert np.array_equal(s0["z"], s1["z"]), "bit-reproducible run to run"
    assert np.isfinite(s0["z"]).all() and np.isfinite(s0["v_z"]).all()
    assert np.allclose(np.diag(k0), 1.0) and np.array_equal(k0, k0.T)
    # a 2-rank engine pair (phase A only) produces the same per-particle gradients as the single-rank engine
    import torch
    E = None
    grads = []
    for r in range(2):
        c2 = make_config(n_vars=50, n_particles=128, n_observations=100, rank=r, n_ranks=2)
        e2 = Engine(c2)  # own stream; e2.sync() below orders the read-back
        e2.set_data(data.x)
        e2.init_particles(prng.PRNGKey(1))
        n = e2.gather_elems_per_rank()
        buf = torch.zeros(n, dtype=torch.float32, device="cuda")
        # phase A of step 0 (estimators + packing) for this rank's shard
        e2.step_local(0, buf.data_ptr())
        e2.sync()
        E = n // 64
        grads.append(buf.cpu().numpy().reshape(64, E)[:, 5000:10000])
        e2.close()
    eng = _engine(cfg, data.x)
    eng.init_particles(prng.PRNGKey(1))
    eng.run(0, 1)
    gfull = eng.read("GRAD_Z").reshape(128, -1)
    eng.close()
    assert np.array_equal(np.concatenate(grads), gfull), "estimators must not depend on the particle sharding"


def test_sample_api_contract():
    """MarginalDiBS.sample(): return type, callback protocol, step overshoot (svgd.py:311-324)."""
    from dibs_amd.inference import MarginalDiBS
    data, gm, lm = make_data(8, seed=1)
    dibs = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    calls = []
    g = dibs.sample(key=prng.PRNGKey(0), n_particles=6, steps=10, callback=lambda **kw: calls.append((kw["t"], kw["zs"].shape, kw["dibs"] is dibs)),
                    callback_every=4)
    assert g.shape == (6, 8, 8) and g.dtype == np.int32 and (np.diagonal(g, axis1=1, axis2=2) == 0).all()
    assert calls == [(4, (6, 8, 8, 2), True), (8, (6, 8, 8, 2), True), (12, (6, 8, 8, 2), True)]  # 12 steps, not 10
    assert abs(dibs.latent_prior_std - 1 / np.sqrt(8)) < 1e-7
    g0 = dibs.sample(key=prng.PRNGKey(0), n_particles=6, steps=0)
    z0 = dibs.last_state["z"]
    assert np.array_equal(g0, dibs.particle_to_g_lim(z0)) and not dibs.last_state["v_z"].any()
    dist = dibs.get_empirical(g)
    assert abs(np.exp(dist.logp).sum() - 1) < 1e-9


@pytest.mark.parametrize("d,M,S,Sa,est,prior,interv,steps", [
    (5, 3, 16, 4, "reparam", "er", False, (1, 2)),
    (5, 3, 16, 4, "score", "sf", True, (1, 3)),
    (6, 260, 8, 4, "reparam", "er", False, (1, 2)),   # >= 256 particles: k_phi_gemm on both segments (z and theta)
    (20, 6, 64, 16, "reparam", "er", True, (1, 4)),
    (50, 4, 128, 32, "reparam", "er", False, (2,)),
    (33, 3, 32, 8, "score", "sf", True, (1,)),        # 33..64: k_lin_logprobs_hf (two-piece f16 operands); 33..48 skips the fourth column tile
    (40, 3, 32, 8, "reparam", "er", True, (2,)),
    (48, 3, 32, 8, "score", "er", False, (1,)),
    (49, 3, 32, 8, "reparam", "sf", True, (1,)),
    (50, 3, 64, 8, "reparam", "sf", True, (1, 3)),
    (57, 3, 32, 8, "reparam", "er", False, (2,)),     # 51..64: eight operand elements per thread
    (64, 3, 32, 8, "score", "er", True, (1,)),
    (100, 3, 32, 8, "reparam", "er", True, (2,)),     # d of BASELINE config 5: largest LDS footprint of the LinG kernels
    (112, 2, 16, 4, "score", "sf", False, (1,)),      # engine maximum
])
def test_joint_lingauss_step_stages(c_oracle64, d, M, S, Sa, est, prior, interv, steps):
    _lingauss_step_stages(c_oracle64, d, M, S, Sa, est, prior, interv, steps)


@pytest.mark.parametrize("d,M,S,Sa,est,prior,interv,steps", [
    (5, 3, 16, 4, "reparam", "er", False, (1, 2)),    # D = 50, P = 25: scalar staging, one ragged chunk, one ragged tile
    (6, 260, 8, 4, "reparam", "er", False, (1, 2)),   # 9 x 9 tiles (the last ragged), D = 72: float4 staging
    (20, 70, 16, 4, "score", "sf", True, (1,)),       # D = 800: four chunks, the last short; 3 x 3 tiles
    (33, 3, 32, 8, "score", "sf", True, (1,)),        # D = 2178, P = 1089: scalar staging over several chunks
    (50, 4, 128, 32, "reparam", "er", False, (2,)),   # D = 5000 (headline vector length), P = 2500
])
def test_joint_lingauss_tiled_kernel_matrix(c_oracle64, monkeypatch, d, M, S, Sa, est, prior, interv, steps):
    """The tiled kernel matrix (k_kmat_tile + k_kmat_finish, default from 256 particles) forced at every size: same stages, same bounds."""
    monkeypatch.setenv("DIBS_KMAT_TILED_MIN", "1")
    _lingauss_step_stages(c_oracle64, d, M, S, Sa, est, prior, interv, steps)


def _lingauss_step_stages(c_oracle64, d, M, S, Sa, est, prior, interv, steps):
    data, _, _ = make_data(d, seed=2, joint=True)
    mask = None
    if interv:
        mask = (np.random.default_rng(0).random((100, d)) < 0.1).astype(np.int32)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, edges_per_node=1 if d <= 5 else 2, joint=True,
                      likelihood="lingauss", grad_estimator_z=est, graph_prior=prior, n_grad_mc_samples=S,
                      n_acyclicity_mc_samples=Sa, has_interventions=interv,
                      score_function_baseline=0.001 if est == "score" else 0.0)  # c > 0 multiplies by exp(-b): keep b small
    st = c_oracle64.new_state(cfg, prng.PRNGKey(3))
    eng = _engine(cfg, data.x, mask)
    eng.init_particles(prng.PRNGKey(3))
    g0 = eng.get_state()
    assert (g0["key"] == st["key"]).all() and rel_err(g0["z"], st["z"]) < 1e-6 and rel_err(g0["theta"], st["theta"]) < 1e-6
    for t in steps:
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, mask, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert (g["key"] == st["key"]).all()
        assert rel_err(eng.read("LOGPROBS_THETA"), dbg["logprobs_th"]) < 2e-5
        assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < 2e-5
        stage_err("GRAD_THETA", eng.read("GRAD_THETA"), dbg["grad_theta"], 5e-4)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5
        stage_err("GRAD_Z", eng.read("GRAD_Z"), dbg["grad_z"], 1e-4)
        assert rel_err(eng.read("KXX"), dbg["kxx"]) < 1e-5
        stage_err("PHI_THETA", eng.read("PHI_THETA"), dbg["phi_theta"], 2e-3)
        assert rel_err(g["baseline"], st["baseline"]) < 1e-5 or np.abs(st["baseline"]).max() == 0
        assert rel_err(g["theta"], st["theta"]) < 1e-4
        assert rel_err(g["z"], st["z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("model,d,M,S,est,noise", [
    ("lingauss", 20, 3, 64, "reparam", 1e4),    # every sample keeps a weight: 8 samples per block, all 8 blocks of a particle add up
    ("lingauss", 50, 4, 128, "reparam", 1e4),
    ("lingauss", 50, 3, 40, "score", 1e4),      # the Z estimator's score form (no matrix products) through the same split
    ("lingauss", 100, 2, 16, "reparam", 1e4),   # two row tiles per wave
    ("lingauss", 20, 3, 5, "reparam", 1e4),     # fewer weighted samples than blocks: only 5 partial sums exist
    ("densenn", 20, 3, 64, "reparam", 1e4),
    ("densenn", 50, 2, 24, "score", 1e4),
    ("densenn", 100, 2, 12, "reparam", 1e4),
    ("lingauss-gram", 20, 3, 64, "reparam", 1e4),   # the Gram-matrix path (k_ling_grad) shares the samples the same way
    ("lingauss-gram", 50, 2, 40, "score", 1e4),
    ("densenn-deep", 12, 3, 40, "reparam", 1e4),    # two hidden layers: the general-stack kernels (k_nng_grad)
    ("densenn-deep", 20, 2, 24, "score", 1e4),
])
def test_joint_gradients_with_many_weighted_samples(c_oracle64, monkeypatch, model, d, M, S, est, noise):
    """Late in a run many samples keep a non-zero softmax weight (dibs.py:376-382, 531-549) and the gradient kernels deal them to GRAD_NS
    blocks per particle, the last block adding the partial sums (kernels_joint.h: GradSplit).  A large observation noise flattens the
    log-probabilities so that EVERY sample has a weight from the first step on; same stages, same bounds as the step tests."""
    data, _, _ = make_data(d, seed=4, joint=True)
    gram = model == "lingauss-gram"
    if gram:
        monkeypatch.setenv("DIBS_LIN_GRAM", "1")   # (latched when the engine is created: tuning.h)
        model = "lingauss"
    deep = model == "densenn-deep"
    if deep:
        model = "densenn"
    kw = dict(lin_obs_noise=noise) if model == "lingauss" else dict(nn_obs_noise=noise, nn_hidden=(4, 3) if deep else (5,))
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, joint=True, likelihood=model, grad_estimator_z=est, n_grad_mc_samples=S,
                      n_acyclicity_mc_samples=4, score_function_baseline=0.001 if est == "score" else 0.0, **kw)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(6))
    eng = _engine(cfg, data.x)
    eng.init_particles(prng.PRNGKey(6))
    for t in (400, 401):   # (late: the edge probabilities have saturated, the sampled graphs of a particle are nearly the same graph)
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
        eng.run(t, 1)
        for name in ("LOGPROBS_THETA", "LOGPROBS_Z"):
            lp = eng.read(name).reshape(M, S).astype(np.float64)
            w = np.exp(lp - lp.max(1, keepdims=True))
            w = (w / w.sum(1, keepdims=True)).astype(np.float32)
            print(name, "samples with a weight per particle:", (w > 0).sum(1))
            if name == "LOGPROBS_THETA" and d <= 50:   # (at d = 100 the prior term of the sampled edges still separates the samples: those cases only re-check the one-block path)
                assert (w > 0).sum(1).max() >= 2, (name, (w > 0).sum(1))   # at least one particle's gradient is shared between blocks
        assert rel_err(eng.read("LOGPROBS_THETA"), dbg["logprobs_th"]) < 2e-5
        stage_err("GRAD_THETA", eng.read("GRAD_THETA"), dbg["grad_theta"], 5e-4)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        g = eng.get_state()
        # (the Gram path rounds x^T r differently -- double sums of C -- and with gradients flattened by the large noise RMSprop turns a theta
        #  coordinate whose phi is rounding noise into a full step: 2.3e-4 there; the stages above are the comparison)
        assert (gram or rel_err(g["theta"], st["theta"]) < 1e-4) and rel_err(g["z"], st["z"]) < 1e-4
    eng.close()


@pytest.mark.parametrize("model,d,M,S,est", [
    ("densenn", 20, 6, 64, "reparam"),    # k_nn_grad: no-return atomic adds into the partial rows, persistent blocks taking items in any order
    ("densenn", 100, 3, 32, "reparam"),   # (one block per CU, 8 waves)
    ("densenn", 20, 4, 48, "score"),
    ("lingauss", 50, 6, 64, "reparam"),   # k_lin_grad: partial sums in registers
    ("densenn-deep", 12, 4, 40, "reparam"),
])
def test_gradient_kernels_are_run_to_run_deterministic(model, d, M, S, est):
    """Which block takes which (particle, share) item, and when, differs from run to run; the results must not: a share's partial sum has one
    owner per element, and the partial sums are added in share order (kernels_joint.h: GradSplit; kernels_nn.h: nn_acc, k_grad_plan).  The
    same late step (every sample weighted: large observation noise) eight times from one state, bit for bit."""
    data, _, _ = make_data(d, seed=4, joint=True)
    deep = model == "densenn-deep"
    if deep:
        model = "densenn"
    kw = dict(lin_obs_noise=1e4) if model == "lingauss" else dict(nn_obs_noise=1e4, nn_hidden=(4, 3) if deep else (5,))
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, joint=True, likelihood=model, grad_estimator_z=est, n_grad_mc_samples=S,
                      n_acyclicity_mc_samples=4, score_function_baseline=0.001 if est == "score" else 0.0, **kw)
    eng = _engine(cfg, data.x)
    eng.init_particles(prng.PRNGKey(6))
    eng.run(400, 1)
    st0 = eng.get_state()
    ref = None
    for rep in range(8):
        eng.set_state(**{k: st0[k] for k in ("z", "v_z", "theta", "v_theta", "key", "baseline")})
        eng.run(401, 1)
        cur = dict(gt=eng.read("GRAD_THETA").copy(), wl=eng.read("W_LIK").copy(), **{k: v.copy() for k, v in eng.get_state().items() if k in ("z", "theta")})
        if ref is None:
            ref = cur
            lp = eng.read("LOGPROBS_THETA").reshape(M, S).astype(np.float64)
            w = np.exp(lp - lp.max(1, keepdims=True))
            assert ((w / w.sum(1, keepdims=True)).astype(np.float32) >= 2.0 ** -30).sum(1).max() >= 2   # shares exist
        else:
            for k in ref:
                assert np.array_equal(ref[k].view(np.uint32), cur[k].view(np.uint32)), (rep, k)
    eng.close()


@pytest.mark.parametrize("d,M,S,Sa,est,interv,N,force", [
    (20, 4, 32, 8, "reparam", False, 100, True),    # same sizes as the MFMA path: both device paths against one oracle
    (20, 4, 32, 8, "score", True, 100, True),
    (50, 3, 32, 8, "reparam", True, 100, True),
    (20, 3, 32, 8, "reparam", True, 900, False),    # x [900, 20] does not fit LDS: the engine picks the Gram path by itself
    (50, 2, 16, 4, "reparam", False, 400, False),
    (112, 2, 8, 4, "score", False, 500, False),     # one Gram matrix that no longer fits LDS beside the operands (d > 100): read through the caches
    (104, 2, 8, 4, "reparam", False, 300, False),   # (launch failure found by tests/tools/gpu_fuzz.py)
    (128, 2, 8, 2, "reparam", True, 300, False),    # > 112 variables: Gram path + the global-memory acyclicity / back-projection kernels
    (140, 2, 4, 2, "score", False, 200, False),     # the last size with both operands of the gradient kernel in LDS (141)
    (150, 2, 4, 2, "reparam", False, 200, False),   # round 5: graph + masked weights of the gradient kernel in global scratch (142 .. 198)
    (200, 2, 4, 2, "score", True, 250, False),      # ... and the masked weights of the log-prob kernel too (> 198); one Gram matrix per node
    (210, 2, 2, 2, "reparam", False, 300, False),   # (beyond ~220 variables the acyclicity gradient of a fresh particle leaves float32 -- in the
                                                    #  reference's arithmetic as here: (I + G/d)^(d-1) with G ~ 1/2 is 1.5^255 = 8e44 at d = 256)
])
def test_joint_lingauss_gram_path(c_oracle64, monkeypatch, d, M, S, Sa, est, interv, N, force):
    """LinearGaussian for any number of observations (linearGaussian.py:292-316): the Gram-matrix path of kernels_lin_gram.h,
    stage by stage against the oracle; held-out scoring on the same path."""
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.models import LinearGaussian
    if force:
        monkeypatch.setenv("DIBS_LIN_GRAM", "1")
    rng = np.random.default_rng(3)
    wts = (rng.random((d, d)) < 2.0 / d) * rng.normal(size=(d, d))
    x = rng.normal(size=(N, d)).astype(np.float32)
    for j in range(d):   # some structure in the data (lower-triangular mechanism)
        x[:, j] += (x[:, :j] @ np.tril(wts.T, -1)[j, :j]).astype(np.float32)
    mask = (rng.random((N, d)) < 0.1).astype(np.int32) if interv else None
    cfg = make_config(n_vars=d, n_particles=M, n_observations=N, joint=True, likelihood="lingauss", grad_estimator_z=est,
                      n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, has_interventions=interv)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(3))
    eng = _engine(cfg, x, mask)
    eng.init_particles(prng.PRNGKey(3))
    for t in (1, 3):
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, x, mask, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert (g["key"] == st["key"]).all()
        assert rel_err(eng.read("LOGPROBS_THETA"), dbg["logprobs_th"]) < 2e-5
        assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < 2e-5
        stage_err("GRAD_THETA", eng.read("GRAD_THETA"), dbg["grad_theta"], 5e-4)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        stage_err("GRAD_Z", eng.read("GRAD_Z"), dbg["grad_z"], 1e-4)
        stage_err("PHI_THETA", eng.read("PHI_THETA"), dbg["phi_theta"], 2e-3)
        assert rel_err(g["theta"], st["theta"]) < 1e-4
        stage_err("PHI_Z", eng.read("PHI_Z"), dbg["phi_z"], 1e-4)
        if 0.1 * float(np.abs(dbg["phi_z"]).max()) ** 2 > 1e38:   # (d >= 128: phi^2 beyond float32 in RMSprop, see test_marginal_bge_step_stages;
            assert d >= 128                                       #  the update at these sizes is covered by tests/test_gpu_max_size.py)
            continue
        assert rel_err(g["z"], st["z"]) < 1e-4
    eng.close()
    gs = (rng.random((5, d, d)) < 0.1).astype(np.int32)
    gs[:, np.arange(d), np.arange(d)] = 0
    th = rng.normal(size=(5, d, d)).astype(np.float32)
    ref = c_oracle64.score_graphs(cfg, x, mask, gs, th.reshape(5, -1).astype(np.float64))
    got = score_graphs(LinearGaussian(n_vars=d), gs, th, x, mask)
    assert rel_err(got, ref) < 2e-5


def test_golden_joint_lingauss():
    gold = np.load(os.path.join(GOLD, "joint_lingauss_d5.npz"))
    cfg = make_config(n_vars=5, n_particles=3, n_observations=100, edges_per_node=1, joint=True, likelihood="lingauss",
                      n_grad_mc_samples=16, n_acyclicity_mc_samples=4, has_interventions=True)
    eng = _engine(cfg, gold["x"], gold["mask"])
    eng.init_particles(gold["key"])
    g = eng.get_state()
    assert rel_err(g["z"], gold["z_init"]) < 1e-6 and rel_err(g["theta"], gold["theta_init"].reshape(3, -1)) < 1e-6
    for i, t in enumerate((1, 2, 3)):  # the fixture steps t = 1, 2, 3 (alpha(0) = 0 is uninformative)
        eng.run(t, 1)
        g = eng.get_state()
        assert rel_err(g["z"], gold["z_autograd_t1to3"][i]) < 1e-4
        assert rel_err(g["theta"], gold["theta_autograd_t1to3"][i].reshape(3, -1)) < 1e-4
    assert (g["key"] == gold["key_after"]).all()
    eng.close()


def test_joint_sample_api():
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(8, seed=1, joint=True)
    dibs = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    seen = []
    g, theta = dibs.sample(key=prng.PRNGKey(0), n_particles=5, steps=6, callback_every=3,
                           callback=lambda **kw: seen.append((kw["t"], kw["zs"].shape, kw["thetas"].shape)))
    assert g.shape == (5, 8, 8) and theta.shape == (5, 8, 8) and theta.dtype == np.float32
    assert seen == [(3, (5, 8, 8, 2), (5, 8, 8)), (6, (5, 8, 8, 2), (5, 8, 8))]
    dist = dibs.get_empirical(g, theta)
    assert np.allclose(np.exp(dist.logp).sum(), 1.0)


def test_score_graphs_and_mixture(c_oracle64):
    """dibs_score_graphs (device) == oracle log p(D | G) / log p(theta, D | G); get_mixture / held-out evaluators."""
    from dibs_amd.inference import JointDiBS, MarginalDiBS
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.metrics import expected_shd, neg_ave_log_marginal_likelihood, neg_ave_log_likelihood
    rng = np.random.default_rng(0)
    for d in (6, 50, 70):
        data, gm, lm = make_data(d, seed=1)
        g = (rng.random((9, d, d)) < 0.15).astype(np.int32)
        g[:, np.arange(d), np.arange(d)] = 0
        g[0] = data.g
        g[1] = 0
        cfg = make_config(n_vars=d, n_particles=1, n_observations=100, edges_per_node=1 if d <= 6 else 2)
        ref = c_oracle64.score_graphs(cfg, data.x, None, g)
        got = score_graphs(lm, g, None, data.x, None)
        assert rel_err(got, ref) < 2e-5
        mask = (rng.random((100, d)) < 0.1).astype(np.int32)
        ref = c_oracle64.score_graphs(cfg, data.x_ho, mask, g)
        got = score_graphs(lm, g, None, data.x_ho, mask)
        assert rel_err(got, ref) < 2e-5
    data, gm, lm = make_data(6, seed=1)
    dibs = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    g = (rng.random((5, 6, 6)) < 0.2).astype(np.int32)
    g[:, np.arange(6), np.arange(6)] = 0
    mix = dibs.get_mixture(g)
    assert abs(np.exp(mix.logp).sum() - 1) < 1e-6
    assert np.isfinite(neg_ave_log_marginal_likelihood(dist=mix, eltwise_log_marginal_likelihood=dibs.eltwise_log_marginal_likelihood_observ, x=data.x_ho))
    assert expected_shd(dist=mix, g=data.g) >= 0
    # joint
    dataj, gmj, lmj = make_data(6, seed=2, joint=True)
    th = rng.normal(size=(5, 6, 6)).astype(np.float32)
    cfgj = make_config(n_vars=6, n_particles=1, n_observations=100, edges_per_node=1, joint=True, likelihood="lingauss")
    ref = c_oracle64.score_graphs(cfgj, dataj.x, None, g, th.reshape(5, -1).astype(np.float64))
    got = score_graphs(lmj, g, th, dataj.x, None)
    assert rel_err(got, ref) < 2e-5
    jd = JointDiBS(x=dataj.x, graph_model=gmj, likelihood_model=lmj)
    mixj = jd.get_mixture(g, th)
    assert abs(np.exp(mixj.logp).sum() - 1) < 1e-6
    assert np.isfinite(neg_ave_log_likelihood(dist=mixj, eltwise_log_likelihood=jd.eltwise_log_likelihood_observ, x=dataj.x_ho))


@pytest.mark.parametrize("d", [3, 8, 20, 50, 70])
def test_device_bge_scores_against_closed_forms(d):
    """The device's hard-graph BGe scorer against ground truth that does not involve the oracle (tests/test_known_answers.py pins the oracle
    the same way): a complete DAG in any variable order scores the normal-Wishart evidence of the data (Geiger & Heckerman 2002 with the
    constants of linearGaussian.py:63-118), evaluated here in double with scipy; Markov-equivalent graphs score the same."""
    import math
    from scipy import special
    from dibs_amd.inference.scoring import score_graphs
    data, _, lm = make_data(d, seed=4)
    x = np.asarray(data.x, np.float64)
    n, am, al = x.shape[0], 1.0, d + 2.0
    t = am * (al - d - 1) / (am + 1)
    xbar = x.mean(0, keepdims=True)
    R = t * np.eye(d) + (x - xbar).T @ (x - xbar) + n * am / (n + am) * xbar.T @ xbar
    want = (-0.5 * n * d * math.log(math.pi) + 0.5 * d * math.log(am / (am + n)) + special.multigammaln(0.5 * (al + n), d)
            - special.multigammaln(0.5 * al, d) + 0.5 * al * d * math.log(t) - 0.5 * (al + n) * np.linalg.slogdet(R)[1])
    rng = np.random.default_rng(d)
    gs = []
    for _ in range(4):
        order = rng.permutation(d)
        g = np.zeros((d, d), np.int32)
        for a in range(d):
            g[order[a], order[a + 1:]] = 1
        gs.append(g)
    chain = np.zeros((d, d), np.int32)
    chain[np.arange(d - 1), np.arange(1, d)] = 1
    gs += [chain, chain.T.copy()]                       # a chain and its reversal are Markov equivalent
    got = np.asarray(score_graphs(lm, np.stack(gs), None, data.x, None), np.float64)
    assert np.abs(got[:4] - want).max() < 2e-5 * abs(want), (got[:4], want)
    assert abs(got[4] - got[5]) < 2e-5 * abs(got[4])


@pytest.mark.parametrize("d,M,S,Sa,H,act,bias,est,interv,steps,N", [
    (5, 3, 16, 4, 4, "relu", True, "reparam", True, (1, 2), 60),
    (6, 3, 16, 4, 3, "tanh", False, "score", False, (1, 2), 60),
    (20, 4, 32, 8, 5, "relu", True, "reparam", False, (2,), 60),
    (20, 3, 16, 4, 5, "leakyrelu", True, "reparam", True, (3,), 60),
    (100, 2, 16, 4, 5, "tanh", True, "reparam", True, (2,), 100),   # BASELINE config 5 geometry: d=100, hidden (5,), interv_mask
    (100, 2, 8, 4, 5, "relu", True, "score", True, (1,), 100),
    # more hidden units than k_nn_grad keeps in registers at once (8 per group; fewer when LDS is short): groups, the forward product repeated
    (20, 3, 16, 4, 12, "relu", True, "reparam", False, (2,), 60),       # 8 + 4
    (12, 2, 8, 2, 20, "sigmoid", True, "score", True, (1,), 40),        # 8 + 8 + 4
    (100, 2, 8, 4, 8, "tanh", True, "reparam", True, (1,), 100),        # d = 100: LDS holds 7 units' slices -> 7 + 1
    # d >= 65: the register-operand kernels of kernels_nn_f16x.h (x^T image always 7 / 8 observation tiles: with FEW observations the LDS
    # size must still be the instantiation's -- found by tests/tools/gpu_fuzz.py FUZZ_NN); odd and even tile counts, 7- and 8-tile images
    (80, 3, 8, 2, 5, "leakyrelu", False, "reparam", False, (2,), 20),
    (96, 2, 8, 2, 4, "relu", True, "score", True, (1,), 120),
    (66, 2, 6, 2, 7, "sigmoid", True, "reparam", True, (1,), 33),
    (48, 3, 8, 2, 5, "relu", True, "reparam", False, (1,), 50),          # 33 <= d <= 64: the image variant (kernels_nn_f16.h)
    # the LDS size of the register-operand kernel depends on hard / soft graphs: in these windows the theta pass (hard graphs) takes it and
    # the Z-reparam pass of the same step (soft graphs: + the graph bytes) falls to the image variant, which must then build ITS tables
    # (round 4 built only the theta pass's: uninitialised first-layer tables)
    (108, 2, 6, 2, 5, "relu", True, "reparam", False, (1,), 128),
    (105, 2, 4, 2, 8, "tanh", True, "reparam", True, (1,), 128),
])
def test_joint_densenn_step_stages(c_oracle64, d, M, S, Sa, H, act, bias, est, interv, steps, N):
    rng = np.random.default_rng(1)
    x = rng.normal(size=(N, d)).astype(np.float32)
    mask = (rng.random((N, d)) < 0.1).astype(np.int32) if interv else None
    cfg = make_config(n_vars=d, n_particles=M, n_observations=N, edges_per_node=1 if d <= 6 else 2, joint=True,
                      likelihood="densenn", grad_estimator_z=est, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa,
                      nn_hidden=(H,), nn_activation=act, nn_bias=bias, has_interventions=interv)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(6))
    eng = _engine(cfg, x, mask)
    eng.init_particles(prng.PRNGKey(6))
    g0 = eng.get_state()
    assert (g0["key"] == st["key"]).all() and rel_err(g0["theta"], st["theta"]) < 1e-6, "stax init stream"
    for t in steps:
        _sync_states(eng, st)
        th_prev, vth_prev = st["theta"].copy(), st["v_theta"].copy()
        dbg = c_oracle64.step(cfg, x, mask, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert (g["key"] == st["key"]).all()
        assert rel_err(eng.read("LOGPROBS_THETA"), dbg["logprobs_th"]) < 2e-5
        assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < 2e-5
        stage_err("GRAD_THETA", eng.read("GRAD_THETA"), dbg["grad_theta"], 5e-4)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        stage_err("GRAD_Z", eng.read("GRAD_Z"), dbg["grad_z"], 1e-4)
        stage_err("PHI_THETA", eng.read("PHI_THETA"), dbg["phi_theta"], 2e-3)
        if H <= 7:
            assert rel_err(g["theta"], st["theta"]) < 1e-4
        else:
            # (wide layers: thousands of weights whose phi is float32 noise of the largest one, and RMSprop from a small second moment turns such a
            #  phi into a full step of either sign -- 5.5e-4 of max |theta| at H = 8, d = 100 with PHI_THETA within 9e-6; the step criterion of
            #  tests/conftest.py instead: signal coordinates within 1e-4, every coordinate the optimizer applied to the device's own phi)
            u = update_check(cfg, th_prev, vth_prev, eng.read("PHI_THETA"), dbg["phi_theta"], g["theta"], st["theta"])
            print(f"densenn H={H} d={d} t={t}: {u}")
            assert_update_parity(u, 0.4, f"densenn H={H} d={d} theta")
        # piecewise-linear activations: a pre-activation within fp32 rounding of 0 flips relu' between the f32 device
        # and the f64 oracle, and RMSprop turns the resulting small phi differences into O(stepsize) differences
        assert rel_err(g["z"], st["z"]) < 5e-4
    eng.close()


@pytest.mark.parametrize("d,M,S,Sa,hidden,act,bias,est,interv,steps,N", [
    (20, 4, 32, 8, (8, 8), "relu", True, "reparam", False, (2,), 60),       # two hidden layers
    (10, 3, 16, 4, (6, 4, 3), "tanh", True, "reparam", True, (1, 2), 40),   # three hidden layers, interventions
    (8, 3, 16, 4, (5, 5), "sigmoid", False, "score", False, (1,), 30),      # no bias, score-function estimator for Z
    (12, 3, 16, 4, (80,), "leakyrelu", True, "reparam", False, (2,), 40),   # one layer wider than the MFMA kernels take
    (6, 3, 16, 4, (5,), "relu", True, "reparam", True, (1,), 150),          # more observations than the MFMA kernels take
    (20, 3, 16, 4, (32,), "relu", True, "reparam", False, (2,), 60),        # (32,): MFMA path, listed next to (8, 8) for comparison
    (7, 2, 8, 2, (4, 4, 3, 3, 2, 2), "tanh", True, "reparam", True, (1,), 30),   # six hidden layers (the config struct carries up to eight)
    (128, 2, 4, 2, (4,), "relu", True, "reparam", True, (1,), 60),               # > 112 variables: general path + global-memory kernels
    (200, 2, 2, 2, (3,), "relu", True, "reparam", False, (1,), 40),              # round 5, > 198 variables: the sampled graph of a block in global scratch
    (210, 2, 2, 2, (2,), "tanh", False, "score", True, (1,), 30),                # (beyond ~220 variables the acyclicity gradient of a fresh particle
                                                                                 #  -- (I + G/d)^(d-1), G ~ 1/2 -- leaves float32: 1.5^255 = 8e44)
])
def test_joint_densenn_general_stacks(c_oracle64, d, M, S, Sa, hidden, act, bias, est, interv, steps, N):
    """DenseNonlinearGaussian with an arbitrary tuple of hidden layers / width / observation count (nonlinearGaussian.py:35-81,
    155-186, 248-326): the general device path of kernels_nn_generic.h against the oracle, stage by stage."""
    rng = np.random.default_rng(2)
    x = rng.normal(size=(N, d)).astype(np.float32)
    mask = (rng.random((N, d)) < 0.1).astype(np.int32) if interv else None
    cfg = make_config(n_vars=d, n_particles=M, n_observations=N, edges_per_node=1 if d <= 6 else 2, joint=True,
                      likelihood="densenn", grad_estimator_z=est, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa,
                      nn_hidden=hidden, nn_activation=act, nn_bias=bias, has_interventions=interv)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(7))
    eng = _engine(cfg, x, mask)
    eng.init_particles(prng.PRNGKey(7))
    g0 = eng.get_state()
    assert (g0["key"] == st["key"]).all() and rel_err(g0["theta"], st["theta"]) < 1e-6, "stax init stream of the whole stack"
    for t in steps:
        _sync_states(eng, st)
        dbg = c_oracle64.step(cfg, x, mask, st, t, debug=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert (g["key"] == st["key"]).all()
        assert rel_err(eng.read("LOGPROBS_THETA"), dbg["logprobs_th"]) < 2e-5
        assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < 2e-5
        stage_err("GRAD_THETA", eng.read("GRAD_THETA"), dbg["grad_theta"], 5e-4)
        stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
        stage_err("GRAD_Z", eng.read("GRAD_Z"), dbg["grad_z"], 1e-4)
        stage_err("PHI_THETA", eng.read("PHI_THETA"), dbg["phi_theta"], 2e-3)
        assert rel_err(g["theta"], st["theta"]) < 1e-4
        stage_err("PHI_Z", eng.read("PHI_Z"), dbg["phi_z"], 1e-4)
        if 0.1 * float(np.abs(dbg["phi_z"]).max()) ** 2 > 1e38:   # (d >= 128: phi^2 beyond float32 in RMSprop, see test_marginal_bge_step_stages;
            assert d >= 128                                       #  the update at these sizes is covered by tests/test_gpu_max_size.py)
            continue
        assert rel_err(g["z"], st["z"]) < 5e-4
    eng.close()


def test_densenn_deep_sample_and_scoring(c_oracle64):
    """JointDiBS.sample() and the held-out scorer with a two-hidden-layer model (the reference's constructor takes any tuple)."""
    from dibs_amd.inference import JointDiBS
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.target import make_nonlinear_gaussian_model
    from dibs_amd import random
    data, gm, lm = make_nonlinear_gaussian_model(key=random.PRNGKey(0), n_vars=8, graph_prior_str="er", n_observations=50,
                                                 hidden_layers=(6, 4))
    dibs = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    g, theta = dibs.sample(key=random.PRNGKey(1), n_particles=4, steps=4)
    assert g.shape == (4, 8, 8) and theta[0][0].shape == (4, 8, 8, 6) and theta[2][0].shape == (4, 8, 6, 4) and theta[4][0].shape == (4, 8, 4, 1)
    flat = lm.tree_to_flat(theta)
    cfg = make_config(n_vars=8, n_particles=1, n_observations=50, joint=True, likelihood="densenn", nn_hidden=(6, 4))
    ref = c_oracle64.score_graphs(cfg, data.x_ho[:50], None, g, flat.astype(np.float64))
    got = score_graphs(lm, g, flat, data.x_ho[:50], None)
    assert rel_err(got, ref) < 2e-5


def test_densenn_sample_and_scoring(c_oracle64):
    from dibs_amd.inference import JointDiBS
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.models import DenseNonlinearGaussian
    from dibs_amd.target import make_nonlinear_gaussian_model
    from dibs_amd import random
    data, gm, lm = make_nonlinear_gaussian_model(key=random.PRNGKey(0), n_vars=8, graph_prior_str="er", n_observations=50)
    dibs = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    g, theta = dibs.sample(key=random.PRNGKey(1), n_particles=4, steps=4)
    assert g.shape == (4, 8, 8) and theta[0][0].shape == (4, 8, 8, 5) and theta[0][1].shape == (4, 8, 5) and theta[1] == ()
    assert theta[2][0].shape == (4, 8, 5, 1) and theta[2][1].shape == (4, 8, 1)
    flat = lm.tree_to_flat(theta)
    cfg = make_config(n_vars=8, n_particles=1, n_observations=50, joint=True, likelihood="densenn")
    ref = c_oracle64.score_graphs(cfg, data.x_ho[:50], None, g, flat.astype(np.float64))
    got = score_graphs(lm, g, flat, data.x_ho[:50], None)
    assert rel_err(got, ref) < 2e-5
    mix = dibs.get_mixture(g, theta)
    assert abs(np.exp(mix.logp).sum() - 1) < 1e-6


@pytest.mark.parametrize("d", [124, 130, 160])   # 124: two mask words, per-node matrices read through the caches; 130 / 160: three words
def test_large_n_vars_paths(c_oracle64, d):
    """113 .. 256 variables (reference: no size limit, graph_utils.py:8-28, linearGaussian.py:63-118): the global-memory paths of the
    engine -- three / four mask words, one factorisation per wave, matrix powers through HBM, W through global memory -- with interventions
    (one R_j per node), the hard-graph scorer at that size, the public sample() call, and two rank engines against one."""
    import torch
    from dibs_amd.engine import Engine
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.inference.scoring import score_graphs
    N, M, S, Sa = 2 * d, 4, 8, 2
    data, gm, lm = make_data(d, seed=2, n_obs=N)
    rng = np.random.default_rng(3)
    mask = (rng.random((N, d)) < 0.08).astype(np.int32)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, has_interventions=True)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(5))
    eng = _engine(cfg, data.x, mask)
    _sync_states(eng, st)
    dbg = c_oracle64.step(cfg, data.x, mask, st, 2, debug=True)
    eng.run(2, 1)
    assert np.array_equal(_graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d), dbg["g_samples"])
    ns = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1)
    assert rel_err(ns, dbg["node_scores"]) < 1e-3
    assert rel_err(eng.read("LOGPROBS_Z"), dbg["logprobs_z"]) < 5e-5
    stage_err("W_LIK", eng.read("W_LIK"), dbg["w_lik"], 2e-3)
    assert rel_err(eng.read("W_ACYC"), dbg["w_acyc"]) < 1e-5
    assert rel_err(eng.read("GRAD_Z"), dbg["grad_z"]) < 1e-4
    assert rel_err(eng.read("PHI_Z"), dbg["phi_z"]) < 1e-4
    eng.close()
    # hard-graph scorer (dibs_score_graphs): given parent sets of up to four mask words
    g = (rng.random((7, d, d)) < 0.05).astype(np.int32)
    g[:, np.arange(d), np.arange(d)] = 0
    g[0], g[1] = data.g, 0
    g[2] = np.triu(np.ones((d, d), np.int32), 1)   # complete DAG: parent sets of every size up to d - 1 (complement form)
    ref = c_oracle64.score_graphs(cfg, data.x, mask, g)
    assert rel_err(score_graphs(lm, g, None, data.x, mask), ref) < 5e-5
    # public API + sharding: two rank engines (packed rows) == one engine, bit for bit
    gs = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa).sample(
        key=prng.PRNGKey(1), n_particles=M, steps=3)
    assert gs.shape == (M, d, d)
    cfg1 = make_config(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    ref_e = _engine(cfg1, data.x)
    ref_e.init_particles(prng.PRNGKey(8))
    ref_e.run(0, 3)
    zref = ref_e.get_state()["z"]
    ref_e.close()
    ts = torch.cuda.Stream()
    engs = []
    for r in range(2):
        e = Engine(make_config(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, rank=r, n_ranks=2),
                   stream=ts.cuda_stream)
        e.set_data(data.x)
        e.init_particles(prng.PRNGKey(8))
        engs.append(e)
    n = engs[0].gather_elems_per_rank()
    with torch.cuda.stream(ts):
        sends = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
        recv = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        for t in range(3):
            for r in range(2):
                engs[r].step_local(t, sends[r].data_ptr())
            torch.cat(sends, out=recv)
            for r in range(2):
                engs[r].step_update(t, recv.data_ptr())
    torch.cuda.synchronize()
    z2 = np.concatenate([e.get_state()["z"] for e in engs])
    for e in engs:
        e.close()
    assert np.array_equal(z2, zref)


@pytest.mark.parametrize("joint,d,M", [(False, 20, 16), (True, 20, 16), (False, 50, 16), (True, 50, 16), (True, 6, 264)])
def test_sharded_engines_overlapped_exchange_matches_single_rank(joint, d, M):
    """The overlapped exchange of dibs_amd.distributed.run_sharded_overlapped on ONE GPU: engines for rank 0..R-1 of R in one process; the
    values [z | theta] are "gathered" (device concat on a SIDE stream, event-ordered exactly as the RCCL path orders them) right after
    the optimizer step, each rank's kernel-matrix slab is computed from them on that side stream behind the gather, and
    only the gradient rows are exchanged between the phases.  Must be bit-identical to the single-rank engine."""
    import torch
    from dibs_amd.engine import Engine
    R, steps = 4, 5
    data, _, _ = make_data(d, seed=3, joint=joint)
    kw = dict(joint=True, likelihood="lingauss") if joint else {}
    cfg1 = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=32, n_acyclicity_mc_samples=8, **kw)
    ref = _engine(cfg1, data.x)
    ref.init_particles(prng.PRNGKey(8))
    ref.run(0, steps)
    sref = ref.get_state()
    ref.close()
    tstream, side = torch.cuda.Stream(), torch.cuda.Stream()
    engs = []
    for r in range(R):
        c = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=32, n_acyclicity_mc_samples=8, rank=r, n_ranks=R, **kw)
        e = Engine(c, stream=tstream.cuda_stream)
        e.set_data(data.x)
        e.init_particles(prng.PRNGKey(8))
        engs.append(e)
    n = engs[0].plane_elems_per_rank()
    exported, ready = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(tstream):
        vsends = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(R)]
        gsends = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(R)]
        planes = torch.zeros(2 * n * R, dtype=torch.float32, device="cuda")
        vals, grads = planes[:n * R], planes[n * R:]

        def exchange_values(done=False):
            for r in range(R):
                if not done:
                    engs[r].export_values(vsends[r].data_ptr())
            exported.record(tstream)
            with torch.cuda.stream(side):
                side.wait_event(exported)
                torch.cat(vsends, out=vals)   # stands in for dist.all_gather_into_tensor(vals, vsend) on the side stream
                for r in range(R):
                    engs[r].kmat_values(vals.data_ptr(), side.cuda_stream)
                ready.record(side)

        exchange_values()
        for t in range(steps):
            for r in range(R):
                engs[r].step_local_grads(t, gsends[r].data_ptr())
            torch.cat(gsends, out=grads)      # stands in for dist.all_gather_into_tensor(grads, gsend)
            tstream.wait_event(ready)
            for r in range(R):   # (odd steps: the optimizer kernel writes the send rows itself; even steps: the separate export call)
                engs[r].step_update_planes(t, planes.data_ptr(), vsends[r].data_ptr() if t % 2 else None)
            exchange_values(done=bool(t % 2))
    torch.cuda.synchronize()
    states = [e.get_state() for e in engs]
    assert np.array_equal(np.concatenate([s["z"] for s in states]), sref["z"]), "overlapped sharded run must be bit-identical to the single-rank run"
    assert all((s["key"] == sref["key"]).all() for s in states)
    if joint:
        assert np.array_equal(np.concatenate([s["theta"] for s in states]), sref["theta"])
    D = d * d * 2
    v = vals.view(M, -1).cpu().numpy()     # plane 0 = the values of the final state (what sample_sharded returns)
    assert np.array_equal(v[:, :D], sref["z"].reshape(M, D))
    for e in engs:
        e.close()


def test_run_sharded_overlapped_single_rank_on_gpu():
    """dibs_amd.distributed.run_sharded_overlapped driven as bench.py / sample_sharded drive it (one rank: copies instead of collectives,
    the same streams and events) == dibs_engine_run, bit for bit, across two chunks."""
    import torch
    from dibs_amd.distributed import OverlapBuffers, run_sharded_overlapped
    from dibs_amd.engine import Engine
    d, M = 20, 16
    data, _, _ = make_data(d, seed=3)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    ref = _engine(cfg, data.x)
    ref.init_particles(prng.PRNGKey(8))
    ref.run(0, 7)
    sref = ref.get_state()
    ref.close()
    tstream = torch.cuda.Stream()
    eng = Engine(cfg, stream=tstream.cuda_stream)
    eng.set_data(data.x)
    eng.init_particles(prng.PRNGKey(8))
    with torch.cuda.stream(tstream):
        buf = OverlapBuffers(eng, 1, torch.device("cuda", 0), torch.float32)
        run_sharded_overlapped(eng, 0, 4, buf)
        run_sharded_overlapped(eng, 4, 3, buf)
    torch.cuda.synchronize()
    st = eng.get_state()
    assert np.array_equal(st["z"], sref["z"]) and (st["key"] == sref["key"]).all()
    eng.close()


@pytest.mark.parametrize("joint,d,M", [(False, 20, 16), (True, 20, 16), (False, 50, 16), (False, 40, 16), (True, 50, 16),
                                       (False, 6, 272), (True, 6, 264)])   # >= 256 particles: k_phi_gemm, 68 / 66 particles per rank
def test_sharded_engines_match_single_rank(joint, d, M):
    """The N > 1 path of bench.py / dibs_amd.distributed on ONE GPU: engines for rank 0..R-1 of R in one process, the
    all-gather replaced by a device-side concat.  Must be bit-identical to the single-rank engine (PRNG rows are global,
    phi sums over b in global order).  d = 50 / 40: both instantiations of the split-bf16 acyclicity kernel, on the ranks with the score
    estimator's blocks riding along in its launch and on its own stream for the single engine."""
    import torch
    from dibs_amd.engine import Engine
    R, steps = 4, 5
    data, _, _ = make_data(d, seed=3, joint=joint)
    kw = dict(joint=True, likelihood="lingauss") if joint else {}
    cfg1 = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=32, n_acyclicity_mc_samples=8, **kw)
    ref = _engine(cfg1, data.x)
    ref.init_particles(prng.PRNGKey(8))
    ref.run(0, steps)
    sref = ref.get_state()
    ref.close()
    tstream = torch.cuda.Stream()  # a real (non-default) stream shared by the engines and the "collective"
    stream = tstream.cuda_stream
    engs = []
    for r in range(R):
        c = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=32, n_acyclicity_mc_samples=8,
                        rank=r, n_ranks=R, **kw)
        e = Engine(c, stream=stream)
        e.set_data(data.x)
        e.init_particles(prng.PRNGKey(8))
        engs.append(e)
    n = engs[0].gather_elems_per_rank()
    with torch.cuda.stream(tstream):
        sends = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(R)]
        recv = torch.zeros(n * R, dtype=torch.float32, device="cuda")
        for t in range(steps):
            for r in range(R):
                engs[r].step_local(t, sends[r].data_ptr())
            torch.cat(sends, out=recv)  # stands in for dist.all_gather_into_tensor(recv, send)
            for r in range(R):
                engs[r].step_update(t, recv.data_ptr())
    torch.cuda.synchronize()
    states = [e.get_state() for e in engs]
    z = np.concatenate([s["z"] for s in states])
    assert np.array_equal(z, sref["z"]), "sharded device run must be bit-identical to the single-rank run"
    assert all((s["key"] == sref["key"]).all() for s in states)
    if joint:
        assert np.array_equal(np.concatenate([s["theta"] for s in states]), sref["theta"])
    for e in engs:
        e.close()


@pytest.mark.parametrize("d,M,S,Sa,interv", [(5, 2, 6, 4, False), (8, 2, 4, 2, True), (12, 1, 4, 2, False), (20, 1, 4, 2, False), (40, 1, 2, 2, True),
                                             (50, 4, 16, 4, False), (64, 4, 16, 4, True),   # headline size / the last one-row-per-lane size
                                             # block boundaries of k_bge_soft_mf (16 x 16 blocks, node j ordered last): full last block, one real row in it
                                             (16, 2, 4, 2, False), (17, 2, 4, 2, True), (33, 1, 4, 2, False), (48, 1, 2, 2, True), (49, 1, 2, 2, False), (63, 1, 2, 2, False),
                                             (65, 1, 2, 2, False), (100, 1, 2, 2, True),    # two matrix rows per lane
                                             (130, 1, 2, 2, False), (160, 2, 2, 2, True)])  # > 128 (round 6): four rows per lane, triangles in global scratch
def test_marginal_bge_reparam_estimator(d, M, S, Sa, interv):
    """MarginalDiBS(grad_estimator_z='reparam'): BGe on Gumbel-soft graphs (dibs.py:395-459 with linearGaussian.py:63-170 on a
    real-valued parent vector).  Checked against the torch-autograd oracle (the C port has no soft BGe), which differentiates
    the reference's masked slogdet formula directly -- the device uses the closed forms of kernels_bge_soft.h."""
    import torch
    from oracle import dibs_oracle as O
    data, _, _ = make_data(d, seed=4)
    x = data.x.astype(np.float32)
    mask = (np.random.default_rng(1).random(x.shape) < 0.15).astype(np.int32) if interv else None
    epn = 1 if d <= 5 else 2
    cfg = make_config(n_vars=d, n_particles=M, n_observations=x.shape[0], edges_per_node=epn, grad_estimator_z="reparam",
                      n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, has_interventions=interv)
    ocfg = O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa,
                    prior=O.GraphPrior("er", epn))
    st = O.init_state(ocfg, prng.PRNGKey(9), M, d)
    eng = _engine(cfg, x, mask)
    eng.init_particles(prng.PRNGKey(9))
    xt = torch.as_tensor(x.astype(np.float64))
    it = torch.as_tensor((mask if mask is not None else np.zeros_like(x)).astype(np.float64))
    for t in ((1, 3) if d < 50 else (2,)):   # (the autograd oracle takes ~1 min per step at d = 64 with 64 soft graphs)
        st.z = torch.as_tensor(st.z.numpy().astype(np.float32).astype(np.float64))
        st.v_z = torch.as_tensor(st.v_z.numpy().astype(np.float32).astype(np.float64))
        eng.set_state(z=st.z.numpy(), v_z=st.v_z.numpy(), key=st.key, baseline=np.zeros(M))
        st2, aux = O.svgd_step(ocfg, st, xt, it, t, return_aux=True)
        eng.run(t, 1)
        g = eng.get_state()
        assert (g["key"] == st2.key).all()
        lp_o = np.stack([a["logprobs"].numpy() for a in aux["lik_aux"]])
        # float32 factorisation of M_pa (condition ~1e3..1e4) and the Schur complement R_jj - |L^-1 b|^2, which cancels two digits and
        # enters with a factor (N + l) / 2 ~ 60: measured 1e-6 .. 3e-5 up to d = 40 and 6e-5 .. 1.2e-4 at d = 50 .. 100 for this kernel AND for
        # round 2's (LDS-resident) one (tests/tools/gpu_soft_err.py); the reference computes the same quantities in float32
        assert rel_err(eng.read("LOGPROBS_Z"), lp_o) < (5e-5 if d < 50 else 3e-4)
        dz = (aux["dz_lik"] + aux["dz_prior"]).numpy()
        assert rel_err(eng.read("GRAD_Z"), dz) < 2e-3
        phi_o = aux["phi_z"].numpy()
        phi_dev = eng.read("PHI_Z").reshape(phi_o.shape)
        assert rel_err(phi_dev, phi_o) < 2e-3
        # the step criterion of every step test (tests/conftest.py): signal coordinates within 1e-4 of the oracle's z, every coordinate within
        # 1e-6 of the optimizer applied to the DEVICE's phi (RMSprop from v = 0 maps phi to a step of +-stepsize / sqrt(0.1) whatever its size:
        # a coordinate whose phi lies below the float32 noise of the largest one may take that step with the other sign)
        u = update_check(cfg, st.z.numpy(), st.v_z.numpy(), phi_dev, phi_o, g["z"], st2.z.numpy())
        print(f"soft BGe d={d} t={t}: {u}")
        if d <= 128:   # (beyond ~128 variables phi^2 of the dense early soft graphs leaves float32: RMSprop's second moment is inf and the step 0, for
            #  the reference's float32 arithmetic as for the device -- INTEGRATION.md, limits table; the stages above are the comparison there.
            #  The update beyond 128 variables, on states where phi^2 stays inside float32: tests/test_gpu_max_size.py)
            assert_update_parity(u, 0.9, f"soft BGe d={d} t={t}")
        st = st2
    eng.close()


def test_marginal_bge_reparam_free_running_30_steps():
    """MarginalDiBS with the reparam estimator (soft-graph BGe, k_bge_soft_mf) free-running for 30 steps from PRNGKey(9) against the torch-autograd
    oracle (float64) on the same inputs: identical keys, identical limit graphs, Z within 2.5e-4 of max |Z| on every coordinate, within 5e-5 on
    90 % and within 1e-5 on half of them.  (tests/tools/gpu_soft_freerun_trace.py follows the run step by step: the deviation is made in steps
    1, 3 and 4 by a handful of coordinates whose phi is a small difference of the particles' terms -- there the float32 noise of the soft-graph
    gradients is a few per cent of phi and RMSprop, still at v ~ 0.1 phi^2, turns it into a few per cent of a full step; afterwards it stays.
    Round 4's build and round 5's (other summation order in k_phi_update) both show 1.1e-4 .. 1.2e-4 at step 3; at step 30 the maxima are
    8.3e-5 and 1.5e-4, the medians 6.2e-6 and 3.7e-6.)"""
    import torch
    from oracle import dibs_oracle as O
    d, M, S, Sa, steps = 12, 4, 8, 4, 30
    data, _, _ = make_data(d, seed=4)
    x = data.x.astype(np.float32)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=x.shape[0], edges_per_node=2, grad_estimator_z="reparam",
                      n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    ocfg = O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, prior=O.GraphPrior("er", 2))
    st = O.init_state(ocfg, prng.PRNGKey(9), M, d)
    eng = _engine(cfg, x, None)
    eng.init_particles(prng.PRNGKey(9))
    xt = torch.as_tensor(x.astype(np.float64))
    it = torch.zeros_like(xt)
    for t in range(steps):
        st = O.svgd_step(ocfg, st, xt, it, t)
    eng.run(0, steps)
    g = eng.get_state()
    eng.close()
    z_o = st.z.numpy()
    err = rel_err(g["z"], z_o)
    dev = np.abs(g["z"] - z_o).ravel() / np.abs(z_o).max()
    print(f"soft BGe free run, {steps} steps: Z rel {err:.2e}, p90 {np.percentile(dev, 90):.2e}, median {np.median(dev):.2e}")
    assert (g["key"] == st.key).all()
    assert err < 2.5e-4 and np.percentile(dev, 90) < 5e-5 and np.median(dev) < 1e-5

    def lim(z):   # particle_to_g_lim (dibs.py:84-100): edge i -> j iff u_i . v_j > 0, no self loops
        gl = np.einsum("mik,mjk->mij", z[..., 0], z[..., 1]) > 0
        gl[:, np.arange(d), np.arange(d)] = False
        return gl
    assert np.array_equal(lim(g["z"].astype(np.float64)), lim(z_o))


def test_config2_free_running_200_steps(c_oracle64):
    """north_star's criterion on BASELINE.json configs[1] (MarginalDiBS + BGe, d=20, 32 particles): Z within 1e-4 relative of
    the (float64) oracle after N free-running steps on identical PRNG-seeded inputs, and the same posterior graphs / E-SHD.
    N = 200: beyond ~300 steps fp32 trajectories decorrelate -- the oracle's own f32 and f64 builds do too
    (tests/tools/oracle_f32_vs_f64.py)."""
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.metrics import expected_shd
    d, M, steps = 20, 32, 200
    data, gm, lm = make_data(d, seed=0)
    dibs = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    g_gpu = dibs.sample(key=prng.PRNGKey(1), n_particles=M, steps=steps)
    z_gpu = dibs.last_state["z"]
    cfg = dibs._make_config(M, d)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(1))
    c_oracle64.run(cfg, data.x, None, st, 0, steps, n_threads=min(os.cpu_count() or 1, 16))
    assert rel_err(z_gpu, st["z"]) < 1e-4
    g_or = dibs.particle_to_g_lim(st["z"])
    assert np.array_equal(g_gpu, g_or)
    e_gpu = expected_shd(dist=dibs.get_empirical(g_gpu), g=data.g)
    e_or = expected_shd(dist=dibs.get_empirical(g_or), g=data.g)
    assert abs(e_gpu - e_or) < 1e-3


@pytest.mark.parametrize("model,tol", [("lingauss", 1e-4), ("densenn", 5e-4)])
def test_joint_free_running_100_steps(c_oracle64, model, tol):
    """JointDiBS (reparam estimator, defaults) free-running for 100 steps from PRNGKey(1): Z within `tol` of the f64 oracle and
    identical posterior graphs (d=20, 16 particles).  DenseNN: relu' flips at pre-activations within fp32 rounding of 0 (see
    test_joint_densenn_step_stages) set the larger tolerance."""
    from dibs_amd.inference import JointDiBS
    from dibs_amd.target import make_linear_gaussian_model, make_nonlinear_gaussian_model
    d, M, steps = 20, 16, 100
    f = make_linear_gaussian_model if model == "lingauss" else make_nonlinear_gaussian_model
    data, gm, lm = f(key=prng.PRNGKey(0), n_vars=d, graph_prior_str="er")
    dibs = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    g, _ = dibs.sample(key=prng.PRNGKey(1), n_particles=M, steps=steps)
    cfg = dibs._make_config(M, d)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(1))
    c_oracle64.run(cfg, data.x, None, st, 0, steps, n_threads=min(os.cpu_count() or 1, 16))
    assert rel_err(dibs.last_state["z"], st["z"]) < tol
    assert np.array_equal(g, dibs.particle_to_g_lim(st["z"]))


def test_kernel_matrix_fusion_is_transparent(monkeypatch):
    """Single rank: the latent kernel matrix computed inside the k_bge_nodes launch (default) equals the stand-alone k_kmat
    launch (DIBS_NO_KMAT_FUSE=1) bit for bit, and so does the trajectory."""
    data, _, _ = make_data(20, seed=0)
    cfg = make_config(n_vars=20, n_particles=12, n_observations=100)
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DIBS_NO_KMAT_FUSE", "1")
        eng = _engine(cfg, data.x)
        eng.init_particles(prng.PRNGKey(5))
        eng.run(0, 7)
        outs.append((eng.read("KXX").copy(), eng.get_state()["z"].copy()))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("mode,n,seed", [("", 25, 101), ("FUZZ_BIG", 6, 102), ("FUZZ_SCALE", 12, 103), ("FUZZ_PARTICLES", 8, 104)])
def test_randomised_differential(monkeypatch, mode, n, seed):
    """A fixed-seed slice of tests/tools/gpu_fuzz.py (random sizes, priors, estimators, optimizers, interventions, PRNG layouts and model
    families, one or two steps each against the f64 oracle) as a regression net: the full runs found two defects this round."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "tools"))
    import gpu_fuzz
    for m in ("FUZZ_BIG", "FUZZ_SCALE", "FUZZ_PARTICLES"):
        monkeypatch.delenv(m, raising=False)
    if mode:
        monkeypatch.setenv(mode, "1")
    monkeypatch.setattr(sys, "argv", ["gpu_fuzz.py", str(n), str(seed)])
    assert gpu_fuzz.main() == 0


def test_kernel_matrix_units_in_particle_grad_launch(monkeypatch):
    """128+ particles, single rank, marginal model: the latent kernel matrix is computed by tile units riding in the k_particle_grad launch
    (pieces stored at agent scope, the last unit of a tile adds them -- no fence, no second pass).  200 steps in lock step with an engine
    that computes the matrix inside k_bge_sample (DIBS_NO_KMAT_GRAD=1, read per step): a piece read too early would be the previous
    step's (the buffer is reused), i.e. an entry off by ~1e-3.  Same sums in another order: 2e-6.  kernel.py:20-30, svgd.py:165-176"""
    d, M = 20, 128
    data, _, _ = make_data(d, seed=0)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    a, b = _engine(cfg, data.x), _engine(cfg, data.x)
    a.init_particles(prng.PRNGKey(5))
    worst = 0.0
    for t in range(200):
        st = {k: v for k, v in a.get_state().items() if v is not None}
        b.set_state(**st)
        monkeypatch.delenv("DIBS_NO_KMAT_GRAD", raising=False)
        a.run(t, 1)
        monkeypatch.setenv("DIBS_NO_KMAT_GRAD", "1")
        b.run(t, 1)
        ka, kb = a.read("KXX"), b.read("KXX")
        worst = max(worst, float(np.abs(ka - kb).max() / np.abs(kb).max()))
        assert worst < 2e-6, (t, worst)
        assert rel_err(a.get_state()["z"], b.get_state()["z"]) < 1e-5
    monkeypatch.delenv("DIBS_NO_KMAT_GRAD", raising=False)
    a.close(); b.close()


@pytest.mark.parametrize("joint,d,M", [(False, 8, 520), (True, 6, 260), (False, 20, 130), (True, 12, 1024)])
def test_kernel_matrix_tile64_equals_tile32(monkeypatch, joint, d, M):
    """The 64 x 64-tile kernel-matrix kernel (default from 512 particles) against the 32 x 32-tile one on the same particles: a wave's float
    sums cover the same 16 aligned elements in the same order and everything above them is added in double, so the entries are
    bit-identical -- ragged tile counts (520 = 8 x 64 + 8, 260, 130), symmetric single-rank slabs, the joint models' second matrix and
    their sum included (the trajectory is compared bit for bit as well).  kernel.py:20-30, svgd.py:165-176 / 537-551"""
    data, _, _ = make_data(d, seed=1, joint=joint)
    kw = dict(joint=True, likelihood="lingauss") if joint else {}
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=4, n_acyclicity_mc_samples=2, edges_per_node=1, **kw)
    outs = []
    for t64 in ("1", "1000000"):
        monkeypatch.setenv("DIBS_KMAT_T64_MIN", t64)
        monkeypatch.setenv("DIBS_NO_KMAT_GRAD", "1")   # (the units riding in k_particle_grad are 32 x 32 in both runs: take the launch of its own)
        eng = _engine(cfg, data.x)
        eng.init_particles(prng.PRNGKey(4))
        eng.run(0, 3)
        st = eng.get_state()
        outs.append((eng.read("KXX").copy(), st["z"].copy(), None if st.get("theta") is None else st["theta"].copy()))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    if joint:
        assert np.array_equal(outs[0][2], outs[1][2])
