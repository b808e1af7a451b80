"""GPU tests of the per-problem hyper-parameters of the batched engine (include/dibs_hip.h, dibs_engine_set_problem_hparams) and of
sample_sweep: problem p of a sweep must end BIT-IDENTICAL to a standalone engine configured with p's values and run with (x_p, mask_p,
key_p) and the same chunking -- particles, RMSprop moments, score-function baselines and the loop-carry key.  Every comparison is
np.array_equal.  Non-vacuity: two problems with the same data and key but different hyper-parameters must NOT end with equal particles.

One exception to the non-vacuity rule, by the model and not by the engine: the scale-free prior's (unnormalised) log-probability does not
contain n_edges_per_node (dibs/models/graph.py:182-196 of the reference: only the sampler uses it), so sf problems that differ in nothing
else must end EQUAL -- asserted as such, with a further sf problem that also differs in beta_linear to keep the case non-vacuous."""
import itertools

import numpy as np
import pytest

from conftest import make_data
from dibs_amd import _lib, random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine
from dibs_amd.inference import MarginalDiBS, sample_sweep
from dibs_amd.kernel import AdditiveFrobeniusSEKernel

pytestmark = pytest.mark.gpu

# make_config keyword -> field of dibs_problem_hparams
_FIELD = dict(alpha_linear="alpha_linear", beta_linear="beta_linear", h_latent="h_latent", stepsize="stepsize",
              score_function_baseline="score_function_baseline", latent_prior_std="latent_prior_std",
              edges_per_node="graph_prior_edges_per_node")
ALL_SEVEN = dict(alpha_linear=0.7, beta_linear=1.3, h_latent=3.0, stepsize=0.01, score_function_baseline=0.01, latent_prior_std=0.3,
                 edges_per_node=3)


def _problem(d, n_obs, seed, interv=False):
    data, gm, lm = make_data(d, n_obs=n_obs, seed=seed)
    x = np.asarray(data.x, np.float32)[:n_obs]
    mask = None
    if interv:  # hard interventions on a few nodes for a block of rows each
        mask = np.zeros(x.shape, np.int32)
        for q, j in enumerate((1, d // 2, d - 1)):
            mask[5 * q:5 * q + 4 + q, j] = 1
    return x, mask


def _standalone(kw, hp, x, mask, key, chunks):
    e = Engine(make_config(n_observations=x.shape[0], **{**kw, **hp}))
    try:
        e.set_data(x, mask)
        e.init_particles(random.PRNGKey(key))
        z0 = e.get_state()["z"]
        for t0, n in chunks:
            e.run(t0, n)
        return dict(e.get_state(), z0=z0)
    finally:
        e.close()


def _swept(kw, hps, probs, keys, chunks):
    B = len(probs)
    e = Engine(make_config(n_observations=probs[0][0].shape[0], n_problems=B, **kw))
    try:
        for p, ((x, mask), hp) in enumerate(zip(probs, hps)):
            e.set_data_problem(p, x, mask)
            if hp:  # (a problem that never had its values set has the configuration's)
                e.set_problem_hparams(p, **{_FIELD[k]: v for k, v in hp.items()})
                got = e.get_problem_hparams(p)
                assert all(getattr(got, _FIELD[k]) == float(v) for k, v in hp.items())
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        z0 = e.get_state()["z"]
        for t0, n in chunks:
            e.run(t0, n)
        return dict(e.get_state(), z0=z0)
    finally:
        e.close()


def _assert_problem_equal(bst, p, M, st):
    sl = slice(p * M, (p + 1) * M)
    assert np.isfinite(st["z"]).all(), p
    assert np.array_equal(bst["z0"][sl], st["z0"]), p
    assert np.array_equal(bst["z"][sl], st["z"]), (p, np.abs(bst["z"][sl] - st["z"]).max())
    assert np.array_equal(bst["v_z"][sl], st["v_z"]), p
    assert np.array_equal(bst["baseline"][sl], st["baseline"]), p
    assert np.array_equal(bst["key"][p], st["key"]), p


def _check(kw, hps, probs, keys, chunks, same=()):
    """every problem against its standalone engine; then non-vacuity over the pairs with the same data and key (`same`: pairs that must end
    EQUAL instead, see the module docstring)"""
    M = kw["n_particles"]
    bst = _swept(kw, hps, probs, keys, chunks)
    assert bst["z"].shape[0] == len(probs) * M and bst["key"].shape == (len(probs), 2)
    for p, ((x, mask), hp, key) in enumerate(zip(probs, hps, keys)):
        _assert_problem_equal(bst, p, M, _standalone(kw, hp, x, mask, key, chunks))
    n_pairs = 0
    for p, q in itertools.combinations(range(len(probs)), 2):
        if probs[p][0] is probs[q][0] and keys[p] == keys[q] and hps[p] != hps[q]:
            zp, zq = bst["z"][p * M:(p + 1) * M], bst["z"][q * M:(q + 1) * M]
            if (p, q) in same:
                assert np.array_equal(zp, zq), (p, q)
            else:
                assert not np.array_equal(zp, zq), (p, q, hps[p], hps[q])
                n_pairs += 1
    assert n_pairs > 0
    return bst


def _config2_case():
    d, M = 20, 32
    kw = dict(n_vars=d, n_particles=M, graph_prior="er")
    a, b, c = _problem(d, 100, 10), _problem(d, 80, 11, interv=True), _problem(d, 50, 12)
    probs = [a, a, a, a, b, b, c, c]
    keys = [3, 3, 3, 3, 4, 4, 5, 5]
    hps = [dict(),                                                       # none different: never set
           dict(ALL_SEVEN),                                              # every setting different
           dict(alpha_linear=0.5),
           dict(beta_linear=2.0, h_latent=8.0),
           dict(stepsize=0.002, score_function_baseline=0.01),
           dict(latent_prior_std=0.5),
           dict(edges_per_node=3),
           dict(h_latent=2.5, alpha_linear=1.5, latent_prior_std=0.1)]
    return kw, hps, probs, keys


def test_config2_shape_eight_problems_each_with_its_own_subset():
    kw, hps, probs, keys = _config2_case()
    _check(kw, hps, probs, keys, [(0, 6)])


def test_config2_shape_both_chunkings():
    kw, hps, probs, keys = _config2_case()
    a = _check(kw, hps, probs, keys, [(0, 5), (5, 3)])
    b = _swept(kw, hps, probs, keys, [(0, 8)])
    for k in ("z", "v_z", "baseline", "key"):
        assert np.array_equal(a[k], b[k]), k


def test_split_f16_acyclicity_tier():
    d, M = 50, 16
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=64, n_acyclicity_mc_samples=16)
    a, b = _problem(d, 100, 30), _problem(d, 70, 31, interv=True)
    # (the baseline of the reference is an average of log-likelihoods, ~ -1.3e4 at this size, and scales W_lik by exp(-baseline): a rate of
    #  0.01 overflows float32 within a step in any engine, so this size sweeps it at 1e-4)
    every = dict(ALL_SEVEN, score_function_baseline=1e-4)
    _check(kw, [dict(), every, dict(alpha_linear=0.6, h_latent=9.0)], [a, a, b], [1, 1, 2], [(0, 4)])


def test_tiled_kernel_matrix_with_two_bandwidths():
    d, M = 8, 128
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 60, 40)
    _check(kw, [dict(h_latent=2.0), dict(h_latent=20.0)], [a, a], [6, 6], [(0, 4)])


def test_gd_with_different_step_sizes():
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, optimizer="gd", n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 50, 41)
    _check(kw, [dict(), dict(stepsize=0.02), dict(stepsize=0.0007)], [a, a, a], [7, 7, 7], [(0, 5), (5, 3)])


def test_er_prior_edges_per_node():
    d, M = 20, 8
    kw = dict(n_vars=d, n_particles=M, graph_prior="er", n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 60, 42)
    _check(kw, [dict(edges_per_node=1), dict(), dict(edges_per_node=3)], [a, a, a], [8, 8, 8], [(0, 5)])


def test_sf_prior_edges_per_node():
    d, M = 20, 8
    kw = dict(n_vars=d, n_particles=M, graph_prior="sf", n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 60, 43)
    hps = [dict(edges_per_node=1), dict(), dict(edges_per_node=3), dict(edges_per_node=3, beta_linear=2.0)]
    # (the sf log-probability does not contain edges_per_node: problems 0, 1, 2 must end equal, see the module docstring)
    _check(kw, hps, [a] * 4, [9] * 4, [(0, 5)], same={(0, 1), (0, 2), (1, 2)})


def test_score_function_baseline_off_and_on():
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 50, 44)
    _check(kw, [dict(), dict(score_function_baseline=0.01)], [a, a], [10, 10], [(0, 6)])


def test_initial_particles_follow_latent_prior_std():
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    a = _problem(d, 50, 45)
    hps = [dict(), dict(latent_prior_std=0.5)]
    bst = _swept(kw, hps, [a, a], [11, 11], [])
    assert not np.array_equal(bst["z0"][:M], bst["z0"][M:])
    for p in range(2):
        assert np.array_equal(bst["z0"][p * M:(p + 1) * M], _standalone(kw, hps[p], *a, 11, [])["z0"]), p


def test_alpha_and_beta_of_a_step_equal_the_host_expression():
    """the standalone engine forms alpha = (float)(alpha_linear * t) in double on the host; the batched step forms it on the device"""
    d, M = 8, 4
    lin = [(1.0, 1.0), (0.1, 1.0 / 3.0), (0.7, 2.9), (1e-3, 123.456)]
    e = Engine(make_config(n_vars=d, n_particles=M, n_observations=50, n_problems=len(lin), n_grad_mc_samples=16, n_acyclicity_mc_samples=4))
    try:
        for p, (al, be) in enumerate(lin):
            e.set_data_problem(p, _problem(d, 50, 46)[0])
            if p:
                e.set_problem_hparams(p, alpha_linear=al, beta_linear=be)
        e.init_particles_batch(np.stack([random.PRNGKey(1)] * len(lin)))
        for t in (0, 1, 2, 3, 7, 10, 333, 1999, 123457):
            e.run(t, 1)
            got = e.read("PROBLEM_STEP").reshape(len(lin), 2)
            want = np.array([[np.float32(al * t), np.float32(be * t)] for al, be in lin], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (t, got, want)
    finally:
        e.close()


def test_sample_sweep_grid_equals_the_sample_runs_with_callbacks():
    d, M, steps, every = 8, 4, 20, 8   # (callback_every does not divide steps: the last chunk overshoots to step 24, as in sample())
    data, gm, lm = make_data(d, seed=80)
    grid = [(al, h) for al in (0.5, 1.0) for h in (3.0, 7.0)]
    ms = [MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, alpha_linear=al, kernel=AdditiveFrobeniusSEKernel,
                       kernel_param={"h": h}, n_grad_mc_samples=32, n_acyclicity_mc_samples=8) for al, h in grid] * 2
    keys = [21] * 4 + [22] * 4
    seen_b, seen_s = [], []
    gb = sample_sweep(ms, keys=keys, n_particles=M, steps=steps, callback_every=every,
                      callback=lambda dibs, t, zs: seen_b.append((id(dibs), t, zs.copy())))
    states = [dict(m.last_state) for m in ms[:4]]   # (of the second seed: every model object appears twice)
    assert len(gb) == 8
    n_chunks = -(-steps // every)
    for i, (m, k) in enumerate(zip(ms, keys)):
        g = m.sample(key=random.PRNGKey(k), n_particles=M, steps=steps, callback_every=every,
                     callback=lambda dibs, t, zs: seen_s.append((id(dibs), t, zs.copy())))
        assert np.array_equal(gb[i], g), i
        if i >= 4:
            for name in ("z", "v_z", "baseline", "key"):
                assert np.array_equal(states[i - 4][name], m.last_state[name]), (i, name)
    assert len(seen_b) == len(seen_s) == 8 * n_chunks
    for c in range(n_chunks):
        for i in range(8):
            ib, tb, zb = seen_b[c * 8 + i]
            is_, ts, zs = seen_s[i * n_chunks + c]
            assert ib == is_ == id(ms[i]) and tb == ts == (c + 1) * every
            assert np.array_equal(zb, zs), (c, i)
    # the grid is not vacuous: the four grid points of one seed end differently
    for i, j in itertools.combinations(range(4), 2):
        assert not np.array_equal(seen_b[-8 + i][2], seen_b[-8 + j][2]), (i, j)


def test_sweep_of_one_is_plain_sample():
    data, gm, lm = make_data(8, seed=90)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, alpha_linear=0.5, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    g1 = sample_sweep([m], keys=[5], n_particles=4, steps=4)[0]
    z1 = m.last_state["z"]
    g2 = m.sample(key=random.PRNGKey(5), n_particles=4, steps=4)
    assert np.array_equal(g1, g2) and np.array_equal(z1, m.last_state["z"])


def test_set_problem_hparams_rejections():
    d, M = 8, 4
    small = dict(n_vars=d, n_particles=M, n_observations=50, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    e = Engine(make_config(**small))
    try:
        with pytest.raises(_lib.DibsHipError, match="^batched engine: "):
            e.set_problem_hparams(0, alpha_linear=0.5)
        with pytest.raises(_lib.DibsHipError, match="^batched engine: "):
            e.get_problem_hparams(0)
    finally:
        e.close()
    e = Engine(make_config(n_problems=2, **small))
    try:
        with pytest.raises(_lib.DibsHipError, match="^batched engine: .*out of range"):
            e.set_problem_hparams(2, alpha_linear=0.5)
        with pytest.raises(_lib.DibsHipError, match="^batched engine: .*edge probability must be in \\(0, 1\\)"):
            e.set_problem_hparams(1, graph_prior_edges_per_node=3.5)   # (d = 8: p = 2 * 3.5 / 7 = 1)
        with pytest.raises(TypeError, match="tau"):
            e.set_problem_hparams(1, tau=0.5)
        assert e.get_problem_hparams(1).graph_prior_edges_per_node == 2.0   # (a refused call changes nothing)
        e.set_problem_hparams(1, alpha_linear=0.5)
        for p in range(2):
            e.set_data_problem(p, _problem(d, 50, 70 + p)[0])
        e.init_particles_batch(np.stack([random.PRNGKey(1), random.PRNGKey(2)]))
        with pytest.raises(_lib.DibsHipError, match="^batched engine: .*after the particles were initialised"):
            e.set_problem_hparams(0, alpha_linear=0.25)
        assert e.get_problem_hparams(1).alpha_linear == 0.5
        e.run(0, 2)
    finally:
        e.close()
    e = Engine(make_config(n_problems=2, **small))
    try:
        e.set_state(z=np.zeros((2 * M, d, d, 2), np.float32))
        with pytest.raises(_lib.DibsHipError, match="^batched engine: .*after the particles were initialised"):
            e.set_problem_hparams(0, stepsize=0.01)
    finally:
        e.close()
    e = Engine(make_config(n_vars=80, n_particles=2, n_observations=40, n_problems=2, n_grad_mc_samples=8, n_acyclicity_mc_samples=2))
    try:
        with pytest.raises(_lib.DibsHipError, match="^batched engine: .*n_vars <= 64"):
            e.set_problem_hparams(1, alpha_linear=0.5)
        e.set_problem_hparams(1, alpha_linear=1.0)   # (the configuration's own value: accepted at any size)
    finally:
        e.close()
