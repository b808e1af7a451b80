"""GPU tests of the chains engine (include/dibs_hip.h, n_chains > 1) and of sample_chains: chain c of a chains engine must end BIT-IDENTICAL
to a standalone engine run with key_c on the same data and the same chunking -- particles, parameters, RMSprop moments of both, the
score-function baselines and the loop-carry key.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from conftest import make_data
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu

STATE = ("z", "v_z", "theta", "v_theta", "baseline")


def _data(d, n_obs, seed=1, interv=False):
    data, gm, lm = make_data(d, n_obs=n_obs, seed=seed, joint=True)
    x = np.asarray(data.x, np.float32)[:n_obs]
    mask = None
    if interv:  # hard interventions on three nodes for a block of rows each
        mask = np.zeros(x.shape, np.int32)
        for q, j in enumerate((1, d // 2, d - 1)):
            mask[5 * q:5 * q + 4 + q, j] = 1
    return x, mask


def _lin(d, M, S=16, Sa=8, **kw):
    return dict(dict(n_vars=d, n_particles=M, joint=True, likelihood="lingauss", n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa), **kw)


def _nn(d, M, hidden, S=16, Sa=8, **kw):
    return dict(dict(n_vars=d, n_particles=M, joint=True, likelihood="densenn", nn_hidden=hidden, n_grad_mc_samples=S,
                     n_acyclicity_mc_samples=Sa), **kw)


def _standalone(kw, x, mask, key, chunks):
    e = Engine(make_config(n_observations=x.shape[0], has_interventions=mask is not None, **kw))
    try:
        e.set_data(x, mask)
        e.init_particles(random.PRNGKey(key))
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _chains(kw, x, mask, keys, chunks):
    e = Engine(make_config(n_observations=x.shape[0], has_interventions=mask is not None, n_chains=len(keys), **kw))
    try:
        e.set_data(x, mask)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _assert_chain_equal(cst, c, M, st):
    sl = slice(c * M, (c + 1) * M)
    assert np.isfinite(st["z"]).all() and np.isfinite(st["theta"]).all(), c
    assert np.isfinite(cst["z"][sl]).all() and np.isfinite(cst["theta"][sl]).all(), c
    for k in STATE:
        assert np.array_equal(cst[k][sl], st[k]), (c, k, np.abs(cst[k][sl].astype(np.float64) - st[k]).max())
    assert np.array_equal(cst["key"][c], st["key"]), c


def _check(kw, x, mask, keys, chunks):
    M = kw["n_particles"]
    cst = _chains(kw, x, mask, keys, chunks)
    assert cst["z"].shape[0] == cst["theta"].shape[0] == len(keys) * M and cst["key"].shape == (len(keys), 2)
    for c, key in enumerate(keys):
        _assert_chain_equal(cst, c, M, _standalone(kw, x, mask, key, chunks))
    return cst


CHUNKS = [(0, 5), (5, 3)]
# The score-function estimator with a baseline multiplies W_lik by exp(-b) in float32 (dibs.py:295-321), and b moves by
# score_function_baseline * mean_s log p(theta, D | G_s) per step: with log-probabilities of -1e4 .. -7e4 (40 observations of 8 variables
# against freshly drawn parameters) b passes -88.7 = -log(FLT_MAX) within three steps on most data sets and exp(-b) is inf -- in the
# standalone engine and in the reference alike.  The two score cases therefore use a data set on which the float64 CPU oracle
# (oracle/dibs_oracle.c, eight steps, the keys and masks used below) keeps every baseline above -57, 30 away from the overflow; found by
# scanning make_data seeds with the oracle alone.
SCORE_SEED = 382


# ---- 1, 2: LinearGaussian, the LDS-resident kernels at their smallest ------------------------------------------------------------------
def test_lingauss_baseline_case():
    x, mask = _data(8, 40)
    _check(_lin(8, 4), x, mask, [3, 4, 5, 6, 7], CHUNKS)


def test_lingauss_score_estimator_with_baseline():
    x, mask = _data(8, 40, seed=SCORE_SEED)
    _check(_lin(8, 4, grad_estimator_z="score", score_function_baseline=0.001), x, mask, [11, 12, 13], CHUNKS)


def test_lingauss_gd():
    x, mask = _data(8, 40)
    _check(_lin(8, 4, optimizer="gd"), x, mask, [11, 12, 13], CHUNKS)


@pytest.mark.parametrize("prior", ["sf", "uniform"])
def test_lingauss_graph_priors(prior):
    x, mask = _data(8, 40)
    _check(_lin(8, 4, graph_prior=prior), x, mask, [21, 22, 23], CHUNKS)


def test_lingauss_interventions():
    x, mask = _data(8, 40, interv=True)
    _check(_lin(8, 4), x, mask, [31, 32, 33], CHUNKS)


def test_lingauss_odd_sample_count_unpaired_kernel():
    x, mask = _data(8, 40)
    _check(_lin(8, 4, S=15), x, mask, [41, 42, 43], CHUNKS)


# ---- 3: the split-f16 tiers (k_lin_logprobs_hf, k_acyc_hf) ------------------------------------------------------------------------------
def test_lingauss_split_f16_tiers():
    x, mask = _data(40, 40)
    _check(_lin(40, 8), x, mask, [1, 2], [(0, 4)])


# ---- 4: the Gram path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interv", [True, False])
def test_lingauss_gram_path(interv):
    x, mask = _data(8, 300, interv=interv)
    _check(_lin(8, 4), x, mask, [51, 52], [(0, 4)])


# ---- 5: phi's FULL instantiation, the tiled kernel matrix ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [64, 128])
def test_lingauss_phi_full_and_tiled_kernel_matrix(M):
    x, mask = _data(8, 40)
    _check(_lin(8, M, S=8, Sa=8), x, mask, [61, 62], [(0, 3)])


# ---- 6: DenseNonlinearGaussian ---------------------------------------------------------------------------------------------------------
def test_densenn_one_hidden_layer():
    x, mask = _data(8, 40)
    _check(_nn(8, 4, (5,)), x, mask, [71, 72, 73], CHUNKS)


def test_densenn_score_no_bias_interventions():
    x, mask = _data(8, 40, seed=SCORE_SEED, interv=True)
    _check(_nn(8, 4, (5,), grad_estimator_z="score", score_function_baseline=0.001, nn_bias=False), x, mask, [74, 75, 76], CHUNKS)


def test_densenn_two_hidden_layers_general_path():
    x, mask = _data(12, 40)
    _check(_nn(12, 4, (6, 4), nn_activation="tanh"), x, mask, [77, 78], [(0, 4)])


def test_densenn_f16_logprob_tiers():
    x, mask = _data(40, 40)
    _check(_nn(40, 4, (8,), S=16), x, mask, [79, 80], [(0, 3)])


# ---- 7, 8 -----------------------------------------------------------------------------------------------------------------------------
def test_chunking_is_transparent():
    x, mask = _data(8, 40)
    a = _chains(_lin(8, 4), x, mask, [1, 2, 3], [(0, 10), (10, 10)])
    b = _chains(_lin(8, 4), x, mask, [1, 2, 3], [(0, 20)])
    for k in STATE + ("key",):
        assert np.array_equal(a[k], b[k]), k


def test_chains_are_isolated():
    M = 4
    x, mask = _data(8, 40)
    a = _chains(_lin(8, M), x, mask, [1, 2], [(0, 8)])
    b = _chains(_lin(8, M), x, mask, [1, 9], [(0, 8)])
    for k in STATE:
        assert np.array_equal(a[k][:M], b[k][:M]), k
        assert not np.array_equal(a[k][M:], b[k][M:]) or k == "baseline", k   # (the reparam estimator keeps no baseline)
    assert np.array_equal(a["key"][0], b["key"][0]) and not np.array_equal(a["key"][1], b["key"][1])


def test_engine_rules():
    from dibs_amd import _lib
    x, mask = _data(8, 40)
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin(8, 4)))
    try:
        pre = r"^chains engine \(n_chains > 1\): "
        with pytest.raises(_lib.DibsHipError, match="set_data has not been called"):
            e.run(0, 1)
        e.set_data(x, mask)
        with pytest.raises(_lib.DibsHipError, match=pre):
            e.init_particles(random.PRNGKey(0))
        with pytest.raises(_lib.DibsHipError, match=pre):
            e.set_data_problem(0, x)
        with pytest.raises(_lib.DibsHipError, match=pre):
            e.eval_gradients(1, keys_prior=np.zeros((8, 2), np.uint32))
        with pytest.raises(_lib.DibsHipError, match=pre):
            e.run_sharded(0, 1)
        with pytest.raises(_lib.DibsHipError, match=pre):
            e.comm_init(None)
        buf = np.zeros(e.gather_elems_per_rank(), np.float32)
        for call in (lambda: e.step_local(1, buf.ctypes.data), lambda: e.step_update(1, buf.ctypes.data),
                     lambda: e.step_local_grads(1, buf.ctypes.data), lambda: e.step_update_planes(1, buf.ctypes.data),
                     lambda: e.kmat_values(buf.ctypes.data, 1)):
            with pytest.raises(_lib.DibsHipError, match=pre):
                call()
        e.init_particles_batch(np.stack([random.PRNGKey(1), random.PRNGKey(2)]))
        k = np.array([[1, 2], [3, 4]], np.uint32)
        e.set_keys(k)
        assert np.array_equal(e.get_keys(), k)
        e.run(0, 2)
        assert e.read("THETA").size == 2 * 4 * 64 and e.read("KXX").size == 2 * 4 * 4
    finally:
        e.close()


# ---- 9: sample_chains against sequential sample() ---------------------------------------------------------------------------------------
def _leaves(theta):
    if isinstance(theta, np.ndarray):
        return [theta]
    return [leaf for layer in theta for leaf in layer]


def _model(kind):
    from dibs_amd.inference import JointDiBS
    if kind == "lingauss":
        data, gm, lm = make_data(8, n_obs=40, seed=1, joint=True)
    else:
        from dibs_amd.target import make_nonlinear_gaussian_model
        data, gm, lm = make_nonlinear_gaussian_model(key=random.PRNGKey(0), n_vars=8, graph_prior_str="er", n_observations=40)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8)


@pytest.mark.parametrize("kind", ["lingauss", "densenn"])
def test_sample_chains_equals_sequential_sample_with_callbacks(kind):
    from dibs_amd.inference import sample_chains
    M, steps, every = 4, 7, 3   # (callback_every does not divide steps: the last chunk overshoots to step 9, as in sample())
    m = _model(kind)
    keys = [11, 12, 13, 14]
    seen_c, seen_s = [], []
    rec = lambda seen: (lambda dibs, t, zs, thetas: seen.append((dibs, t, zs.copy(), [l.copy() for l in _leaves(thetas)])))
    m.last_state = "untouched"
    out = sample_chains(m, keys=keys, n_particles=M, steps=steps, callback_every=every, callback=rec(seen_c))
    assert m.last_state == "untouched" and len(out) == len(m.last_chain_states) == 4
    n_chunks = -(-steps // every)
    for c, k in enumerate(keys):
        g, theta = m.sample(key=random.PRNGKey(k), n_particles=M, steps=steps, callback_every=every, callback=rec(seen_s))
        assert np.array_equal(out[c][0], g), c
        la, lb = _leaves(out[c][1]), _leaves(theta)
        assert len(la) == len(lb) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(la, lb)), c
        cs = m.last_chain_states[c]
        assert set(cs) == set(m.last_state)
        for name in m.last_state:
            assert np.array_equal(cs[name], m.last_state[name]), (c, name)
    assert len(seen_c) == len(seen_s) == 4 * n_chunks
    for ch in range(n_chunks):   # after every chunk, every chain in order (the sequential runs give them chain by chain)
        for c in range(4):
            dc, tc, zc, thc = seen_c[ch * 4 + c]
            ds, ts, zs, ths = seen_s[c * n_chunks + ch]
            assert dc is ds is m and tc == ts == (ch + 1) * every
            assert np.array_equal(zc, zs) and len(thc) == len(ths) and all(np.array_equal(a, b) for a, b in zip(thc, ths)), (ch, c)


def test_sample_chains_marginal_model_goes_through_the_batched_engine():
    from dibs_amd.inference import MarginalDiBS, sample_chains
    data, gm, lm = make_data(8, seed=80)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    seen = []
    out = sample_chains(m, keys=[5, 6, 7], n_particles=4, steps=4, callback=lambda dibs, t, zs: seen.append((dibs, t)))
    assert [s[0] is m for s in seen] == [True] * 3 and not hasattr(m, "last_state")
    for c, k in enumerate((5, 6, 7)):
        g = m.sample(key=random.PRNGKey(k), n_particles=4, steps=4)
        assert np.array_equal(out[c], g)
        for name in ("z", "v_z", "baseline", "key"):
            assert np.array_equal(m.last_chain_states[c][name], m.last_state[name]), (c, name)


# ---- 10: chains whose particles have MANY weighted samples (tests/weight_states.py) -----------------------------------------------------
# Every case above runs steps 0 .. 8 from the initial draw: one weighted sample per particle, the gradient kernels' one-block form.  Here
# one launch holds a chain with one sample above the 2^-30 cut everywhere, a chain with 2 .. NS - 1 and a chain with more than NS (asserted
# on the oracles by tests/test_weight_states_host.py): the shares of a particle are dealt, summed and counted per chain row.
@pytest.mark.parametrize("name", ["lingauss_reparam", "lingauss_score", "densenn", "densenn_deep"])
def test_chains_with_many_weighted_samples(c_oracle64, name):
    import weight_states as W
    W.assert_chains_match_standalone([W.build(case, c_oracle64) for case in W.CHAIN_CASES[name]])
