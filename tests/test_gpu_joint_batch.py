"""GPU tests of per-chain data in the chains engine (include/dibs_hip.h, CHAINS ENGINE: dibs_engine_set_data_problem for every chain) and of
sample_joint_batch: chain c, run on data set c, must end BIT-IDENTICAL to a standalone engine given that data set and key_c with the same
chunking -- particles, parameters, RMSprop moments of both, the score-function baselines and the loop-carry key.  Every comparison is
np.array_equal, and every state is asserted finite."""
import os

import numpy as np
import pytest

from conftest import make_data
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu

STATE = ("z", "v_z", "theta", "v_theta", "baseline")
CHUNKS = [(0, 5), (5, 3)]
PRE = r"^chains engine \(n_chains > 1\): "


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


_standalone_cache = {}


def _standalone(kw, x, mask, key, chunks):
    """The reference of a chain: computed once per (settings, data, key, chunking), shared between the tests and never written to."""
    env = tuple(os.environ.get(k) for k in ("DIBS_LIN_GRAM", "DIBS_LIN_F32"))   # (path switches, latched when an engine is created: tuning.h)
    ident = (repr(sorted(kw.items())), x.tobytes(), None if mask is None else mask.tobytes(), key, repr(chunks), env)
    if ident not in _standalone_cache:
        e = Engine(make_config(n_observations=x.shape[0], has_interventions=mask is not None, **kw))
        try:
            e.set_data(x, mask)
            e.init_particles(random.PRNGKey(key))
            for t0, n in chunks:
                e.run(t0, n)
            st = e.get_state()
        finally:
            e.close()
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _standalone_cache[ident] = st
    return _standalone_cache[ident]


def _batch(kw, datasets, keys, chunks):
    """A chains engine with data set c = (x, mask) given to chain c through set_data_problem."""
    e = Engine(make_config(n_observations=datasets[0][0].shape[0], has_interventions=any(m is not None for _, m in datasets),
                           n_chains=len(keys), **kw))
    try:
        for c, (x, mask) in enumerate(datasets):
            e.set_data_problem(c, x, mask)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _assert_chain_equal(cst, c, M, st):
    sl = slice(c * M, (c + 1) * M)
    for k in STATE:
        assert np.isfinite(st[k]).all() and np.isfinite(cst[k][sl]).all(), (c, k)
        assert np.array_equal(cst[k][sl], st[k]), (c, k, np.abs(cst[k][sl].astype(np.float64) - st[k]).max())
    assert np.array_equal(cst["key"][c], st["key"]), c


def _check(kw, datasets, keys, chunks=CHUNKS):
    M = kw["n_particles"]
    cst = _batch(kw, datasets, keys, chunks)
    assert cst["z"].shape[0] == cst["theta"].shape[0] == len(keys) * M and cst["key"].shape == (len(keys), 2)
    for c, key in enumerate(keys):
        _assert_chain_equal(cst, c, M, _standalone(kw, datasets[c][0], datasets[c][1], key, chunks))
    return cst


def _sets(d, n_obs, seeds, interv=False):
    return [_data(d, n_obs, seed=s, interv=interv) for s in seeds]


# ---- 1: the LDS-resident kernels at their smallest (k_lin_logprobs_pair, k_lin_grad) --------------------------------------------------
CASE1_KEYS, CASE1_SEEDS = [3, 4, 5, 6, 7], [1, 2, 3, 4, 5]


def test_five_problems_reparam():
    _check(_lin(8, 4), _sets(8, 40, CASE1_SEEDS), CASE1_KEYS)


# ---- 2: mixed interventions: chains 0 and 2 with a mask, chain 1 without (its standalone engine: mask = None) ----------------------------
def test_mixed_interventions():
    sets = [_data(8, 40, seed=1, interv=True), _data(8, 40, seed=2), _data(8, 40, seed=3, interv=True)]
    assert sets[1][1] is None
    _check(_lin(8, 4), sets, [31, 32, 33])


# ---- 3: the unpaired kernel (odd S), plain gradient descent, the other graph priors ---------------------------------------------------
@pytest.mark.parametrize("kw", [dict(S=15), dict(optimizer="gd"), dict(graph_prior="sf"), dict(graph_prior="uniform")],
                         ids=["odd_S_unpaired_kernel", "gd", "prior_sf", "prior_uniform"])
def test_unpaired_kernel_gd_and_graph_priors(kw):
    _check(_lin(8, 4, **kw), _sets(8, 40, [1, 2, 3]), [41, 42, 43])


# ---- 4: the split-f16 tiers (k_lin_logprobs_hf, k_acyc_hf), and every instantiation the per-chain launchers choose ----------------------
def test_split_f16_tiers():
    _check(_lin(40, 8), _sets(40, 40, [1, 2]), [1, 2], [(0, 4)])   # k_lin_logprobs_hf<5, false, 8> (d <= 48)


# Both forms of the kernels are selected by one launch text (lin_launch.h, compiled in tu_lin.hip and tu_lin_chains.hip): one size per branch.
#   d = 50: hf<5, true> (49 <= d, ceil(d d / 512) <= 5), d = 56: hf<8, true>; d = 72: NT = 5, the paired kernel with EPQ = 0 and k_lin_grad<5>;
#   DIBS_LIN_F32=1 keeps the f32 paired kernel at 33 <= d <= 64: d = 40 has ceil(d d / 256) = 7 -> EPQ 10, d = 56 has 13 -> EPQ 16 (NT = 3, 4);
#   d = 20 with odd S: the unpaired kernel and the gradient kernel at NT = 2.
@pytest.mark.parametrize("d,S,f32", [(50, 16, False), (56, 16, False), (72, 16, False), (40, 16, True), (56, 16, True), (20, 15, False)],
                         ids=["hf5_four", "hf8_four", "nt5_pair_epq0", "f32_pair_epq10", "f32_pair_epq16", "nt2_unpaired"])
def test_every_instantiation_of_the_per_chain_launchers(d, S, f32, monkeypatch):
    if f32:
        monkeypatch.setenv("DIBS_LIN_F32", "1")
    _check(_lin(d, 4, S=S), _sets(d, 40, [1, 2]), [1, 2], [(0, 3)])


# ---- 5: the Gram path ---------------------------------------------------------------------------------------------------------------------
# joint_lin_fast_path (tu_lin.hip), the rule by which an engine takes the LDS-resident kernels: d <= 112 and x, the operand and the
# residuals of the gradient kernel fit LDS.  At d = 8 that holds up to about 1100 observations, so N = 300 takes the Gram path only when
# DIBS_LIN_GRAM=1 forces it (tuning.h, latched when an engine is created -- set before the chains engine AND the references exist).
def _fast_path(d, N):
    nt, np_, kp = (d + 15) // 16, (N + 15) & ~15, (d + 3) & ~3
    ld = 16 * nt + 2
    lds = (((np_ * ld + kp * ld + np_ * ld) * 4 + 15) & ~15) + 512      # lin_lds_bytes(d, N, nt, true), kernels_joint.h
    return d <= 112 and lds <= 160 * 1024 - 2048


GRAM_INTERV = [(True, True), (False, False), (True, False)]
GRAM_IDS = ["all_interv", "no_interv", "mixed"]


# Mixed batches are supported on the Gram path: the stacked matrices hold d per chain as soon as one chain has interventions, and a chain
# without them carries its single matrix d times -- the doubles its standalone engine reads (from LDS) in the same order of summation.
@pytest.mark.parametrize("interv", GRAM_INTERV, ids=GRAM_IDS)
def test_gram_path_forced(interv, monkeypatch):
    assert _fast_path(8, 300)   # (without the switch this size runs the LDS-resident kernels)
    kw, keys, chunks = _lin(8, 4), [51, 52], [(0, 4)]
    sets = [_data(8, 300, seed=1 + c, interv=iv) for c, iv in enumerate(interv)]
    lds_path = [_standalone(kw, x, mask, k, chunks) for (x, mask), k in zip(sets, keys)]
    monkeypatch.setenv("DIBS_LIN_GRAM", "1")
    cst = _check(kw, sets, keys, chunks)
    # that the Gram kernels ran: they evaluate the quadratic form in double from second moments, so their states differ from the LDS path's
    # in the last bits -- the references of this run are not those of the LDS path, and neither is the batch
    for c, (key, ref) in enumerate(zip(keys, lds_path)):
        gram_ref = _standalone(kw, sets[c][0], sets[c][1], key, chunks)
        assert not np.array_equal(gram_ref["z"], ref["z"]) and not np.array_equal(cst["z"][c * 4:(c + 1) * 4], ref["z"]), c


@pytest.mark.parametrize("interv", GRAM_INTERV, ids=GRAM_IDS)
def test_gram_path_by_size(interv):
    """1200 observations of 8 variables do not fit LDS: every engine here takes the Gram path by itself."""
    assert not _fast_path(8, 1200) and "DIBS_LIN_GRAM" not in os.environ
    _check(_lin(8, 4), [_data(8, 1200, seed=1 + c, interv=iv) for c, iv in enumerate(interv)], [53, 54], [(0, 4)])


def test_gram_path_single_matrix_read_through_the_caches(monkeypatch):
    """d = 104 without interventions: one Gram matrix per chain, which fits LDS beside the operand of the log-probability kernel
    (n_gram argument 1, ling_lds = 8 d d + 4 d d + 128 = 129 920 bytes) but not beside the two operands of the gradient kernel
    (8 d d + 8 d d + 128 = 173 184 > 160 KiB: n_gram argument -1, chain c's matrix read from global memory at stride ONE matrix)."""
    monkeypatch.setenv("DIBS_LIN_GRAM", "1")
    _check(_lin(104, 2, S=4, Sa=2), _sets(104, 40, [1, 2]), [55, 56], [(0, 2)])


def test_gram_path_global_operands_mixed_interventions():
    """d = 144 > 112 takes the Gram path by itself, and the gradient kernel keeps graph and masked weights in global scratch
    (ling_shape, `glob`: 8 d d + 128 > 159 KiB from d = 142); chain 0 has interventions (144 matrices), chain 1 its one matrix repeated.
    One step of plain gradient descent at t = 1: from 128 variables on the acyclicity gradient of a fresh particle is ~1.5^(d - 1), and
    its square leaves float32 in RMSprop's second moment -- in the standalone engine and the reference alike (test_gpu_parity.py,
    test_joint_lingauss_gram_path) -- so an RMSprop run at this size has no finite state to compare; t = 0 would have alpha = beta = 0."""
    assert not _fast_path(144, 40)
    _check(_lin(144, 2, S=4, Sa=2, optimizer="gd"), [_data(144, 40, seed=1, interv=True), _data(144, 40, seed=2)], [57, 58], [(1, 1)])


# ---- 6: the score-function estimator ----------------------------------------------------------------------------------------------------
# With a baseline, W_lik is multiplied by exp(-b) in float32 and b moves by score_function_baseline * mean_s log p per step; on most data
# sets of this size b passes -88.7 = -log(FLT_MAX) within a few steps and exp(-b) is inf, in the standalone engine and the reference alike
# (see SCORE_SEED in test_gpu_chains.py).  The data sets below were found as that one was: make_data(8, n_obs=40, seed=s, joint=True) for
# s in 0 .. 1199, eight steps of the float64 C oracle (oracle/dibs_oracle.c) on the CPU with the keys SCORE_KEYS, no mask, S = 16, Sa = 8,
# score_function_baseline = 0.001; a seed qualifies when every baseline of every one of the four keys stays above -57 over the eight steps
# (more than the test needs: chain c runs key c on data set c only).  37 of the 1200 seeds qualify: 3, 56, 68, 77, 83, 90, 183, 217, 224,
# 358, 382, 392, 420, 495, 530, 540, 576, 580, 589, 603, 604, 609, 628, 638, 639, 654, 701, 760, 763, 837, 843, 878, 947, 963, 1045, 1051,
# 1141.  Used: the four with the widest margin, lowest baseline -43.3 (382), -31.4 (420), -38.0 (654), -38.0 (1045).
SCORE_KEYS = [81, 82, 83, 84]
SCORE_SEEDS = [382, 420, 654, 1045]


def test_score_estimator_without_baseline():
    _check(_lin(8, 4, grad_estimator_z="score"), _sets(8, 40, [1, 2, 3]), [11, 12, 13])


def test_score_estimator_with_baseline():
    _check(_lin(8, 4, grad_estimator_z="score", score_function_baseline=0.001), _sets(8, 40, SCORE_SEEDS), SCORE_KEYS)


# ---- 7: phi's FULL instantiation and the tiled kernel matrix with per-chain data ------------------------------------------------------
def test_phi_full_and_tiled_kernel_matrix():
    _check(_lin(8, 64, S=8, Sa=8), _sets(8, 40, [1, 2]), [61, 62], [(0, 3)])


# ---- 8: isolation; per-chain copies of one data set equal the shared-data engine -------------------------------------------------------
def test_chains_are_isolated_from_each_others_data():
    M, kw = 4, _lin(8, 4)
    sets = _sets(8, 40, CASE1_SEEDS)
    a = _batch(kw, sets, CASE1_KEYS, CHUNKS)
    other = list(sets)
    other[1] = _data(8, 40, seed=9)
    b = _batch(kw, other, CASE1_KEYS, CHUNKS)
    for c in range(5):
        sl = slice(c * M, (c + 1) * M)
        for k in ("z", "v_z", "theta", "v_theta"):
            assert np.array_equal(a[k][sl], b[k][sl]) == (c != 1), (c, k)
        assert np.array_equal(a["key"][c], b["key"][c]), c   # (the keys do not depend on the data)


@pytest.mark.parametrize("interv", [False, True])
def test_same_data_for_every_chain_equals_the_shared_data_engine(interv):
    kw, keys = _lin(8, 4), [1, 2, 3]
    x, mask = _data(8, 40, interv=interv)
    a = _batch(kw, [(x, mask)] * 3, keys, CHUNKS)
    e = Engine(make_config(n_observations=40, has_interventions=interv, n_chains=3, **kw))
    try:
        e.set_data(x, mask)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in CHUNKS:
            e.run(t0, n)
        b = e.get_state()
    finally:
        e.close()
    for k in STATE + ("key",):
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


# ---- 9: the rules of the engine -----------------------------------------------------------------------------------------------------------
def test_engine_rules():
    from dibs_amd import _lib
    x, mask = _data(8, 40)
    keys = np.stack([random.PRNGKey(1), random.PRNGKey(2), random.PRNGKey(3)])
    e = Engine(make_config(n_observations=40, n_chains=3, **_lin(8, 4)))
    try:
        with pytest.raises(_lib.DibsHipError, match="set_data has not been called"):   # (no data at all: today's message)
            e.run(0, 1)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: chain index 3 out of range"):
            e.set_data_problem(3, x)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: chain index -1 out of range"):
            e.set_data_problem(-1, x)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: n_obs = 39 but dibs_config.n_observations = 40"):
            e.set_data_problem(0, x[:39])
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: bge_mean_obs must be NULL"):
            e.set_data_problem(0, x, None, np.zeros(8, np.float32))
        with pytest.raises(_lib.DibsHipError, match="set_data has not been called"):   # (the refused calls left no data behind)
            e.run(0, 1)
        e.set_data_problem(0, x)
        e.set_data_problem(2, x, np.zeros(x.shape, np.int32))
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data after dibs_engine_set_data_problem is not supported"):
            e.set_data(x, mask)
        e.init_particles_batch(keys)   # (initialising needs no data; hyper-parameters and, from here on, the data are final)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_run: dibs_engine_set_data_problem has not been called for chain 1"):
            e.run(0, 1)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: called after the particles were initialised"):
            e.set_data_problem(1, x)
    finally:
        e.close()
    # every chain given its data, then the particles: runs; a chain's data may be given again before the particles are initialised
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin(8, 4)))
    try:
        e.set_data_problem(0, x)
        e.set_data_problem(1, x)
        e.set_data_problem(0, _data(8, 40, seed=2)[0])
        e.init_particles_batch(keys[:2])
        e.run(0, 2)
        assert np.isfinite(e.get_state()["z"]).all()
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: called after the particles were initialised"):
            e.set_data_problem(0, x)
    finally:
        e.close()
    # shared data first: per-chain data is refused, naming the shared data set (the case test_gpu_chains.py pins)
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin(8, 4)))
    try:
        e.set_data(x, mask)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem after dibs_engine_set_data is not supported "
                                                          r"\(the chains share the data set given by dibs_engine_set_data"):
            e.set_data_problem(0, x)
    finally:
        e.close()
    # DenseNonlinearGaussian chains share one data set
    e = Engine(make_config(n_observations=40, n_chains=2, **dict(_lin(8, 4), likelihood="densenn", nn_hidden=(5,))))
    try:
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data_problem: per-chain data is LinearGaussian only "
                                                          r"\(DenseNonlinearGaussian chains share one data set"):
            e.set_data_problem(0, x)
    finally:
        e.close()


# ---- 10: sample_joint_batch against sequential sample() ----------------------------------------------------------------------------------
def _model(seed):
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(8, n_obs=40, seed=seed, joint=True)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8)


def test_sample_joint_batch_equals_sequential_sample_with_callbacks():
    from dibs_amd.inference import sample_joint_batch
    M, steps, every = 4, 7, 3   # (callback_every does not divide steps: the last chunk overshoots to step 9, as in sample())
    batch, seq = [_model(s) for s in (1, 2, 3)], [_model(s) for s in (1, 2, 3)]
    keys = [11, 12, 13]
    seen_b, seen_s = [], []
    rec = lambda seen: (lambda dibs, t, zs, thetas: seen.append((dibs, t, zs.copy(), thetas.copy())))
    out = sample_joint_batch(batch, keys=keys, n_particles=M, steps=steps, callback_every=every, callback=rec(seen_b))
    n_chunks = -(-steps // every)
    assert len(out) == 3
    for i, k in enumerate(keys):
        g, theta = seq[i].sample(key=random.PRNGKey(k), n_particles=M, steps=steps, callback_every=every, callback=rec(seen_s))
        assert out[i][0].shape == g.shape and np.array_equal(out[i][0], g), i
        assert out[i][1].shape == theta.shape and np.isfinite(theta).all() and np.array_equal(out[i][1], theta), i
        assert set(batch[i].last_state) == set(seq[i].last_state)
        for name in seq[i].last_state:
            a, b = batch[i].last_state[name], seq[i].last_state[name]
            assert a is not None and a.shape == b.shape and np.array_equal(a, b), (i, name)
        assert batch[i].latent_prior_std == seq[i].latent_prior_std
    assert len(seen_b) == len(seen_s) == 3 * n_chunks
    for ch in range(n_chunks):   # after every chunk, every problem in order (the sequential runs give them problem by problem)
        for i in range(3):
            db, tb, zb, thb = seen_b[ch * 3 + i]
            ds, ts, zs, ths = seen_s[i * n_chunks + ch]
            assert db is batch[i] and ds is seq[i] and tb == ts == (ch + 1) * every
            assert np.array_equal(zb, zs) and np.array_equal(thb, ths), (ch, i)


# ---- per-chain data with MANY weighted samples (tests/weight_states.py) -------------------------------------------------------------------
# Every case above runs from the initial draw: one weighted sample per particle.  Here chain c has its own data set AND a state built on it
# with one sample above the 2^-30 cut everywhere (chain 0), 2 .. NS - 1 (chain 1, with interventions in the first case) and more than NS
# (chain 2): the per-chain forms of k_lin_grad / k_ling_grad deal, sum and count a particle's shares.  GRAD_THETA, W_LIK after run(t, 1) and
# the state after three further steps, bit for bit against standalone engines.
@pytest.mark.parametrize("name", ["data_lingauss", "data_gram_n300"])
def test_per_chain_data_with_many_weighted_samples(c_oracle64, monkeypatch, name):
    import weight_states as W
    bs = [W.build(case, c_oracle64) for case in W.CHAIN_CASES[name]]
    if bs[0]["gram"]:
        monkeypatch.setenv("DIBS_LIN_GRAM", "1")
    W.assert_chains_match_standalone(bs, per_chain_data=True)
