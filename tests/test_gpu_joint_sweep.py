"""GPU tests of the per-chain hyper-parameters of the chains engine (include/dibs_hip.h, dibs_engine_set_chain_hparams) and of
sample_joint_sweep: chain c, run with its own values on data set c, must end BIT-IDENTICAL to a standalone engine configured with those
values, that data set and key_c with the same chunking -- particles, parameters, RMSprop moments of both, the score-function baselines and
the loop-carry key.  Every comparison is np.array_equal, and every state is asserted finite.  Every case runs at least three steps, so
that alpha and beta are non-zero and differ between the chains and both RMSprop moments have moved."""
import os

import numpy as np
import pytest

from conftest import make_data
from dibs_amd import random
from dibs_amd._abi import JOINT_SWEEPABLE, chain_hparams, make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu

STATE = ("z", "v_z", "theta", "v_theta", "baseline")
CHUNKS = [(0, 3)]
PRE = r"^chains engine \(n_chains > 1\): "
# make_config's keyword of a per-chain field where it is not the field's name
_KW = {"graph_prior_edges_per_node": "edges_per_node"}
# data sets on which the score-function baselines stay finite (tests/test_gpu_joint_batch.py, SCORE_SEEDS: how they were found)
SCORE_SEEDS = [382, 420, 654, 1045]


def _data(d, n_obs, seed=1, interv=False):
    data, gm, lm = make_data(d, n_obs=n_obs, seed=seed, joint=True)
    x = np.asarray(data.x, np.float32)[:n_obs]
    mask = None
    if interv:  # hard interventions on three nodes for a block of rows each
        mask = np.zeros(x.shape, np.int32)
        for q, j in enumerate((1, d // 2, d - 1)):
            mask[5 * q:5 * q + 4 + q, j] = 1
    return x, mask


def _lin(d=8, M=4, S=16, Sa=4, **kw):
    return dict(dict(n_vars=d, n_particles=M, joint=True, likelihood="lingauss", n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa), **kw)


def _cfg_kw(kw, hp):
    """make_config keywords of a standalone engine configured with the chain's own values"""
    return dict(kw, **{_KW.get(f, f): v for f, v in hp.items()})


_standalone_cache = {}


def _standalone(kw, x, mask, key, chunks):
    """The reference of a chain: computed once per (settings, data, key, chunking), shared between the tests and never written to."""
    env = tuple(os.environ.get(k) for k in ("DIBS_LIN_GRAM", "DIBS_LIN_F32", "DIBS_KMAT_TILED_MIN"))   # (latched at creation: tuning.h)
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


def _sweep(kw, datasets, keys, hps, chunks, set_all=False):
    """A chains engine with data set c and the values hps[c] (a dict of per-chain fields; empty: never set, unless set_all) for chain c."""
    e = Engine(make_config(n_observations=datasets[0][0].shape[0], has_interventions=any(m is not None for _, m in datasets),
                           n_chains=len(keys), **kw))
    try:
        for c, (x, mask) in enumerate(datasets):
            e.set_data_problem(c, x, mask)
            if hps[c] or set_all:
                e.set_chain_hparams(c, **hps[c])
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


def _check(kw, datasets, keys, hps, chunks=CHUNKS):
    M = kw["n_particles"]
    cst = _sweep(kw, datasets, keys, hps, chunks)
    assert cst["z"].shape[0] == cst["theta"].shape[0] == len(keys) * M and cst["key"].shape == (len(keys), 2)
    refs = [_standalone(_cfg_kw(kw, hps[c]), datasets[c][0], datasets[c][1], key, chunks) for c, key in enumerate(keys)]
    for c in range(len(keys)):
        _assert_chain_equal(cst, c, M, refs[c])
    return cst, refs


def _differ(refs, a, b):
    """the references of chains a and b differ (the swept field reached the computation)"""
    return not np.array_equal(refs[a]["z"], refs[b]["z"])


# ---- 1: one field at a time; chain 0 keeps the configuration's values ------------------------------------------------------------------
ONE_FIELD = [
    ("alpha_linear", {}, [0.1, 0.02]),
    ("beta_linear", {}, [2.0, 0.5]),
    ("h_latent", {}, [3.0, 8.0]),
    ("h_theta", {}, [100.0, 250.0]),
    ("stepsize", {}, [0.01, 0.002]),
    ("score_function_baseline", dict(grad_estimator_z="score", score_function_baseline=0.001), [0.002, 0.0]),
    ("latent_prior_std", {}, [0.5, 0.2]),
    ("graph_prior_edges_per_node", dict(graph_prior="er"), [1.0, 1.5]),
]
assert [f for f, _, _ in ONE_FIELD] == list(JOINT_SWEEPABLE)   # (the eight fields, each once)


@pytest.mark.parametrize("field,extra,values", ONE_FIELD, ids=[f for f, _, _ in ONE_FIELD])
def test_one_field_at_a_time(field, extra, values):
    kw = _lin(**extra)
    score = field == "score_function_baseline"
    sets = [_data(8, 40, seed=s) for s in SCORE_SEEDS[:3]] if score else [_data(8, 40)] * 3   # (one data set, uploaded per chain)
    keys = [81, 82, 83] if score else [3, 3, 3]   # (same key and data: the chains differ in the field alone)
    _, refs = _check(kw, sets, keys, [{}] + [{field: v} for v in values])
    if not score:
        assert _differ(refs, 0, 1) and _differ(refs, 0, 2) and _differ(refs, 1, 2), field


# ---- 2: all fields at once ------------------------------------------------------------------------------------------------------------------
def _all_fields(est, i):
    hp = dict(alpha_linear=[0.1, 0.02][i], beta_linear=[2.0, 0.5][i], h_latent=[3.0, 8.0][i], h_theta=[100.0, 250.0][i],
              stepsize=[0.01, 0.002][i], latent_prior_std=[0.5, 0.2][i], graph_prior_edges_per_node=[1.0, 1.5][i])
    if est == "score":
        hp["score_function_baseline"] = [0.002, 0.0][i]
    return hp


@pytest.mark.parametrize("prior", ["er", "sf"])
@pytest.mark.parametrize("opt", ["rmsprop", "gd"])
@pytest.mark.parametrize("est", ["reparam", "score"])
def test_all_fields_at_once(est, opt, prior):
    kw = _lin(grad_estimator_z=est, optimizer=opt, graph_prior=prior, **(dict(score_function_baseline=0.001) if est == "score" else {}))
    _, refs = _check(kw, [_data(8, 40, seed=s) for s in SCORE_SEEDS[:3]], [81, 82, 83], [{}, _all_fields(est, 0), _all_fields(est, 1)])
    assert _differ(refs, 0, 1) and _differ(refs, 1, 2)


# ---- 3: every _chains instantiation reachable with n_vars <= 64 ------------------------------------------------------------------------
# Read off lin_logprobs / lin_launch_pair / lin_launch_hf / lin_all_grads (lin_launch.h) and batch_launch_acyc_power (tu_batch.hip), NT = ceil(d / 16) <= 4:
#   even S (legacy PRNG layout, N <= 128), d <= 32: k_lin_logprobs_pair_chains<1, 4> (d = 8), <2, 4> (d = 20: two tiles);
#   33 <= d: k_lin_logprobs_hf_chains<5, false, 8> (d = 40), <5, true, 8> (d = 50: ceil(d d / 512) <= 5), <8, true, 8> (d = 56);
#   DIBS_LIN_F32=1 keeps the paired f32 kernel there: <3, 10> (d = 40), <4, 10> (d = 50: ceil(d d / 256) = 10), <4, 16> (d = 56);
#   odd S: the unpaired k_lin_logprobs_chains<NT>, NT = 1 .. 4 (d = 8, 20, 40, 56); k_lin_grad_chains<NT> at the same four sizes;
#   acyclicity: k_acyc_hf_batch<false> (33 <= d <= 48), <true> (d >= 49) with paired chains (even Sa), k_acyc_batch<NT, true> below, and
#   with odd Sa k_acyc_batch<NT, false> at every size;
#   the Gram kernels k_ling_logprobs_chains / k_ling_grad_chains: case 4.
# Also: n_dim < n_vars once, and 64 particles with DIBS_KMAT_TILED_MIN=64 -- the tiled kernel matrix (k_kmat_tile_chains_hp) and phi's FULL form.
INST = [
    ("pair_nt2_two_tiles", dict(d=20), None),
    ("hf5", dict(d=40), None),
    ("hf5_four", dict(d=50), None),
    ("hf8_four", dict(d=56), None),
    ("f32_pair_nt3_epq10", dict(d=40), ("DIBS_LIN_F32", "1")),
    ("f32_pair_nt4_epq10", dict(d=50), ("DIBS_LIN_F32", "1")),
    ("f32_pair_nt4_epq16", dict(d=56), ("DIBS_LIN_F32", "1")),
    ("unpaired_nt1_odd_Sa", dict(d=8, S=15, Sa=3), None),
    ("unpaired_nt2_odd_Sa", dict(d=20, S=15, Sa=3), None),
    ("unpaired_nt3_odd_Sa", dict(d=40, S=15, Sa=3), None),
    ("unpaired_nt4_odd_Sa", dict(d=56, S=15, Sa=3), None),
    ("k_below_d", dict(d=8, n_dim=5), None),
    ("tiled_kmat_phi_full", dict(d=8, M=64, S=8), ("DIBS_KMAT_TILED_MIN", "64")),
]


@pytest.mark.parametrize("name,shape,env", INST, ids=[n for n, _, _ in INST])
def test_every_instantiation_of_the_per_chain_kernels(name, shape, env, monkeypatch):
    if env:
        monkeypatch.setenv(*env)
    kw = _lin(**shape)
    d = kw["n_vars"]
    hp = dict(alpha_linear=0.1, beta_linear=2.0, h_latent=3.0, h_theta=100.0, stepsize=0.01, latent_prior_std=0.5,
              graph_prior_edges_per_node=1.0)
    _, refs = _check(kw, [_data(d, 40, seed=1), _data(d, 40, seed=2)], [1, 2], [{}, hp])


# ---- 4: the Gram path; the chains differ in alpha_linear ----------------------------------------------------------------------------------
GRAM_INTERV = [(True, True), (False, False), (True, False)]
GRAM_IDS = ["all_interv", "no_interv", "mixed"]
GRAM_HPS = [{}, dict(alpha_linear=0.1)]


@pytest.mark.parametrize("interv", GRAM_INTERV, ids=GRAM_IDS)
def test_gram_path_forced(interv, monkeypatch):
    kw, keys = _lin(), [51, 52]
    sets = [_data(8, 300, seed=1 + c, interv=iv) for c, iv in enumerate(interv)]
    lds_path = [_standalone(_cfg_kw(kw, hp), x, mask, k, CHUNKS) for (x, mask), k, hp in zip(sets, keys, GRAM_HPS)]
    monkeypatch.setenv("DIBS_LIN_GRAM", "1")
    cst, refs = _check(kw, sets, keys, GRAM_HPS)
    for c in range(2):   # (that the Gram kernels ran: double-precision second moments, other last bits than the LDS-resident kernels)
        assert not np.array_equal(refs[c]["z"], lds_path[c]["z"]), c


@pytest.mark.parametrize("interv", GRAM_INTERV, ids=GRAM_IDS)
def test_gram_path_by_size(interv):
    """1200 observations of 8 variables do not fit LDS: every engine here takes the Gram path by itself."""
    assert "DIBS_LIN_GRAM" not in os.environ
    _check(_lin(), [_data(8, 1200, seed=1 + c, interv=iv) for c, iv in enumerate(interv)], [53, 54], GRAM_HPS)


# ---- 5: per-chain data and per-chain values together ------------------------------------------------------------------------------------
def test_per_chain_data_and_values_together():
    sets = [_data(8, 40, seed=1, interv=True), _data(8, 40, seed=2), _data(8, 40, seed=3, interv=True), _data(8, 40, seed=4)]
    hps = [dict(alpha_linear=0.1), {}, dict(h_latent=3.0, stepsize=0.01), dict(beta_linear=2.0, h_theta=100.0, latent_prior_std=0.5)]
    _check(_lin(), sets, [31, 32, 33, 34], hps, [(0, 4)])


# ---- 6: isolation ---------------------------------------------------------------------------------------------------------------------------
def test_changing_one_chains_values_leaves_the_others_bit_identical():
    kw, sets, keys = _lin(), [_data(8, 40, seed=s) for s in (1, 2, 3)], [41, 42, 43]
    a = _sweep(kw, sets, keys, [{}, dict(alpha_linear=0.1), dict(h_latent=3.0)], CHUNKS)
    b = _sweep(kw, sets, keys, [{}, dict(alpha_linear=0.2, stepsize=0.01), dict(h_latent=3.0)], CHUNKS)
    for c in range(3):
        sl = slice(c * 4, (c + 1) * 4)
        for k in ("z", "v_z", "theta", "v_theta"):
            assert np.isfinite(a[k]).all() and np.array_equal(a[k][sl], b[k][sl]) == (c != 1), (c, k)
        assert np.array_equal(a["key"][c], b["key"][c]), c   # (the keys do not depend on the values)


# ---- 7: chunking ----------------------------------------------------------------------------------------------------------------------------
def test_one_chunk_equals_two():
    kw, sets, keys = _lin(), [_data(8, 40, seed=s) for s in (1, 2)], [61, 62]
    hps = [dict(alpha_linear=0.1, beta_linear=2.0), dict(h_latent=3.0, h_theta=100.0, stepsize=0.01)]
    a = _sweep(kw, sets, keys, hps, [(0, 4)])
    b = _sweep(kw, sets, keys, hps, [(0, 2), (2, 2)])
    for k in STATE + ("key",):
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    for c in range(2):
        _assert_chain_equal(b, c, 4, _standalone(_cfg_kw(kw, hps[c]), sets[c][0], sets[c][1], keys[c], [(0, 2), (2, 2)]))


# ---- 8: values equal to the configuration's run the path of an engine on which nothing was set ----------------------------------------
def test_configuration_values_change_nothing():
    kw, sets, keys = _lin(), [_data(8, 40, seed=s) for s in (1, 2)], [71, 72]
    cfg = make_config(n_observations=40, **kw)
    same = {f: getattr(cfg, f) for f in JOINT_SWEEPABLE}
    a = _sweep(kw, sets, keys, [{}, {}], CHUNKS)
    b = _sweep(kw, sets, keys, [same, same], CHUNKS, set_all=True)
    for k in STATE + ("key",):
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    # ... also on shared data, on a DenseNonlinearGaussian engine and beyond 64 latent dimensions, where differing values are refused
    x, mask = sets[0]
    for extra, shared in ((dict(), True), (dict(likelihood="densenn", nn_hidden=(5,)), True), (dict(n_dim=65), False)):
        kw2 = dict(kw, **extra)
        c2 = make_config(n_observations=40, n_chains=2, **kw2)
        e = Engine(c2)
        try:
            if shared:
                e.set_data(x, mask)
            else:
                e.set_data_problem(0, x)
                e.set_data_problem(1, x)
            e.set_chain_hparams(1, **{f: getattr(c2, f) for f in JOINT_SWEEPABLE})
            e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
            e.run(0, 3)
            st = e.get_state()
        finally:
            e.close()
        _assert_chain_equal(st, 1, 4, _standalone(kw2, x, None, keys[1], CHUNKS))


# ---- 9: the rules of the engine ---------------------------------------------------------------------------------------------------------
def test_engine_rules(monkeypatch):
    from dibs_amd import _lib
    x, mask = _data(8, 40)
    keys = np.stack([random.PRNGKey(1), random.PRNGKey(2), random.PRNGKey(3)])
    SET, GET = PRE + "dibs_engine_set_chain_hparams: ", PRE + "dibs_engine_get_chain_hparams: "
    cfg = make_config(n_observations=40, n_chains=3, **_lin())
    e = Engine(cfg)
    try:
        for c in range(3):   # a chain never set has the configuration's values
            hp = e.get_chain_hparams(c)
            assert all(getattr(hp, f) == getattr(cfg, f) for f in JOINT_SWEEPABLE), c
        e.set_chain_hparams(1, alpha_linear=0.1, h_theta=100.0, latent_prior_std=0.5)
        hp = e.get_chain_hparams(1)   # round trip
        assert (hp.alpha_linear, hp.h_theta, hp.latent_prior_std, hp.beta_linear, hp.h_latent) == (0.1, 100.0, 0.5, cfg.beta_linear, cfg.h_latent)
        assert e.get_chain_hparams(0).alpha_linear == cfg.alpha_linear == e.get_chain_hparams(2).alpha_linear
        with pytest.raises(_lib.DibsHipError, match=SET + "chain index 3 out of range"):
            e.set_chain_hparams(3, e.get_chain_hparams(0))
        with pytest.raises(_lib.DibsHipError, match=GET + "chain index -1 out of range"):
            e.get_chain_hparams(-1)
        with pytest.raises(_lib.DibsHipError, match=SET + "chain 2: Erdos-Renyi prior: edge probability must be in"):
            e.set_chain_hparams(2, graph_prior_edges_per_node=3.5)   # (d = 8: p = 2 * 3.5 / 7 = 1)
        with pytest.raises(TypeError, match="tau is not a per-chain setting"):
            e.set_chain_hparams(2, tau=0.5)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_problem_hparams .*dibs_engine_set_chain_hparams"):
            e.set_problem_hparams(0, alpha_linear=0.5)
        # differing values and no data at all / one shared data set
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_run: some chain's hyper-parameters differ .*needs per-chain data"):
            e.run(0, 1)
        with pytest.raises(_lib.DibsHipError, match=PRE + "dibs_engine_set_data: some chain's hyper-parameters differ .*needs per-chain data"):
            e.set_data(x, mask)
        for c in range(3):
            e.set_data_problem(c, x)
        e.init_particles_batch(keys)
        with pytest.raises(_lib.DibsHipError, match=SET + "called after the particles were initialised"):
            e.set_chain_hparams(0, alpha_linear=0.2)
        assert e.get_chain_hparams(1).alpha_linear == 0.1   # (reading stays allowed)
        e.run(0, 3)
        assert np.isfinite(e.get_state()["z"]).all()
    finally:
        e.close()
    # the other order: shared data first, then differing values
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin()))
    try:
        e.set_data(x, mask)
        with pytest.raises(_lib.DibsHipError, match=SET + "chain 1: hyper-parameters that differ .*need per-chain data .*dibs_engine_set_data"):
            e.set_chain_hparams(1, stepsize=0.01)
    finally:
        e.close()
    # DenseNonlinearGaussian: no per-chain forms
    e = Engine(make_config(n_observations=40, n_chains=2, **dict(_lin(), likelihood="densenn", nn_hidden=(5,))))
    try:
        with pytest.raises(_lib.DibsHipError, match=SET + "chain 0: hyper-parameters that differ .*are LinearGaussian only"):
            e.set_chain_hparams(0, alpha_linear=0.1)
    finally:
        e.close()
    # beyond 64 latent dimensions, and on the bf16 acyclicity pipe
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin(n_dim=65)))
    try:
        with pytest.raises(_lib.DibsHipError, match=SET + r"chain 0: hyper-parameters that differ .*need n_vars <= 64 and n_dim <= 64 \(got 8, 65\)"):
            e.set_chain_hparams(0, alpha_linear=0.1)
    finally:
        e.close()
    monkeypatch.setenv("DIBS_ACYC_BF16", "1")
    e = Engine(make_config(n_observations=40, n_chains=2, **_lin()))
    monkeypatch.delenv("DIBS_ACYC_BF16")
    try:
        with pytest.raises(_lib.DibsHipError, match=SET + "chain 0: hyper-parameters that differ .*an acyclicity pipe other than bf16"):
            e.set_chain_hparams(0, alpha_linear=0.1)
    finally:
        e.close()
    # not a chains engine
    e = Engine(make_config(n_observations=40, **_lin()))
    try:
        with pytest.raises(_lib.DibsHipError, match=SET + "needs a chains engine"):
            e.set_chain_hparams(0, chain_hparams(cfg))
        with pytest.raises(_lib.DibsHipError, match=GET + "needs a chains engine"):
            e.get_chain_hparams(0)
    finally:
        e.close()


# ---- 10: sample_joint_sweep against sequential sample() ---------------------------------------------------------------------------------
def _grid():
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(8, n_obs=40, seed=1, joint=True)
    return [JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=4, alpha_linear=al,
                      kernel_param={"h_latent": h, "h_theta": 500.0}) for al in (0.05, 0.1) for h in (5.0, 3.0)]


@pytest.mark.parametrize("with_callback", [False, True], ids=["no_callback", "callback"])
def test_sample_joint_sweep_equals_sequential_sample(with_callback):
    from dibs_amd.inference import sample_joint_sweep
    M, steps, every = 4, 5, 2   # (callback_every does not divide steps: the last chunk overshoots to step 6, as in sample())
    sweep, seq, keys = _grid(), _grid(), [11, 12, 13, 14]
    seen_b, seen_s = [], []
    rec = lambda seen: (lambda dibs, t, zs, thetas: seen.append((dibs, t, zs.copy(), thetas.copy())))
    cb = dict(callback_every=every, callback=rec(seen_b)) if with_callback else {}
    out = sample_joint_sweep(sweep, keys=keys, n_particles=M, steps=steps, **cb)
    assert len(out) == 4
    for i, k in enumerate(keys):
        cs = dict(callback_every=every, callback=rec(seen_s)) if with_callback else {}
        g, theta = seq[i].sample(key=random.PRNGKey(k), n_particles=M, steps=steps, **cs)
        assert out[i][0].shape == g.shape and np.array_equal(out[i][0], g), i
        assert out[i][1].shape == theta.shape and np.isfinite(theta).all() and np.array_equal(out[i][1], theta), i
        assert set(sweep[i].last_state) == set(seq[i].last_state)
        for name in seq[i].last_state:
            a, b = sweep[i].last_state[name], seq[i].last_state[name]
            assert a is not None and a.shape == b.shape and np.array_equal(a, b), (i, name)
        assert sweep[i].latent_prior_std == seq[i].latent_prior_std
    for i in range(1, 4):   # (the grid points differ from one another)
        assert not np.array_equal(seq[0].last_state["z"], seq[i].last_state["z"]), i
    if with_callback:
        n_chunks = -(-steps // every)
        assert len(seen_b) == len(seen_s) == 4 * n_chunks
        for ch in range(n_chunks):   # after every chunk, every model in order (the sequential runs give them model by model)
            for i in range(4):
                db, tb, zb, thb = seen_b[ch * 4 + i]
                ds, ts, zs, ths = seen_s[i * n_chunks + ch]
                assert db is sweep[i] and ds is seq[i] and tb == ts == (ch + 1) * every
                assert np.array_equal(zb, zs) and np.array_equal(thb, ths), (ch, i)


# ---- per-chain values with MANY weighted samples (tests/weight_states.py) ------------------------------------------------------------------
# alpha_linear and h_theta differ per chain; every chain's state is built with its own alpha so that chain 0 has one sample above the 2^-30
# cut everywhere, chain 1 2 .. NS - 1 and chain 2 more than NS: the gradient kernels read this step's alpha from the chain's row of the
# table while they deal and sum shares.  Bit for bit against standalone engines configured with the chain's values.
def test_per_chain_values_with_many_weighted_samples(c_oracle64):
    import weight_states as W
    bs = [W.build(case, c_oracle64) for case in W.CHAIN_CASES["sweep_lingauss"]]
    W.assert_chains_match_standalone(bs, hps=W.SWEEP_HPS)
