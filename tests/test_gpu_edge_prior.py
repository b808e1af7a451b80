"""The edge-wise graph prior on the device (DIBS_PRIOR_EDGEWISE, dibs_engine_set_edge_prior; k_particle_grad_edge, k64_grad).
Two anchors: a table with the Erdos-Renyi probability in every entry reproduces the Erdos-Renyi engine bit for bit, and a non-uniform table
has a closed form that numpy evaluates in float64."""
import numpy as np
import pytest

from conftest import make_data, rel_err, stage_err
from dibs_amd._abi import make_config
from oracle import prng

pytestmark = pytest.mark.gpu
STATE = ("z", "v_z", "theta", "v_theta", "baseline", "key")


def _er_table(d, epn=2):
    from dibs_amd.models import ErdosReniDAGDistribution
    return np.full((d, d), ErdosReniDAGDistribution(d, epn).p)


def _table(d, seed=0):
    """seeded, in [0.01, 0.99], asymmetric"""
    p = np.random.default_rng(seed).uniform(0.01, 0.99, size=(d, d))
    assert np.abs(p - p.T).max() > 0.5
    return p


def _engine(cfg, x, table=None):
    from dibs_amd.engine import Engine
    eng = Engine(cfg)
    eng.set_data(np.asarray(x, np.float64 if eng.precision == 64 else np.float32))
    if table is not None:
        eng.set_edge_prior(table)
    return eng


def _run(cfg, x, table, key, t0=0, n=3):
    """one engine alone in the process (the polled join flag is used only then): init, run, state, close"""
    eng = _engine(cfg, x, table)
    try:
        eng.init_particles(key)
        eng.run(t0, n)
        return eng.get_state()
    finally:
        eng.close()


def _same_state(a, b, what=""):
    for name in STATE:
        if a[name] is None:
            assert b[name] is None
            continue
        assert np.array_equal(a[name], b[name]), (what, name, rel_err(a[name], b[name]))


# ---- 1. a uniform table is the Erdos-Renyi engine, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,M,kw", [
    ("bge_score", 8, 4, dict(n_grad_mc_samples=32, n_acyclicity_mc_samples=8)),
    ("bge_reparam", 8, 4, dict(grad_estimator_z="reparam", n_grad_mc_samples=16, n_acyclicity_mc_samples=8)),
    ("lingauss", 8, 4, dict(joint=True, likelihood="lingauss", n_grad_mc_samples=32, n_acyclicity_mc_samples=8)),
    ("densenn", 8, 4, dict(joint=True, likelihood="densenn", nn_hidden=(5,), n_grad_mc_samples=16, n_acyclicity_mc_samples=8)),
    ("second_pass_d56", 56, 4, dict(n_grad_mc_samples=4, n_acyclicity_mc_samples=4)),       # d^2 = 3136 > 3072: two passes of the element loop
    # w_tot + k_backproject_big.  beta_linear = 0 on both sides: from a random state of 120 variables the acyclicity gradient is ~1e18
    # (measured, Erdos-Renyi engine alike), under which no prior term reaches the float32 sum and any table would pass
    ("w_tot_d120", 120, 2, dict(n_grad_mc_samples=2, n_acyclicity_mc_samples=2, beta_linear=0.0)),
    ("headline_schedule", 20, 128, dict()),                                                  # polled join flag, kernel-matrix tiles in the tail launch
])
def test_uniform_table_equals_the_erdos_renyi_engine(name, d, M, kw):
    data, _, _ = make_data(d, joint=bool(kw.get("joint")))
    base = dict(n_vars=d, n_particles=M, n_observations=data.x.shape[0], edges_per_node=2, **kw)
    key = prng.PRNGKey(7)
    er = _run(make_config(graph_prior="er", **base), data.x, None, key)
    ew = _run(make_config(graph_prior="edgewise", **base), data.x, _er_table(d), key)
    _same_state(ew, er, name)
    # (not vacuous: another table moves the particles)
    other = _run(make_config(graph_prior="edgewise", **base), data.x, _table(d), key)
    assert not np.array_equal(other["z"], er["z"])


# ---- 2. a non-uniform, asymmetric table against the closed form -----------------------------------------------------------------------------
def _closed_form(z, table, alpha, inv_sig2):
    """(prior part [Wp V, Wp^T U], whole expected gradient) in float64; z [M, d, k, 2]: U = z[..., 0], V = z[..., 1]"""
    z = np.asarray(z, np.float64)
    u, v = z[..., 0], z[..., 1]
    p = 1.0 / (1.0 + np.exp(-alpha * (u @ np.swapaxes(v, -1, -2))))
    lo = np.log(table) - np.log(1.0 - table)
    wp = alpha * p * (1.0 - p) * lo
    idx = np.arange(z.shape[1])
    wp[:, idx, idx] = 0.0
    prior = np.stack([wp @ v, np.swapaxes(wp, -1, -2) @ u], axis=-1)
    return prior, prior - z * inv_sig2


def _closed_form_case(d, M=3):
    """state, table, t: z scaled so that alpha * U V^T is of order 1 (edge probabilities away from saturation), alpha = 5"""
    rng = np.random.default_rng(100 + d)
    t, alpha = 5, 5.0   # (MarginalDiBS: alpha_linear = 1)
    s = np.sqrt(0.2 / np.sqrt(d))
    z = (rng.normal(size=(M, d, d, 2)) * s).astype(np.float32)
    return z, _table(d, seed=d), t, alpha


@pytest.mark.parametrize("d", [8, 56, 120])
def test_nonuniform_table_against_the_closed_form(d):
    M = 3
    z, table, t, alpha = _closed_form_case(d, M)
    sig = 1.0
    prior, want = _closed_form(z, table, alpha, 1.0 / sig ** 2)
    # numpy side alone: the prior part carries the expected gradient (a table ignored or transposed cannot pass)
    assert np.abs(prior).max() >= 0.1 * np.abs(want).max()
    prior_t, _ = _closed_form(z, table.T, alpha, 1.0 / sig ** 2)
    assert np.abs(prior - prior_t).max() > 0.1 * np.abs(want).max()
    u, v = z[..., 0].astype(np.float64), z[..., 1].astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-alpha * (u @ np.swapaxes(v, -1, -2))))
    assert 0.02 < np.percentile(p, 5) and np.percentile(p, 95) < 0.98   # away from saturation
    data, _, _ = make_data(d)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=data.x.shape[0], graph_prior="edgewise", alpha_linear=1.0, beta_linear=0.0,
                      latent_prior_std=sig, n_grad_mc_samples=4, n_acyclicity_mc_samples=2)
    eng = _engine(cfg, data.x, table)
    try:
        eng.set_state(z=z)
        keys = np.stack([prng.PRNGKey(50 + m) for m in range(M)])
        got = eng.eval_gradients(t, keys_prior=keys)["grad_z_prior"]
    finally:
        eng.close()
    stage_err(f"GRAD_Z prior d={d}", got, want, 1e-4)


# ---- 3. the float64 engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 40])
def test_f64_uniform_table_equals_the_erdos_renyi_engine(d):
    data, _, _ = make_data(d)
    base = dict(n_vars=d, n_particles=4, n_observations=data.x.shape[0], edges_per_node=2, n_grad_mc_samples=16, n_acyclicity_mc_samples=4,
                precision=64)
    key = prng.PRNGKey(9)
    er = _run(make_config(graph_prior="er", **base), data.x, None, key)
    ew = _run(make_config(graph_prior="edgewise", **base), data.x, _er_table(d), key)
    assert er["z"].dtype == np.float64
    _same_state(ew, er, f"f64 d={d}")


@pytest.mark.parametrize("d", [8, 40])
def test_f64_nonuniform_table_adds_the_closed_form_to_the_gradient(d):
    """GRAD_Z of one step against a float64 engine that differs only in having the uniform prior (no prior term), same key: the first step
    samples the same graphs, so the difference is the prior part alone."""
    M, t = 4, 2
    data, _, _ = make_data(d)
    table = _table(d, seed=3 * d)
    base = dict(n_vars=d, n_particles=M, n_observations=data.x.shape[0], n_grad_mc_samples=16, n_acyclicity_mc_samples=4, precision=64)
    out = {}
    for prior, tab in (("uniform", None), ("edgewise", table)):
        cfg = make_config(graph_prior=prior, **base)
        eng = _engine(cfg, data.x, tab)
        try:
            eng.init_particles(prng.PRNGKey(11))
            z0 = eng.get_state()["z"]
            eng.run(t, 1)
            out[prior] = (z0, eng.read("GRAD_Z").reshape(M, d, d, 2), eng.read("PARENT_MASKS").copy())
        finally:
            eng.close()
    assert np.array_equal(out["uniform"][0], out["edgewise"][0]) and np.array_equal(out["uniform"][2], out["edgewise"][2])
    alpha = cfg.alpha_linear * t   # (the step's alpha as step_f64 forms it: a double product)
    want, _ = _closed_form(out["edgewise"][0], table, alpha, 0.0)
    diff = out["edgewise"][1] - out["uniform"][1]
    e = rel_err(diff, want)
    print(f"f64 d={d}: GRAD_Z(edge-wise) - GRAD_Z(uniform) against [Wp V, Wp^T U]: {e:.1e}")
    # (the two gradients are ~1e5 times the prior part at d = 40: the rounding of their difference stays a tenth of the bound)
    assert np.finfo(np.float64).eps * np.abs(out["uniform"][1]).max() < 1e-10 * np.abs(want).max()
    assert e < 1e-9


# ---- 4. chains -----------------------------------------------------------------------------------------------------------------------------
def test_chains_engine_shares_the_table():
    from dibs_amd.engine import Engine
    C, d, M = 3, 8, 4
    data, _, _ = make_data(d, joint=True)
    table = _table(d, seed=21)
    base = dict(n_vars=d, n_particles=M, n_observations=data.x.shape[0], joint=True, likelihood="lingauss", graph_prior="edgewise",
                n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    keys = np.stack([prng.PRNGKey(30 + c) for c in range(C)])
    alone = [_run(make_config(**base), data.x, table, keys[c]) for c in range(C)]
    eng = Engine(make_config(n_chains=C, **base))
    try:
        eng.set_data(data.x)
        eng.set_edge_prior(table)
        eng.init_particles_batch(keys)
        eng.run(0, 3)
        st = eng.get_state()
    finally:
        eng.close()
    for c in range(C):
        for name in STATE:
            got = st[name][c] if name == "key" else st[name].reshape((C, M) + st[name].shape[1:])[c]
            assert np.array_equal(got, alone[c][name]), (c, name)


def test_sample_chains_equals_three_sample_calls():
    from dibs_amd.inference import JointDiBS, sample_chains
    from dibs_amd.models import EdgePriorDAGDistribution
    d = 8
    data, _, lm = make_data(d, joint=True)
    gm = EdgePriorDAGDistribution(d, _table(d, seed=22))
    model = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    keys = [prng.PRNGKey(40 + c) for c in range(3)]
    out = sample_chains(model, keys=keys, n_particles=4, steps=4)
    for c, key in enumerate(keys):
        g, th = model.sample(key=key, n_particles=4, steps=4)
        assert np.array_equal(out[c][0], g) and np.array_equal(out[c][1], th)
        _same_state(model.last_chain_states[c], model.last_state, f"chain {c}")


# ---- 5. rules ------------------------------------------------------------------------------------------------------------------------------
def _small(prior="edgewise", **kw):
    d = 8
    data, _, _ = make_data(d, joint=bool(kw.get("joint")))
    return d, data, make_config(n_vars=d, n_particles=4, n_observations=data.x.shape[0], graph_prior=prior, n_grad_mc_samples=16,
                                n_acyclicity_mc_samples=4, **kw)


def test_running_before_the_table_is_set_fails():
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    d, data, cfg = _small()
    eng = Engine(cfg)
    try:
        eng.set_data(data.x)
        eng.init_particles(prng.PRNGKey(0))
        z0 = eng.get_state()["z"]
        with pytest.raises(DibsHipError, match="dibs_engine_set_edge_prior has not been called"):
            eng.run(0, 1)
        with pytest.raises(DibsHipError, match="dibs_engine_set_edge_prior has not been called"):
            eng.eval_gradients(1, keys_prior=np.stack([prng.PRNGKey(m) for m in range(4)]))
        assert np.array_equal(eng.get_state()["z"], z0)   # (nothing ran)
        eng.set_edge_prior(_table(d))
        eng.run(0, 1)
        # the table may be given again between runs
        eng.set_edge_prior(_er_table(d))
        eng.run(1, 1)
    finally:
        eng.close()


def test_setting_the_table_on_an_erdos_renyi_engine_fails():
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    d, data, cfg = _small("er")
    eng = Engine(cfg)
    try:
        with pytest.raises(DibsHipError, match="dibs_engine_set_edge_prior: this engine's graph prior is not edge-wise"):
            eng.set_edge_prior(_table(d))
    finally:
        eng.close()


@pytest.mark.parametrize("bad", [0.0, 1.0])
def test_an_entry_of_zero_or_one_is_refused_and_named(bad):
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    d, data, cfg = _small()
    eng = Engine(cfg)
    try:
        p = _table(d)
        p[2, 5] = bad
        with pytest.raises(DibsHipError, match=r"dibs_engine_set_edge_prior: entry \(2, 5\) = " + str(int(bad)) + r".*strictly inside \(0, 1\)"):
            eng.set_edge_prior(p)
        np.fill_diagonal(p, bad)   # (the diagonal is ignored)
        p[2, 5] = 0.5
        eng.set_edge_prior(p)
    finally:
        eng.close()


def test_the_batched_engine_refuses_the_prior():
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    _, _, cfg = _small(n_problems=2)
    with pytest.raises(DibsHipError, match=r"batched engine \(n_problems > 1\): the edge-wise graph prior is not supported.*per-problem tables are not built"):
        Engine(cfg)


def test_the_per_chain_tier_refuses_the_prior():
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    d, data, cfg = _small(joint=True, likelihood="lingauss", n_chains=2)
    eng = Engine(cfg)
    try:
        for c in range(2):
            eng.set_data_problem(c, data.x)
        eng.set_edge_prior(_table(d))
        eng.set_chain_hparams(1, alpha_linear=0.1)
        with pytest.raises(DibsHipError, match=r"chains engine \(n_chains > 1\): the edge-wise graph prior is not supported together with per-chain "
                                                 r"hyper-parameters.*per-problem tables are not built"):
            eng.init_particles_batch(np.stack([prng.PRNGKey(1), prng.PRNGKey(2)]))
    finally:
        eng.close()


# ---- 6. direction --------------------------------------------------------------------------------------------------------------------------
def test_the_prior_moves_the_edges_it_names():
    """the same key and data twice: P = 0.999 on a fixed edge set E and 0.001 elsewhere (A), the two values swapped (B)"""
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.models import EdgePriorDAGDistribution
    d, steps = 8, 100
    data, _, lm = make_data(d)
    on_e = np.zeros((d, d), bool)
    for i, j in ((0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (0, 7)):
        on_e[i, j] = True
    off_e = ~on_e & ~np.eye(d, dtype=bool)
    mean_p = {}
    for name, hi_on_e in (("A", True), ("B", False)):
        table = np.where(on_e == hi_on_e, 0.999, 0.001)
        dibs = MarginalDiBS(x=data.x, graph_model=EdgePriorDAGDistribution(d, table), likelihood_model=lm)
        dibs.sample(key=prng.PRNGKey(5), n_particles=8, steps=steps)
        p = np.mean([dibs.edge_probs(z, steps) for z in dibs.last_state["z"]], axis=0)
        mean_p[name] = (float(p[on_e].mean()), float(p[off_e].mean()))
    print("mean final edge probability (on E, off E):", mean_p)
    assert mean_p["A"][0] > mean_p["B"][0]
    assert mean_p["A"][1] < mean_p["B"][1]
