"""GPU tests along the hyper-parameter axis (tests/hparam_states.py: the case table and the restated dispatch): one step of every kernel
family with tau, the edge / parameter priors, the BGe prior, beta_linear and the kernel scales all OFF make_config's defaults, stage by
stage against the float64 C oracle (the soft-graph BGe kernels: against the torch-autograd oracle) with the bounds the project already
holds those stages to at those sizes -- test_marginal_bge_step_stages, test_joint_lingauss_step_stages / test_joint_densenn_step_stages
(obs_axis.BOUNDS), test_marginal_bge_reparam_estimator; the update through conftest.update_check / assert_update_parity.  No tolerance
is new.  tests/test_hparam_states_host.py shows on the CPU that each moved parameter changes a compared stage by 20 bounds or more and
that the float32 oracle stays within half of every bound.  The hard-graph scorers and the batched, chains and float64 engines run with the
same off-default values.

`pytest -s` prints every stage error (one `hparams` line per case; profiles/hparam_errors.txt keeps one run)."""
import numpy as np
import pytest

import hparam_states as H
import obs_axis as A
from conftest import assert_update_parity, rel_err, update_check
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _graphs_from_masks(masks, M, S, d):
    gm = masks.reshape(M, d, S, -1)  # [m][j][s][w]: bit i of word i // 64 = g[i, j]
    gg = np.zeros((M, S, d, d), np.uint8)
    for i in range(d):
        gg[:, :, i, :] = ((gm[:, :, :, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1)
    return gg


def _device_step(b, before, monkeypatch, fresh=True):
    """one step at the case's t from `before` on a fresh engine (tuning switches of the case latched at its creation): the debug stages
    of H.bounds, the sampled graphs of the marginal model and the state after"""
    for k, v in H.engine_env(b).items():
        monkeypatch.setenv(k, v)
    M, d, S = b["M"], b["d"], b["S"]
    eng = Engine(make_config(**b["cfg_kw"]))
    try:
        eng.set_data(b["x"], b["mask"], b["mean_obs"])
        eng.init_particles(random.PRNGKey(H.KEY))
        g0 = eng.get_state()
        assert not fresh or ((g0["key"] == before["key"]).all() and rel_err(g0["z"], before["z"]) < 1e-6), "init stream"
        kw = dict(z=before["z"], v_z=before["v_z"], key=before["key"], baseline=before.get("baseline", np.zeros(M)))
        if before.get("theta") is not None:
            kw.update(theta=before["theta"], v_theta=before["v_theta"])
        eng.set_state(**kw)
        eng.run(H.t_step(b), 1)
        dbg = {H.STAGE_KEYS[s]: eng.read(s) for s in H.bounds(b)}
        if "node_scores" in dbg:
            dbg["node_scores"] = dbg["node_scores"].reshape(M, d, S).transpose(0, 2, 1)   # device layout [m][j][s]
        graphs = _graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d) if b["model"] == "bge" and b["est"] == "score" else None
        return dbg, graphs, eng.get_state()
    finally:
        eng.close()


def _assert_update(b, seg, before, ref_phi, ref_after, dbg, after):
    u = update_check(make_config(**b["cfg_kw"]), before[seg], before["v_" + seg], dbg["phi_" + seg], ref_phi, after[seg], ref_after[seg])
    print(f"  hparams {b['id']} update {seg}: signal={u['signal']:.1e} all_p95={u['all_p95']:.1e} vs_own_phi={u['vs_own_phi']:.1e} share={u['signal_share']:.2f}")
    assert_update_parity(u, H.MIN_SHARE[seg], f"{b['id']} {seg}")


@pytest.mark.parametrize("case", H.ORACLE_CASES, ids=[H.case_id(c) for c in H.ORACLE_CASES])
def test_step_stages_off_the_defaults(c_oracle64, monkeypatch, case):
    b = H.built_case(case, c_oracle64)
    dbg, graphs, after = _device_step(b, b["before"], monkeypatch)
    errs = H.stage_errors(case, dbg, b["dbg"])
    print(f"\n  hparams {b['id']} [{case['kernel']}]: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    assert (after["key"] == b["after"]["key"]).all()                          # keys and sampled graphs: bit for bit
    if graphs is not None:
        assert np.array_equal(graphs, b["dbg"]["g_samples"]), "sampled graphs must be bit-identical"
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():                                                 # (in the order of the step: the first stage that is off is named)
        assert e < H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    assert rel_err(after["baseline"], b["after"]["baseline"]) < 1e-5 or np.abs(b["after"]["baseline"]).max() == 0
    if H.phi_overflows(b["dbg"]):
        assert case["d"] >= 128
        return
    for seg in ("z", "theta") if case["model"] != "bge" else ("z",):
        _assert_update(b, seg, b["before"], b["dbg"]["phi_" + seg], b["after"], dbg, after)


@pytest.mark.parametrize("case", H.SOFT_CASES, ids=[H.case_id(c) for c in H.SOFT_CASES])
def test_soft_graph_bge_off_the_defaults(monkeypatch, case):
    """k_bge_soft_mf, both forms of k_bge_soft and k_soft_combine at tau = 0.7 on the off-default BGe prior, with and without interventions.
    W_LIK is the check of their gradient (autograd's per-sample d log p / d scores, summed with the device's own softmax weights as in
    tests/test_gpu_soft_bge.py): GRAD_Z and PHI_Z are all acyclicity term from 49 variables on."""
    b = H.built_soft_case(case)
    ref = b["ref"]
    dbg, _, after = _device_step(b, ref["before"], monkeypatch)
    errs = H.stage_errors(case, dbg, H.reference_stages(case, ref, dbg))
    print(f"\n  hparams {b['id']} [{case['kernel']}]: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    assert (after["key"] == ref["after"]["key"]).all()
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():
        assert e < H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    if case["d"] <= 128:    # (beyond: phi^2 leaves float32 in RMSprop's second moment, test_marginal_bge_reparam_estimator)
        u = update_check(make_config(**b["cfg_kw"]), ref["before"]["z"], ref["before"]["v_z"], dbg["phi_z"], ref["phi_z"], after["z"], ref["after"]["z"])
        print(f"  hparams {b['id']} update z: {u}")
        assert_update_parity(u, 0.9, b["id"])


# ---- logistic_minval_tiny: a draw without a set bit among its 23, on an edge with alpha s = 16 -------------------------------------------
@pytest.mark.parametrize("case", H.TINY_CASES, ids=[H.case_id(c) for c in H.TINY_CASES])
def test_zero_bits_draw_under_both_settings_of_logistic_minval_tiny(c_oracle64, monkeypatch, case):
    """the soft graph of the hit edge is 0.51 with the default lower limit of the uniform and e^-71 with logistic_minval_tiny: a kernel
    whose own copy of the limit ignored the switch misses W_ACYC / LOGPROBS_Z by 20 to 11 000 bounds (tests/test_hparam_states_host.py)"""
    b = H.built_tiny_case(case, c_oracle64)
    dbg, graphs, after = _device_step(b, b["before"], monkeypatch, fresh=False)
    errs = H.stage_errors(case, dbg, H.reference_stages(case, b["dbg"], dbg))
    stage, v_ref = H.tiny_hit_value(case, b["dbg"])
    _, v_dev = H.tiny_hit_value(case, dbg)
    print(f"\n  hparams {b['id']} [{case['kernel']}]: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()) + f" | {stage} at the hit {v_dev:.6g} (reference {v_ref:.6g})")
    assert (after["key"] == b["after"]["key"]).all()
    if graphs is not None:
        assert np.array_equal(graphs, b["dbg"]["g_samples"])
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():
        assert e < H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    for seg in ("z", "theta") if case["model"] != "bge" else ("z",):
        _assert_update(b, seg, b["before"], b["dbg"]["phi_" + seg], b["after"], dbg, after)


# ---- the hard-graph scorers ---------------------------------------------------------------------------------------------------------------
def score_graphs_of(model, gs, theta, x, mask):
    from dibs_amd.inference.scoring import score_graphs
    return score_graphs(model, gs, theta, x, mask)


@pytest.mark.parametrize("interv", (False, True), ids=("obs", "interv"))
@pytest.mark.parametrize("d", H.SCORE_D)
def test_score_graphs_on_the_off_default_bge_prior(c_oracle64, d, interv):
    """the hard-graph scorer on the data and prior of the BGe rows; the graph list holds the empty graph and a complete DAG"""
    from dibs_amd.inference import scoring
    from dibs_amd.models import BGe
    scoring._close_all()
    case, kw, mean_obs, x, mask, gs = H.bge_score_inputs(d, interv)
    ref = c_oracle64.score_graphs(make_config(**kw), x, mask, gs, mean_obs=mean_obs)
    got = score_graphs_of(BGe(n_vars=d, mean_obs=mean_obs, alpha_mu=kw["bge_alpha_mu"], alpha_lambd=kw["bge_alpha_lambd"]), gs, None, x, mask)
    bound = H.bounds(case)["LOGPROBS_Z"]
    print(f"\n  hparams score_graphs bge d={d} interv={interv}: {rel_err(got, ref):.1e} (bound {bound:.0e})")
    assert np.isfinite(got).all() and rel_err(got, ref) < bound


@pytest.mark.parametrize("d,n_ho", H.LIN_SCORE_CASES, ids=[f"d{d}-n{n}" for d, n in H.LIN_SCORE_CASES])
def test_lin_score_given_off_the_default_edge_prior(c_oracle64, d, n_ho):
    """joint_lin_score_given takes mean_edge and sig_edge separately (bound: test_score_graphs_along_n_ho's)"""
    from dibs_amd.inference import scoring
    from dibs_amd.models import LinearGaussian
    scoring._close_all()
    kw, x, mask, gs, th = H.lin_score_inputs(d, n_ho)
    ref = c_oracle64.score_graphs(make_config(**kw), x, mask, gs, th.reshape(5, -1).astype(np.float64))
    got = score_graphs_of(LinearGaussian(n_vars=d, obs_noise=H.LIN["lin_obs_noise"], mean_edge=H.LIN["lin_mean_edge"], sig_edge=H.LIN["lin_sig_edge"]), gs, th, x, mask)
    print(f"\n  hparams score_graphs lingauss d={d} n_ho={n_ho}: {rel_err(got, ref):.1e}")
    assert np.isfinite(got).all() and rel_err(got, ref) < H.LIN_SCORE_BOUND


# ---- the other engines: bit for bit against standalone engines, as tests/test_gpu_batch.py and tests/test_gpu_chains.py ------------------
def _run(cfg_kw, sets, keys, t0, n, batch_kw=None):
    e = Engine(make_config(**cfg_kw, **(batch_kw or {})))
    try:
        if batch_kw and "n_problems" in batch_kw:
            for p, (x, mask, mo) in enumerate(sets):
                e.set_data_problem(p, x, mask, mo)
        else:
            e.set_data(*sets[0])
        if batch_kw:
            e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        else:
            e.init_particles(random.PRNGKey(keys[0]))
        e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


@pytest.mark.parametrize("d", (20, 50))
def test_batched_engine_off_the_defaults(d):
    """two problems of one batched engine (tau is a config-level argument of the _batch kernels) against two standalone engines"""
    case = next(c for c in H.ACYC_CASES if c["d"] == d and c["tau"] == 0.7 and c["layout"] == "legacy" and c["Sa"] == 4)
    kw, mean_obs = H.config_kwargs(case)
    M, N = case["M"], case["N"]
    sets = [(A.structured_x(d, N, seed=21 + p), A.random_mask(d, N, 0.15) if p == 1 else None, mean_obs * (1 + p)) for p in range(2)]
    bst = _run(kw, sets, [71, 72], H.T_MARGINAL, 3, dict(n_problems=2))
    for p in range(2):
        st, sl = _run(kw, [sets[p]], [71 + p], H.T_MARGINAL, 3), slice(p * M, (p + 1) * M)
        for k in ("z", "v_z", "baseline"):
            assert np.isfinite(st[k]).all() and np.array_equal(bst[k][sl], st[k]), (p, k)
        assert np.array_equal(bst["key"][p], st["key"]), p
    assert not np.array_equal(bst["z"][:M], bst["z"][M:])


def test_chains_engine_off_the_defaults():
    """two chains of one chains engine, LinearGaussian d = 8 with the Z pass on soft graphs, against two standalone engines"""
    case = next(c for c in H.LIN_CASES if c["d"] == 8 and c["est"] == "reparam" and c["kernel"].startswith("pair<"))
    kw, _ = H.config_kwargs(case)
    M = case["M"]
    x, mask = H.data(case)
    cst = _run(kw, [(x, mask)], [81, 82], H.T_JOINT, 3, dict(n_chains=2))
    for c in range(2):
        st, sl = _run(kw, [(x, mask)], [81 + c], H.T_JOINT, 3), slice(c * M, (c + 1) * M)
        for k in ("z", "v_z", "theta", "v_theta", "baseline"):
            assert np.isfinite(st[k]).all() and np.array_equal(cst[k][sl], st[k]), (c, k)
        assert np.array_equal(cst["key"][c], st["key"]), c
    assert not np.array_equal(cst["z"][:M], cst["z"][M:])


@pytest.mark.parametrize("d", (12, 40))
def test_f64_engine_off_the_defaults(c_oracle64, d):
    """the float64 engine with tau = 0.7, scale_latent = 0.5 and the off-default BGe prior: every stage within tests/test_gpu_f64.py's 1e-9"""
    from oracle import prng
    case = H._case("f64", "float64 engine", "bge", d, S=4, Sa=4, interv=d == 12)
    kw, mean_obs = H.config_kwargs(case)
    x, mask = H.data(case)
    cfg = make_config(precision=64, **kw)
    M, S = case["M"], case["S"]
    st = c_oracle64.new_state(cfg, prng.PRNGKey(H.KEY))
    eng = Engine(cfg)
    try:
        assert eng.precision == 64
        eng.set_data(np.asarray(x, np.float64), mask, mean_obs)
        eng.set_state(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
        ref = c_oracle64.step(cfg, x, mask, st, H.T_MARGINAL, debug=True, mean_obs=mean_obs)
        eng.run(H.T_MARGINAL, 1)
        g = eng.get_state()
        gm = eng.read("PARENT_MASKS").reshape(M, d, S)
        gg = np.stack([((gm >> np.uint64(i)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1) for i in range(d)], axis=2)
        assert np.array_equal(gg, ref["g_samples"]) and (g["key"] == st["key"]).all()
        dbg = {H.STAGE_KEYS[s]: eng.read(s) for s in H.bounds(case)}
        dbg["node_scores"] = dbg["node_scores"].reshape(M, d, S).transpose(0, 2, 1)
        errs = dict(H.stage_errors(case, dbg, ref), V_Z=rel_err(g["v_z"], st["v_z"]), Z=rel_err(g["z"], st["z"]))
        print(f"\n  hparams f64 d={d}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
        bad = {k: v for k, v in errs.items() if not v < 1e-9}
        assert not bad, bad
    finally:
        eng.close()
