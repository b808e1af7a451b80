"""GPU tests along the Monte-Carlo sample axes S and Sa (tests/sample_axis.py: the restated choices, `classify` and the case table): one
step per row through the C ABI, stage by stage against the float64 C oracle, at the sample counts where a loop over the samples makes its
second, third or ninth trip, where tail_nsplit changes, where the softmax of particle_grad_block leaves the wave for the block, where the
parent sets no longer fit LDS, where the last block of a log-probability launch is ragged, and where k_acyc_reduce runs a full group AND
its tail.  The bounds are the project's own at those sizes (hparam_states.bounds: test_marginal_bge_step_stages,
test_joint_lingauss_step_stages / test_joint_densenn_step_stages, tests/test_gpu_soft_bge.py; the update through
conftest.assert_update_parity; the float64 engine at 1e-9).  No tolerance is new.  tests/test_sample_axis_host.py shows on the CPU that the
float32 oracle stays within half of every bound on every row and that the rows are not vacuous.

`pytest -s` prints every stage error (one `sample_axis` line per row; profiles/sample_axis_errors.txt keeps one run)."""
import numpy as np
import pytest

import hparam_states as H
import obs_axis as A
import sample_axis as X
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


def _er_table(d, epn):
    from dibs_amd.models import ErdosReniDAGDistribution
    return np.full((d, d), ErdosReniDAGDistribution(d, epn).p)


def _engine(b, monkeypatch):
    """a fresh engine of the row with its data (tuning switches latched at creation); `edge`: the edge-wise prior with the Erdos-Renyi
    probability in every entry -- k_particle_grad_edge on the numbers the oracle computes for the Erdos-Renyi prior"""
    for k, v in H.engine_env(b).items():
        monkeypatch.setenv(k, v)
    kw = dict(b["cfg_kw"], graph_prior="edgewise") if b["engine"] == "edge" else b["cfg_kw"]
    eng = Engine(make_config(**kw))
    eng.set_data(b["x"], b["mask"], b["mean_obs"])
    if b["engine"] == "edge":
        eng.set_edge_prior(_er_table(b["d"], kw["edges_per_node"]))
    return eng


def _device_step(b, before, monkeypatch):
    """one step at T_STEP from `before`: the debug stages of H.bounds, the sampled graphs of the marginal score rows, the state after"""
    M, d, S = b["M"], b["d"], b["S"]
    eng = _engine(b, monkeypatch)
    try:
        eng.init_particles(random.PRNGKey(b["key"]))
        g0 = eng.get_state()
        assert (g0["key"] == before["key"]).all() and rel_err(g0["z"], before["z"]) < 1e-6, "init stream"
        kw = dict(z=before["z"], v_z=before["v_z"], key=before["key"], baseline=before.get("baseline", np.zeros(M)))
        if before.get("theta") is not None:
            kw.update(theta=before["theta"], v_theta=before["v_theta"])
        eng.set_state(**kw)
        eng.run(X.T_STEP, 1)
        dbg = {H.STAGE_KEYS[s]: eng.read(s) for s in H.bounds(b)}
        if "node_scores" in dbg:
            dbg["node_scores"] = dbg["node_scores"].reshape(M, d, S).transpose(0, 2, 1)   # device layout [m][j][s]
        graphs = _graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d) if b["model"] == "bge" and b["est"] == "score" else None
        return dbg, graphs, eng.get_state()
    finally:
        eng.close()


def _line(b, cl, errs):
    worst = max((e / (X.BASELINE_BOUND if s == "baseline" else X.bound(b, s)), s) for s, e in errs.items())
    print(f"\n  sample_axis {b['id']} [{b['kernel']}] {sorted(cl)}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items())
          + f" | worst {worst[1]} at {worst[0]:.2f} of its bound")


def _assert_update(b, seg, before, ref_phi, ref_after, dbg, after, min_share=None):
    u = update_check(make_config(**b["cfg_kw"]), before[seg], before["v_" + seg], dbg["phi_" + seg], ref_phi, after[seg], ref_after[seg])
    print(f"  sample_axis {b['id']} update {seg}: signal={u['signal']:.1e} all_p95={u['all_p95']:.1e} vs_own_phi={u['vs_own_phi']:.1e} share={u['signal_share']:.2f}")
    assert_update_parity(u, H.MIN_SHARE[seg] if min_share is None else min_share, f"{b['id']} {seg}")


@pytest.mark.parametrize("case", X.ORACLE_CASES, ids=[X.case_id(c) for c in X.ORACLE_CASES])
def test_step_stages_along_the_sample_axes(c_oracle64, monkeypatch, case):
    b = X.built_case(case, c_oracle64)
    dbg, graphs, after = _device_step(b, b["before"], monkeypatch)
    errs = X.stage_errors(case, dbg, after, b)
    _line(b, X.classify(case, int(X.nnz_of(b["dbg"]).max())), errs)
    assert (after["key"] == b["after"]["key"]).all()                          # keys and sampled parent sets: bit for bit
    if graphs is not None:
        assert np.array_equal(graphs, b["dbg"]["g_samples"]), "sampled graphs must be bit-identical"
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():                                                 # (in the order of the step: the first stage that is off is named)
        if s != "baseline":
            assert e < X.bound(case, s), (b["id"], s, e, X.bound(case, s))
    assert errs["baseline"] < X.BASELINE_BOUND, (b["id"], errs["baseline"])   # sm / S: every sample with the same weight
    if H.phi_overflows(b["dbg"]):
        assert case["d"] >= 128
        return
    for seg in ("z", "theta") if case["model"] != "bge" else ("z",):
        _assert_update(b, seg, b["before"], b["dbg"]["phi_" + seg], b["after"], dbg, after)


@pytest.mark.parametrize("case", X.SOFT_CASES, ids=[X.case_id(c) for c in X.SOFT_CASES])
def test_soft_graph_bge_along_s(monkeypatch, case):
    """k_soft_combine strides S by 256 three times: 130 samples in one trip, 258 in two.  Reference and bounds as
    test_soft_graph_bge_off_the_defaults: autograd's per-sample d log p / d scores, summed with the device's own softmax weights."""
    b = dict(H.built_soft_case(case), key=case["key"], engine=case["engine"])
    ref = b["ref"]
    dbg, _, after = _device_step(b, ref["before"], monkeypatch)
    errs = H.stage_errors(case, dbg, H.reference_stages(case, ref, dbg))
    _line(dict(b, id=X.case_id(case)), X.classify(case), errs)
    assert (after["key"] == ref["after"]["key"]).all()
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():
        assert e < H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    u = update_check(make_config(**b["cfg_kw"]), ref["before"]["z"], ref["before"]["v_z"], dbg["phi_z"], ref["phi_z"], after["z"], ref["after"]["z"])
    print(f"  sample_axis {X.case_id(case)} update z: {u}")
    assert_update_parity(u, 0.9, b["id"])


# ---- the other engines: bit for bit against standalone engines, as tests/test_gpu_batch.py and tests/test_gpu_chains.py ------------------
def _run(cfg_kw, sets, keys, chunks, batch_kw=None):
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
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


BATCH_CASES = [c for c in X.BITWISE_CASES if c["engine"] == "batch"]


@pytest.mark.parametrize("case", BATCH_CASES, ids=[X.case_id(c) for c in BATCH_CASES])
def test_batched_engine_along_the_sample_axes(case):
    """k_particle_grad_batch / k_acyc_batch: two problems of one batched engine end two steps bit-identical to two standalone engines.
    Problem 0 is the row's own data and key (tests/test_sample_axis_host.py: its weights reach past the first pass)."""
    kw, mean_obs = X.config_kwargs(case)
    M, d, N = case["M"], case["d"], case["N"]
    x, mask = H.data(case)
    sets = [(x, mask, mean_obs), (A.structured_x(d, N, seed=21), None, mean_obs * 2)]
    keys, chunks = [case["key"], case["key"] + 70], [(X.T_STEP, 2)]
    bst = _run(kw, sets, keys, chunks, dict(n_problems=2))
    for p in range(2):
        st, sl = _run(kw, [sets[p]], [keys[p]], chunks), slice(p * M, (p + 1) * M)
        for k in ("z", "v_z", "baseline"):
            assert np.isfinite(st[k]).all() and np.array_equal(bst[k][sl], st[k]), (p, k)
        assert np.array_equal(bst["key"][p], st["key"]), p
    assert not np.array_equal(bst["z"][:M], bst["z"][M:])


def test_chains_engine_at_258_samples():
    """three chains of one chains engine (LinearGaussian, 8 variables, S = 258) end two steps bit-identical to three standalone engines"""
    case = next(c for c in X.BITWISE_CASES if c["engine"] == "chains")
    kw, _ = X.config_kwargs(case)
    M = case["M"]
    x, mask = H.data(case)
    keys, chunks = [case["key"], 82, 83], [(X.T_STEP, 2)]
    cst = _run(kw, [(x, mask)], keys, chunks, dict(n_chains=3))
    for c in range(3):
        st, sl = _run(kw, [(x, mask)], [keys[c]], chunks), slice(c * M, (c + 1) * M)
        for k in ("z", "v_z", "theta", "v_theta", "baseline"):
            assert np.isfinite(st[k]).all() and np.array_equal(cst[k][sl], st[k]), (c, k)
        assert np.array_equal(cst["key"][c], st["key"]), c
    assert not np.array_equal(cst["z"][:M], cst["z"][M:2 * M])


@pytest.mark.parametrize("case", X.F64_CASES, ids=[X.case_id(c) for c in X.F64_CASES])
def test_f64_engine_along_the_sample_axes(c_oracle64, case):
    """the float64 engine at S = 258, Sa = 34: every stage within tests/test_gpu_f64.py's 1e-9"""
    b = X.built_case(case, c_oracle64)
    M, d, S = case["M"], case["d"], case["S"]
    st = b["before"]
    eng = Engine(make_config(precision=64, **b["cfg_kw"]))
    try:
        assert eng.precision == 64
        eng.set_data(np.asarray(b["x"], np.float64), b["mask"], b["mean_obs"])
        eng.set_state(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
        eng.run(X.T_STEP, 1)
        g = eng.get_state()
        assert np.array_equal(_graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d), b["dbg"]["g_samples"]) and (g["key"] == b["after"]["key"]).all()
        dbg = {H.STAGE_KEYS[s]: eng.read(s) for s in H.bounds(case)}
        dbg["node_scores"] = dbg["node_scores"].reshape(M, d, S).transpose(0, 2, 1)
        errs = dict(X.stage_errors(case, dbg, g, b), V_Z=rel_err(g["v_z"], b["after"]["v_z"]), Z=rel_err(g["z"], b["after"]["z"]))
        print(f"\n  sample_axis {b['id']} [{case['kernel']}] {sorted(X.classify(case, int(X.nnz_of(b['dbg']).max())))}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
        bad = {k: v for k, v in errs.items() if not v < 1e-9}
        assert not bad, bad
    finally:
        eng.close()


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------------------
CHUNK_CASES = [next(c for c in X.BGE_CASES if c["S"] == 258 and c["d"] == 8 and c["layout"] == "legacy"),
               next(c for c in X.ACYC_CASES if c["kernel"] == "k_acyc_hf" and c["Sa"] == 34 and c["tau"] == 1.0)]


@pytest.mark.parametrize("case", CHUNK_CASES, ids=[X.case_id(c) for c in CHUNK_CASES])
def test_chunking_does_not_change_the_bits(case):
    """run(0, 4) equals run(0, 2); run(2, 2) bit for bit on the block-wide softmax and on a reduction with a full group and a tail"""
    kw, mean_obs = X.config_kwargs(case)
    x, mask = H.data(case)
    one = _run(kw, [(x, mask, mean_obs)], [case["key"]], [(0, 4)])
    two = _run(kw, [(x, mask, mean_obs)], [case["key"]], [(0, 2), (2, 2)])
    for k in ("z", "v_z", "baseline", "key"):
        assert np.isfinite(np.asarray(one[k], np.float64)).all() and np.array_equal(one[k], two[k]), k
