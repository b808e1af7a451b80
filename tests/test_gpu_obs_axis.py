"""GPU tests along the observation axis N (tests/obs_axis.py: the case table and the restated path choice): one step of the joint models,
stage by stage against the float64 C oracle with the bounds of test_joint_lingauss_step_stages / test_joint_densenn_step_stages, at the
N where the launchers change kernel or tile count -- one row tile, a full and a ragged last tile, the eighth tile, 128 | 129 (paired |
unpaired kernels, tuned | general DenseNN kernels), and the last N on the LDS-resident LinearGaussian path | the first on the Gram path.
The path probe holds the restated cut against the engine; hard-graph scoring and the per-chain launchers are run at the same sizes.

`pytest -s` prints every stage error (one `obs_axis` line per case; profiles/obs_axis_errors.txt keeps one run)."""
import os

import numpy as np
import pytest

import obs_axis as A
from conftest import rel_err
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _device_step(b):
    """one step at T_STEP from the case's start state on a fresh engine (path switches of the environment are latched here): the debug
    stages of STAGE_KEYS, W_ACYC, KXX and the state after"""
    eng = Engine(make_config(**b["cfg_kw"]))
    try:
        eng.set_data(b["x"], b["mask"])
        eng.init_particles(random.PRNGKey(A.KEY))
        g0 = eng.get_state()
        st = b["before"]
        assert (g0["key"] == st["key"]).all() and rel_err(g0["z"], st["z"]) < 1e-6 and rel_err(g0["theta"], st["theta"]) < 1e-6, "init stream"
        eng.set_state(z=st["z"], v_z=st["v_z"], theta=st["theta"], v_theta=st["v_theta"], key=st["key"], baseline=st["baseline"])
        eng.run(A.T_STEP, 1)
        dbg = {k: eng.read(s) for s, k in A.STAGE_KEYS.items()}
        dbg.update(w_acyc=eng.read("W_ACYC"), kxx=eng.read("KXX"))
        return dbg, eng.get_state()
    finally:
        eng.close()


def _assert_stages(case, b, dbg, after, ran=None):
    """(ran: what to print as the case's class where the environment moves the engine off the path classify() restates)"""
    errs, keys_equal = A.stage_errors(b, dbg, after)
    print(f"\n  obs_axis {b['id']} {ran or A.classify(case)}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    assert keys_equal                                                        # keys: bit for bit
    assert all(np.isfinite(v).all() for v in dbg.values())
    for s, e in errs.items():                                                # (in the order of the step: the first stage that is off is named)
        assert e < A.bound(case, s), (b["id"], s, e, A.bound(case, s))
    assert rel_err(dbg["w_acyc"], b["dbg"]["w_acyc"]) < 1e-5 and rel_err(dbg["kxx"], b["dbg"]["kxx"]) < 1e-5
    assert rel_err(after["baseline"], b["after"]["baseline"]) < 1e-5 or np.abs(b["after"]["baseline"]).max() == 0
    return errs


@pytest.mark.parametrize("case", A.LIN_CASES, ids=[A.case_id(c) for c in A.LIN_CASES])
def test_lingauss_stages_along_n(c_oracle64, case):
    b = A.built_case(case, c_oracle64)
    _assert_stages(case, b, *_device_step(b))


@pytest.mark.parametrize("case,kernel", list(zip(A.LIN_F32_CASES, A.LIN_F32_KERNELS)), ids=[A.case_id(c) for c in A.LIN_F32_CASES])
def test_lingauss_f32_paired_kernels(c_oracle64, monkeypatch, case, kernel):
    """DIBS_LIN_F32=1: k_lin_logprobs_pair<3,10>, <4,10> and <4,16> (the f32-MFMA kernels that the split-f16 kernels replace at
    33 <= d <= 64 by default) against the oracle, with the bounds of every other case.  Elsewhere they run in chains-versus-standalone
    bit comparisons only, whose two sides take one selection (lin_launch.h)."""
    monkeypatch.setenv("DIBS_LIN_F32", "1")
    assert A.lin_kernel(case["d"], case["N"], case["S"], case["layout"], lin_f32=True) == kernel
    b = A.built_case(case, c_oracle64)
    _assert_stages(case, b, *_device_step(b), ran=("lingauss", f"DIBS_LIN_F32=1 {kernel}") + A.row_tiles(case["N"]))


@pytest.mark.parametrize("case", A.NN_CASES, ids=[A.case_id(c) for c in A.NN_CASES])
def test_densenn_stages_along_n(c_oracle64, case):
    b = A.built_case(case, c_oracle64)
    _assert_stages(case, b, *_device_step(b))


@pytest.mark.parametrize("case", A.EDGE_CASES, ids=[A.case_id(c) for c in A.EDGE_CASES])
def test_intervention_edges(c_oracle64, case):
    """a node intervened in every observation (empty likelihood sum, Gram count 0), an observation intervened on every node, a mask of
    ones but one entry per column (tests/test_obs_axis_host.py: two oracles agree on the expected values to 1e-9)"""
    b = A.built_case(case, c_oracle64)
    _assert_stages(case, b, *_device_step(b))


# ---- path probe: the restated cut against the engine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", A.PROBE_D)
def test_path_probe_cut_is_the_last_size_on_the_lds_path(c_oracle64, monkeypatch, d):
    """At N = cut + 1 the default engine and one created under DIBS_LIN_GRAM=1 run the same kernels: GRAD_THETA and LOGPROBS_THETA end a
    step bit-identical.  At N = cut they do not -- both within the oracle bounds, different bits: the default engine ran the LDS-resident
    kernels at their largest footprint."""
    assert "DIBS_LIN_GRAM" not in os.environ
    cut = A.lin_cut(d)
    for N, same in ((cut + 1, True), (cut, False)):
        case = A._case("lingauss", d, N, est="reparam", interv=0.1)
        b = A.built_case(case, c_oracle64)
        monkeypatch.delenv("DIBS_LIN_GRAM", raising=False)
        dflt, after = _device_step(b)
        _assert_stages(case, b, dflt, after)
        monkeypatch.setenv("DIBS_LIN_GRAM", "1")
        gram, after_g = _device_step(b)
        _assert_stages(case, b, gram, after_g)
        eq = [np.array_equal(dflt[k].view(np.uint32), gram[k].view(np.uint32)) for k in ("grad_theta", "logprobs_th")]
        # (at the cut the M d d gradient values must differ; the M S = 16 log-probabilities are float32 roundings of sums both paths carry in
        #  double and may coincide -- they do at d = 40)
        print(f"\n  obs_axis probe d={d} N={N}: GRAD_THETA bits equal {eq[0]}, LOGPROBS_THETA bits equal {eq[1]}")
        assert all(eq) if same else not eq[0], (d, N, eq)


# ---- hard-graph scoring: dibs_score_graphs chooses its path from n_ho ---------------------------------------------------------------------
def _score_inputs(d):
    rng = np.random.default_rng(d)
    gs = (rng.random((5, d, d)) < 0.1).astype(np.int32)
    gs[:, np.arange(d), np.arange(d)] = 0
    return gs, rng.normal(size=(5, d, d)).astype(np.float32)


def _score_both(c_oracle64, d, n_ho, interv):
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.models import LinearGaussian
    gs, th = _score_inputs(d)
    x, mask = A.structured_x(d, n_ho), (A.random_mask(d, n_ho) if interv else None)
    cfg = make_config(n_vars=d, n_particles=1, n_observations=n_ho, joint=True, likelihood="lingauss", has_interventions=interv)
    ref = c_oracle64.score_graphs(cfg, x, mask, gs, th.reshape(5, -1).astype(np.float64))
    return score_graphs(LinearGaussian(n_vars=d), gs, th, x, mask), ref


@pytest.mark.parametrize("d,i", [(d, i) for d in A.SCORE_D for i in range(6)], ids=lambda v: str(v))
def test_score_graphs_along_n_ho(c_oracle64, d, i):
    """an engine-less model: the scoring engine is created for this call, its path follows from n_ho alone"""
    from dibs_amd.inference import scoring
    scoring._close_all()
    n_ho = A.score_n_ho(d)[i]
    got, ref = _score_both(c_oracle64, d, n_ho, interv=i % 2 == 1)
    print(f"\n  obs_axis score d={d} n_ho={n_ho} {'k_lin_logprobs (LDS)' if A.joint_lin_fast_path(d, n_ho) else 'gram'}: {rel_err(got, ref):.1e}")
    assert np.isfinite(got).all() and rel_err(got, ref) < 2e-5


@pytest.mark.parametrize("d", (20, 40))
def test_score_graphs_on_the_lds_path_after_a_gram_sized_set(c_oracle64, d):
    """ONE scoring engine (kept per model by scoring.py) given held-out sets on either side of the cut in turn: a set that takes the
    LDS-resident kernel must not be scored against the Gram matrices of the set before it."""
    from dibs_amd.inference import scoring
    scoring._close_all()
    cut = A.lin_cut(d)
    for n_ho in (cut + 1, cut, 16, cut + 1, 129):
        got, ref = _score_both(c_oracle64, d, n_ho, interv=False)
        assert rel_err(got, ref) < 2e-5, (d, n_ho, rel_err(got, ref))
    assert len(scoring._ENGINES) == 1


# ---- per-chain data: the launch text of lin_launch.h as compiled in tu_lin_chains.hip, at the same sizes  --------------------------------
STATE = ("z", "v_z", "theta", "v_theta", "baseline")
CHUNKS = [(0, 3)]


def _lin(d):
    return dict(n_vars=d, n_particles=A.M, joint=True, likelihood="lingauss", n_grad_mc_samples=A.S, n_acyclicity_mc_samples=A.SA)


def _standalone(kw, x, mask, key):
    e = Engine(make_config(n_observations=x.shape[0], has_interventions=mask is not None, **kw))
    try:
        e.set_data(x, mask)
        e.init_particles(random.PRNGKey(key))
        for t0, n in CHUNKS:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _batch(kw, datasets, keys):
    e = Engine(make_config(n_observations=datasets[0][0].shape[0], has_interventions=any(m is not None for _, m in datasets),
                           n_chains=len(keys), **kw))
    try:
        for c, (x, mask) in enumerate(datasets):
            e.set_data_problem(c, x, mask)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in CHUNKS:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


@pytest.mark.parametrize("d,N", A.CHAIN_CASES, ids=[f"d{d}-N{N}" for d, N in A.CHAIN_CASES])
def test_per_chain_data_along_n(d, N):
    """three chains with a data set each (chain 1 with interventions, chains 0 and 2 without) end three steps bit-identical to three
    standalone engines: the per-chain paired / split-f16 kernels below 129 observations, the unpaired ones above, k_lin_grad_chains at its
    largest LDS footprint"""
    N = A.lin_cut(d) if N == "cut" else N
    sets = [(A.structured_x(d, N, seed=11 + c), A.random_mask(d, N) if c == 1 else None) for c in range(3)]
    keys, kw = [61, 62, 63], _lin(d)
    cst = _batch(kw, sets, keys)
    assert cst["z"].shape[0] == 3 * A.M and cst["key"].shape == (3, 2)
    for c, key in enumerate(keys):
        st, sl = _standalone(kw, sets[c][0], sets[c][1], key), slice(c * A.M, (c + 1) * A.M)
        for k in STATE:
            assert np.isfinite(st[k]).all() and np.isfinite(cst[k][sl]).all(), (c, k)
            assert np.array_equal(cst[k][sl], st[k]), (c, k, np.abs(cst[k][sl].astype(np.float64) - st[k]).max())
        assert np.array_equal(cst["key"][c], st["key"]), c
    assert not np.array_equal(cst["z"][:A.M], cst["z"][A.M:2 * A.M])   # (the chains are not copies of one another)
