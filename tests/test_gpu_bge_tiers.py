"""GPU tests of the BGe node scores at EVERY parent-set size and in every queue tier of the factorisation kernels (k_bge_chol,
k_bge_chol_wide and the queueing of k_bge_sample, dibs_amd/csrc/kernels_bge.h), in each of their instantiations.

The other step tests score graphs sampled from freshly initialised particles, whose parent sets have l ~ Binomial(d - 1, 1/2) members: two
or three of the nine tiers per size.  Here the particles come from tests/bge_states.py (tier_sweep_state): one step at t = 1 in lock-step
with the f64 C oracle, sampled graphs bit-identical, every l in 0 .. d - 1 and every (direct / complement form, tier) cell that exists at
the size asserted present on the graphs read back from the device, node scores compared ENTRY BY ENTRY:

    |dev - ref| < tol(d) max |ref|,   tol = 1e-4 (d <= 50), 5e-4 (d <= 112), 1e-3 beyond

-- the bound test_marginal_bge_step_stages holds the array's worst entry to, so every cell is held to it (node scores of these states run
from about -480 to +70 and cross zero: no division by an entry's own size).  The float64 engine is held to the 1e-9 of test_gpu_f64.py.
Every comparison prints the worst error per cell (`pytest -s`), beside it the same error of the float32 build of the C oracle as the
yardstick of what float32 arithmetic gives; profiles/bge_tier_errors.txt keeps one run.

LDS cut: bge_launch_chol takes k_bge_chol<false, true> WITHOUT interventions once bge_chol_lds_bytes(d, true) exceeds 150 KiB.  No d <= 128
does with the present layout (149 648 bytes at d = 128; tests/test_bge_states_host.py pins that), so that case skips; d = 128, the largest
LDS-resident pair, is in the list of plain cases instead."""
import numpy as np
import pytest

import bge_states as bs
from conftest import rel_err
from dibs_amd._abi import make_config

pytestmark = pytest.mark.gpu
TOL_F64 = 1e-9   # tests/test_gpu_f64.py


def tol(d):
    return 1e-4 if d <= 50 else (5e-4 if d <= 112 else 1e-3)   # tests/test_gpu_parity.py, test_marginal_bge_step_stages


_CASES, _REFS = {}, {}


def _case(d, M=4, S=8, interv=False, seed=0):
    key = (d, M, S, interv, seed)
    if key not in _CASES:
        _CASES[key] = bs.sweep_case(d, M, S, interv=interv, seed=seed)
    return _CASES[key]


def _ref(oracles, d, M=4, S=8, interv=False, seed=0):
    """the f64 oracle's step of a case (computed once, shared by the tests, never modified) and the f32 oracle's node scores beside it"""
    key = (d, M, S, interv, seed)
    if key not in _REFS:
        o64, o32 = oracles
        case = _case(*key)
        r = bs.oracle_step(o64, case)
        r32 = bs.oracle_step(o32, case)
        # (a Bernoulli draw of the f32 oracle may fall on the other side of a threshold: those samples are left out of the yardstick)
        same = (r32["g_samples"] == r["g_samples"]).all(axis=(2, 3))[:, :, None]
        ref = dict(g_samples=r["g_samples"], node_scores=r["node_scores"], ns_f32=np.where(same, r32["node_scores"].astype(np.float64), r["node_scores"]))
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.fixture(scope="module")
def oracles(c_oracle64, c_oracle32):
    return c_oracle64, c_oracle32


def _engine_step(case, precision=32):
    """one engine step of the case: (graphs from PARENT_MASKS, node scores [M, S, d])"""
    from dibs_amd.engine import Engine
    d, M, S = case["d"], case["M"], case["S"]
    kw = dict(case["cfg_kw"], precision=precision) if precision != 32 else case["cfg_kw"]
    eng = Engine(make_config(**kw))
    try:
        assert eng.precision == precision
        eng.set_data(case["x"], case["mask"])
        z = case["z"]
        eng.set_state(z=z, v_z=np.zeros_like(z), key=case["key"], baseline=np.zeros(M))
        eng.run(case["t"], 1)
        gg = bs.graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d)
        ns = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1).copy()   # device layout [m][j][s]
        return gg, ns
    finally:
        eng.close()


def _compare(what, case, ref, gg, ns, bound):
    d = case["d"]
    assert np.array_equal(gg, ref["g_samples"]), "sampled graphs must be bit-identical"
    bs.assert_coverage(bs.tier_histogram(gg, d), d)
    want = ref["node_scores"]
    scale = float(np.abs(want).max())
    assert np.isfinite(ns).all() and np.isfinite(want).all() and scale > 0
    dev = {name: (n, e) for name, n, e in bs.cell_errors(ns, want, gg, d)}
    f32 = {name: e for name, n, e in bs.cell_errors(ref["ns_f32"], want, gg, d)}
    print(f"\nbge-tier | {what}: max |ref| {scale:.1f}, bound {bound:.0e} max |ref|")
    for name, (n, e) in dev.items():
        print(f"bge-tier |   {name:18s} problems {n:5d}  device abs {e:.3e} scaled {e / scale:.2e}   f32 oracle abs {f32[name]:.3e} scaled {f32[name] / scale:.2e}"
              + ("   ABOVE HALF THE BOUND" if e / scale > 0.5 * bound else ""))
    bad = {name: f"{e / scale:.2e}" for name, (n, e) in dev.items() if not e / scale < bound}
    assert not bad, (what, "scaled error per cell", bad, "bound", bound)
    assert (np.abs(ns - want) < bound * scale).all()
    if case["all_intervened"] is not None:
        assert not ns[:, :, case["all_intervened"]].any(), "a node intervened in every row scores exactly 0 at every l"


# ---- standalone float32 engine -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [50, 63, 64, 65, 80, 112, 128])
def test_no_interventions(oracles, d):
    """k_bge_chol<true, false> (d <= 64) / <true, true>: one matrix pair in LDS.  63 / 64: odd / even direct-complement boundary with up to
    32 rows; 65: first size with the one-problem-per-wave tier (l = 32 only, direct form); 112: 16-byte + 16-byte queue entries at the
    largest MFMA-tile size; 128: both mask words full, the largest LDS-resident pair."""
    case, ref = _case(d), _ref(oracles, d)
    gg, ns = _engine_step(case)
    _compare(f"d={d} k_bge_chol<R_LDS,{'W2' if d > 64 else 'W1'}>", case, ref, gg, ns, tol(d))


def test_lds_cut_without_interventions(oracles):
    """k_bge_chol<false, true> without interventions: the smallest d <= 128 beyond the 150 KiB cut of bge_launch_chol"""
    d = bs.lds_cut_size()
    if d is None:
        pytest.skip("bge_chol_lds_bytes(d, true) stays below the 150 KiB cut for every d <= 128 (149 648 bytes at d = 128): the cut is not reachable")
    case, ref = _case(d), _ref(oracles, d)
    gg, ns = _engine_step(case)
    _compare(f"d={d} k_bge_chol<cached,W2> (LDS cut)", case, ref, gg, ns, tol(d))


@pytest.mark.parametrize("d", [50, 80])
def test_interventions(oracles, d):
    """k_bge_chol<false, false / true>: one matrix pair per node (n_mats = d) read through the caches, N_j different per node, one node
    without observational data"""
    case, ref = _case(d, interv=True), _ref(oracles, d, interv=True)
    gg, ns = _engine_step(case)
    _compare(f"d={d} interventions k_bge_chol<cached,{'W2' if d > 64 else 'W1'}>", case, ref, gg, ns, tol(d))


@pytest.mark.parametrize("d", [130, 200])
def test_wide(oracles, d):
    """k_bge_chol_wide<false>: three (d = 130) / four (d = 200) mask words, one problem per wave whatever its size, complement form with up
    to 100 rows.  Every problem is in the last queue there; the cells of the table are those of the narrow kernels, for comparison."""
    case, ref = _case(d, 2, 4), _ref(oracles, d, 2, 4)
    gg, ns = _engine_step(case)
    _compare(f"d={d} k_bge_chol_wide", case, ref, gg, ns, tol(d))


# ---- batched engine: bit-identical to standalone engines (the contract of tests/test_gpu_batch.py) -------------------------------------------
@pytest.mark.parametrize("d,M,S", [(50, 4, 8), (80, 4, 8), (130, 2, 4)])
def test_batched_equals_standalone(oracles, d, M, S):
    """k_bge_sample<4, true, true> + k_bge_chol<false, false / true, true> / k_bge_chol_wide<true>: two problems with different data, the
    second with interventions, each from its own tier-sweep state and key.  Node scores and parent sets of problem p must equal those of a
    standalone engine given the same z, key and data bit for bit; problem 0's standalone result is the one test_no_interventions /
    test_wide hold to the oracle, problem 1's the one of test_interventions (d = 130: held to the oracle here).
    (First run, d = 80, problem 0: 1.4e-14 apart, one unit in the last place -- k_bge_chol<true, true> scores through bge_score, the batched
    instantiation through bge_score_pre, and the compiler fused their multiply-adds differently; contraction is off in both since.)"""
    from dibs_amd.engine import Engine
    cases = [_case(d, M, S), _case(d, M, S, interv=True)]
    eng = Engine(make_config(**dict(cases[0]["cfg_kw"], has_interventions=False, n_problems=2)))
    try:
        for p, c in enumerate(cases):
            eng.set_data_problem(p, c["x"], c["mask"])
        z = np.concatenate([c["z"] for c in cases])
        eng.set_state(z=z, v_z=np.zeros_like(z), baseline=np.zeros(2 * M))
        eng.set_keys(np.stack([c["key"] for c in cases]))
        eng.run(1, 1)
        masks = eng.read("PARENT_MASKS").reshape(2, -1)
        ns = eng.read("NODE_SCORES").reshape(2, M, d, S)
    finally:
        eng.close()
    for p, c in enumerate(cases):
        gg, ns_alone = _engine_step(c)
        gb = bs.graphs_from_masks(masks[p], M, S, d)
        assert np.array_equal(gb, gg), p
        bs.assert_coverage(bs.tier_histogram(gb, d), d)
        assert np.array_equal(ns[p].transpose(0, 2, 1), ns_alone), (p, np.abs(ns[p].transpose(0, 2, 1) - ns_alone).max())
        if p == 1:
            assert not ns[p][:, c["all_intervened"]].any()
            if d > 128:
                _compare(f"d={d} interventions k_bge_chol_wide", c, _ref(oracles, d, M, S, interv=True), gg, ns_alone, tol(d))


# ---- float64 engine --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [50, 64])
def test_f64_engine(oracles, d):
    """the float64 engine's factorisations (kernels_f64.h) on the same states: nothing but z is rounded to float32; entry-wise to 1e-9"""
    case, ref = _case(d), _ref(oracles, d)
    gg, ns = _engine_step(case, precision=64)
    _compare(f"d={d} float64 engine", case, ref, gg, ns, TOL_F64)


# ---- dibs_score_graphs: the queueing of GIVEN parent sets (k_bge_sample<4, false>) --------------------------------------------------------------
@pytest.mark.parametrize("d,M,S", [(50, 4, 8), (70, 4, 8), (130, 2, 4)])
def test_score_graphs(oracles, d, M, S):
    """The sampled graphs of the state as hard graphs, plus the complete digraph without its diagonal (l = d - 1 at every node) and the
    empty graph (l = 0 at every node), with and without a held-out intervention mask, against the oracle's scorer to the 2e-5 of
    test_score_graphs_and_mixture."""
    from dibs_amd.inference.scoring import score_graphs
    case, ref = _case(d, M, S), _ref(oracles, d, M, S)
    g = np.concatenate([ref["g_samples"].reshape(M * S, d, d).astype(np.int32), 1 - np.eye(d, dtype=np.int32)[None], np.zeros((1, d, d), np.int32)])
    bs.assert_coverage(bs.tier_histogram(g, d), d)
    cfg = make_config(n_vars=d, n_particles=1, n_observations=case["x"].shape[0])
    want = oracles[0].score_graphs(cfg, case["x"], None, g)
    got = score_graphs(case["lm"], g, None, case["x"], None)
    print(f"\nbge-tier | d={d} dibs_score_graphs: observational {rel_err(got, want):.2e} (bound 2e-5)")
    assert rel_err(got, want) < 2e-5
    mask = (np.random.default_rng(d).random(case["x"].shape) < 0.1).astype(np.int32)   # (scored as held-out data: N_j per node)
    want = oracles[0].score_graphs(cfg, case["x"], mask, g)
    got = score_graphs(case["lm"], g, None, case["x"], mask)
    print(f"bge-tier | d={d} dibs_score_graphs: held-out with interventions {rel_err(got, want):.2e} (bound 2e-5)")
    assert rel_err(got, want) < 2e-5
