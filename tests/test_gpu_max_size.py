"""GPU tests of every model family at 192 .. 256 variables -- the engine maximum included -- on states at which the WHOLE step is finite and
non-trivial: stage by stage and through the optimizer update, through the C ABI in lock-step with the oracle.

The other large-d tests start from freshly initialised particles.  There phi^2 leaves float32 in RMSprop's second moment from d = 128 on, so
they stop after PHI_Z, and the kernel matrix between two particles is ~1e-89, so the cross-particle terms of k_phi_update add nothing.
The cases of tests/large_states.py (LARGE_CASES; tests/test_large_states_host.py pins on the oracles alone that they are finite in float32,
have neighbouring particles, non-trivial parent sets and a non-trivial acyclicity gradient) have neither problem, so here NOTHING is
skipped: sampled graphs and key bit-identical, every stage buffer, v_z, z (and theta) by the step criterion of tests/conftest.py, and a
second step from the device's own next state.

Bounds.  Kept from the existing tests beyond 112 variables: SCORES 2e-6, KXX 1e-5, LOGPROBS_Z 5e-5, LOGPROBS_THETA 2e-5, W_LIK / PHI_THETA
2e-3, GRAD_THETA 5e-4.  NODE_SCORES, W_ACYC, GRAD_Z, PHI_Z and v_z: plain float32 evaluation of the reference's own formulas does not
meet the small-d bounds at these sizes (a product of 255 factors in float32: the float32 build of the C oracle is 3e-5 .. 1.2e-4 from the
float64 build), so the bound of a buffer is

    max(existing large-d bound, 4 x |float32 oracle - float64 oracle|)       (max-norm, relative to the largest entry)

with the yardstick computed here, on the same case, from the two oracle builds alone -- never from device output.  The factor 4: the device
sums the products and the chain mean in another order than the C port and the yardstick is a single draw of the rounding; it is the margin
test_acyclicity_f16_pipe_worst_cases gives its float32 floor.  The soft-graph BGe cases have no float32 oracle: the bounds of
test_marginal_bge_reparam_estimator for d >= 50.  Every comparison prints yardstick, bound and device error (`pytest -s`);
profiles/max_size_stage_errors.txt keeps one run.

What the sizes reach (tests/large_states.py): four full mask words and k_bgemm's exact 4 x 4 tile grid (256), the pad row / the 15 pad rows
and columns of k_acycb_init inside a full grid (255 / 241), a partly filled last tile (225, 193), no padding at all (192), k_bge_soft with
four rows in every lane (256).  What W_ACYC notices there: a transposed or wrong-stride read of the powers in k_acycb_out, or pad rows AND
columns filled.  A single missing guard of k_acycb_init (`a < d` or `b < d` alone) is invisible: the padded matrix stays block-triangular,
[[A, B], [0, 0]] or [[A, 0], [C, D]], and its powers keep A^n in the block that is read.

Sampled graphs: the engine keeps PARENT_MASKS for the BGe model only, so the bit-identical graph comparison is made in the marginal cases.
The joint engine does not expose the graphs of its score estimator (densenn, d = 225); there the per-sample LOGPROBS_Z / LOGPROBS_THETA,
held to 5e-5 / 2e-5 of the largest, would show a sample whose graph differs, and the key is compared in every case."""
import numpy as np
import pytest

import bge_states as bs
import large_states as ls
from conftest import assert_update_parity, rel_err, update_check
from dibs_amd._abi import make_config

pytestmark = pytest.mark.gpu

FIXED = dict(SCORES=2e-6, KXX=1e-5, LOGPROBS_Z=5e-5, LOGPROBS_THETA=2e-5, W_LIK=2e-3, PHI_THETA=2e-3, GRAD_THETA=5e-4)
FLOOR = dict(NODE_SCORES=1e-3, W_ACYC=1e-5, GRAD_Z=1e-4, PHI_Z=1e-4, V_Z=2e-4)   # the existing large-d bounds; raised to 4 x yardstick
SOFT_BGE = dict(LOGPROBS_Z=3e-4, GRAD_Z=2e-3, PHI_Z=2e-3)                        # test_marginal_bge_reparam_estimator, d >= 50
ORACLE_NAME = dict(SCORES="scores", KXX="kxx", LOGPROBS_Z="logprobs_z", LOGPROBS_THETA="logprobs_th", W_LIK="w_lik", PHI_THETA="phi_theta",
                   GRAD_THETA="grad_theta", NODE_SCORES="node_scores", W_ACYC="w_acyc", GRAD_Z="grad_z", PHI_Z="phi_z")


def _cases(family):
    return [c for c in ls.LARGE_CASES if c["family"] == family]


def _engine(b):
    from dibs_amd.engine import Engine
    eng = Engine(make_config(**b["cfg_kw"]))
    eng.set_data(b["x"], b["mask"])
    st = ls.fresh_state(b)
    kw = dict(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
    if st["theta"] is not None:
        kw.update(theta=st["theta"], v_theta=st["v_theta"])
    eng.set_state(**kw)
    return eng


def _report(b, name, err, bound, yardstick=None):
    y = "      -  " if yardstick is None else f"{yardstick:.2e}"
    print(f"max-size | {b['id']:82s} {name:14s} f32-oracle {y}  bound {bound:.1e}  device {err:.2e}" + ("   ABOVE THE BOUND" if not err < bound else ""))
    return err < bound


def _second_step(eng, b, first):
    """one more step from the device's own next state: the optimizer state was really written"""
    eng.run(b["t"] + 1, 1)
    g = eng.get_state()
    assert np.isfinite(g["z"]).all() and np.isfinite(g["v_z"]).all()
    assert not np.array_equal(g["z"], first["z"])
    if g["theta"] is not None:
        assert np.isfinite(g["theta"]).all() and not np.array_equal(g["theta"], first["theta"])


def _c_oracle_case(case, o64, o32, buffers):
    """One step of a case on the device against the float64 C oracle; `buffers`: the stage buffers of the family's stage test."""
    b = ls.large_case(case, o64)
    cfg = make_config(**b["cfg_kw"])
    M, S, d = b["M"], b["S"], b["d"]
    before, ref, nxt = ls.oracle_step(o64, b)
    _, r32, n32 = ls.oracle_step(o32, b)
    assert np.array_equal(r32["g_samples"], ref["g_samples"])   # (pinned by the host test: the yardstick compares the same problems)
    eng = _engine(b)
    try:
        eng.run(b["t"], 1)
        g = eng.get_state()
        dev = {name: eng.read(name) for name in buffers}
        masks = eng.read("PARENT_MASKS") if "NODE_SCORES" in buffers else None
        _second_step(eng, b, g)
    finally:
        eng.close()
    assert (g["key"] == nxt["key"]).all()
    if masks is not None:
        assert np.array_equal(bs.graphs_from_masks(masks, M, S, d), ref["g_samples"]), "sampled graphs must be bit-identical"
        dev["NODE_SCORES"] = dev["NODE_SCORES"].reshape(M, d, S).transpose(0, 2, 1)   # device layout [m][j][s]
    ok = []
    for name in buffers:
        want = ref[ORACLE_NAME[name]]
        assert np.isfinite(dev[name]).all() and np.abs(want).max() > 0, name
        if name in FIXED:
            ok.append(_report(b, name, rel_err(dev[name], want), FIXED[name]))
        else:
            y = rel_err(r32[ORACLE_NAME[name]], want)
            ok.append(_report(b, name, rel_err(dev[name], want), max(FLOOR[name], 4 * y), y))
    y = rel_err(n32["v_z"], nxt["v_z"])
    ok.append(_report(b, "V_Z", rel_err(g["v_z"], nxt["v_z"]), max(FLOOR["V_Z"], 4 * y), y))
    assert all(ok), "a stage buffer is beyond its bound (see the lines printed above)"
    u = update_check(cfg, before["z"], before["v_z"], dev["PHI_Z"], ref["phi_z"], g["z"], nxt["z"])
    print(f"max-size | {b['id']:82s} z update      {u}")
    assert_update_parity(u, 0.5 * b["share_z"], f"{b['id']} z")
    if b["theta"] is not None:
        u = update_check(cfg, before["theta"], before["v_theta"], dev["PHI_THETA"], ref["phi_theta"], g["theta"], nxt["theta"])
        print(f"max-size | {b['id']:82s} theta update  {u}")
        assert_update_parity(u, 0.5 * b["share_theta"], f"{b['id']} theta")
    return b


MARGINAL = ("SCORES", "NODE_SCORES", "LOGPROBS_Z", "W_LIK", "W_ACYC", "GRAD_Z", "KXX", "PHI_Z")
JOINT = ("SCORES", "LOGPROBS_THETA", "LOGPROBS_Z", "GRAD_THETA", "W_LIK", "W_ACYC", "GRAD_Z", "KXX", "PHI_THETA", "PHI_Z")


@pytest.mark.parametrize("case", _cases("marginal_score"), ids=ls.case_id)
def test_marginal_bge_score_estimator(c_oracle64, c_oracle32, case):
    """MarginalDiBS + BGe, score estimator: k_bge_sample with three / four mask words, k_bge_chol_wide (parent sets of ~22, some beyond 32
    members), the global-memory acyclicity kernels (k_acycb_init, k_bgemm, k_acycb_out), k_phi_update with kernel-matrix entries of 0.6."""
    _c_oracle_case(case, c_oracle64, c_oracle32, MARGINAL)


@pytest.mark.parametrize("case", _cases("lingauss"), ids=ls.case_id)
def test_joint_lingauss(c_oracle64, c_oracle32, case):
    """JointDiBS + LinearGaussian, reparam estimator, 300 observations: the engine takes the Gram path (kernels_lin_gram.h) by itself, the
    operands of its kernels in global scratch; held-out scoring of 5 sparse graphs and the complete DAG on the same path, to the 2e-5 of
    test_joint_lingauss_gram_path."""
    from dibs_amd.inference.scoring import score_graphs
    from dibs_amd.models import LinearGaussian
    b = _c_oracle_case(case, c_oracle64, c_oracle32, JOINT)
    d = b["d"]
    rng = np.random.default_rng(3)
    gs = (rng.random((6, d, d)) < 0.1).astype(np.int32)
    gs[:, np.arange(d), np.arange(d)] = 0
    gs[5] = np.triu(np.ones((d, d), np.int32), 1)   # the complete DAG: node j has j parents
    th = rng.normal(size=(6, d, d)).astype(np.float32)
    want = c_oracle64.score_graphs(make_config(**b["cfg_kw"]), b["x"], b["mask"], gs, th.reshape(6, -1).astype(np.float64))
    got = score_graphs(LinearGaussian(n_vars=d), gs, th, b["x"], b["mask"])
    assert _report(b, "score_graphs", rel_err(got, want), 2e-5)


@pytest.mark.parametrize("case", _cases("densenn"), ids=ls.case_id)
def test_joint_densenn(c_oracle64, c_oracle32, case):
    """JointDiBS + DenseNonlinearGaussian, hidden (3,): the general device path (kernels_nn_generic.h) with the sampled graph of a block in
    global scratch; tanh without bias and the score estimator at 225, relu with bias and the reparam estimator at 256."""
    _c_oracle_case(case, c_oracle64, c_oracle32, JOINT)


@pytest.mark.parametrize("case", _cases("marginal_reparam"), ids=ls.case_id)
def test_marginal_bge_reparam_estimator(c_oracle64, case):
    """MarginalDiBS + BGe on Gumbel-soft graphs (k_bge_soft<.., 4, true>: four matrix rows per lane, every lane full at 256, the triangles in
    global scratch) against the torch-autograd oracle, as test_gpu_parity.py::test_marginal_bge_reparam_estimator, update included."""
    b = ls.large_case(case, c_oracle64)
    cfg = make_config(**b["cfg_kw"])
    r = ls.autograd_step(b)
    eng = _engine(b)
    try:
        eng.run(b["t"], 1)
        g = eng.get_state()
        dev = {name: eng.read(name) for name in SOFT_BGE}
        _second_step(eng, b, g)
    finally:
        eng.close()
    assert (g["key"] == r["key"]).all()
    ok = [_report(b, name, rel_err(dev[name], r[ORACLE_NAME[name]]), SOFT_BGE[name]) for name in SOFT_BGE]
    assert all(np.isfinite(dev[name]).all() for name in SOFT_BGE) and all(ok)
    v0 = np.zeros_like(b["z"])
    u = update_check(cfg, b["z"], v0, dev["PHI_Z"], r["phi_z"], g["z"], r["z"])
    print(f"max-size | {b['id']:82s} z update      {u}")
    assert_update_parity(u, 0.5 * b["share_z"], f"{b['id']} z")
    assert _report(b, "V_Z", rel_err(g["v_z"], r["v_z"]), 2 * SOFT_BGE["PHI_Z"] + SOFT_BGE["PHI_Z"] ** 2)   # v = 0.1 phi^2 from v = 0


def _bge_score_plain(g, x, mask, alpha_mu=1.0):
    """BGe log marginal likelihood of a hard graph in plain numpy float64 (linearGaussian.py:63-170): R_j by the triple loop over the rows
    in which node j is not intervened, masked log-determinants by slogdet of the sub-matrices"""
    from math import lgamma, log, pi
    N, d = x.shape
    al = d + 2.0
    small_t = alpha_mu * (al - d - 1) / (alpha_mu + 1)
    total = 0.0
    for j in range(d):
        rows = [n for n in range(N) if not mask[n, j]]
        Nn = float(len(rows))
        if Nn == 0:
            continue
        xb = [sum(float(x[n, a]) for n in rows) / Nn for a in range(d)]
        R = np.zeros((d, d))
        for a in range(d):
            for b in range(d):
                sab = 0.0
                for n in rows:
                    sab += (float(x[n, a]) - xb[a]) * (float(x[n, b]) - xb[b])
                R[a, b] = (small_t if a == b else 0.0) + sab + (Nn * alpha_mu / (Nn + alpha_mu)) * xb[a] * xb[b]
        pa = [i for i in range(d) if g[i, j]]
        l = len(pa)
        ld = lambda idx: np.linalg.slogdet(R[np.ix_(idx, idx)])[1] if idx else 0.0
        total += (0.5 * (log(alpha_mu) - log(Nn + alpha_mu)) + lgamma(0.5 * (Nn + al - d + l + 1)) - lgamma(0.5 * (al - d + l + 1))
                  - 0.5 * Nn * log(pi) + 0.5 * (al - d + 2 * l + 1) * log(small_t)
                  + 0.5 * (Nn + al - d + l) * ld(pa) - 0.5 * (Nn + al - d + l + 1) * ld(pa + [j]))
    return total


@pytest.mark.parametrize("d,N", [(7, 30), (13, 40)])
def test_host_bge_statistics_with_interventions_against_plain_loops(d, N):
    """The per-node matrices R_j the engine builds on the host (bge_host_stats, engine_data.hip: sums over centred rows with b innermost,
    since set_data of the 256-variable interventions case above took 18 s as a triple loop) against that triple loop written out in numpy,
    through dibs_score_graphs -- independent of the C oracle, whose copy of the loop changed alongside.  N_j differs per node, one node is
    intervened in every row (scores 0); random graphs, the empty graph and the complete DAG; 2e-5 as test_score_graphs_and_mixture."""
    from conftest import make_data
    from dibs_amd.inference.scoring import score_graphs
    data, _, lm = make_data(d, seed=5, n_obs=N)
    x = np.asarray(data.x)[:N].astype(np.float32)
    rng = np.random.default_rng(d)
    mask = (rng.random((N, d)) < 0.2).astype(np.int32)
    mask[:, d // 3] = 1
    gs = (rng.random((6, d, d)) < 0.3).astype(np.int32)
    gs[:, np.arange(d), np.arange(d)] = 0
    gs[4] = 0
    gs[5] = np.triu(np.ones((d, d), np.int32), 1)
    want = np.array([_bge_score_plain(g, x, mask) for g in gs])
    got = np.asarray(score_graphs(lm, gs, None, x, mask), np.float64)
    print(f"max-size | host BGe statistics d={d} N={N}: device {rel_err(got, want):.2e} (bound 2e-5)")
    assert rel_err(got, want) < 2e-5
