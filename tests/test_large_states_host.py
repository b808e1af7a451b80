"""Host tests (no GPU) of tests/large_states.py: every case of LARGE_CASES is finite in FLOAT32 and non-vacuous -- conditions on the inputs,
checked on the float64 and the float32 build of the C oracle (the torch-autograd oracle for the soft-graph BGe cases, which the C port does
not have).  tests/test_gpu_max_size.py runs the same cases on the device; what it can notice depends on what is pinned here:

  finite        every stage buffer and the next z, v_z (theta, v_theta) of the float32 oracle, and 0.1 max |phi|^2 < 1e37: RMSprop's second
                moment stays inside float32, the update is compared, not skipped
  same draws    sampled graphs and loop-carry key identical between the two oracles
  parent sets   mean size in [2, 40] (sampled graphs where the estimator samples them, and the expected size under the edge probabilities
                sigmoid(alpha u_i . v_j) in every case); on the dense-ish state at least 8 problems with more than 32 parents
  neighbours    every off-diagonal entry of the kernel matrix in [0.2, 0.9]: the cross-particle terms of the transform count
  acyclicity    max |w_acyc| > 0 and at least 10 % of its off-diagonal entries above 1e-3 of the maximum
  signal share  the share of coordinates with |phi| > 1e-3 max |phi| (conftest.update_check) is at least the one recorded in LARGE_CASES"""
import numpy as np
import pytest

import large_states as ls
from conftest import update_check
from dibs_amd._abi import make_config

C_CASES = [c for c in ls.LARGE_CASES if c["family"] != "marginal_reparam"]
AUTOGRAD_CASES = [c for c in ls.LARGE_CASES if c["family"] == "marginal_reparam"]


def test_case_list_covers_the_sizes():
    by = {}
    for c in ls.LARGE_CASES:
        by.setdefault(c["family"], []).append(c["d"])
    assert sorted(set(by["marginal_score"])) == [192, 193, 225, 241, 255, 256] and by["marginal_score"].count(256) == 3
    assert sorted(by["marginal_reparam"]) == [193, 256] and sorted(by["lingauss"]) == [193, 256] and sorted(by["densenn"]) == [225, 256]
    assert len({ls.case_id(c) for c in ls.LARGE_CASES}) == len(ls.LARGE_CASES)


def test_state_construction():
    rng = np.random.default_rng(0)
    M, d = 3, 40
    z0 = rng.standard_normal((M, d, d, 2)) / np.sqrt(d)
    z = ls.clustered_sparse_state(z0, 0.6, 2.0)
    assert z.shape == z0.shape and np.array_equal(z, z.astype(np.float32))
    assert np.array_equal(z, ls.clustered_sparse_state(z0, 0.6, 2.0)), "seeded"
    c = np.float64(np.float32(0.6))
    assert (z[:, :, 0, 0] == c).all() and (z[:, :, 0, 1] == -c).all()
    # column 0 shifts every edge score by -c^2
    rest = np.einsum("mik,mjk->mij", z[:, :, 1:, 0], z[:, :, 1:, 1])
    assert np.allclose(np.einsum("mik,mjk->mij", z[..., 0], z[..., 1]), rest - c * c, rtol=0, atol=1e-12)
    # every particle is the scaled first one plus noise of 0.05 sd(z0[0]) per entry
    dev = (z - 2.0 * z0[:1])[:, :, 1:]
    assert abs(dev.std() / (0.05 * z0[0].std()) - 1) < 0.05 and abs(dev.mean()) < 1e-3


def _expected_parents(z, alpha):
    s = alpha * np.einsum("mik,mjk->mij", z[..., 0], z[..., 1])
    p = 1.0 / (1.0 + np.exp(-s))
    p[:, np.arange(p.shape[1]), np.arange(p.shape[1])] = 0.0
    return float(p.sum(axis=1).mean())


def _check_share(case, measured, which):
    rec = case[which]
    print(f"large-state | {ls.case_id(case)}: {which} measured {measured:.4f}, recorded {rec}")
    assert rec is not None and measured >= rec, (ls.case_id(case), which, measured, rec)


@pytest.mark.parametrize("case", C_CASES, ids=ls.case_id)
def test_case_is_finite_and_not_vacuous(c_oracle64, c_oracle32, case):
    b = ls.large_case(case, c_oracle64)
    cfg = make_config(**b["cfg_kw"])
    M, d = b["M"], b["d"]
    before, d64, s64 = ls.oracle_step(c_oracle64, b)
    _, d32, s32 = ls.oracle_step(c_oracle32, b)
    joint = b["theta"] is not None
    # finite in float32, RMSprop's second moment inside float32
    for name, a in d32.items():
        assert np.isfinite(a).all(), name
    for name in ("z", "v_z") + (("theta", "v_theta") if joint else ()):
        assert np.isfinite(s32[name]).all(), name
        assert not np.array_equal(s32[name], before[name]), (name, "the step moved nothing")
    assert 0.1 * float(np.abs(d32["phi_z"]).max()) ** 2 < 1e37
    if joint:
        assert 0.1 * float(np.abs(d32["phi_theta"]).max()) ** 2 < 1e37
    # the same draws in both oracles
    assert np.array_equal(d32["g_samples"], d64["g_samples"]) and np.array_equal(s32["key"], s64["key"])
    # parent sets
    alpha = cfg.alpha_linear * b["t"]
    assert 2 <= _expected_parents(b["z"], alpha) <= 40
    sampled = bool(d64["g_samples"].any())
    assert sampled == (b["cfg_kw"].get("grad_estimator_z", "score") == "score")
    if sampled:
        mean_l, n_wide = ls.parent_stats(d64["g_samples"])
        print(f"large-state | {b['id']}: parents per node {mean_l:.1f}, problems with more than 32 parents {n_wide}")
        assert 2 <= mean_l <= 40
        if b["c"] == ls.DENSE["c"] and b["scale"] == ls.DENSE["scale"]:
            assert n_wide >= 8
    # neighbouring particles
    off = d64["kxx"][~np.eye(M, dtype=bool)]
    assert off.size == M * (M - 1) and (off >= 0.2).all() and (off <= 0.9).all(), off
    # a non-trivial acyclicity gradient
    wa = np.abs(d64["w_acyc"])
    assert wa.max() > 0 and (wa[:, ~np.eye(d, dtype=bool)] > 1e-3 * wa.max()).mean() >= 0.10
    # the float32 oracle passes the step criterion, and the share of signal coordinates is the recorded one
    u = update_check(cfg, before["z"], before["v_z"], d32["phi_z"], d64["phi_z"], s32["z"], s64["z"])
    _check_share(case, u["signal_share"], "share_z")
    if joint:
        u = update_check(cfg, before["theta"], before["v_theta"], d32["phi_theta"], d64["phi_theta"], s32["theta"], s64["theta"])
        _check_share(case, u["signal_share"], "share_theta")


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=ls.case_id)
def test_soft_bge_case_is_finite_and_not_vacuous(c_oracle64, case):
    """MarginalDiBS with the reparam estimator: one particle (the kernel matrix is 1 x 1), no float32 oracle.  The float64 autograd step must
    leave RMSprop's second moment inside float32 and carry signal (about 4 s of autograd per case, on one thread)."""
    b = ls.large_case(case, c_oracle64)
    r = ls.autograd_step(b)
    for name, a in r.items():
        assert np.isfinite(a).all(), name
    assert 0.1 * float(np.abs(r["phi_z"]).max()) ** 2 < 1e37
    assert 2 <= _expected_parents(b["z"], make_config(**b["cfg_kw"]).alpha_linear * b["t"]) <= 40
    assert np.abs(r["grad_z"]).max() > 0 and not np.array_equal(r["z"], b["z"])
    _check_share(case, float((np.abs(r["phi_z"]) > 1e-3 * np.abs(r["phi_z"]).max()).mean()), "share_z")
