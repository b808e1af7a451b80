"""Host tests (no GPU) of tests/transform_states.py: on the two builds of the C oracle alone, every case of tests/test_gpu_transform.py is
finite in float32 and NOT VACUOUS for the last stage of a step -- conditions on the states, not measurements:

  weights     median off-diagonal kernel entry (per segment, over its scale) in [0.2, 0.9], none above 0.98      (every case but `far`)
  cross       max |phi - phi(K := diag K)| / max |phi| >= 0.25 per segment: a quarter of phi comes from OTHER particles
  repulsion   t = 0: max |repulsion term| / max |phi| >= 0.3 per segment
  ratio       offset_cluster: mean |x| over mean |x_a - x_b| >= 30 per segment
  tiny        far: kernel entries below 1e-15 and above 1e-30
  reference   the float64 numpy reference (transform_states.reference_transform) equals the float64 C oracle's kxx / phi_* to 1e-12

A case lists in `exempt` the conditions that cannot hold for it by construction (a single particle; `far`).  For every case the float32
oracle's own error in the quantities of the GPU test is printed (`pytest -s`): sequential arithmetic with direct differences, the yardstick
beside the device's numbers in profiles/transform_errors.txt."""
import numpy as np
import pytest

import transform_states as ts
from conftest import rel_err
from dibs_amd._abi import make_config


@pytest.mark.parametrize("case", ts.CASES, ids=ts.case_id)
def test_case_is_finite_and_not_vacuous(c_oracle64, c_oracle32, case):
    b = ts.build(case, c_oracle64)
    cfg = make_config(**b["cfg_kw"])
    M, joint = b["M"], b["theta"] is not None
    _, ref, nxt = ts.oracle_step(c_oracle64, b)
    _, r32, n32 = ts.oracle_step(c_oracle32, b)
    segs = ("z", "theta") if joint else ("z",)
    for r, n in ((ref, nxt), (r32, n32)):   # finite in float32 as in float64, and the step moves every segment
        for s in segs:
            assert np.isfinite(r["phi_" + s]).all() and np.isfinite(n[s]).all() and np.isfinite(n["v_" + s]).all(), s
            assert np.abs(r["phi_" + s]).max() > 0, s
        assert np.isfinite(r["kxx"]).all() and np.isfinite(r["grad_z"]).all()
    assert cfg.optimizer == 0 or np.abs(b["v_z"]).max() > 0   # (RMSprop: the second moment the case starts from)

    # the numpy reference against the float64 oracle, fed the oracle's gradients
    mine = ts.reference_transform(cfg, b["z"], b["theta"], ref["grad_z"], ref["grad_theta"], b["v_z"], b["v_theta"])
    assert rel_err(mine["kxx"], ref["kxx"]) < 1e-12
    for s in segs:
        assert rel_err(mine["phi_" + s], ref["phi_" + s]) < 1e-12, s
        assert rel_err(mine[s], nxt[s]) < 1e-12 and rel_err(mine["v_" + s], nxt["v_" + s]) < 1e-12, s

    diag = ts.reference_transform(cfg, b["z"], b["theta"], ref["grad_z"], ref["grad_theta"], diag_only=True)
    xs = dict(z=b["z"].reshape(M, -1), theta=b["theta"])
    note = []
    for s, kname, scale in (("z", "kz", cfg.scale_latent), ("theta", "kt", cfg.scale_theta))[:len(segs)]:
        phi = mine["phi_" + s].reshape(M, -1)
        top = np.abs(phi).max()
        if M > 1:
            off = ts.off_diagonal(mine[kname]) / scale
            note.append(f"{s}: K median {np.median(off):.2f} max {off.max():.2f}")
            if "weights" not in b["exempt"]:
                assert 0.2 <= np.median(off) <= 0.9 and off.max() <= 0.98, (s, np.median(off), off.max())
            if b["state"] == "far":
                assert ((off < 1e-15) & (off > 1e-30)).any(), s
        cross = np.abs(phi - diag["phi_" + s].reshape(M, -1)).max() / top
        rep = np.abs(mine["rep_" + s]).max() / top
        note.append(f"cross {cross:.2f} repulsion {rep:.2f}")
        if "cross" not in b["exempt"]:
            assert cross >= 0.25, (s, cross)
        if b["t"] == 0 and not {"repulsion", "cross"} & set(b["exempt"]):
            assert rep >= 0.3, (s, rep)
        # the share of coordinates that carry signal (conftest.update_check): the GPU test asks for half of ts.SIGNAL_SHARE
        share = float((np.abs(ref["phi_" + s]) > 1e-3 * np.abs(ref["phi_" + s]).max()).mean())
        note.append(f"signal share {share:.3f}")
        assert share >= ts.SIGNAL_SHARE[s], (s, share)
        if s == "theta":
            assert "oddP" not in b["name"] or b["theta"].shape[1] % 2 == 1
        if b["state"] == "offset_cluster":
            ratio = np.linalg.norm(xs[s], axis=1).mean() / np.sqrt(ts.off_diagonal(ts.sq_dists(xs[s]))).mean()
            note.append(f"|x| / |x_a - x_b| {ratio:.0f}")
            assert ratio >= 30, (s, ratio)

    # the float32 oracle's own error in the GPU test's quantities
    y = ts.transform_errors(b, cfg, r32["kxx"], r32["phi_z"], r32["phi_theta"], r32["grad_z"], r32["grad_theta"])
    assert y["kmat_tiny_ok"] and y["kmat_over_bound"] <= 1.0   # (the reference's float32 build is inside the entry-wise bound itself)
    print(f"\ntransform-host | {b['id']:36s} " + " | ".join(note))
    print(f"transform-host | {b['id']:36s} f32-oracle: K entry-wise {y['kmat_over_bound']:.2f} of its bound on {y['kmat_entries']} entries, "
          + " ".join(f"phi_{s} {y['phi_' + s]:.1e} (p99 {y['phi_' + s + '_p99']:.1e})" for s in segs)
          + " | end to end " + " ".join(f"phi_{s} {rel_err(r32['phi_' + s], ref['phi_' + s]):.1e}" for s in segs))


def test_every_branch_of_the_case_table_is_named():
    """the branches of the issue's case table, by the prefix of the cases that exist for them"""
    names = [c["name"] for c in ts.CASES]
    for prefix in ("phi4_ragged_M1", "phi4_ragged_M5", "phi4_ragged_M33", "phi4_full", "phi8_", "phi16_ragged", "phi16_full", "phi4_joint_lin_d5",
                   "phi4_joint_lin_d6", "phi4_joint_nn_oddP", "gemm_marginal_M257", "gemm_marginal_M1024_offset_cluster", "gemm_joint_d5",
                   "gemm_joint_d6", "kmat_direct", "kmat_insample", "kmat_tiled_ns1", "kmat_tiled_split_finish", "kmat_intail", "kmat_stream2",
                   "kmat_tile64"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert {c["optimizer"] for c in ts.CASES} == {"rmsprop", "gd"}
    for fam in ("marginal", "lingauss"):
        assert any(c["optimizer"] == "gd" and c["family"] == fam for c in ts.CASES), fam
