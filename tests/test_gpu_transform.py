"""GPU tests of the LAST stage of a step -- kernel matrix, SVGD transform, optimizer (kernels_kmat.h, k_phi_update, k_phi_gemm) -- on states
whose particles INTERACT: off-diagonal kernel weights of 0.2 .. 0.9 (tests/transform_states.py; tests/test_transform_states_host.py pins on
the oracles alone that every case is finite in float32 and not vacuous).  Everywhere else in the suite the kernel matrix is the identity to
float32 from d = 20 on, and phi_a = -grad_a / M whatever the transform kernels do with the other rows.

One step from set_state (second moments from one oracle step: RMSprop's step then depends on the SIZE of phi), eng.run(t, 1), three checks:

  kernel matrix, entry by entry   |K_dev - K_ref| / K_ref <= 2e-6 (1 + |ln(K_ref / scale)|) for every entry with K_ref >= 1e-30 scale;
                                  smaller entries non-negative and <= 2 K_ref + the smallest denormal; joint models: kz + kt with the sum of the
                                  parts' bounds, where neither part is that small.  Derived (transform_states.KMAT_REL), not measured.  The
                                  suite's 1e-5 in max-norm stays beside it.
  transform in isolation          PHI_Z / PHI_THETA against the float64 numpy reference fed the DEVICE'S OWN GRAD_* and the float64 kernel
                                  matrix of the state: max-norm relative to max |phi_ref| <= 1e-5 on every path -- the figure k_phi_gemm's
                                  header claimed for its regrouped repulsion; the direct-difference kernel is far inside it.
  end to end                      against COracle("f64").step(debug=True) with the suite's bounds (GRAD_Z / PHI_Z 1e-4, GRAD_THETA 5e-4,
                                  PHI_THETA 2e-3, KXX 1e-5) and conftest's step criterion with half the host-pinned signal share.

Every comparison prints the device's figure beside the float32 oracle's for the same case (`pytest -s`); profiles/transform_errors.txt keeps
one run (bit-reproducible).  Measured there, worst over the cases of a kernel family, isolated phi (device | float32 oracle):
    k_phi_update, marginal   1.65e-7 | 7.8e-8     (phi4_ragged_M255)
    k_phi_update, JOINT      2.25e-6 | 5.5e-8     (phi4_joint_lin_d5_M33, offset_cluster: the JOINT form subtracts two rounded products
                                                   -(2/h) x_b - -(2/h) x_a, 6e-8 |x| / |x_a - x_b| = 2.4e-6 at a ratio of 40; 3.3e-7 elsewhere)
    k_phi_gemm               2.19e-6 | 6.7e-8     (gemm_joint_d6_M319_wide, gradient regime; offset_cluster <= 9.8e-7)
ISOLATED_FAMILY is 4 x the device's worst (compiler drift) -- 6.6e-7, 9.0e-6, 8.8e-6 -- each above 4 x the oracle's worst, 3.1e-7, and none
above the 1e-5 that holds on every path.  Before k_phi_gemm took its value half relative to particle 0 (kernels_marginal.h) the
offset_cluster cases measured 4.1e-5 (marginal, M = 272), 7.5e-5 (M = 1024), 3.1e-5 / 6.0e-5 (joint): the finding of these tests.

What the cases notice (spot checks; K ~ 0.5, |g| and |x_b - x_a| of the size of phi M):
  - the single-row pair of an odd quarter dropped (phi4_ragged_M33: quarters of 9): phi_a loses K_ab (g_b - (2/h)(x_b - x_a)) / M, one of 33
    terms of random sign: ~ 0.5 / sqrt(33) ~ 9e-2 of max |phi| >> 1e-5;
  - a ragged 32-particle chunk of k_phi_gemm not zeroed (gemm_*_M257: one live row, 31 dead ones): columns b >= M of row a of the kernel
    matrix are the entries (a + 1, b - M), ~0.5, and the dead rows of the B tile repeat particle M - 1: 31 spurious terms of 0.5 g / M
    beside 257 of random sign, ~1 of max |phi|.  (The A tile's `bok` and the B tile's `rok` each zero those products alone: ONE of the
    two missing is invisible to any test, both missing is not.);
  - kz / kt swapped in the joint repulsion (phi4_joint_*, gemm_joint_*): the two matrices differ entry by entry by tens of percent
    (independent spreads), the repulsion is >= 0.3 of phi: >= 3e-2;
  - a wrong row index / m0 / rlast clamp: another particle's x_a enters every term of the repulsion: O(1)."""
import numpy as np
import pytest

import transform_states as ts
from conftest import assert_update_parity, rel_err, update_check
from dibs_amd._abi import make_config

pytestmark = pytest.mark.gpu

KXX_MAXNORM = 1e-5
ISOLATED = 1e-5   # on every path; per kernel family (module docstring) below
ISOLATED_FAMILY = dict(phi_update=6.6e-7, phi_update_joint=9.0e-6, phi_gemm=8.8e-6)
END_TO_END = dict(GRAD_Z=1e-4, PHI_Z=1e-4, GRAD_THETA=5e-4, PHI_THETA=2e-3)
ORACLE_NAME = dict(GRAD_Z="grad_z", PHI_Z="phi_z", GRAD_THETA="grad_theta", PHI_THETA="phi_theta")


def _engine(b, monkeypatch, **cfg_over):
    from dibs_amd.engine import Engine
    for k, v in b["env"].items():   # (latched when the engine is created: tuning.h)
        monkeypatch.setenv(k, v)
    eng = Engine(make_config(**dict(b["cfg_kw"], **cfg_over)))
    eng.set_data(b["x"], b["mask"])
    st = ts.fresh_state(b)
    kw = dict(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
    if st["theta"] is not None:
        kw.update(theta=st["theta"], v_theta=st["v_theta"])
    eng.set_state(**kw)
    return eng


def _report(b, what, err, bound, yardstick=None):
    y = "      -  " if yardstick is None else f"{yardstick:.2e}"
    print(f"transform | {b['id']:36s} {what:24s} f32-oracle {y}  bound {bound:.1e}  device {err:.2e}" + ("   ABOVE THE BOUND" if not err <= bound else ""))
    return err <= bound


def _step(b, monkeypatch):
    """one step of the case on a standalone float32 engine: (stage buffers, state after)"""
    joint = b["theta"] is not None
    eng = _engine(b, monkeypatch)
    try:
        eng.run(b["t"], 1)
        dev = {n: eng.read(n) for n in ("KXX", "GRAD_Z", "PHI_Z") + (("GRAD_THETA", "PHI_THETA") if joint else ())}
        return dev, eng.get_state()
    finally:
        eng.close()


@pytest.mark.parametrize("case", ts.CASES, ids=ts.case_id)
def test_transform_with_interacting_particles(c_oracle64, c_oracle32, case, monkeypatch):
    b = ts.build(case, c_oracle64)
    cfg = make_config(**b["cfg_kw"])
    M, joint = b["M"], b["theta"] is not None
    segs = ("z", "theta") if joint else ("z",)
    before, ref, nxt = ts.oracle_step(c_oracle64, b)
    _, r32, _ = ts.oracle_step(c_oracle32, b)
    dev, g = _step(b, monkeypatch)
    for name, a in dev.items():
        assert np.isfinite(a).all(), name
    gth = dev["GRAD_THETA"].reshape(M, -1) if joint else None
    e = ts.transform_errors(b, cfg, dev["KXX"], dev["PHI_Z"], dev.get("PHI_THETA"), dev["GRAD_Z"].reshape(b["z"].shape), gth)
    y = ts.transform_errors(b, cfg, r32["kxx"], r32["phi_z"], r32["phi_theta"], r32["grad_z"], r32["grad_theta"])
    family = "phi_gemm" if M >= 256 else ("phi_update_joint" if joint else "phi_update")   # (step_update: the GEMM from 256 particles)
    ok = [_report(b, f"K entry-wise / bound ({e['kmat_entries']})", e["kmat_over_bound"], 1.0, y["kmat_over_bound"]),
          _report(b, "K max-norm", e["kmat_maxnorm"], KXX_MAXNORM, y["kmat_maxnorm"]), e["kmat_tiny_ok"]]
    for s in segs:
        ok.append(_report(b, f"phi_{s} isolated ({family})", e["phi_" + s], min(ISOLATED, ISOLATED_FAMILY[family]), y["phi_" + s]))
        print(f"transform | {b['id']:36s} phi_{s} isolated p99       f32-oracle {y['phi_' + s + '_p99']:.2e}  {'':14s}  device {e['phi_' + s + '_p99']:.2e}")
    for name in END_TO_END:
        if name in dev:
            want = ref[ORACLE_NAME[name]]
            ok.append(_report(b, name + " end to end", rel_err(dev[name], want), END_TO_END[name], rel_err(r32[ORACLE_NAME[name]], want)))
    assert e["kmat_tiny_ok"], "a kernel-matrix entry below 1e-30 scale is negative or more than twice the reference"
    assert all(ok), "beyond a bound (see the lines printed above)"
    assert (g["key"] == nxt["key"]).all()
    for s in segs:
        u = update_check(cfg, before[s], before["v_" + s], dev["PHI_" + s.upper()], ref["phi_" + s], g[s], nxt[s])
        print(f"transform | {b['id']:36s} {s} update {u}")
        assert_update_parity(u, 0.5 * ts.SIGNAL_SHARE[s], f"{b['id']} {s}")
        if cfg.optimizer == 1:
            assert rel_err(g["v_" + s], nxt["v_" + s]) < 2e-4, s   # (v = 0.9 v + 0.1 phi^2 with phi to 1e-4: test_gpu_max_size.py's floor)


# ---- the multi-run engines: run c of ONE engine against the standalone engine on the same state, bit for bit --------------------------------
STATE = ("z", "v_z", "theta", "v_theta", "baseline")


def _assert_run_equal(many, phis, c, M, one, phi_one):
    sl = slice(c * M, (c + 1) * M)
    for k in STATE:
        if one[k] is not None:
            assert np.isfinite(one[k]).all() and np.array_equal(many[k][sl], one[k]), (c, k)
    assert np.array_equal(many["key"][c], one["key"]), c
    for name, a in phi_one.items():
        assert np.array_equal(phis[name].reshape(len(many["z"]), -1)[sl], a.reshape(M, -1)), (c, name)


def _multi(cases, oracle, monkeypatch, hp_fields, setter, **cfg_multi):
    from dibs_amd.engine import Engine
    bs = [ts.build(c, oracle) for c in cases]
    M, t, names = bs[0]["M"], bs[0]["t"], ("PHI_Z",) + (("PHI_THETA",) if bs[0]["theta"] is not None else ())
    assert all(b["t"] == t and b["M"] == M for b in bs)
    assert all({k: v for k, v in b["cfg_kw"].items() if k not in hp_fields} == {k: v for k, v in bs[0]["cfg_kw"].items() if k not in hp_fields}
               for b in bs), "the runs may differ in per-run fields only"
    hps = [{k: b["cfg_kw"][k] for k in hp_fields if k in b["cfg_kw"]} for b in bs]
    assert hps[0] != hps[1]
    e = Engine(make_config(**dict({k: v for k, v in bs[0]["cfg_kw"].items() if k not in hp_fields}, **cfg_multi)))
    try:
        for c, b in enumerate(bs):
            e.set_data_problem(c, b["x"], b["mask"])
            getattr(e, setter)(c, **hps[c])
        sts = [ts.fresh_state(b) for b in bs]
        if cfg_multi.get("n_chains"):
            e.init_particles_batch(np.stack([b["key"] for b in bs]))   # (a chains engine is initialised before it is given a state)
        e.set_state(**{k: np.concatenate([s[k] for s in sts]) for k in STATE if sts[0][k] is not None})
        e.set_keys(np.stack([b["key"] for b in bs]))
        e.run(t, 1)
        many, phis = e.get_state(), {n: e.read(n) for n in names}
    finally:
        e.close()
    for c, b in enumerate(bs):
        eng = _engine(b, monkeypatch)
        try:
            eng.run(t, 1)
            one, phi_one = eng.get_state(), {n: eng.read(n) for n in names}
        finally:
            eng.close()
        _assert_run_equal(many, phis, c, M, one, phi_one)
    assert not np.array_equal(phis["PHI_Z"].reshape(2 * M, -1)[:M], phis["PHI_Z"].reshape(2 * M, -1)[M:])


def test_batched_engine_with_two_bandwidths(c_oracle64, monkeypatch):
    """k_phi_update<.., BATCH> and k_kmat_batch with dense kernel matrices: two problems of 33 particles with h_latent = 5 / ~35."""
    _multi(ts.BATCH_CASES, c_oracle64, monkeypatch, ("h_latent", "latent_prior_std"), "set_problem_hparams", n_problems=2)


def test_chains_engine_with_per_chain_bandwidths(c_oracle64, monkeypatch):
    """k_kmat_chains_hp and k_phi_update's JOINT + BATCH instantiation: two chains with (h_latent, h_theta) = (5, 500) / (~25, ~150)."""
    _multi(ts.CHAIN_CASES, c_oracle64, monkeypatch, ("h_latent", "h_theta"), "set_chain_hparams", n_chains=2)


def test_f64_engine_with_interacting_particles(c_oracle64, monkeypatch):
    """k64_kmat / k64_phi on a dense kernel matrix against the float64 oracle, at the 1e-9 of tests/test_gpu_f64.py."""
    b = ts.build(ts.F64_CASE, c_oracle64)
    _, ref, nxt = ts.oracle_step(c_oracle64, b)
    eng = _engine(b, monkeypatch, precision=64)
    try:
        assert eng.precision == 64
        eng.run(b["t"], 1)
        g = eng.get_state()
        errs = dict(KXX=rel_err(eng.read("KXX"), ref["kxx"]), GRAD_Z=rel_err(eng.read("GRAD_Z"), ref["grad_z"]),
                    PHI_Z=rel_err(eng.read("PHI_Z"), ref["phi_z"]), Z=rel_err(g["z"], nxt["z"]), V_Z=rel_err(g["v_z"], nxt["v_z"]))
    finally:
        eng.close()
    ok = [_report(b, k + " (float64 engine)", v, 1e-9) for k, v in errs.items()]
    assert all(ok) and (g["key"] == nxt["key"]).all()
