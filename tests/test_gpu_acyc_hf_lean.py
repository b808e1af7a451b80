"""k_acyc_hf (kernels_acyc_f16.h, 33 <= d <= 64) pinned bit for bit: the instruction-count pass over its draw loop, hand-over, first
fragments, maximum tree, epilogue and chain copy may not move a single bit of W_ACYC.

tests/golden/acyc_hf_parent_digests.json holds the SHA-256 of eng.read("W_ACYC") recorded on an MI355X at the commit BEFORE that pass
(`python tests/test_gpu_acyc_hf_lean.py OUT.json` is the recorder), for every case and both steps.  Each case takes a path the pass touches:

   d  Sa  M
  33   2  2   odd row stride, 4.25 draw iterations, squarings only
  34   4  2
  48   2  2   d^2 = 9 x 256 exactly (no partial draw iteration), FOUR = false, fourth wave idle
  49   4  2   first FOUR = true size, odd d, exponent 48 ends on a squaring
  50   2  3   headline size, Mloc not a multiple of 8, exponent ends on a multiply
  63   2  2
  64   4  2   d^2 = 16 x 256, a multiply after every squaring, no pad columns

Harness of test_acyclicity_kernel_sizes_33_to_64 (S = 4, one step at t = 1 and one at t = 6).  The state of both steps is built from the
seeded initial particles alone (t = 6: latents scaled by 5/4, the key the engine carried out of the first step), so that the digests depend
on nothing but integer PRNG arithmetic, the edge-score kernel and k_acyc_hf / k_acyc_reduce.  No tolerance: the 1e-5 comparisons with the
oracle in test_gpu_parity.py keep guarding the arithmetic itself."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import make_data  # noqa: E402
from dibs_amd._abi import make_config  # noqa: E402
from oracle import prng  # noqa: E402

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acyc_hf_parent_digests.json")
CASES = [(33, 2, 2), (34, 4, 2), (48, 2, 2), (49, 4, 2), (50, 2, 3), (63, 2, 2), (64, 4, 2)]
STEPS = (1, 6)


def _oracle():
    from oracle.c_oracle import COracle
    return COracle("f64")


def _w_acyc(co, d, Sa, M):
    """W_ACYC after one step at t = 1 and one at t = 6, as float32 arrays"""
    from dibs_amd.engine import Engine
    data, _, _ = make_data(d, seed=2)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=4, n_acyclicity_mc_samples=Sa)
    st = co.new_state(cfg, prng.PRNGKey(5))
    z0 = st["z"].astype(np.float32)
    zero_v, zero_b = np.zeros_like(st["v_z"]), np.zeros_like(st["baseline"])
    eng = Engine(cfg)
    eng.set_data(data.x, None)
    out = []
    key = st["key"]
    for t in STEPS:
        z = z0 if t == STEPS[0] else (z0 * np.float32(1.25)).astype(np.float32)
        eng.set_state(z=z.astype(np.float64), v_z=zero_v, key=key, baseline=zero_b)
        eng.run(t, 1)
        out.append(np.ascontiguousarray(eng.read("W_ACYC")).copy())
        key = eng.get_state()["key"]
    eng.close()
    return out


def _digest(w):
    return hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest()


def _case_id(d, Sa, M, t):
    return f"d{d}_Sa{Sa}_M{M}_t{t}"


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


@pytest.mark.parametrize("d,Sa,M", CASES)
def test_acyc_hf_bits_equal_parent(c_oracle64, recorded, d, Sa, M):
    for t, w in zip(STEPS, _w_acyc(c_oracle64, d, Sa, M)):
        assert w.dtype == np.float32 and w.size == M * d * d
        assert np.isfinite(w).all() and w.any(), "vacuous: no acyclicity gradient at all"
        got = _digest(w)
        print(f"{_case_id(d, Sa, M, t)}: {got}")
        assert got == recorded[_case_id(d, Sa, M, t)], f"W_ACYC of d = {d}, Sa = {Sa}, M = {M}, t = {t} differs from the parent's bits"


def test_acyc_hf_saturated_soft_graphs_give_exact_zero(c_oracle64):
    """d = 50 set up as test_acyclicity_gradient_of_saturated_soft_graphs_is_zero: every edge saturated, g = u / den with den == u must
    be exactly 1 (the select of the draw loop; max(u, ulo) formed by v_max_f32), so W_ACYC is exactly zero"""
    from dibs_amd.engine import Engine
    d, M, Sa = 50, 2, 4
    data, _, _ = make_data(d, seed=1)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=4, n_acyclicity_mc_samples=Sa, n_dim=1)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(3))
    z = np.sign(st["z"]) * (6.0 + np.abs(st["z"]))
    z = z.astype(np.float32).astype(np.float64)
    assert np.abs(z).min() >= 6.0   # |score| = |u_i v_j| >= 36, alpha |s| >= 720 at t = 20
    eng = Engine(cfg)
    eng.set_data(data.x, None)
    eng.set_state(z=z, v_z=np.zeros_like(st["v_z"]), key=st["key"], baseline=np.zeros_like(st["baseline"]))
    eng.run(20, 1)
    w = eng.read("W_ACYC")
    eng.close()
    assert w.size == M * d * d and not w.any(), "saturated soft graphs must have an exactly zero acyclicity gradient"


@pytest.mark.parametrize("d,Sa", [(33, 2), (50, 4)])
def test_acyc_hf_general_temperature_path_against_oracle(c_oracle64, d, Sa):
    """tau != 1 takes the kernel's general draw loop (logistic noise + sigmoid instead of u / (u + (1 - u) exp(-alpha s))), which shares
    the linear LDS layout and the hand-over with the fast one.  Same bound as test_acyclicity_kernel_sizes_33_to_64 (1e-5 of the largest
    entry: the float32 arithmetic of the stage against the float64 oracle)."""
    from dibs_amd.engine import Engine
    from conftest import rel_err
    M = 2
    data, _, _ = make_data(d, seed=2)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, n_grad_mc_samples=4, n_acyclicity_mc_samples=Sa, tau=0.7)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(5))
    for k in ("z", "v_z", "baseline"):
        st[k] = st[k].astype(np.float32).astype(np.float64)
    eng = Engine(cfg)
    eng.set_data(data.x, None)
    eng.set_state(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
    dbg = c_oracle64.step(cfg, data.x, None, st, 2, debug=True)
    eng.run(2, 1)
    w = eng.read("W_ACYC")
    eng.close()
    assert np.abs(np.asarray(dbg["w_acyc"])).max() > 0
    err = rel_err(w, dbg["w_acyc"])
    print(f"d={d} Sa={Sa} tau=0.7: W_ACYC rel err {err:.2e}")
    assert err < 1e-5


if __name__ == "__main__":   # recorder: python tests/test_gpu_acyc_hf_lean.py OUT.json
    co = _oracle()
    rec = {}
    for d, Sa, M in CASES:
        for t, w in zip(STEPS, _w_acyc(co, d, Sa, M)):
            assert np.isfinite(w).all() and w.any()
            rec[_case_id(d, Sa, M, t)] = _digest(w)
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
