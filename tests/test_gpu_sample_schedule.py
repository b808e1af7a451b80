"""k_bge_sample deals the Mloc * d columns (particle m, node j) to its waves from a flat index -- wave w of block b takes column
WAVES * b + w -- so a block may span two particles, only the last block can hold idle waves, and the kernel-matrix riders of a small
marginal run sit in a block range of their own behind the sampling blocks (dibs_amd/csrc/kernels_bge.h, K2).  The schedule is integer
only: the sampled parent sets either equal the oracle's bit for bit or the indexing is wrong.

Every case runs a few steps through the step-by-step entry points from a state shared with the float64 oracle.  The parent-set masks
must be array_equal to the oracle's sampled graphs; node scores and z keep the bounds of tests/test_gpu_parity.py (1e-4 of the largest
magnitude up to 50 variables, 5e-4 up to 112 for the node scores -- fp32 Cholesky pivots; 1e-4 on z).

Shapes: where the flat index can go wrong, not the workload's own.
  d = 5,  M = 3, S = 8    15 columns: no multiple of 4 or 8 -- the last block partly filled, blocks spanning two particles
  d = 7,  M = 5, S = 8    every block spans two particles
  d = 33, M = 2, S = 16   one bit in the second 32-bit half-word
  d = 65, M = 2, S = 16   two mask words
  d = 6,  M = 4, S = 7    odd S: the unpaired generic path
  batched, 2 problems x 3 particles, d = 5: the statistics row (problem) changes inside a block
  d = 20, M = 32          config 2's shape: the riders compute the latent kernel matrix (KXX against the oracle, 1e-5 as in the parity file)
"""
import numpy as np
import pytest

from conftest import make_data, rel_err
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine
from oracle import prng

pytestmark = pytest.mark.gpu


def _graphs_from_masks(masks, M, S, d):
    gm = masks.reshape(M, d, S, -1)  # [m][j][s][w]: bit i of word i // 64 = g[i, j]
    gg = np.zeros((M, S, d, d), np.uint8)
    for i in range(d):
        gg[:, :, i, :] = ((gm[:, :, :, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1)
    return gg


def _round_state(st):
    """the device holds float32: both sides start a step from the same representable state"""
    for k in ("z", "v_z", "baseline"):
        st[k] = st[k].astype(np.float32).astype(np.float64)


def _node_score_bound(d):
    return 1e-4 if d <= 50 else 5e-4


@pytest.mark.parametrize("d,M,S,Sa,steps", [
    (5, 3, 8, 4, (0, 1, 3)),
    (7, 5, 8, 4, (0, 1, 3)),
    (33, 2, 16, 4, (0, 2)),
    (65, 2, 16, 4, (0, 2)),
    (6, 4, 7, 3, (0, 1, 3)),
    (20, 32, 128, 8, (0, 2)),
])
def test_flat_column_index_matches_oracle(c_oracle64, d, M, S, Sa, steps):
    data, _, _ = make_data(d, seed=0, n_obs=100)
    cfg = make_config(n_vars=d, n_particles=M, n_observations=100, edges_per_node=1 if d <= 7 else 2, n_grad_mc_samples=S,
                      n_acyclicity_mc_samples=Sa)
    st = c_oracle64.new_state(cfg, prng.PRNGKey(1))
    eng = Engine(cfg)
    eng.set_data(data.x, None)
    try:
        for t in steps:
            _round_state(st)
            eng.set_state(z=st["z"], v_z=st["v_z"], key=st["key"], baseline=st["baseline"])
            dbg = c_oracle64.step(cfg, data.x, None, st, t, debug=True)
            eng.run(t, 1)
            g = eng.get_state()
            gg = _graphs_from_masks(eng.read("PARENT_MASKS"), M, S, d)
            assert np.array_equal(gg, dbg["g_samples"]), f"step {t}: sampled graphs must be bit-identical"
            assert (g["key"] == st["key"]).all()
            ns = eng.read("NODE_SCORES").reshape(M, d, S).transpose(0, 2, 1)  # device layout [m][j][s]
            e_ns, e_k, e_z = rel_err(ns, dbg["node_scores"]), rel_err(eng.read("KXX"), dbg["kxx"]), rel_err(g["z"], st["z"])
            print(f"d={d} M={M} S={S} t={t}: node scores {e_ns:.2e} kxx {e_k:.2e} z {e_z:.2e}")
            assert e_ns < _node_score_bound(d)
            assert e_k < 1e-5
            assert e_z < 1e-4
    finally:
        eng.close()


def test_flat_column_index_batched_engine(c_oracle64):
    """2 problems x 3 particles, d = 5: 30 columns, and the block of columns 12 .. 15 holds the last node of problem 0 and the first of
    problem 1 -- the statistics row is taken per wave.  Each problem against the oracle run on its own data and key."""
    d, M, S, Sa, B = 5, 3, 8, 4, 2
    xs = [np.asarray(make_data(d, seed=10 + p, n_obs=60 + 20 * p)[0].x, np.float32)[:60] for p in range(B)]
    keys = [prng.PRNGKey(3 + p) for p in range(B)]
    kw = dict(n_vars=d, n_particles=M, n_observations=60, edges_per_node=1, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa)
    cfg1 = make_config(**kw)
    sts = [c_oracle64.new_state(cfg1, k) for k in keys]
    eng = Engine(make_config(n_problems=B, **kw))
    try:
        for p in range(B):
            eng.set_data_problem(p, xs[p], None)
        eng.init_particles_batch(np.stack(keys))
        for t in (0, 1, 3):
            for st in sts:
                _round_state(st)
            eng.set_state(**{k: np.concatenate([st[k] for st in sts]) for k in ("z", "v_z", "baseline")})
            eng.set_keys(np.stack([st["key"] for st in sts]))
            dbgs = [c_oracle64.step(cfg1, xs[p], None, sts[p], t, debug=True) for p in range(B)]
            eng.run(t, 1)
            g = eng.get_state()
            gg = _graphs_from_masks(eng.read("PARENT_MASKS"), B * M, S, d)
            ns = eng.read("NODE_SCORES").reshape(B * M, d, S).transpose(0, 2, 1)
            for p in range(B):
                sl = slice(p * M, (p + 1) * M)
                assert np.array_equal(gg[sl], dbgs[p]["g_samples"]), f"step {t}, problem {p}: sampled graphs must be bit-identical"
                assert (g["key"][p] == sts[p]["key"]).all()
                e_ns, e_z = rel_err(ns[sl], dbgs[p]["node_scores"]), rel_err(g["z"][sl], sts[p]["z"])
                print(f"batched t={t} problem {p}: node scores {e_ns:.2e} z {e_z:.2e}")
                assert e_ns < _node_score_bound(d)
                assert e_z < 1e-4
    finally:
        eng.close()
