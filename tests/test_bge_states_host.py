"""Host tests (no GPU) of tests/bge_states.py: the constructed particle states reach every parent-set size and every (form, tier) cell of
the BGe factorisation kernels.  The f64 C oracle samples the graphs; its samples are bit-identical to the device's (asserted by the GPU
tests), so the coverage claimed in tests/test_gpu_bge_tiers.py is pinned here, where it runs without a GPU."""
import os
import re

import numpy as np
import pytest

import bge_states as bs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dibs_amd", "csrc")


def test_rows_and_tiers_restate_the_kernel_header():
    src = open(os.path.join(CSRC, "kernels_bge.h")).read()
    assert "inline int bge_rows(int l, int d) { return l + 1 <= d - l ? l + 1 : d - l; }" in src
    assert "inline int bge_tier(int n) { return n <= 32 ? (n + 3) / 4 - 1 : BGE_NQ - 1; }" in src
    assert int(re.search(r"#define BGE_NQ (\d+)", src).group(1)) == bs.BGE_NQ
    assert int(re.search(r"#define BGE_PS (\d+)", src).group(1)) == bs.BGE_PS
    assert "return (64 + 64 + 8) * 4;" in src   # bge_generic_wave_bytes
    assert "bge_chol_lds_bytes(d, true) > (size_t)150 * 1024" in open(os.path.join(CSRC, "tu_bge.hip")).read()
    d = 65
    l = np.arange(d)
    n = bs.bge_rows(l, d)
    assert n[0] == 1 and n[32] == 33 and n[33] == 32 and n[64] == 1 and n.max() == 33
    assert bs.bge_tier(np.array([1, 4, 5, 16, 17, 32, 33, 64])).tolist() == [0, 0, 1, 3, 4, 7, 8, 8]
    assert bs.tiers_present(65) == {"direct": list(range(9)), "complement": list(range(8))}   # tier 8 only as l = 32, direct
    assert bs.tiers_present(64) == {"direct": list(range(8)), "complement": list(range(8))}
    assert bs.tiers_present(20) == {"direct": [0, 1, 2], "complement": [0, 1, 2]}


def test_no_size_up_to_128_variables_reaches_the_lds_cut():
    """bge_launch_chol reads R / Q through the caches without interventions once bge_chol_lds_bytes(d, true) exceeds 150 KiB.  With the
    present layout no d <= 128 does (d = 128: 149 648 bytes), so k_bge_chol<false, true> runs only with per-node matrices; the GPU case
    that would cover the cut appears by itself should the layout grow."""
    assert bs.chol_lds_bytes(128, True) == 149648
    assert bs.lds_cut_size() is None


def test_state_layout():
    d, M = 12, 4
    z = bs.tier_sweep_state(d, M, np.random.default_rng(0))
    assert z.shape == (M, d, d, 2) and np.array_equal(z, z.astype(np.float32))
    scores = np.einsum("mik,mjk->mij", z[..., 0], z[..., 1])
    for m in range(M):
        c2 = np.float64(np.float32(np.sqrt(40.0 if m == 0 else 3.0))) ** 2
        assert np.allclose(np.abs(scores[m]), c2, rtol=0, atol=1e-12)
        assert (np.diagonal(scores[m]) < 0).all()
        assert ((scores[m] > 0).sum(axis=0) == (np.arange(d) + m * d // M) % d).tolist()


@pytest.mark.parametrize("d,M,S,interv", bs.SWEEP_SIZES)
def test_constructed_states_cover_every_tier(c_oracle64, d, M, S, interv):
    case = bs.sweep_case(d, M, S, interv=interv)
    ref = bs.oracle_step(c_oracle64, case)
    g = ref["g_samples"]
    assert g.shape == (M, S, d, d) and not g[:, :, np.arange(d), np.arange(d)].any()
    assert (g[0].sum(axis=1) == np.arange(d)).all(), "saturated particle: node j has exactly j parents in every sample"
    hist = bs.tier_histogram(g, d)
    assert hist["sizes"].sum() == M * S * d == hist["l0"] + hist["direct"].sum() + hist["complement"].sum()
    bs.assert_coverage(hist, d)
    assert np.isfinite(ref["node_scores"]).all()
    if interv:
        assert not ref["node_scores"][:, :, case["all_intervened"]].any()


def test_coverage_assertion_notices_a_fresh_state(c_oracle64):
    """graphs of freshly initialised particles (what every other step test scores) do not pass assert_coverage"""
    from dibs_amd._abi import make_config
    from oracle import prng
    d, M, S = 50, 4, 8
    case = bs.sweep_case(d, M, S)
    st = c_oracle64.new_state(make_config(**case["cfg_kw"]), prng.PRNGKey(1))
    ref = bs.oracle_step(c_oracle64, dict(case, z=st["z"], key=st["key"]))
    with pytest.raises(AssertionError):
        bs.assert_coverage(bs.tier_histogram(ref["g_samples"], d), d)
