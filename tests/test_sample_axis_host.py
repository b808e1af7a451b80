"""The sample-axis table of tests/sample_axis.py on the CPU: that its rows reach every branch `classify` can name and the kernel each row is
there for, that the grid of every acyclicity kernel is one block per unit wide, and that the REFERENCE of
tests/test_gpu_sample_axis.py holds on its own -- the float32 C oracle stays within HALF of every stage bound of the float64 one on every
row (the bounds do not ask float32 for the impossible at 1 000+ samples), the weighted sums really carry weight on the samples past a
loop's first pass, the unstaged rows really have more non-zero weights than parent sets fit LDS, and every single acyclicity chain moves
W_ACYC by 20 bounds or more.  The two refusals of dibs_engine_create that depend on S are read here too: the checks precede the first
device call."""
import hashlib

import numpy as np
import pytest

import hparam_states as H
import sample_axis as X
from dibs_amd._abi import make_config

IDS = [X.case_id(c) for c in X.ALL_CASES]
C_CASES = X.ORACLE_CASES + X.F64_CASES + [c for c in X.BITWISE_CASES if c["model"] == "bge"]     # rows the C oracle steps (soft BGe: autograd)


def _nnz(case, oracle64):
    if H.is_soft(case) or case["engine"] == "chains":
        return None
    return int(X.nnz_of(X.built_case(case, oracle64)["dbg"]).max())


def test_boundaries_of_the_restatement():
    # tail_nsplit: 8 up to 128 samples, then 7, 6, 5, 4 up to 256, 3 up to 341, 2 up to 512, 1 above; clamped by d
    edges = {128: 8, 129: 7, 146: 7, 147: 6, 170: 6, 171: 5, 204: 5, 205: 4, 256: 4, 257: 3, 341: 3, 342: 2, 512: 2, 513: 1, 4000: 1}
    assert {S: X.tail_nsplit(S, 8) for S in edges} == edges
    assert X.tail_nsplit(64, 5) == 5 and X.tail_nsplit(258, 5) == 3 and X.tail_nsplit(128, 9) == 8
    assert set(edges) - {4000} <= {c["S"] for c in X.BGE_CASES if c["d"] == 8 and c["layout"] == "legacy"}       # both sides of every change are rows
    # the largest S of the BGe score estimator at 8 variables: derived, about 3 360
    smax = X.bge_s_max(8)
    assert 3300 < smax < 3400 and smax % 2 == 0 and not X.bge_refused(8, smax) and X.bge_refused(8, smax + 2)
    assert any(c["S"] == smax for c in X.BGE_CASES)
    # FINDING.  No S reaches "a particle's sample weights do not fit in LDS".  The test of dibs_engine_create is tail_lds_bytes(d, 0, S, W,
    # score_lik, 0): without the score estimator (every joint model, soft-graph BGe) it does not depend on S at all, and with it k_bge_sample's
    # four per-wave areas (4 (8 W + 4) S bytes) are refused long before the block's 28 S.  That refusal is reachable through n_vars only.
    for d in (2, 8, 64, 65, 128, 129, 256):
        assert X.tail_lds_bytes(d, 0, 1, (d + 63) // 64, False, 0) == X.tail_lds_bytes(d, 0, 1 << 20, (d + 63) // 64, False, 0)
        S = 2
        while not X.bge_refused(d, S):
            S += 1
        assert not X.tail_refused(d, S, True), (d, S)
    # k_acyc_reduce: 16 units are one full group and an empty tail
    assert [X.reduce_trips(n) for n in (1, 16, 17, 32, 33)] == ["tail", "full", "full+tail", "two_full", "two_full+tail"]
    assert X.gram_gx(512, 2) == 512 and X.gram_gx(514, 2) == 512 and X.gram_gx(100, 2) == 100


def test_the_table_reaches_every_branch_and_every_row_its_kernel(c_oracle64):
    assert len(set(IDS)) == len(IDS) and len(X.ALL_CASES) <= X.MAX_CASES
    assert sorted(map(X.case_id, X.ORACLE_CASES + X.BITWISE_CASES + X.F64_CASES + X.SOFT_CASES)) == sorted(IDS)     # every row is run by one GPU test
    classes = {X.case_id(c): X.classify(c, _nnz(c, c_oracle64)) for c in X.ALL_CASES}
    # the case ids and the branches each reaches, as they stood while tests/sample_axis.py still restated engine_alloc's chains-per-block
    # search (which could only return 1): sha256 of repr(sorted((id, sorted(branches))))
    # (a failure prints the rows themselves: every id with the branches it reaches now)
    rows = sorted((cid, sorted(cl)) for cid, cl in classes.items())
    assert hashlib.sha256(repr(rows).encode()).hexdigest() == "64fb7919b35e807509885d8068255778afe042ced3960d210327e66cc2277500", rows
    seen = set().union(*classes.values())
    assert seen == X.BRANCHES, (sorted(X.BRANCHES - seen), sorted(seen - X.BRANCHES))
    for c in X.ALL_CASES:
        cl, cid = classes[X.case_id(c)], X.case_id(c)
        if c["d"] <= 112:       # one unit per block: the grid of every acyclicity kernel, and k_acyc_reduce's sum, is acyc_units wide
            units = X.acyc_units(c["d"], c["Sa"], c["layout"])
            assert {"reduce:" + X.reduce_trips(units), "acyc_grid>16" if units > 16 else "acyc_grid<=16"} <= cl, (cid, cl)
        if c["group"] == "Sa":
            k = "k_acyc" if c["kernel"] == "k_acyc_batch" else c["kernel"]
            assert "acyc:" + k in cl and (c["d"] > 112 or "acyc_grid>16" in cl), (cid, cl)
            assert c["d"] > 112 or cl & {"reduce:full+tail", "reduce:two_full", "reduce:two_full+tail"}, (cid, cl)
        elif c["kernel"] == "unstaged":
            assert "unstaged" in cl and X.stage_cap_of(c["d"], c["S"]) < c["S"], (cid, cl)
        elif c["kernel"] == "k_soft_combine":
            assert cl & {"soft_combine:1", "soft_combine:2"}, (cid, cl)
        elif c["kernel"] == "k_ling_logprobs glob":
            assert {"lingauss:gram", "gram_gx_clamped"} <= cl and c["S"] == X.gram_gx(c["S"], c["M"]) + 2, (cid, cl)
        elif c["kernel"] == "k_bge_sample even":
            assert cl & {"bge_sample:even:2", "bge_sample:even:3+"}, (cid, cl)
        elif c["model"] != "bge":
            assert cl & {"softmax_stats:2", "softmax_stats:3+"}, (cid, cl)
    # the three compilations of particle_grad_block: the wave softmax with its slots u >= 2 and the block-wide softmax, each
    for e in ("single", "batch", "edge"):
        forms = {f for c in X.ALL_CASES if c["engine"] == e and c["group"] == "S" and c["model"] == "bge" for f in classes[X.case_id(c)] if f.startswith("softmax:")}
        assert {"softmax:wave_u>=2", "softmax:block"} <= forms, (e, forms)
    # odd S on every softmax form; both estimators on both joint models; a ragged last block on both
    odd = {X.softmax_form(c["S"]) for c in X.BGE_CASES if c["S"] % 2}
    assert odd == {"wave_u<=1", "wave_u>=2", "block"}
    for model in ("lingauss", "densenn"):
        rows = [c for c in X.JOINT_CASES if c["model"] == model and c["engine"] == "single" and c["d"] == 8]
        assert {c["est"] for c in rows} == {"reparam", "score"} and any(c["S"] % 2 and c["S"] > 256 for c in rows)
        assert any("ragged_last_block" in classes[X.case_id(c)] for c in rows) and any("softmax_stats:3+" in classes[X.case_id(c)] for c in rows)
    # the S = S_max row reads its parent sets unstaged at 8 variables as well: its cap is a third of S and its weights are flat
    top = next(c for c in X.BGE_CASES if c["S"] == X.bge_s_max(8))
    assert "unstaged" in classes[X.case_id(top)] and "idx_second_trip" in classes[X.case_id(top)]


@pytest.mark.parametrize("case", C_CASES, ids=[X.case_id(c) for c in C_CASES])
def test_f32_oracle_within_half_of_every_bound(c_oracle64, c_oracle32, case):
    """The float32 C oracle from the same float32-representable state stays within HALF of every bound the device is held to (a row in
    X.WIDENED: above a quarter of the stage's bound and within the widened value).  The same step shows that the row is not vacuous."""
    b = X.built_case(case, c_oracle64)
    before32, dbg32, after32 = X.c_step(c_oracle32, case)
    assert np.array_equal(before32["z"].astype(np.float64), b["before"]["z"]) and (after32["key"] == b["after"]["key"]).all()
    if case["model"] == "bge":
        assert np.array_equal(dbg32["g_samples"], b["dbg"]["g_samples"])
    errs = X.stage_errors(case, dbg32, after32, b)
    w = X.weights(b["dbg"])
    print(f"\n  {b['id']} {sorted(X.classify(case, _nnz(case, c_oracle64)))}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()) + f" | nnz={X.nnz_of(b['dbg'])} wmax={w.max():.2f}")
    assert all(np.isfinite(np.asarray(v)).all() for v in b["dbg"].values() if v.dtype != np.uint8)
    widened = X.WIDENED.get(b["id"], {})
    for s, e in errs.items():
        base = X.BASELINE_BOUND if s == "baseline" else H.bounds(case)[s]
        if s in widened:
            assert base / 4 < e <= widened[s], (s, e, widened[s])
        else:
            assert e <= base / 2, (s, e, base)
    # ---- non-vacuity
    assert np.abs(b["dbg"]["w_lik"]).max() > 0 and np.abs(b["dbg"]["w_acyc"]).max() > 0
    assert X.weights_reach(case, b["dbg"]), [float(w[:, list(i)].max()) for i in X.weight_index_sets(case)]
    if case["est"] == "score":       # `baseline` after the step = 0.001 sm / S: every sample with the same weight
        assert np.abs(b["after"]["baseline"]).min() > 0
    if case["kernel"] == "unstaged":
        assert X.nnz_of(b["dbg"]).max() > X.stage_cap_of(case["d"], case["S"])
    if case["group"] == "S" and case["model"] == "bge" and case["d"] <= 12 and case["S"] > 1:
        # near-flat weights: the sum over the samples is no one-hot pick (in some particle a tenth of the samples carry 1e-3 / S or more)
        assert (w >= 1e-3 / case["S"]).sum(1).max() >= case["S"] // 10


@pytest.mark.parametrize("case", X.SOFT_CASES, ids=[X.case_id(c) for c in X.SOFT_CASES])
def test_soft_rows_carry_weight_past_the_first_stride(case):
    ref = H.built_soft_case(case)["ref"]
    assert np.isfinite(ref["w_lik"]).all() and np.abs(ref["w_lik"]).max() > 0
    assert X.weights_reach(case, ref), X.weights(ref)[:, 256:].max()


SA_CASES = [c for c in X.ACYC_CASES if c["engine"] == "single"]


@pytest.mark.parametrize("case", SA_CASES, ids=[X.case_id(c) for c in SA_CASES])
def test_leaving_out_any_one_chain_moves_w_acyc_by_twenty_bounds(c_oracle64, case):
    """k_acyc_reduce without its guarded tail, or a grid one unit short, drops chains from the sum (the scale stays 1 / Sa): each chain's
    own term is about 1 / Sa of W_ACYC against a bound of 1e-5.  The per-chain terms are numpy's; their mean is the oracle's W_ACYC."""
    b = X.built_case(case, c_oracle64)
    terms = X.acyc_chain_terms(case, b, c_oracle64)
    ref = np.asarray(b["dbg"]["w_acyc"], np.float64)
    assert H.rel(terms.mean(1), ref) < 1e-9
    moves = [H.rel((terms.sum(1) - terms[:, s]) / case["Sa"], ref) for s in range(case["Sa"])]
    print(f"\n  {b['id']}: leaving out one chain moves W_ACYC by {min(moves):.1e} .. {max(moves):.1e} (bound {H.bounds(case)['W_ACYC']:.0e})")
    assert min(moves) >= 20 * H.bounds(case)["W_ACYC"]


def test_the_refusals_that_depend_on_s():
    """dibs_engine_create validates the configuration before it touches the device: the messages are read without one"""
    from dibs_amd._lib import DibsHipError
    from dibs_amd.engine import Engine
    smax = X.bge_s_max(8)
    with pytest.raises(DibsHipError, match="BGe: n_grad_mc_samples too large"):
        Engine(make_config(n_vars=8, n_particles=2, n_observations=6, n_grad_mc_samples=smax + 2, n_acyclicity_mc_samples=2))
    # ("sample weights do not fit": no S reaches it, test_boundaries_of_the_restatement; tests/test_gpu_sample_axis.py runs S = smax one
    #  step right)
