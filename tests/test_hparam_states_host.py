"""The hyper-parameter table of tests/hparam_states.py on the CPU: conditions on the CASES, chosen so that they hold.

  coverage      every draw loop that branches on tau == 1 and every tau alpha g (1 - g) epilogue is reached by a row's restated dispatch,
                and every row reaches the kernel it names;
  non-vacuity   for every case and every parameter it moves off its default, the reference with that ONE parameter put back differs
                from the case's own reference by at least 20 x the GPU test's bound in the stage hparam_states.SHOWS_IN names -- a
                kernel that ignored the parameter could not pass;
  the reference alone stays within the bounds: the float32 build of the C oracle is within HALF of every bound that
                tests/test_gpu_hparams.py applies, on every case it is the reference of (the soft-graph BGe cases have the
                torch-autograd oracle, float64 only, as reference: their yardstick is tests/test_soft_states_host.py's);
  tiny          the committed PRNG keys of the logistic_minval_tiny cases really produce a draw without a set bit on the stated
                off-diagonal element (re-derived with oracle/prng.py), and the two settings differ there by 20 bounds or more."""
import numpy as np
import pytest

import hparam_states as H
import obs_axis as A
import soft_states as SS
from conftest import UPDATE_TOL, rel_err, update_check
from dibs_amd._abi import make_config

IDS = [H.case_id(c) for c in H.ALL_CASES]


def test_case_ids_are_unique_and_shapes_small():
    assert len(set(IDS)) == len(IDS)
    for c in H.ALL_CASES:
        assert c["M"] <= 2 and 2 <= c["S"] <= 4 and 2 <= c["Sa"] <= 4 and c["N"] <= max(3 * c["d"], 129), H.case_id(c)
        if c["d"] >= 113:
            assert c["M"] <= 2 and c["S"] == 2 and c["Sa"] == 2
        assert c["tau"] in H.TAUS


def test_every_row_reaches_the_kernel_it_names():
    for c in H.ACYC_CASES:
        assert c["kernel"] == H.acyc_family(H.acyc_kernel(c["d"], c["Sa"], c["layout"], c["hfw_max"])) and c["kernel"] in H.reaches(c), H.case_id(c)
    # the table of the acyclicity kernels, size by size (tu_acyc.hip)
    k = lambda d, Sa=4, **kw: H.acyc_kernel(d, Sa, **kw)
    assert [k(d) for d in (5, 16)] == ["k_acyc<1,true>"] * 2 and [k(d) for d in (20, 32)] == ["k_acyc<2,true>"] * 2
    assert k(20, 3) == k(20, 4, layout="partitionable") == "k_acyc<2,false>"
    assert [k(d) for d in (33, 48, 49, 64)] == ["k_acyc_hf<false,3>"] * 2 + ["k_acyc_hf<true,3>"] * 2
    assert [k(d) for d in (65, 80, 81, 96, 112)] == ["k_acyc_hfw<5>", "k_acyc_hfw<5>", "k_acyc_hfw<6>", "k_acyc_hfw<6>", "k_acyc_hfw<7>"]
    # k_acyc_bfw is no default at any size: acyc_hfw_max = 112 (tuning.h); the rows that reach it lower it to 80
    assert not any(k(d).startswith("k_acyc_bfw") for d in range(1, 200))
    assert [k(d, hfw_max=80) for d in (80, 81, 96, 112)] == ["k_acyc_hfw<5>", "k_acyc_bfw<6>", "k_acyc_bfw<6>", "k_acyc_bfw<7>"]
    assert k(113, 2) == k(130, 2) == "k_acycb" and k(50, 3) == "k_acyc<4,false>"
    for c in H.SOFT_CASES:
        assert c["kernel"] == SS.soft_path(c["d"], c["interv"])["kernel"]
    assert {SS.soft_path(c["d"], c["interv"])["name"].split(",")[0] for c in H.SOFT_CASES} >= {"k_bge_soft_mf<2", "k_bge_soft_mf<4", "k_bge_soft<false", "k_bge_soft<true"}
    assert any(SS.soft_path(c["d"], c["interv"])["GLOB"] for c in H.SOFT_CASES)
    assert {c["kernel"] for c in H.LIN_CASES} == {"pair<1,4>", "hf<5,true>", "unpaired<1>", "unpaired<2>", "gram"}
    for c in H.LIN_CASES:
        assert c["kernel"] == A.lin_kernel(c["d"], c["N"], c["S"], c["layout"])
    assert {(c["kernel"], c["est"]) for c in H.NN_CASES} == {(k_, e) for k_ in ("f32x4", "image", "hx7", "general") for e in ("reparam", "score")}
    assert not A.joint_nn_fast_path(8, 129, 5) and A.joint_nn_fast_path(20, 40, 5)


def test_every_tau_path_is_reached():
    got = set().union(*[H.reaches(c) for c in H.ALL_CASES])
    assert got >= H.REQUIRED, H.REQUIRED - got
    # both tau values on every acyclicity family, and with interventions as without on the BGe prior
    for fam in ("k_acyc", "k_acyc_hf", "k_acyc_hfw", "k_acyc_bfw", "k_acycb"):
        assert {c["tau"] for c in H.ACYC_CASES if c["kernel"] == fam} == set(H.TAUS), fam
    assert {(c["d"], c["interv"]) for c in H.BGE_CASES if c["group"] == "bge"} == {(d, i) for d in H.SCORE_D for i in (False, True)}
    for c in H.ALL_CASES:    # every case is off EVERY default of its family
        m = H.moved(c)
        assert all(k_ in H.DEFAULTS and (H.DEFAULTS[k_] is None or m[k_] != H.DEFAULTS[k_]) for k_ in m), H.case_id(c)


def _update(cfg, before, ref_dbg, ref_after, dbg, after, seg):
    return update_check(cfg, before[seg], before["v_" + seg], dbg["phi_" + seg], ref_dbg["phi_" + seg], after[seg], ref_after[seg])


@pytest.mark.parametrize("case", H.ORACLE_CASES, ids=[H.case_id(c) for c in H.ORACLE_CASES])
def test_f32_oracle_within_half_of_every_bound(c_oracle64, c_oracle32, case):
    b = H.built_case(case, c_oracle64)
    before, dbg, after = H.c_step(c_oracle32, case)
    assert np.array_equal(before["z"].astype(np.float64), b["before"]["z"])
    assert (after["key"] == b["after"]["key"]).all() and np.array_equal(dbg["g_samples"], b["dbg"]["g_samples"])
    errs = H.stage_errors(case, dbg, b["dbg"])
    print(f"\n  hparams f32 oracle {b['id']}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    assert all(np.isfinite(v).all() for k_, v in b["dbg"].items() if k_ != "g_samples")
    for s, e in errs.items():
        assert e <= 0.5 * H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    if H.phi_overflows(b["dbg"]):
        assert case["d"] >= 128
        return
    cfg = make_config(**b["cfg_kw"])
    for seg in ("z", "theta") if case["model"] != "bge" else ("z",):
        u = _update(cfg, b["before"], b["dbg"], b["after"], dbg, after, seg)
        print(f"  update {seg}: {u}")
        assert u["signal"] <= 0.5 * UPDATE_TOL["signal"] and u["all_p95"] <= 0.5 * UPDATE_TOL["all_p95"], (seg, u)
        assert u["signal_count"] >= min(UPDATE_TOL["signal_count"], u["n"])
        assert u["all"] < UPDATE_TOL["signal"] or u["signal_share"] >= 2 * H.MIN_SHARE[seg], (seg, u)


@pytest.mark.parametrize("case", H.ORACLE_CASES, ids=[H.case_id(c) for c in H.ORACLE_CASES])
def test_every_moved_parameter_shows(c_oracle64, case):
    b = H.built_case(case, c_oracle64)
    bd = H.bounds(case)
    for p in H.moved(case):
        _, dbg, _ = H.c_step(c_oracle64, case, **{p: H.DEFAULTS[p]})
        s = H.SHOWS_IN[p]
        diff = H.rel(dbg[H.STAGE_KEYS[s]], b["dbg"][H.STAGE_KEYS[s]])
        print(f"  hparams non-vacuity {b['id']}: {p} -> default moves {s} by {diff:.1e} (bound {bd[s]:.0e})")
        assert diff >= 20 * bd[s], (b["id"], p, s, diff, bd[s])
        if p == "tau" and case["est"] == "reparam":
            # the row names a LIKELIHOOD kernel's general draw loop / tau alpha epilogue: tau must show in a stage of that kernel too
            lik = {s_: H.rel(dbg[H.STAGE_KEYS[s_]], b["dbg"][H.STAGE_KEYS[s_]]) / bd[s_] for s_ in H.TAU_LIK_STAGES}
            print(f"  hparams non-vacuity {b['id']}: tau -> default moves " + ", ".join(f"{s_} by {v:.0f} bounds" for s_, v in lik.items()))
            assert max(lik.values()) >= 20, (b["id"], lik)


def test_the_soft_graph_rows_need_the_likelihood_gradient_on_its_own():
    """why W_LIK is compared in the soft-graph BGe rows: the likelihood's share of GRAD_Z in the max-norm is below the GRAD_Z bound from 49
    variables on, so GRAD_Z and PHI_Z there say nothing about k_bge_soft* / k_soft_combine; and W_LIK is no empty stage"""
    for c in H.SOFT_CASES:
        ref = H.built_soft_case(c)["ref"]
        share = np.abs(ref["dz_lik"]).max() / np.abs(ref["grad_z"]).max()
        print(f"  hparams soft {H.case_id(c)}: max|dz_lik| / max|grad_z| = {share:.1e}, max|W_LIK| = {np.abs(ref['w_lik']).max():.2e}")
        assert share < H.bounds(c)["GRAD_Z"] or c["d"] < 49
        assert np.isfinite(ref["w_lik"]).all() and np.abs(ref["w_lik"]).max() > 0
        assert H.bounds(c)["W_LIK"] == SS.W_LIK_MAXNORM


@pytest.mark.parametrize("case", H.SOFT_CASES, ids=[H.case_id(c) for c in H.SOFT_CASES])
def test_every_moved_parameter_shows_in_the_soft_graph_cases(case):
    """W_LIK with the weights held at the case's own (soft_w_lik of the re-run's per-sample terms): what must move is the per-sample
    gradient of k_bge_soft*, not only the softmax of the log-probabilities"""
    b = H.built_soft_case(case)
    ref = b["ref"]
    assert np.isfinite(ref["logprobs_z"]).all() and np.isfinite(ref["phi_z"]).all()
    assert set(H.moved(case)) == set(H.SOFT_SHOWS_IN)
    for p in H.moved(case):
        r = H.autograd_step(case, **{p: H.DEFAULTS[p]})
        r = dict(r, w_lik=H.soft_w_lik(r["lik_terms"], ref["logprobs_z"]))
        for s in H.SOFT_SHOWS_IN[p]:
            bound, diff = H.bounds(case)[s], H.rel(r[H.STAGE_KEYS[s]], ref[H.STAGE_KEYS[s]])
            print(f"  hparams non-vacuity {b['id']}: {p} -> default moves {s} by {diff:.1e} (bound {bound:.0e})")
            assert diff >= 20 * bound, (b["id"], p, s, diff, bound)


@pytest.mark.parametrize("d,n_ho", H.LIN_SCORE_CASES)
def test_held_out_scorer_inputs_show_every_edge_prior_parameter(c_oracle64, c_oracle32, d, n_ho):
    kw, x, mask, gs, th = H.lin_score_inputs(d, n_ho)
    assert gs[1].sum() == d * (d - 1) // 2 and not gs[0].any()
    th = th.reshape(5, -1).astype(np.float64)
    ref = c_oracle64.score_graphs(make_config(**kw), x, mask, gs, th)
    assert np.isfinite(ref).all() and rel_err(c_oracle32.score_graphs(make_config(**kw), x, mask, gs, th), ref) <= 0.5 * H.LIN_SCORE_BOUND
    for p in H.LIN:
        diff = rel_err(c_oracle64.score_graphs(make_config(**dict(kw, **{p: H.DEFAULTS[p]})), x, mask, gs, th), ref)
        print(f"  hparams non-vacuity score_graphs lingauss d={d} n_ho={n_ho}: {p} -> default moves the scores by {diff:.1e}")
        assert diff >= 20 * H.LIN_SCORE_BOUND, (p, diff)


@pytest.mark.parametrize("interv", (False, True))
@pytest.mark.parametrize("d", H.SCORE_D)
def test_bge_scorer_inputs_show_every_prior_parameter(c_oracle64, c_oracle32, d, interv):
    case, kw, mean_obs, x, mask, gs = H.bge_score_inputs(d, interv)
    assert gs[1].sum() == d * (d - 1) // 2 and not gs[0].any()      # a complete DAG and the empty graph
    bound = H.bounds(case)["LOGPROBS_Z"]
    ref = c_oracle64.score_graphs(make_config(**kw), x, mask, gs, mean_obs=mean_obs)
    assert np.isfinite(ref).all() and rel_err(c_oracle32.score_graphs(make_config(**kw), x, mask, gs, mean_obs=mean_obs), ref) <= 0.5 * bound
    for p in ("bge_alpha_mu", "bge_alpha_lambd", "mean_obs"):
        kw2, mo2 = H.config_kwargs(case, **{p: H.DEFAULTS[p]})
        diff = rel_err(c_oracle64.score_graphs(make_config(**kw2), x, mask, gs, mean_obs=mo2), ref)
        print(f"  hparams non-vacuity score_graphs bge d={d}: {p} -> default moves the scores by {diff:.1e} (bound {bound:.0e})")
        assert diff >= 20 * bound, (p, diff)


# ---- logistic_minval_tiny ----------------------------------------------------------------------------------------------------------------
def test_committed_keys_give_the_zero_bits_draw_on_the_stated_element(c_oracle64):
    for name in H.TINY_FAMILIES:
        c = H.tiny_case(name, False)
        n, hit = H.TINY_HITS[name]
        assert hit in H.zero_bit_draws(c, (H.TINY_K0, n)) and hit[2] != hit[3], name
        assert hit[0] < c["M"] and hit[1] < (c["S"] if c["draws"] == "lik" else c["Sa"])
        assert H.find_tiny_key(name, n + 1) == (n, hit), name            # the FIRST key of the search, as committed
        st = H.tiny_state(c, c_oracle64)
        m, _, i, j = hit
        assert 2.0 * st["z"][m, j, i, 1] == H.TINY_A and np.abs(2.0 * st["z"][..., 1]).max() == H.TINY_A
        assert np.array_equal(st["z"][..., 0], np.broadcast_to(np.eye(c["d"]), st["z"].shape[:-1]))
    # every family reaches its kernel by the restated dispatch
    k = {n: H.tiny_case(n, False) for n in H.TINY_FAMILIES}
    assert [H.acyc_kernel(k[n]["d"], k[n]["Sa"], hfw_max=k[n]["hfw_max"]) for n in ("k_acyc", "k_acyc_hf", "k_acyc_hfw", "k_acyc_bfw")] == \
        ["k_acyc<2,true>", "k_acyc_hf<true,3>", "k_acyc_hfw<5>", "k_acyc_bfw<6>"]
    c = k["k_lin_logprobs_hf"]
    assert A.lin_kernel(c["d"], c["N"], c["S"]).startswith("hf<") and "k_lin_logprobs_hf" in H.reaches(c)
    c = k["kernels_nn_f16"]
    assert A.nn_logprob_kernel(c["d"], c["N"], 5, c["S"], True) == "image" and "kernels_nn_f16.h" in H.reaches(c)
    assert SS.soft_path(k["k_bge_soft_mf"]["d"], False)["kernel"] == "k_bge_soft_mf"


@pytest.mark.parametrize("name", list(H.TINY_FAMILIES))
def test_the_two_settings_differ_at_the_hit(c_oracle64, name):
    vals = {}
    for tiny in (False, True):
        c = H.tiny_case(name, tiny)
        b = H.built_tiny_case(c, c_oracle64)
        stage, v = H.tiny_hit_value(c, b["dbg"])
        vals[tiny] = v
        top, bound = np.abs(b["dbg"][H.STAGE_KEYS[stage]]).max(), H.bounds(c)[stage]
    diff = abs(vals[False] - vals[True]) / top
    print(f"  hparams tiny {name}: {stage} at the hit {vals[False]:.6g} | {vals[True]:.6g}: {diff / bound:.0f} bounds apart")
    assert diff >= 20 * bound, (name, stage, vals, bound)


@pytest.mark.parametrize("case", [c for c in H.TINY_CASES if not H.is_soft(c)], ids=[H.case_id(c) for c in H.TINY_CASES if not H.is_soft(c)])
def test_f32_oracle_within_half_of_every_bound_on_the_tiny_cases(c_oracle64, c_oracle32, case):
    b = H.built_tiny_case(case, c_oracle64)
    before, dbg, after = H.tiny_step(c_oracle32, case)
    assert (after["key"] == b["after"]["key"]).all()
    errs = H.stage_errors(case, dbg, b["dbg"])
    print(f"\n  hparams f32 oracle {b['id']}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    for s, e in errs.items():
        assert e <= 0.5 * H.bounds(case)[s], (b["id"], s, e, H.bounds(case)[s])
    cfg = make_config(**b["cfg_kw"])
    for seg in ("z", "theta") if case["model"] != "bge" else ("z",):
        u = _update(cfg, b["before"], b["dbg"], b["after"], dbg, after, seg)
        assert u["signal"] <= 0.5 * UPDATE_TOL["signal"] and u["all_p95"] <= 0.5 * UPDATE_TOL["all_p95"], (seg, u)
        assert u["all"] < UPDATE_TOL["signal"] or u["signal_share"] >= 2 * H.MIN_SHARE[seg], (seg, u)
