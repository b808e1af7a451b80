"""The observation-axis table of tests/obs_axis.py on the CPU: that its cases visit every path and tile class of the restated path choice,
and that the REFERENCE of tests/test_gpu_obs_axis.py holds on its own -- the float32 C oracle stays within the stage bounds of the
float64 one on every case (so a failure on the device points at the kernel), and on the intervention edges the float64 C oracle and the
torch-autograd oracle, two implementations of an empty sum, agree to 1e-9."""
import numpy as np
import pytest
import torch

import obs_axis as A
from conftest import rel_err
from dibs_amd._abi import make_config
from oracle import dibs_oracle as O, prng

IDS = [A.case_id(c) for c in A.ALL_CASES]


def test_cut_is_the_last_size_on_the_lds_path():
    for d in (8, 20, 40, 50, 56, 64, 80, 100, 112):
        cut = A.lin_cut(d)
        assert A.joint_lin_fast_path(d, cut) and not A.joint_lin_fast_path(d, cut + 1) and cut % 16 == 0, d
        assert A.lin_lds_bytes(d, cut, (d + 15) // 16, True) <= 160 * 1024 - 2048 < A.lin_lds_bytes(d, cut + 1, (d + 15) // 16, True)
    # at 100 and 112 variables the cut lies below 128: observations 113 .. 128 run the Gram path although the paired kernels would take them
    assert A.lin_cut(100) == A.lin_cut(112) == 112
    assert A.lin_kernel(100, 113, 8) == A.lin_kernel(112, 128, 8) == "gram" and A.lin_paired(112, 128, 8)
    # k_nn_grad's LDS never ends the DenseNN fast path below 128 observations (no such case to add to the table)
    assert not any(A._nn_hcs_edge(d, H) for d in range(1, 113) for H in (1, 5, 8, 64))


def test_every_case_is_in_exactly_one_class_and_every_class_is_visited():
    assert len(set(IDS)) == len(IDS)
    classes = [A.classify(c) for c in A.ALL_CASES]       # (classify returns ONE tuple per case: nothing is left out, the skipped share is 0)
    assert all(cl is not None and len(cl) in (4, 6) for cl in classes) and len(classes) == len(A.ALL_CASES)
    lin = [cl for cl in classes if cl[0] == "lingauss"]
    assert {cl[1] for cl in lin} == set(A.LIN_KERNELS), {cl[1] for cl in lin} ^ set(A.LIN_KERNELS)
    # the paired window: one tile, a ragged and a full last tile, the eighth tile ragged and full -- for the f32 and for the f16 kernels
    for fam in ("pair<", "hf<"):
        seen = {cl[2:] for cl in lin if cl[1].startswith(fam)}
        assert {(1, "one"), (7, "full"), (8, "full")} <= seen and any(t == "ragged" for _, t in seen), (fam, seen)
    assert (8, "ragged") in {cl[2:] for cl in lin if cl[1] == "hf<5,false>"} and (8, "ragged") in {cl[2:] for cl in lin if cl[1] == "hf<8,true>"}
    # the unpaired kernel: first size above the paired window (9 tiles, ragged), the cut (full), and inside the paired window (odd S / layout)
    for d in (8, 20, 40, 64, 80):
        nt = (d + 15) // 16
        seen = {cl[2:] for cl in lin if cl[1] == f"unpaired<{nt}>"}
        assert {(8, "full"), (9, "ragged"), (A.lin_cut(d) // 16, "full")} <= seen, (d, seen)
    assert {cl[2] for cl in lin if cl[1] == "gram"} >= {8, A.lin_cut(20) // 16 + 1}
    nn = [cl for cl in classes if cl[0] == "densenn"]
    assert {cl[1:3] for cl in nn} == set(A.NN_KERNELS), {cl[1:3] for cl in nn} ^ set(A.NN_KERNELS)
    for k in ("f32x4", "image", "hx7"):
        assert {(1, "one"), (7, "full")} <= {cl[4:] for cl in nn if cl[1] == k}, k
    for k in ("f32x4", "image", "hx8"):   # the eighth tile: 113 ragged, 128 full (the 8-tile image of the register-operand kernels)
        assert {(8, "ragged"), (8, "full")} <= {cl[4:] for cl in nn if cl[1] == k}, k
    assert {cl[3] for cl in nn} == {"wide", "narrow"}
    # estimators and interventions both ways on every model
    for model in ("lingauss", "densenn"):
        cs = [c for c in A.ALL_CASES if c["model"] == model and not c["edge"]]
        assert {(c["est"], bool(c["interv"])) for c in cs} == {(e, i) for e in ("reparam", "score") for i in (False, True)}


def test_the_paired_classes_are_the_eight_that_are_instantiated():
    """NT = ceil(d / 16) and epq = ceil(d d / 256) are both functions of d: over every size of the LDS-resident path, with the f16 kernels
    and without them (lin_f32), a paired launch names one of eight (NT, EPQ) -- the ones lin_launch.h instantiates"""
    seen = {A.lin_kernel(d, N, S, lin_f32=f32) for d in range(1, 113) for N in (1, 16, 17, 64, 112, 113, 128) for S in (2, 8, 16)
            for f32 in (False, True)}
    assert {k for k in seen if k.startswith("pair<")} == set(A.LIN_PAIR_CLASSES), seen
    # the operand of a class covers every size of it: d d <= 256 EPQ (EPQ 0: no register-resident operand)
    for d in range(1, 65):
        k = A.lin_kernel(d, 16, 2, lin_f32=True)
        assert d * d <= 256 * int(k[k.index(",") + 1:-1]), (d, k)
    # without lin_f32 the f16 kernels take 33 <= d <= 64: the three f32 classes there are reached by DIBS_LIN_F32 only
    assert {A.lin_kernel(d, 16, 2) for d in range(33, 65)} == {"hf<5,false>", "hf<5,true>", "hf<8,true>"}
    assert {A.lin_kernel(d, 16, 2, lin_f32=True) for d in range(33, 65)} == {"pair<3,10>", "pair<4,10>", "pair<4,16>"}
    assert tuple(A.lin_kernel(c["d"], c["N"], c["S"], lin_f32=True) for c in A.LIN_F32_CASES) == A.LIN_F32_KERNELS
    assert [(c["d"] ** 2 + 255) // 256 for c in A.LIN_F32_CASES] == [7, 10, 11, 16] and all(c["S"] % 2 == 0 for c in A.LIN_F32_CASES)


def test_intervention_edge_masks():
    for c in A.EDGE_CASES:
        m = A.make_mask(c)
        N, d = c["N"], c["d"]
        if c["edge"] == "node_always":
            assert m[:, d // 2].all() and m.sum() == N
        elif c["edge"] == "row_always":
            assert m[N // 3].all() and m.sum() == d
        else:
            assert ((m == 0).sum(0) == 1).all() and (m == 0).sum() == d
    assert {A.lin_kernel(c["d"], c["N"], c["S"]) for c in A.EDGE_CASES if c["model"] == "lingauss"} == {"pair<2,4>", "gram"}


def _flat(th, Mp):
    return np.stack([np.concatenate([leaf.numpy().reshape(-1) for leaf in th[m]]) for m in range(Mp)])


@pytest.mark.parametrize("case", A.EDGE_CASES, ids=[A.case_id(c) for c in A.EDGE_CASES])
def test_intervention_edges_c_oracle_vs_autograd(c_oracle64, monkeypatch, case):
    # Both oracles must see the SAME float32 logistic noise: numpy's float32 log and the C library's logf differ by one ulp on 17 % of the
    # draws (measured on 100 000), which alone moves the soft-graph log-probabilities by 1.5e-9 -- with or without interventions.  The
    # autograd oracle takes the C port's draws here, so that what is compared is the arithmetic after them.
    lay = {"legacy": 0, "partitionable": 1}
    monkeypatch.setattr(prng, "logistic", lambda key, shape, layout="legacy": c_oracle64.logistic(key, int(np.prod(shape)), lay[layout]).reshape(shape))
    b = A.built_case(case, c_oracle64)
    kw = b["cfg_kw"]
    nnp = O.DenseNNParams(hidden_layers=tuple(kw.get("nn_hidden", (5,))), activation=kw.get("nn_activation", "relu"), bias=kw.get("nn_bias", True))
    ocfg = O.Config(joint=True, likelihood=case["model"], alpha_linear=0.05, grad_estimator_z=case["est"], prior=O.GraphPrior("er", 2),
                    n_grad_mc_samples=case["S"], n_acyclicity_mc_samples=A.SA, score_function_baseline=kw["score_function_baseline"], nn=nnp)
    st = O.init_state(ocfg, prng.PRNGKey(A.KEY), A.M, case["d"])
    assert np.array_equal(st.z.numpy(), b["before"]["z"]) and np.array_equal(_flat(st.theta, A.M), b["before"]["theta"])
    x, interv = torch.as_tensor(b["x"].astype(np.float64)), torch.as_tensor(b["mask"].astype(np.float64))
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (thousands of small float64 operations: see large_states.autograd_step)
    try:
        kth, _ = O.estimator_keys(ocfg, st.key, A.M)
        lp_th = np.stack([O.grad_theta_likelihood(ocfg, st.z[m], st.theta[m], A.T_STEP, kth[m], x, interv)[1]["logprobs"].numpy() for m in range(A.M)])
        st2, aux = O.svgd_step(ocfg, st, x, interv, A.T_STEP, return_aux=True)
    finally:
        torch.set_num_threads(n_threads)
    dbg = b["dbg"]
    assert np.isfinite(dbg["logprobs_th"]).all() and np.isfinite(dbg["grad_theta"]).all() and np.isfinite(dbg["grad_z"]).all()
    assert rel_err(dbg["logprobs_th"], lp_th) < 1e-9
    assert rel_err(dbg["logprobs_z"], np.stack([a["logprobs"].numpy() for a in aux["lik_aux"]])) < 1e-9
    assert rel_err(dbg["grad_theta"], _flat(aux["dtheta"], A.M)) < 1e-9
    assert rel_err(dbg["grad_z"], (aux["dz_lik"] + aux["dz_prior"]).numpy()) < 1e-9
    assert (b["after"]["key"] == st2.key).all()


@pytest.mark.parametrize("case", A.ALL_CASES, ids=IDS)
def test_f32_oracle_within_the_stage_bounds(c_oracle64, c_oracle32, case):
    """On every case the float32 C oracle, from the same float32-representable state, stays within the bounds the device is held to: the
    reference alone meets them.  Where it uses more than a quarter of one, tests/obs_axis.py must carry the case in WIDENED with a value
    that covers the measurement -- the only way a bound of the GPU test grows."""
    b = A.built_case(case, c_oracle64)
    st = A.start_state(c_oracle32, b["cfg_kw"])
    assert np.array_equal(st["z"].astype(np.float64), b["before"]["z"]) and np.array_equal(st["theta"].astype(np.float64), b["before"]["theta"])
    dbg = c_oracle32.step(make_config(**b["cfg_kw"]), b["x"], b["mask"], st, A.T_STEP, debug=True)
    errs, keys_equal = A.stage_errors(b, dbg, st)
    print(f"\n  {b['id']} {A.classify(case)}: " + " ".join(f"{s}={e:.1e}" for s, e in errs.items()))
    assert keys_equal
    assert all(np.isfinite(np.asarray(v)).all() for v in b["dbg"].values() if v.dtype != np.uint8)
    assert np.abs(b["dbg"]["grad_theta"]).max() > 0 and np.abs(b["dbg"]["w_lik"]).max() > 0   # (non-vacuous: there is a likelihood gradient)
    widened = A.WIDENED.get(b["id"], {})
    for s, e in errs.items():
        base = (A.BOUNDS_NN if case["model"] == "densenn" else A.BOUNDS)[s]
        if s in widened:
            assert base / 4 < e <= widened[s], (s, e, widened[s])
        else:
            assert e <= base / 4, (s, e, base)
