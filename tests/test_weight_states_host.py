"""The constructed weight profiles of tests/weight_states.py, on the float64 oracles alone (CPU): every case builds, every particle's
theta / Z estimator has the participation count asked of it with the samples below the cut and the underflowing ones beside it, no
weight sits where the LOGPROBS bound could move it across the cut, the free edges' gradients are no cancellations, and what the cut
drops is below 1e-6 of the sum.  tests/test_gpu_grad_weights.py relies on each of these."""
import time

import numpy as np
import pytest

import weight_states as W

ALL_CASES = list(W.GRAD_CASES) + [c for cs in W.CHAIN_CASES.values() for c in cs]


def _classes(b, name):
    return [W.classify(p["nnz"], b["S"], b["ns"]) for p in b["profile"][name]]


@pytest.mark.parametrize("case", ALL_CASES, ids=W.case_id)
def test_profiles(c_oracle64, case):
    t0 = time.perf_counter()
    b = W.build(case, c_oracle64)
    took = time.perf_counter() - t0
    S, ns = b["S"], b["ns"]
    print(f"\n{b['id']}: built in {took:.1f} s ({b['rounds']} rounds), margin {b['margin']:.1f}, max |log p| {np.abs(b['dbg']['logprobs_th']).max():.3g}")
    # (the first build of a case in this process; measured 0.1 .. 9 s, and 24 s for the two-particle d = 100 reparam case, whose five
    #  rounds each cost a float64 oracle step at that size: profiles/grad_weight_errors.txt)
    assert took < (60 if b["d"] >= 100 else 20), took
    assert b["margin"] >= W.MARGIN and b["margin"] >= np.exp(2 * 2e-5 * np.abs(b["dbg"]["logprobs_th"]).max())
    assert 5 <= len(b["edges"]) <= 7 and len({j for _, j in b["edges"]}) == len(b["edges"])   # free edges into distinct children
    assert all(b["g0"][i, j] == 0 and i < j for i, j in b["edges"])
    for name, targets in (("theta", b["t_th"]), ("z", b["t_z"])):
        cls = _classes(b, name)
        print(f"  {name:5s}", [(c_, p["nnz"], p["below"], p["zero"], p["near"]) for c_, p in zip(cls, b["profile"][name])])
        for m, (p, tgt) in enumerate(zip(b["profile"][name], targets)):
            if name == "z" and b["z_free"]:
                continue
            if b["t_th"][m] == "straddle":   # at least two weights in (CUT, 1.5 CUT] and two in [CUT / 1.5, CUT) in the theta estimator
                assert name == "z" or (p["above_close"] >= 2 and p["below_close"] >= 2), (name, m, p)
                assert p["nnz"] == S or (p["below"] >= 8 and p["zero"] >= 2), (name, m, p)
                continue
            if p["nnz"] < S:
                assert p["below"] >= 8 and p["zero"] >= 2, (name, m, p)
            if name == "theta" or b["z_margin"]:
                assert p["near"] == 0, (name, m, p)
                if tgt is not None:
                    assert cls[m] in ((tgt,) if isinstance(tgt, str) else tgt), (name, m, cls[m], tgt)


def test_every_kernel_sees_every_class(c_oracle64):
    """per kernel, over its cases: the theta estimator has every class and a straddle; the Z estimators have every class"""
    for kernel in ("k_lin_grad", "k_ling_grad", "k_nn_grad", "k_nng_grad"):
        th, z, straddle = set(), set(), 0
        for case in W.GRAD_CASES:
            if case["kernel"] == kernel:
                b = W.build(case, c_oracle64)
                straddle += sum(t == "straddle" for t in b["t_th"])
                th |= {c for c, t in zip(_classes(b, "theta"), b["t_th"]) if t != "straddle"}
                z |= {c for c, t, p in zip(_classes(b, "z"), b["t_th"], b["profile"]["z"]) if t != "straddle" and p["near"] == 0}
        print(kernel, sorted(th), sorted(z), straddle)
        assert th >= set(W.CLASSES) and z >= set(W.CLASSES) and straddle >= 1, (kernel, th, z, straddle)
    # the chains: chain 0 one sample everywhere, chain 1 two .. NS - 1, chain 2 more than NS (theta; Z where the estimator samples hard graphs)
    for cases in W.CHAIN_CASES.values():
        bs = [W.build(case, c_oracle64) for case in cases]
        if len({b["seed"] for b in bs}) == 1:   # one data set (the per-chain-data cases have one per chain)
            assert all(np.array_equal(b["x"], bs[0]["x"]) and np.array_equal(b["g0"], bs[0]["g0"]) for b in bs)
        assert len({tuple(b["key"]) for b in bs}) == 3
        for name in ("theta",) + (("z",) if bs[0]["est"] == "score" else ()):
            n = np.array([[p["nnz"] for p in b["profile"][name]] for b in bs])
            ns = bs[0]["ns"]
            assert (n[0] == 1).all() and (n[1] >= 2).all() and (n[1] < ns).all() and (n[2] > ns).all(), (bs[0]["id"], name, n)


@pytest.mark.parametrize("case", ALL_CASES, ids=W.case_id)
def test_reference_terms(c_oracle64, case):
    """The per-sample terms behind the GPU test's reference: free-edge gradients that are no cancellations, the cut share of every
    ladder profile below 1e-6, and -- with the oracle's own weights and no cut -- the C oracle's GRAD_THETA / W_LIK to 1e-9 (1e-6 for soft graphs)."""
    b = W.build(case, c_oracle64)
    d, x, mask = b["d"], np.asarray(b["x"], np.float64), b["mask"]
    t0 = time.perf_counter()
    W.sample_terms(b)
    print(f"\n{b['id']}: reference terms in {time.perf_counter() - t0:.1f} s")
    for name, lps, stage in (("theta", b["dbg"]["logprobs_th"], b["dbg"]["grad_theta"]), ("z", b["dbg"]["logprobs_z"], b["dbg"]["w_lik"])):
        shares = []
        for m in range(b["M"]):
            s = W.weighted_sums(b, name, m, W.weights32(lps[m]))
            lp = np.asarray(lps[m], np.float64)
            w64 = np.exp(lp - lp.max())
            w64 /= w64.sum()
            idx, g = W.sample_terms(b)[name][m]
            full = (w64[idx, None] * g).sum(0)
            ref = np.asarray(stage[m], np.float64).reshape(-1)[:full.size]
            tol = 1e-6 if (name == "z" and b["est"] == "reparam") else 1e-9   # (soft graphs: the bound test_oracle.py has for them)
            assert np.abs(full - ref).max() <= tol * np.abs(ref).max(), (name, m, np.abs(full - ref).max() / np.abs(ref).max())
            share = np.abs(s["dropped"]).max() / np.abs(s["kept"] + s["dropped"]).max()
            shares.append(share)
            if b["t_th"][m] != "straddle" and b["profile"][name][m]["near"] == 0:
                assert share <= 1e-6, (name, m, share)
        print(f"  {name:5s} cut share per particle:", " ".join(f"{v:.1e}" for v in shares))
    # no cancellation on the free edges (LinearGaussian: x_i^T r_j; DenseNN: x_i^T dpre_h for every hidden unit)
    for m in range(b["M"]):
        for i, j in b["edges"]:
            g1 = np.array(b["g0"])
            g1[i, j] = 1
            if b["model"] == "lingauss":
                ratio = W.lin_edge_ratio(x, mask, g1, b["theta"][m], (i, j))
            else:
                ratio = W.nn_edge_ratios(b["cfg_kw"], x, mask, g1, b["theta"][m], (i, j)).min(initial=1.0)
            assert ratio >= 1e-2, (m, (i, j), ratio)
