"""CPU-only checks of tests/soft_states.py: the numpy reference pinned to the autograd oracle, every profile's claims held against the
reference alone (so that tests/test_gpu_soft_bge.py compares the device on states that are what they say), the path bookkeeping, and the
yardstick -- the float32 run of the reference against its float64 run -- from which the GPU test's bounds are computed.

The yardstick table is written to the file named by DIBS_SOFT_BGE_TABLE (profiles/soft_bge_errors.txt keeps one run), to pytest's
temporary directory otherwise."""
import os

import numpy as np
import pytest

import soft_states as ss

PIN = 1e-9


def _ocfg(b):
    from oracle import dibs_oracle as O
    return O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=b["S"], alpha_linear=ss.ALPHA_LINEAR, tau=ss.TAU)


def _tensors(b):
    import torch
    x = torch.as_tensor(np.asarray(b["x"], np.float64))
    it = torch.zeros_like(x) if b["mask"] is None else torch.as_tensor(np.asarray(b["mask"], np.float64))
    return x, it


def test_bookkeeping_reaches_every_path():
    """the case table, derived from the restated launcher, holds every path of bge_soft_launch once per RL value"""
    rb = ss.rl_boundary()
    assert rb is not None and ss.soft_rl(rb[0], 1) and not ss.soft_rl(rb[1], 1) and rb[1] == rb[0] + 1
    assert not ss.soft_rl(rb[0], rb[0])                                   # per-node matrices are never LDS-resident
    assert all(ss.soft_waves(d, False) >= 1 for d in range(65, 129))      # engine.hip: the engine refuses a size without one wave
    hit = {ss.path_key(ss.soft_path(c["d"], c["interv"])) for c in ss.CASES}
    assert hit == ss.required_paths(), (hit ^ ss.required_paths())
    sizes = {c["d"] for c in ss.CASES}
    assert {5, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 160, *rb} <= sizes and max(sizes) == 160
    assert max(c["S"] for c in ss.CASES) == 128 and {c["S"] for c in ss.CASES} == {1, 3, 4, 128}
    for d in (17, 49, 64, 65, 129):
        assert {c["profile"] for c in ss.CASES if c["d"] == d} == set(ss.PROFILES), d
    assert {c["N"] for c in ss.CASES if c["profile"] == "few_obs"} == {1, 2, 5}
    for d in sizes - {160}:
        assert {c["interv"] for c in ss.CASES if c["d"] == d and c["profile"] == "mixed"} == {False, True}, d


@pytest.mark.parametrize("case", ss.HOST_PIN_CASES, ids=ss.case_id)
def test_reference_equals_autograd(case):
    """the float64 numpy reference against oracle.dibs_oracle.likelihood_sample_terms (autograd of the masked slogdet formula): 1e-9 of the
    largest entry, and entry by entry on the free edges"""
    import torch
    from oracle import dibs_oracle as O
    b = ss.build(case)
    x, it = _tensors(b)
    for m in range(b["M"]):
        lp, _, terms = O.likelihood_sample_terms(_ocfg(b), "reparam", torch.as_tensor(np.array(b["z"][m])), None, b["t"], b["kz"][m], x, it)
        lp, ds = lp.numpy(), terms[0].numpy()
        ref_lp, ref_ds = b["ref64"]["logprobs"][m], b["ref64"]["dscore"][m]
        assert ss.rel(ref_lp, lp) < PIN, (b["id"], m, ss.rel(ref_lp, lp))
        if np.abs(ds).max() > 1e-30:
            assert ss.rel(ref_ds, ds) < PIN, (b["id"], m, ss.rel(ref_ds, ds))
        else:
            assert np.abs(ref_ds).max() < 1e-30
        sel = np.broadcast_to(np.isin(b["cls"][m], ss.ENTRY_CLASSES), ds.shape) & (np.abs(ds) > 1e-30)
        if sel.any():
            e = np.abs(ref_ds - ds)[sel] / np.abs(ds[sel])
            assert e.max() < PIN, (b["id"], m, e.max())


@pytest.mark.parametrize("case", [c for c in ss.CASES if c["profile"] == "saturated"], ids=ss.case_id)
def test_saturated_is_the_limit_graph(case):
    """every p is exactly 0 or 1 in float32 as the device draws it, the soft graph is the limit graph in every sample, the gradient is below
    1e-30 in float64 and the log-probability is the hard-graph BGe score of the limit graph"""
    import torch
    from oracle import dibs_oracle as O
    b = ss.build(case)
    p32, g = ss.device_p32(b), ss.limit_graph(b)
    assert np.array_equal(p32, np.broadcast_to(g[:, None].astype(np.float32), p32.shape))
    assert np.abs(b["ref64"]["dscore"]).max() < 1e-30
    x, it = _tensors(b)
    for m in range(b["M"]):
        hard = float(O.bge_log_marginal(torch.as_tensor(g[m].astype(np.float64)), x, it, O.BGeParams()))
        assert np.abs(b["ref64"]["logprobs"][m] - hard).max() < PIN * abs(hard)


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_profiles_are_what_they_say(case):
    b = ss.build(case)
    d, M, S, cls, r64 = b["d"], b["M"], b["S"], b["cls"], b["ref64"]
    L, p32 = ss.logits(b), ss.device_p32(b)
    off = ~np.eye(d, dtype=bool)
    assert np.isfinite(r64["logprobs"]).all() and np.isfinite(r64["dscore"]).all()
    assert np.isfinite(b["ref32"]["logprobs"]).all() and np.isfinite(b["ref32"]["dscore"]).all() and (b["ref32"]["s"] > 0).all()
    if S > 1:
        assert ss.second_weight(r64["logprobs"]).min() >= ss.W2_MIN
    # the classes as the device draws them
    for k, test in ((ss.ONE, lambda p: p == 1.0), (ss.ZERO, lambda p: p == 0.0), (ss.TINY, lambda p: (p > 0) & (p < 1e-9)),
                    (ss.SMALL, lambda p: (p > 1e-7) & (p < 1e-3)), (ss.UNDER, lambda p: (p > 1.2e-38) & (p < 1e-20) & (p * p == 0)),
                    (ss.DENSE, lambda p: (p >= 0.9) & (p < 1.0))):
        sel = np.broadcast_to((cls == k)[:, None], p32.shape)
        assert test(p32[sel]).all(), (b["id"], ss.CLASSES[k])
    prof = case["profile"]
    if prof in ("mixed", "few_obs", "collinear", "small_p"):
        sat = (cls == ss.ONE).sum(1)                               # backbone parents per column
        for m in range(M):
            assert {0, 1, d // 2, d - 3 if prof == "collinear" else d - 2} <= set(sat[m].tolist()) or d < 6, (b["id"], sorted(set(sat[m].tolist())))
            nfree = (cls[m] == ss.FREE).sum(0)
            tested = np.flatnonzero(nfree >= 3)
            assert tested.size >= 2 and nfree.max() <= 6
            big = np.abs(r64["dscore"][m]).max(0) >= 1e-3 * np.abs(r64["dscore"][m]).max()     # [i, j]: in some sample
            for j in tested[tested != (-1 if b["all_intervened"] is None else b["all_intervened"])]:   # (that column is exactly 0)
                assert (big[:, j] & (cls[m][:, j] == ss.FREE)).sum() >= 3, (b["id"], m, j)
            A = ss.ALPHA * b["scores"][m].astype(np.float64)
            fa = A[cls[m] == ss.FREE]
            assert fa.min() >= -3 and fa.max() <= 3 and fa.max() - fa.min() > 3
            assert (np.abs(A[off & (cls[m] != ss.FREE) & (cls[m] != ss.SMALL)]) >= 40 - 1e-5).all() or prof == "small_p"
    if prof == "small_p":
        for m in range(M):
            cols_small = [j for j in range(d) if (cls[m][:, j] == ss.SMALL).sum() and not np.isin(cls[m][:, j], (ss.FREE, ss.UNDER)).any()]
            cols_under = [j for j in range(d) if (cls[m][:, j] == ss.UNDER).any()]
            assert len(cols_small) >= 1 and len(cols_under) == 1
            j = cols_under[0]
            assert np.isin(cls[m][:, j], (ss.UNDER, ss.ONE, ss.DIAG)).all()      # EVERY non-backbone parent of the column
            for j in cols_small:                                                  # at least 90 % of the non-backbone parents in range
                nb = ~np.isin(cls[m][:, j], (ss.ONE, ss.DIAG))
                assert (cls[m][nb, j] == ss.SMALL).mean() >= 0.9 or S > 1, (b["id"], j)
                assert (cls[m][nb, j] == ss.SMALL).mean() >= 0.5, (b["id"], j)
    if prof == "saturated":
        assert np.isin(cls[:, off], (ss.ONE, ss.ZERO)).all()
    if prof == "dense":
        assert (cls[:, off] == ss.DENSE).mean() >= (0.9 if S == 1 else 0.5) and np.isin(cls[:, off], (ss.DENSE, ss.ONE)).all()
        assert (p32[:, :, off] >= 0.9).all() and (r64["l"] >= 0.9 * (d - 1)).all() and case["N"] == 3 * d
    if prof == "collinear":
        coll = list(b["collinear"])
        assert len(coll) in (2, 3)
        ratio = r64["s"][:, :, coll] / b["R"][0][coll, coll]
        assert (ratio > ss.COLLINEAR_RATIO[0]).all() and (ratio < ss.COLLINEAR_RATIO[1]).all(), ratio
        nf = (cls[:, :, coll] == ss.FREE).sum(1)
        assert ((nf >= 1) & (nf <= 2)).all()
        s32 = b["ref32"]["s"][:, :, coll]
        assert (s32 > 0).all() and np.abs(s32 / r64["s"][:, :, coll] - 1).max() < 0.05
    if prof == "few_obs":
        a1, a2 = ss.gamma_args(b, r64["l"])
        assert case["N"] in (1, 2, 5) and a2.min() < 2.0 and a1.min() < 8.0 and a1.min() == 0.5 * (case["N"] + 3 + r64["l"].min())
    if case["interv"]:
        ja = b["all_intervened"]
        assert b["Nj"][ja] == 0 and (b["Nj"] > 0).sum() == d - 1 and len(set(b["Nj"].tolist())) > 2 and b["R"].shape[0] == d
        assert not r64["dscore"][:, :, :, ja].any() and (cls[:, :, ja] == ss.FREE).any()      # a zero column that has free edges
    else:
        assert b["R"].shape[0] == 1


def test_yardstick_table(tmp_path):
    """float32 run of the reference against the float64 run, per case and compared quantity; C_SUM beside the measurement"""
    lines = ["# float32 run of the numpy reference (tests/soft_states.py: soft_reference) against its float64 run, summed with the float64 run's weights",
             "# case | path | LOGPROBS_Z max-norm | W_LIK max-norm | per entry class: count, worst |f32 - f64| / |f64|, worst |f32 - f64| / sum_s w_s |dscore_s|"]
    ratios = []
    for c in ss.CASES:
        b = ss.build(c)
        y = ss.yardstick(b)
        ent = "  ".join(f"{k}: {n} {r:.2e} {a:.2e}" for k, (n, r, a) in y["entry"].items()) or "-"
        ratios += [a for _, _, a in y["entry"].values()]
        lines.append(f"{b['id']:34s} {b['path']['name']:26s} {y['lp']:.2e}  {y['w_max']:.2e}  {ent}")
        assert y["lp"] < ss.lp_floor(c["d"]) and y["w_max"] < ss.W_LIK_MAXNORM, (b["id"], y)
    ratios = np.sort(ratios)
    lines.append(f"# |f32 - f64| / sum_s w_s |dscore_s| over the {ratios.size} (case, class) cells: median {np.median(ratios):.2e}, "
                 f"90th percentile {np.percentile(ratios, 90):.2e}, worst {ratios[-1]:.2e}; C_SUM = {ss.C_SUM:.0e}")
    path = os.environ.get("DIBS_SOFT_BGE_TABLE") or str(tmp_path / "soft_bge_yardstick.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    # C_SUM is at least the 90th percentile of what plain float32 evaluation of the reference's formula gives (the cells above it are raised
    # by the 4 x yardstick rule), and no more than the W_LIK max-norm bound
    assert np.percentile(ratios, 90) <= ss.C_SUM <= ss.W_LIK_MAXNORM
