"""Particle states that drive the BGe factorisation kernels (dibs_amd/csrc/kernels_bge.h) through EVERY parent-set size, and the bookkeeping
that says which code path scored which problem.  A plain module, imported by the tests like conftest (no fixtures, no pytest hooks).

k_bge_sample queues a problem (particle m, sample s, node j) by the size l of its sampled parent set: n = min(l + 1, d - l) rows
(bge_rows), direct form on R[pa + j] when l + 1 <= d - l and complement form on Q = R^-1 otherwise, queue tier bge_tier(n) = (n + 3) / 4 - 1
for n <= 32 and the one-problem-per-wave tier (8) beyond; l = 0 is scored without a factorisation.  Graphs sampled from freshly initialised
particles have l ~ Binomial(d - 1, 1/2): two or three tiers per size.  `tier_sweep_state` builds particles whose sampled graphs have every
l in 0 .. d - 1 instead."""
import numpy as np

BGE_NQ = 9    # queue tiers (kernels_bge.h)
FORMS = ("direct", "complement")


def bge_rows(l, d):
    """rows of the factorisation of a node with l parents (kernels_bge.h: bge_rows)"""
    l = np.asarray(l)
    return np.where(l + 1 <= d - l, l + 1, d - l)


def bge_tier(n):
    """queue tier of a factorisation with n rows (kernels_bge.h: bge_tier)"""
    n = np.asarray(n)
    return np.where(n <= 32, (n + 3) // 4 - 1, BGE_NQ - 1)


def tier_sweep_state(d, M, rng):
    """z [M, d, d, 2] (n_dim = d, float32-representable) for one step at t = 1 with alpha_linear = 1.

    Particle m: z[m, :, :, 0] = c_m I and z[m, j, :, 1] = c_m (+1 on a random set of L = (j + m d // M) mod d variables other than j, -1
    elsewhere), so the score of edge i -> j is u_i . v_j = +- c_m^2 and node j has L parents where the Bernoulli draws follow the sign.
    Particle 0 has c^2 = 40: sigmoid(+-40) is 1 / 0 in float32, node j gets exactly j parents in every sample -- every l in 0 .. d - 1 once
    per sample, l = 0 and l = d - 1 included.  The others have c^2 = 3 (p = 0.95 / 0.05): their sizes jitter around L, so the problems
    that share a lane, a pair or a quad of a tier differ in size."""
    z = np.zeros((M, d, d, 2), np.float64)
    for m in range(M):
        c = np.sqrt(40.0 if m == 0 else 3.0)
        z[m, :, :, 0] = c * np.eye(d)
        for j in range(d):
            L = (j + m * d // M) % d
            others = np.delete(np.arange(d), j)
            v = -np.ones(d)
            v[rng.choice(others, size=L, replace=False)] = 1.0
            z[m, j, :, 1] = c * v
    return z.astype(np.float32).astype(np.float64)


def problem_cells(g_samples, d):
    """per problem of g_samples [..., d, d] (g[i, j] = 1: i is a parent of j): l, complement form?, tier -- arrays [..., d]"""
    l = np.asarray(g_samples).astype(np.int64).sum(axis=-2)
    comp = l + 1 > d - l
    return l, comp, bge_tier(bge_rows(l, d))


def tier_histogram(g_samples, d):
    """counts of the problems of g_samples [..., d, d]: per parent-set size, of l = 0, and per (form, tier) among l > 0"""
    l, comp, tier = problem_cells(g_samples, d)
    fact = l > 0
    return dict(sizes=np.bincount(l.ravel(), minlength=d)[:d], l0=int((l == 0).sum()),
                direct=np.bincount(tier[fact & ~comp], minlength=BGE_NQ), complement=np.bincount(tier[fact & comp], minlength=BGE_NQ))


def tiers_present(d):
    """the (form, tier) cells that exist at d: the direct form has n = l + 1 <= (d + 1) // 2 rows, the complement form n = d - l <= d // 2"""
    first = [4 * t + 1 for t in range(BGE_NQ)]   # smallest n of tier t (tier 8: 33)
    return {"direct": [t for t in range(BGE_NQ) if first[t] <= (d + 1) // 2 and d > 1],
            "complement": [t for t in range(BGE_NQ) if first[t] <= d // 2]}


def assert_coverage(hist, d, min_count=8):
    """every parent-set size 0 .. d - 1 occurs, and every (form, tier) cell that exists at d holds at least `min_count` problems"""
    missing = np.flatnonzero(hist["sizes"] == 0)
    assert missing.size == 0, f"d = {d}: no problem with l in {missing.tolist()}"
    assert hist["l0"] > 0
    for form, tiers in tiers_present(d).items():
        for t in tiers:
            assert hist[form][t] >= min_count, f"d = {d}: {form} tier {t} holds {int(hist[form][t])} problems"


def cell_errors(got, ref, g_samples, d):
    """worst |got - ref| per (form, tier) cell and for l = 0: a list of (cell name, count, worst absolute error); got / ref [M, S, d]"""
    l, comp, tier = problem_cells(g_samples, d)
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    rows = []
    sel = l == 0
    if sel.any():
        rows.append(("l=0", int(sel.sum()), float(err[sel].max())))
    for c, form in enumerate(FORMS):
        for t in range(BGE_NQ):
            sel = (l > 0) & (comp == bool(c)) & (tier == t)
            if sel.any():
                rows.append((f"{form} tier {t}", int(sel.sum()), float(err[sel].max())))
    return rows


def graphs_from_masks(masks, M, S, d):
    """PARENT_MASKS of an engine ([m][j][s][w] uint64: bit i of word i // 64 = g[i, j]) as graphs [M, S, d, d]"""
    gm = np.asarray(masks).reshape(M, d, S, -1)
    gg = np.zeros((M, S, d, d), np.uint8)
    for i in range(d):
        gg[:, :, i, :] = ((gm[:, :, :, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.uint8).transpose(0, 2, 1)
    return gg


# ---- LDS footprint of k_bge_chol (kernels_bge.h: bge_chol_lds_bytes; tu_bge.hip: the 150 KiB cut) -----------------------------------------
BGE_PS = 28
LDS_CUT = 150 * 1024


def chol_lds_bytes(d, r_in_lds):
    r = ((2 * (d + 1) * (d + 1) * 4 + 15) & ~15) if r_in_lds else 0
    quad = 32 * BGE_PS * 4
    per_wave = (64 + 64 + 8) * 4
    waves = min(max((160 * 1024 - 2048 - r - 4 * quad) // per_wave, 1), 4)
    return r + 4 * quad + (waves * per_wave if d > 64 else 0)


def lds_cut_size():
    """smallest d <= 128 whose single matrix pair no longer stays in LDS (k_bge_chol<false, true> without interventions), or None"""
    return next((d for d in range(2, 129) if chol_lds_bytes(d, True) > LDS_CUT), None)


# ---- the lock-step cases: data, configuration, state ---------------------------------------------------------------------------------------
# (d, M, S, interventions): every size the GPU tests of tests/test_gpu_bge_tiers.py construct a state for
SWEEP_SIZES = ([(d, 4, 8, False) for d in (50, 63, 64, 65, 70, 80, 112, 128)] + [(50, 4, 8, True), (80, 4, 8, True)]
               + [(130, 2, 4, False), (200, 2, 4, False), (130, 2, 4, True)]
               + ([(lds_cut_size(), 4, 8, False)] if lds_cut_size() not in (None, 128) else []))   # (none today: test_bge_states_host.py)


def sweep_case(d, M=4, S=8, Sa=2, interv=False, seed=0, n_obs=None):
    """One step at t = 1 from tier_sweep_state: data (more observations than variables beyond d = 112, as test_marginal_bge_step_stages),
    optional interventions (density 0.15, so N_j differs per node; node d // 3 is intervened in EVERY row: its score is 0 at every l),
    configuration keywords, particles and loop-carry key."""
    from conftest import make_data
    N = n_obs or (100 if d <= 112 else 3 * d)
    data, _, lm = make_data(d, seed=seed, n_obs=N)
    rng = np.random.default_rng(1000 * seed + d)
    mask, ja = None, None
    if interv:
        ja = d // 3
        mask = (rng.random((N, d)) < 0.15).astype(np.int32)
        mask[:, ja] = 1
    kw = dict(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=Sa, alpha_linear=1.0,
              has_interventions=interv)
    return dict(d=d, M=M, S=S, x=np.asarray(data.x)[:N], mask=mask, all_intervened=ja, cfg_kw=kw, z=tier_sweep_state(d, M, rng),
                key=np.array([seed + 11, d], np.uint32), t=1, data=data, lm=lm)


def oracle_step(oracle, case, **cfg_extra):
    """the C oracle's step of `case` with debug outputs (the case is left untouched)"""
    from dibs_amd._abi import make_config
    cfg = make_config(**dict(case["cfg_kw"], **cfg_extra))
    z = np.array(case["z"], oracle.real)
    st = dict(z=z, v_z=np.zeros_like(z), theta=None, v_theta=None, key=case["key"].copy(), baseline=np.zeros(case["M"], oracle.real))
    return oracle.step(cfg, case["x"], case["mask"], st, case["t"], debug=True)
