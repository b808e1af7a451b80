"""Particle states on which the LAST stage of a step -- kernel matrix, SVGD transform, optimizer (kernels_kmat.h, k_phi_update, k_phi_gemm) --
is not arithmetically trivial, a float64 numpy reference of that stage, and the case table built on both.  A plain module, imported by the
tests like bge_states.py / large_states.py (no fixtures, no pytest hooks).

Fresh particles have |z_a - z_b|^2 ~ 4 d whatever k is; with h_latent = 5 the off-diagonal latent kernel is e^(-4 d / 5): 8e-3 at d = 6,
1e-7 at d = 20, e^-40 at d = 50.  From d = 20 on the kernel matrix is the identity to float32 and phi_a = -grad_a / M: a wrong row index, a
dropped row of an odd quarter, a ragged 32-particle chunk that is not zeroed or swapped kz / kt operands change nothing an assertion sees.
The states here have off-diagonal weights of 0.2 .. 0.9 (`wide`: fresh particles and a bandwidth chosen for them; `neighbours` /
`offset_cluster`: a common vector plus a spread, |x| / |x_a - x_b| ~ 5 / >= 30, at the default bandwidths) or, on purpose, the e^-40
entries (`far`).  Two regimes: t = 0 (alpha = beta = 0: the gradient is the Gaussian prior's alone and, with the prior standard deviation of
the case, the repulsion is at least 0.3 of phi) and a step t > 0 in which the gradient dominates.

tests/test_transform_states_host.py pins on the oracles alone that every case is finite in float32 and non-vacuous;
tests/test_gpu_transform.py runs the cases on the device."""
import numpy as np

LN2 = float(np.log(2.0))
DENORM_MIN, NORM_MIN = 2.0 ** -149, 2.0 ** -126
# the entry-wise bound of a kernel-matrix entry (relative): 2e-6 (1 + |ln(K / scale)|).  Derived, not measured: the device sums the squared
# rounded differences of 16 elements in float32 (relative error <= 18 * 2^-24 ~ 1.1e-6: one rounding of the difference counted twice, one of
# the product, fifteen of the sum), everything above in double; exp multiplies the error of its argument tot / h = |ln(K / scale)| by that
# argument; the rounding of the result to float32 adds 6e-8.
KMAT_REL = 2e-6
KMAT_TINY = 1e-30   # entries below KMAT_TINY * scale: non-negative and <= 2 K_ref + the smallest denormal


def f32(a):
    """float32-representable float64"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- the reference of stage 8 / 9 -----------------------------------------------------------------------------------------------------------
def sq_dists(x):
    """|x_a - x_b|^2 [M, M] of the rows of x [M, len] in float64, from direct differences"""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    out = np.empty((len(x), len(x)))
    for a in range(len(x)):
        df = x - x[a]
        out[a] = np.einsum("bi,bi->b", df, df)
    return out


def kernel_matrix(x, h, scale=1.0):
    """K = scale exp(-|x_a - x_b|^2 / h) (kernels_kmat.h; kernel.py:20-30)"""
    return scale * np.exp(-sq_dists(x) / h)


def segment_phi(x, g, kw, kseg, h, diag_only=False):
    """(phi, repulsion term) of one segment: phi_a = -(1/M) sum_b [ kw_ab g_b - (2/h) kseg_ab (x_b - x_a) ] with the differences taken
    directly (k_phi_update's header; svgd.py:194-224); the repulsion term is +(1/M) (2/h) sum_b kseg_ab (x_b - x_a).  diag_only: K := diag K."""
    M = len(x)
    x, g = np.asarray(x, np.float64).reshape(M, -1), np.asarray(g, np.float64).reshape(M, -1)
    if diag_only:
        kw, kseg = np.diag(np.diag(kw)), np.diag(np.diag(kseg))
    drive = kw @ g
    rep = np.empty_like(x)
    for a in range(M):
        rep[a] = kseg[a] @ (x - x[a])
    rep *= 2.0 / h / M
    return -drive / M + rep, rep


def optimizer_step(cfg, x, v, phi):
    """(x, v) after RMSprop (v <- 0.9 v + 0.1 phi^2, x <- x - step phi / sqrt(v + 1e-8)) or gradient descent (v untouched)"""
    x, v, phi = (np.asarray(a, np.float64).reshape(-1) for a in (x, v, phi))
    if cfg.optimizer == 1:
        v = 0.9 * v + 0.1 * phi * phi
        return x - cfg.stepsize * phi / np.sqrt(v + 1e-8), v
    return x - cfg.stepsize * phi, v


def reference_transform(cfg, z, theta, grad_z, grad_theta, v_z=None, v_theta=None, diag_only=False):
    """Kernel matrices, phi and the optimizer step of a state in float64 numpy, given the gradients -- the oracle's, or the DEVICE'S OWN
    GRAD_Z / GRAD_THETA, which isolates the transform from upstream error."""
    M = len(z)
    kz = kernel_matrix(z, cfg.h_latent, cfg.scale_latent)
    kt = kernel_matrix(theta, cfg.h_theta, cfg.scale_theta) if theta is not None else np.zeros_like(kz)
    out = dict(kz=kz, kt=kt, kxx=kz + kt)
    phi, rep = segment_phi(z, grad_z, kz + kt, kz, cfg.h_latent, diag_only)
    out.update(phi_z=phi.reshape(np.shape(z)), rep_z=rep)
    if v_z is not None:
        xn, vn = optimizer_step(cfg, z, v_z, phi)
        out.update(z=xn.reshape(np.shape(z)), v_z=vn.reshape(np.shape(z)))
    if theta is not None:
        phi, rep = segment_phi(theta, np.asarray(grad_theta).reshape(M, -1), kz + kt, kt, cfg.h_theta, diag_only)
        out.update(phi_theta=phi, rep_theta=rep)
        if v_theta is not None:
            xn, vn = optimizer_step(cfg, theta, v_theta, phi)
            out.update(theta=xn.reshape(np.shape(theta)), v_theta=vn.reshape(np.shape(theta)))
    return out


def kmat_entry_errors(k_dev, parts, scales):
    """Entry-wise check of a kernel matrix against its float64 parts (`parts`: [kz] or [kz, kt], the device matrix being their sum formed
    in float32; `scales`: their scale factors).  Returns (worst error / bound over the entries where every part is >= KMAT_TINY scale and no
    part is denormal, number of such entries, the tiny entries are fine).  Bound of an entry: sum over the parts of
    KMAT_REL (1 + |ln(K / scale)|) K, plus one float32 rounding of the sum (6e-8) when there are two parts."""
    k_dev = np.asarray(k_dev, np.float64).reshape(parts[0].shape)
    ref = sum(parts)
    big = np.all([p >= KMAT_TINY * s for p, s in zip(parts, scales)], axis=0)
    bound = sum(KMAT_REL * (1.0 + np.abs(np.log(np.maximum(p, 1e-300) / s))) * p for p, s in zip(parts, scales))
    if len(parts) > 1:
        bound = bound + 2.0 ** -24 * ref
    worst = float((np.abs(k_dev - ref)[big] / bound[big]).max()) if big.any() else 0.0
    tiny = ~big if len(parts) == 1 else np.zeros_like(big)   # (two parts: the sum is checked where neither part is tiny or denormal)
    tiny_ok = bool(((k_dev[tiny] >= 0) & (k_dev[tiny] <= 2 * ref[tiny] + DENORM_MIN)).all())
    return worst, int(big.sum()), tiny_ok


def off_diagonal(k):
    return k[~np.eye(len(k), dtype=bool)]


# ---- state builders: seeded, float32-representable float64 ----------------------------------------------------------------------------------
def bandwidth_for(x, kappa=0.5):
    """the bandwidth at which the MEDIAN off-diagonal kernel entry of the rows x is kappa (a float32 value)"""
    return float(np.float32(np.median(off_diagonal(sq_dists(x))) / np.log(1.0 / kappa)))


def cluster(x0, h, ratio, kappa=0.5, seed=11):
    """x [M, ...] from freshly initialised x0 of the same shape: a common vector c = x0[0] scaled to |c| = ratio * r plus independent
    N(0, s^2) entries with 2 len s^2 = r^2 = h ln(1 / kappa) -- the squared distance of two particles is ~r^2, the kernel entry ~kappa at
    bandwidth h, and |x| / |x_a - x_b| ~ ratio.  Generalises large_states.clustered_sparse_state; the common offset leaves K unchanged."""
    x0 = np.asarray(x0, np.float64)
    M, n = len(x0), x0[0].size
    r = np.sqrt(h * np.log(1.0 / kappa))
    rng = np.random.default_rng(seed)
    c = x0[0] / np.linalg.norm(x0[0]) * ratio * r
    return f32(c[None] + r / np.sqrt(2.0 * n) * rng.standard_normal(x0.shape))


NEIGHBOUR_RATIO, OFFSET_RATIO = 5.0, 40.0   # (the host test pins >= 30 for offset_cluster on the built states)
# the signal_share of conftest.update_check (coordinates with |phi_ref| > 1e-3 max |phi_ref|): a lower bound that holds for EVERY case
# (pinned by the host test on the float64 oracle); the GPU test asks for half of it
SIGNAL_SHARE = dict(z=0.95, theta=0.75)   # (the float64 oracle has 0.965 .. 0.999 / 0.789 .. 0.999 over the cases)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
SCALED = dict(scale_latent=0.5)                        # the `_scaled` rows: make_config's scale_latent / scale_theta off their default 1
SCALED_JOINT = dict(scale_latent=0.5, scale_theta=3.0)


def _case(name, family, d, M, state, *, t=0, k=None, S=4, Sa=2, N=20, optimizer="rmsprop", env=None, exempt=(), **model_kw):
    """name: the branch the case exists for.  family: marginal | lingauss | densenn.  state: wide | neighbours | offset_cluster | far.
    t = 0: the repulsion regime (prior gradient only); t > 0: the gradient regime.  env: tuning switches set before the engine is created.
    exempt: non-vacuity conditions of the host test that cannot hold for the case by construction (stated where the case is listed)."""
    return dict(name=name, family=family, d=d, k=k or d, M=M, state=state, t=t, S=S, Sa=Sa, N=N, optimizer=optimizer, env=dict(env or {}),
                exempt=tuple(exempt), model_kw=model_kw)


def case_id(case):
    return case["name"]


def _marginal_rows():
    rows = []
    # k_phi_update<4, false>: d = 6 (len 144, three column blocks, the last ragged).  M = 1, 2, 3 leave waves with no rows (M = 1 has no
    # second particle: nothing crosses, every cross-particle condition is void); M = 5: Mq = 2, one wave with a single row and one with
    # none; M = 33: an odd quarter of 9 rows (`two == false` in its last pair); every M here has particle groups past Mloc or rlast clamps
    for M, s, t in ((1, "wide", 2), (2, "neighbours", 0), (3, "wide", 0), (5, "offset_cluster", 0), (7, "wide", 2), (33, "neighbours", 0),
                    (63, "wide", 0), (65, "offset_cluster", 0), (127, "neighbours", 2), (129, "wide", 0), (255, "offset_cluster", 0)):
        rows.append(_case(f"phi4_ragged_M{M}", "marginal", 6, M, s, t=t, exempt=("weights", "cross") if M == 1 else (),
                          optimizer="gd" if M == 63 else "rmsprop"))
    # k_phi_update<4, true>
    rows += [_case(f"phi4_full_M{M}", "marginal", 6, M, s, t=t) for M, s, t in ((64, "neighbours", 0), (128, "wide", 2), (192, "offset_cluster", 0))]
    # TA = 8: cols * ceil(M / 8) >= 1024 > cols * ceil(M / 16): D = 5000 (79 column blocks), M = 128 (FULL) and 127 (not FULL)
    rows += [_case("phi8_full_D5000_M128", "marginal", 50, 128, "neighbours", S=2, N=60),
             _case("phi8_ragged_D5000_M127", "marginal", 50, 127, "wide", S=2, N=60)]
    # TA = 16: cols * ceil(M / 16) >= 1024.  Not FULL: D = 4224 (d = 33, n_dim = 64: 66 blocks), M = 255; FULL: D = 5618 (d = 53: 88), M = 192
    rows += [_case("phi16_ragged_D4224_M255", "marginal", 33, 255, "wide", k=64, S=2, N=40),
             _case("phi16_full_D5618_M192", "marginal", 53, 192, "neighbours", S=2, N=60)]
    # k_phi_gemm<false>: len 144 -- the third column block is ragged (16 of 64 columns).  256: exact; 257: a 32-chunk with one live row and a
    # row block with one live particle; 272 / 319 / 320: half a chunk, all but one row, whole chunks; offset_cluster: the cancellation case
    for M, s, t in ((256, "wide", 0), (257, "neighbours", 0), (272, "offset_cluster", 0), (319, "wide", 2), (320, "neighbours", 0),
                    (1024, "offset_cluster", 0)):
        rows.append(_case(f"gemm_marginal_M{M}_{s}", "marginal", 6, M, s, t=t, optimizer="gd" if M == 320 else "rmsprop"))
    return rows


def _joint_rows():
    rows = []
    lin = dict(grad_estimator_z="reparam")
    # k_phi_update<4, *, true>: LinearGaussian d = 5 (D = 50, P = 25: odd offsets in the packed row) and d = 6 (D = 72, P = 36)
    for M, s, t in ((5, "wide", 0), (33, "offset_cluster", 0), (64, "neighbours", 0), (129, "wide", 2)):
        rows.append(_case(f"phi4_joint_lin_d5_M{M}", "lingauss", 5, M, s, t=t, optimizer="gd" if M == 33 else "rmsprop", **lin))
    rows += [_case("phi4_joint_lin_d6_M33", "lingauss", 6, 33, "neighbours", **lin), _case("phi4_joint_lin_d6_M64", "lingauss", 6, 64, "wide", t=2, **lin)]
    # DenseNonlinearGaussian with an odd P: d = 5, hidden (2,), bias: P = 5 (5 * 2 + 2 + 2 + 1) = 75 (the host test asserts that it is odd)
    rows.append(_case("phi4_joint_nn_oddP_M33", "densenn", 5, 33, "neighbours", grad_estimator_z="reparam", nn_hidden=(2,), nn_activation="tanh", nn_bias=True))
    # k_phi_gemm<true>: d = 5 is the scalar-load branch (vec_ok == false: D = 50, P = 25), d = 6 the float4 one
    for M, s, t in ((257, "wide", 0), (272, "offset_cluster", 0), (1024, "offset_cluster", 0)):
        rows.append(_case(f"gemm_joint_d5_M{M}_{s}", "lingauss", 5, M, s, t=t, **lin))
    rows += [_case("gemm_joint_d6_M256_neighbours", "lingauss", 6, 256, "neighbours", **lin),
             _case("gemm_joint_d6_M319_wide", "lingauss", 6, 319, "wide", t=2, optimizer="gd", **lin)]
    # the kernel scales off 1 (K = scale exp(-|.|^2 / h): the weights of phi's drive AND of its repulsion): k_phi_update<4, *, true> with the
    # direct kernel matrix, and k_phi_gemm<true> at M = 256
    rows += [_case("phi4_joint_lin_d6_M33_scaled", "lingauss", 6, 33, "neighbours", **lin, **SCALED_JOINT),
             _case("gemm_joint_d6_M256_scaled", "lingauss", 6, 256, "neighbours", **lin, **SCALED_JOINT)]
    return rows


def _kmat_rows():
    """The kernel-matrix algorithms on the same states, forced with the engine's existing switches (tuning.h); read off launch_kmat,
    kmat_launch_tiled, plan_step and kmat_pick_nsplit."""
    TILED = lambda n: {"DIBS_KMAT_TILED_MIN": str(n)}
    alone = {"DIBS_NO_KMAT_FUSE": "1"}
    return [
        # direct k_kmat as a launch of its own / riding in k_bge_sample (KmatPlace::InSample: marginal, score estimator, below the tiled minimum)
        _case("kmat_direct_M33", "marginal", 6, 33, "wide", env=alone),
        # (plan_step: a marginal step with both chains puts the matrix on the second stream once M D > 4 S d^2, i.e. M > 2 S at k = d: the
        #  other marginal cases, S = 4, are all there or in phase B; S = 40 keeps 65 particles inside k_bge_sample)
        _case("kmat_insample_M65", "marginal", 6, 65, "neighbours", S=40),
        _case("kmat_direct_far_M33", "marginal", 50, 33, "far", S=2, N=60, env=alone, exempt=("weights", "cross", "repulsion")),
        # direct, scalar staging: the joint model at d = 5 (D = 50, P = 25, unaligned rows)
        _case("kmat_direct_scalar_D50_M33", "lingauss", 5, 33, "wide", grad_estimator_z="reparam"),
        # tiled, nsplit = 1 (many tiles against few chunks) and ragged tiles: M = 520 = 16 tiles + 8 rows, one 144-element chunk
        _case("kmat_tiled_ns1_M520", "marginal", 6, 520, "wide", env=dict(alone, DIBS_KMAT_T64_MIN="100000")),
        # tiled, nsplit > 1 + k_kmat_finish: few tiles (M = 33: 3), many chunks (D = 5000); the last chunk is short
        _case("kmat_tiled_split_finish_M33_D5000", "marginal", 50, 33, "neighbours", S=2, N=60, env=dict(alone, **TILED(32))),
        _case("kmat_tiled_far_M65", "marginal", 50, 65, "far", S=2, N=60, env=dict(alone, **TILED(32)), exempt=("weights", "cross", "repulsion")),
        # tile units riding in k_particle_grad with tile counters (KmatPlace::InTail: marginal, 128 <= M < 256, M D <= 4 S d^2 and more than
        # one chunk): d = 12 (D = 288: a full chunk and one of 32 elements), S = 72; 15 tiles in ns = 2 pieces
        _case("kmat_intail_M130_D288", "marginal", 12, 130, "wide", S=72, N=40),
        # the joint models compute theirs on the second stream (KmatPlace::Stream2), tiled with scalar staging at d = 5
        _case("kmat_stream2_tiled_scalar_M130", "lingauss", 5, 130, "neighbours", grad_estimator_z="reparam"),
        # 64 x 64 tiles: M = 520 (8 full tiles and 8 rows of a ninth), forced from 512 down to 65 particles as well
        _case("kmat_tile64_M520", "marginal", 6, 520, "neighbours", env=alone),
        _case("kmat_tile64_M65", "marginal", 6, 65, "wide", env=dict(alone, DIBS_KMAT_T64_MIN="64", **TILED(64))),
        _case("kmat_tile64_far_M130", "marginal", 50, 130, "far", S=2, N=60, env=dict(alone, DIBS_KMAT_T64_MIN="64"),
              exempt=("weights", "cross", "repulsion")),
        # scale_latent = 0.5 (joint: and scale_theta = 3) on each of the places above: direct, in k_bge_sample, tiled with k_kmat_finish,
        # in-tail riders, second stream tiled, 64 x 64 tiles (k_phi_gemm at M = 256: _joint_rows)
        _case("kmat_direct_scaled_M33", "marginal", 6, 33, "wide", env=alone, **SCALED),
        _case("kmat_insample_scaled_M65", "marginal", 6, 65, "neighbours", S=40, **SCALED),
        _case("kmat_tiled_split_finish_scaled_M33_D5000", "marginal", 50, 33, "neighbours", S=2, N=60, env=dict(alone, **TILED(32)), **SCALED),
        _case("kmat_intail_scaled_M130_D288", "marginal", 12, 130, "wide", S=72, N=40, **SCALED),
        _case("kmat_stream2_tiled_scaled_M130", "lingauss", 5, 130, "neighbours", grad_estimator_z="reparam", **SCALED_JOINT),
        _case("kmat_tile64_scaled_M65", "marginal", 6, 65, "wide", env=dict(alone, DIBS_KMAT_T64_MIN="64", **TILED(64)), **SCALED),
    ]


def _multi_rows():
    """The states of the multi-run engines (tests/test_gpu_transform.py runs problem / chain c of ONE engine against the standalone engine
    on the same state, bit for bit) and of the float64 engine; as standalone cases they pass through every check like the others.
    batch: two problems that differ in h_latent (5 / the wide state's ~35) and latent_prior_std -- k_phi_update<.., BATCH>, k_kmat_batch;
    chains: two chains that differ in h_latent and h_theta (5, 500 / ~25, ~150) -- k_kmat_chains_hp, the JOINT + BATCH instantiation; t > 0,
    where the chains need no per-chain likelihood settings."""
    lin = dict(grad_estimator_z="reparam")
    return [_case("batch_p0_M33_neighbours", "marginal", 6, 33, "neighbours"), _case("batch_p1_M33_wide", "marginal", 6, 33, "wide"),
            _case("chains_c0_lin_d5_M33_neighbours", "lingauss", 5, 33, "neighbours", t=2, **lin),
            _case("chains_c1_lin_d5_M33_wide", "lingauss", 5, 33, "wide", t=2, **lin),
            _case("f64_M65_neighbours", "marginal", 6, 65, "neighbours")]


CASES = tuple(_marginal_rows() + _joint_rows() + _kmat_rows() + _multi_rows())
BATCH_CASES = tuple(c for c in CASES if c["name"].startswith("batch_"))
CHAIN_CASES = tuple(c for c in CASES if c["name"].startswith("chains_"))
F64_CASE = next(c for c in CASES if c["name"].startswith("f64_"))
assert len({c["name"] for c in CASES}) == len(CASES)


def _data(case):
    from conftest import make_data
    d, N = case["d"], case["N"]
    return np.asarray(make_data(d, seed=0, n_obs=N, joint=case["family"] != "marginal")[0].x)[:N].astype(np.float32)


_BUILT = {}


def build(case, oracle):
    """Data, configuration keywords, state and key of a case -- one definition for the host test and the GPU test.  `oracle`: the float64
    COracle (fresh particles from PRNGKey(1); one step of it gives the non-zero second moments v_z / v_theta the case starts from).
    The arrays are shared between callers and read-only: copy the state before stepping it (`fresh_state`)."""
    from dibs_amd._abi import make_config
    from oracle import prng
    name = case["name"]
    if name in _BUILT:
        return _BUILT[name]
    fam, d, M, kind = case["family"], case["d"], case["M"], case["state"]
    joint = fam != "marginal"
    kw = dict(n_vars=d, n_dim=case["k"], n_particles=M, n_observations=case["N"], n_grad_mc_samples=case["S"],
              n_acyclicity_mc_samples=case["Sa"], optimizer=case["optimizer"], edges_per_node=1 if d <= 5 else 2, **case["model_kw"])
    if joint:
        kw.update(joint=True, likelihood=fam)
    st = oracle.new_state(make_config(**kw), prng.PRNGKey(1))
    z0, th0 = f32(st["z"]), None if st["theta"] is None else f32(st["theta"])
    ratio = dict(neighbours=NEIGHBOUR_RATIO, offset_cluster=OFFSET_RATIO).get(kind)
    if kind in ("wide", "far"):
        z, theta = z0, th0
        if kind == "wide" and M > 1:
            kw["h_latent"] = bandwidth_for(z.reshape(M, -1))
            if joint:
                kw["h_theta"] = bandwidth_for(theta)
    else:   # the default bandwidths (make_config: h_latent = 5, h_theta = 500)
        z = cluster(z0, 5.0, ratio)
        theta = None if th0 is None else cluster(th0, 500.0, ratio, seed=12)
    if case["t"] == 0 and kind != "far":
        # Gaussian prior gradient -x / sigma^2 against the repulsion (2 / h) K (x_b - x_a): of the same size for independent particles at
        # sigma^2 = h / 2.8 (entries of x_b - x_a are sqrt(2) those of x); the common vector of a cluster adds up over the M particles
        # while the differences add like sqrt(M).  Half of that gradient, so that the repulsion is the larger part.
        h = kw.get("h_latent", 5.0)
        kw["latent_prior_std"] = float(np.float32(np.sqrt(h * max(1.0, (ratio or 1.0) * np.sqrt(M)))))
    if joint and case["t"] == 0:
        # theta: the likelihood's gradient does not vanish with alpha (hard graphs at probability 1/2); a flat likelihood and a flat prior
        # leave the repulsion of the parameter kernel in charge
        big = 1e4 * max(1.0, (ratio or 1.0) * np.sqrt(M))
        kw.update(dict(lin_obs_noise=big, lin_sig_edge=big) if fam == "lingauss" else dict(nn_obs_noise=big, nn_sig_param=big))
    out = dict(case, id=name, x=_data(case), mask=None, cfg_kw=kw, z=z, theta=theta, key=np.array(st["key"], np.uint32))
    # non-zero second moments: those after one float64 oracle step from the state (0.1 phi^2), as float32 values
    s1 = fresh_state(dict(out, v_z=np.zeros_like(z), v_theta=None if theta is None else np.zeros_like(theta)))
    oracle.step(make_config(**kw), out["x"], None, s1, case["t"])
    out["v_z"] = f32(s1["v_z"])
    out["v_theta"] = None if theta is None else f32(s1["v_theta"])
    for a in (out["x"], z, theta, out["key"], out["v_z"], out["v_theta"]):
        if a is not None:
            a.setflags(write=False)
    _BUILT[name] = out
    return out


def fresh_state(built, real=np.float64):
    """the state dict COracle.step updates in place"""
    z = np.array(built["z"], real)
    th = None if built["theta"] is None else np.array(built["theta"], real)
    return dict(z=z, v_z=np.array(built["v_z"], real), theta=th, v_theta=None if th is None else np.array(built["v_theta"], real),
                key=built["key"].copy(), baseline=np.zeros(built["M"], real))


def oracle_step(oracle, built):
    """(state before, debug stages, state after) of one C-oracle step of the case at its t"""
    from dibs_amd._abi import make_config
    st = fresh_state(built, oracle.real)
    before = {k: (None if v is None else v.copy()) for k, v in st.items()}
    dbg = oracle.step(make_config(**built["cfg_kw"]), built["x"], built["mask"], st, built["t"], debug=True)
    return before, dbg, st


def transform_errors(built, cfg, kxx, phi_z, phi_theta, grad_z, grad_theta):
    """The quantities of tests/test_gpu_transform.py for one implementation's output (the device's, or the float32 oracle's as the
    yardstick): the entry-wise kernel-matrix error over its bound, and phi against the float64 numpy reference fed THAT implementation's
    gradients -- max-norm relative to max |phi_ref| and the element-wise 99th percentile on the signal entries."""
    joint = built["theta"] is not None
    ref = reference_transform(cfg, built["z"], built["theta"], grad_z, grad_theta)
    parts, scales = ([ref["kz"], ref["kt"]], [cfg.scale_latent, cfg.scale_theta]) if joint else ([ref["kz"]], [cfg.scale_latent])
    worst, n, tiny_ok = kmat_entry_errors(kxx, parts, scales)
    out = dict(kmat_over_bound=worst, kmat_entries=n, kmat_tiny_ok=tiny_ok, kmat_maxnorm=_rel(kxx, ref["kxx"]), ref=ref)
    for seg, phi in (("z", phi_z), ("theta", phi_theta))[:2 if joint else 1]:
        want = ref["phi_" + seg].reshape(-1)
        got = np.asarray(phi, np.float64).reshape(-1)[:want.size]
        scale = np.abs(want).max()
        big = np.abs(want) > 1e-3 * scale
        out["phi_" + seg] = float(np.abs(got - want).max() / scale)
        out["phi_" + seg + "_p99"] = float(np.percentile(np.abs(got - want)[big] / np.abs(want)[big], 99))
    return out


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
