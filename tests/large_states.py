"""Particle states at which one whole SVGD step is finite AND non-trivial at 192 .. 256 variables, and the lock-step cases built on them for
every model family.  A plain module, imported by the tests like bge_states.py (no fixtures, no pytest hooks).

Freshly initialised particles have soft graphs around 1/2: (I + G/d)^(d-1) grows like 1.5^d, phi^2 leaves float32 in RMSprop's second
moment from d = 128 on and the acyclicity gradient itself near d = 220 -- for the reference's float32 arithmetic as for the device's.  The
latent kernel between two fresh particles is exp(-|z_a - z_b|^2 / h) ~ 1e-89 at d = 256: the cross-particle terms of the transform are
zero.  Both are properties of the state, not of the size; `clustered_sparse_state` builds what a run has after a few dozen steps instead:
sparse soft graphs (every edge score shifted by -c^2) and particles that are neighbours (kernel-matrix entries 0.6 .. 0.7).

tests/test_large_states_host.py pins on the C oracles alone that every case below is finite in float32 and non-vacuous;
tests/test_gpu_max_size.py runs the same cases on the device."""
import numpy as np

# 256: engine maximum, four full mask words, dp = 256 (an exact 4 x 4 grid of k_bgemm's 64-tiles), every lane of k_bge_soft with four rows
# 255: top bit of the last mask word unused, dp = 256 with one pad row
# 241: dp = 256 with 15 pad rows and columns (the zero padding of k_acycb_init at its widest inside a full tile grid)
# 225: dp = 240, the last 64-tile three quarters full
# 193: first four-word size, dp = 208, the last tile holds 16 columns
# 192: three full mask words, dp = 192, no padding anywhere
SIZES = (192, 193, 225, 241, 255, 256)
DENSE = dict(c=0.6, scale=2.0)    # ~22 parents per node, some problems beyond 32 (the one-problem-per-wave BGe tier)
SPARSE = dict(c=0.5, scale=1.0)   # ~4 parents per node
# the annealing runs on alpha = alpha_linear t with alpha_linear = 1 (MarginalDiBS) / 0.05 (JointDiBS) by default: the same alpha = 20, and
# with it the same soft graphs, at t = 20 / t = 400
MARGINAL_T, JOINT_T = 20, 400


def clustered_sparse_state(z0, c, scale, spread=0.05, seed=7):
    """z [M, d, k, 2] from freshly initialised particles z0 of the same shape (entry sd ~ 1 / sqrt(k)): every particle is
    scale z0[0] + spread sd(z0[0]) N(0, 1) from a seeded generator -- |z_a - z_b|^2 ~ 4 d k (spread sd)^2, kernel-matrix entries
    exp(-0.01 d / 5) for k = d -- and latent column 0 is u[:, 0] = +c, v[:, 0] = -c, which shifts EVERY edge score u_i . v_j by -c^2.
    Returned as float32-representable float64."""
    z0 = np.asarray(z0, np.float64)
    rng = np.random.default_rng(seed)
    z = scale * z0[:1] + spread * z0[0].std() * rng.standard_normal(z0.shape)
    z[:, :, 0, 0] = c
    z[:, :, 0, 1] = -c
    return z.astype(np.float32).astype(np.float64)


def _case(family, d, *, M=3, S=4, Sa=2, N=None, t=MARGINAL_T, c=DENSE["c"], scale=DENSE["scale"], interv=None, share_z=0.95, share_theta=None, **model_kw):
    """share_z / share_theta: the signal_share of conftest.update_check (the share of coordinates with |phi_ref| > 1e-3 max |phi_ref|)
    that tests/test_large_states_host.py measured for the case on the oracles, rounded down to 0.01, and holds as a lower bound; the GPU test asks
    for half of it.  (theta: most weights belong to edges that are absent from every sampled graph and have no likelihood gradient.)"""
    return dict(family=family, d=d, M=M, S=S, Sa=Sa, N=N or 3 * d, t=t, c=c, scale=scale, interv=interv, model_kw=model_kw,
                share_z=share_z, share_theta=share_theta)


def case_id(case):
    extra = "-".join(f"{k}={v}" for k, v in sorted(case["model_kw"].items()) if k in ("rng_layout", "graph_prior", "grad_estimator_z", "nn_activation"))
    return f"{case['family']}-d{case['d']}-c{case['c']}-s{case['scale']}" + ("-interv" if case["interv"] else "") + (f"-{extra}" if extra else "")


LARGE_CASES = (
    # MarginalDiBS + BGe, score estimator: every size on the dense-ish state; 256 again on the sparse state and with the partitionable
    # PRNG layout, interventions and the scale-free prior
    [_case("marginal_score", d) for d in SIZES]
    + [_case("marginal_score", 256, share_z=0.91, **SPARSE),
       _case("marginal_score", 256, interv=0.08, rng_layout="partitionable", graph_prior="sf")]
    # MarginalDiBS + BGe, reparam estimator (soft-graph BGe): no C port, the torch-autograd oracle
    + [_case("marginal_reparam", d, M=1, S=2, grad_estimator_z="reparam") for d in (193, 256)]
    # JointDiBS + LinearGaussian: N = 300 does not fit LDS, the engine takes the Gram path by itself, operands in global scratch
    + [_case("lingauss", 193, N=300, t=JOINT_T, share_theta=0.14, grad_estimator_z="reparam"),
       _case("lingauss", 256, N=300, t=JOINT_T, share_theta=0.12, interv=0.1, grad_estimator_z="reparam")]
    # JointDiBS + DenseNonlinearGaussian, hidden (3,): the general device path
    + [_case("densenn", 225, N=40, t=JOINT_T, share_theta=0.13, grad_estimator_z="score", nn_hidden=(3,), nn_activation="tanh", nn_bias=False),
       _case("densenn", 256, N=40, t=JOINT_T, share_theta=0.10, grad_estimator_z="reparam", nn_hidden=(3,), nn_activation="relu", nn_bias=True)]
)


def _data(case):
    """observations and intervention mask: what the existing stage test of the family uses at its largest sizes"""
    fam, d, N = case["family"], case["d"], case["N"]
    if fam.startswith("marginal"):
        from conftest import make_data
        x = np.asarray(make_data(d, seed=0, n_obs=N)[0].x)[:N].astype(np.float32)
        rng = np.random.default_rng(d)
    elif fam == "lingauss":   # test_joint_lingauss_gram_path: some structure in the data (lower-triangular mechanism)
        rng = np.random.default_rng(3)
        wts = (rng.random((d, d)) < 2.0 / d) * rng.normal(size=(d, d))
        x = rng.normal(size=(N, d)).astype(np.float32)
        for j in range(d):
            x[:, j] += (x[:, :j] @ np.tril(wts.T, -1)[j, :j]).astype(np.float32)
    else:                     # test_joint_densenn_general_stacks
        rng = np.random.default_rng(2)
        x = rng.normal(size=(N, d)).astype(np.float32)
    mask = (rng.random((N, d)) < case["interv"]).astype(np.int32) if case["interv"] else None
    return x, mask


_BUILT = {}


def large_case(case, oracle):
    """Data, mask, configuration keywords, state and key of a case -- one definition for the host test and the GPU test.  `oracle`: a
    COracle (its new_state draws z0 / theta from PRNGKey(1); both builds draw the same float32 values).  The arrays are shared between
    callers and read-only: copy the state before stepping it (`fresh_state`)."""
    from dibs_amd._abi import make_config
    from oracle import prng
    cid = case_id(case)
    if cid not in _BUILT:
        fam, d, M = case["family"], case["d"], case["M"]
        x, mask = _data(case)
        kw = dict(n_vars=d, n_particles=M, n_observations=case["N"], n_grad_mc_samples=case["S"], n_acyclicity_mc_samples=case["Sa"],
                  has_interventions=mask is not None, **case["model_kw"])
        if fam in ("lingauss", "densenn"):
            kw.update(joint=True, likelihood=fam)
        st = oracle.new_state(make_config(**kw), prng.PRNGKey(1))
        z = clustered_sparse_state(st["z"], case["c"], case["scale"])
        theta = None if st["theta"] is None else np.asarray(st["theta"], np.float32).astype(np.float64)
        out = dict(case, id=cid, x=x, mask=mask, cfg_kw=kw, z=z, theta=theta, key=np.array(st["key"], np.uint32))
        for a in (x, mask, z, theta, out["key"]):
            if a is not None:
                a.setflags(write=False)
        _BUILT[cid] = out
    return _BUILT[cid]


def fresh_state(built, real=np.float64):
    """the state dict COracle.step updates in place (second moments and baseline start at zero)"""
    z = np.array(built["z"], real)
    th = None if built["theta"] is None else np.array(built["theta"], real)
    return dict(z=z, v_z=np.zeros_like(z), theta=th, v_theta=None if th is None else np.zeros_like(th), key=built["key"].copy(),
                baseline=np.zeros(built["M"], real))


def oracle_step(oracle, built):
    """(state before, debug stages, state after) of one C-oracle step of the case at its t"""
    from dibs_amd._abi import make_config
    st = fresh_state(built, oracle.real)
    before = {k: (None if v is None else v.copy()) for k, v in st.items()}
    dbg = oracle.step(make_config(**built["cfg_kw"]), built["x"], built["mask"], st, built["t"], debug=True)
    return before, dbg, st


def autograd_step(built):
    """the torch-autograd oracle's step of a marginal reparam case (the C port has no soft-graph BGe): stage arrays as numpy float64"""
    import torch
    from oracle import dibs_oracle as O
    kw = built["cfg_kw"]
    ocfg = O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=built["S"], n_acyclicity_mc_samples=built["Sa"],
                    prior=O.GraphPrior(kw.get("graph_prior", "er"), 2), rng_layout=kw.get("rng_layout", "legacy"))
    st = O.init_state(ocfg, np.zeros(2, np.uint32), built["M"], built["d"])   # (only latent_prior_std is kept of it)
    st.z, st.v_z, st.key = torch.as_tensor(np.array(built["z"])), torch.zeros(built["z"].shape, dtype=torch.float64), built["key"].copy()
    xt = torch.as_tensor(built["x"].astype(np.float64))
    it = torch.as_tensor((built["mask"] if built["mask"] is not None else np.zeros_like(built["x"])).astype(np.float64))
    # thousands of small float64 operations: on one thread the step takes ~4 s whatever else the machine does; spread over a thread pool it
    # waits for the slowest thread at every one of them (2 s on an idle machine, 140 s measured inside the full GPU suite)
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        st2, aux = O.svgd_step(ocfg, st, xt, it, built["t"], return_aux=True)
    finally:
        torch.set_num_threads(n_threads)
    return dict(logprobs_z=np.stack([a["logprobs"].numpy() for a in aux["lik_aux"]]), grad_z=(aux["dz_lik"] + aux["dz_prior"]).numpy(),
                phi_z=aux["phi_z"].numpy(), kxx=aux["kxx"].numpy(), z=st2.z.numpy(), v_z=st2.v_z.numpy(), key=np.asarray(st2.key, np.uint32))


def parent_stats(g_samples):
    """(mean parent-set size, problems with more than 32 parents) of sampled graphs [M, S, d, d]"""
    l = np.asarray(g_samples).astype(np.int64).sum(axis=-2)
    return float(l.mean()), int((l > 32).sum())
