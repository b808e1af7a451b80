"""The hyper-parameter axis: every kernel family away from make_config's defaults (tau = 1, unit edge / parameter priors, bge_alpha_mu = 1,
bge_alpha_lambd = d + 2, no bge_mean_obs, beta_linear = 1, unit kernel scales), where a dropped factor or a wrong sign changes nothing.
A plain-Python restatement of the launchers' path choice, the case table derived from it and the references.  A plain module, imported by
the tests like obs_axis.py and soft_states.py (no fixtures, no pytest hooks).

What tau reaches.  The soft graphs are sigmoid(tau (eps + alpha s)); with tau == 1 the draw loops take u / (u + (1 - u) exp(-alpha s)),
otherwise 1 / (1 + expf(-tau (rng_logistic(bits) + alpha s))), and the epilogues multiply by tau alpha g (1 - g).  The acyclicity kernels
draw soft graphs under either estimator; the likelihood kernels only in the Z pass of grad_estimator_z = "reparam".  `reaches` lists, for
a case, the draw loops and epilogues that its step runs on the general path; REQUIRED is what the table must reach.

References.  The float64 C oracle (oracle/dibs_oracle.c) for everything but the soft-graph BGe kernels, which it does not implement
(orc_step returns 5 for reparam + BGe): those cases take the torch-autograd oracle (oracle/dibs_oracle.py), as
test_marginal_bge_reparam_estimator does, with that test's bounds, and W_LIK -- the likelihood's gradient on its own, see SOFT_SHOWS_IN --
with the bound of tests/test_gpu_soft_bge.py.

tests/test_hparam_states_host.py holds the table against the restatement and the references against themselves;
tests/test_gpu_hparams.py runs the cases on the device."""
import numpy as np

import obs_axis as A
import soft_states as SS

KEY = 3
T_MARGINAL, T_JOINT = 2, 40      # alpha = alpha_linear t = 2 for both (alpha_linear: 1 marginal, 0.05 joint)
TAUS = (0.7, 2.0)

# make_config's defaults of what the cases move (bge_alpha_lambd None: d + 2; mean_obs None: zeros)
DEFAULTS = dict(tau=1.0, beta_linear=1.0, scale_latent=1.0, scale_theta=1.0, bge_alpha_mu=1.0, bge_alpha_lambd=None, mean_obs=None,
                lin_mean_edge=0.0, lin_sig_edge=1.0, lin_obs_noise=0.1, nn_sig_param=1.0, nn_obs_noise=0.1)
COMMON = dict(beta_linear=0.3, scale_latent=0.5)
LIN = dict(lin_mean_edge=0.3, lin_sig_edge=2.0, lin_obs_noise=0.5)
NN = dict(nn_sig_param=0.6, nn_obs_noise=0.4)
# the stage in which putting ONE parameter back to its default must show (tests/test_hparam_states_host.py: by 20 x the stage's bound)
SHOWS_IN = dict(tau="W_ACYC", beta_linear="GRAD_Z", scale_latent="KXX", scale_theta="KXX", bge_alpha_mu="LOGPROBS_Z", bge_alpha_lambd="LOGPROBS_Z",
                mean_obs="LOGPROBS_Z", lin_mean_edge="LOGPROBS_THETA", lin_sig_edge="LOGPROBS_THETA", lin_obs_noise="LOGPROBS_THETA",
                nn_sig_param="LOGPROBS_THETA", nn_obs_noise="LOGPROBS_THETA")
# the joint rows of the reparam estimator are there for the LIKELIHOOD kernels' general draw loop and tau alpha epilogue: there tau must
# also show in one of these, stages of those kernels (W_ACYC is the acyclicity kernel's)
TAU_LIK_STAGES = ("LOGPROBS_Z", "W_LIK")
# The soft-graph BGe cases.  GRAD_Z and PHI_Z are no check of these kernels: from 49 variables on the acyclicity term is 1e6 .. 1e13 times
# the likelihood's gradient in the max-norm.  Their gradient is compared on its own, as W_LIK = sum_s w_s d log p(soft graph_s) / d scores,
# and every parameter the kernels see must show THERE -- with the weights w held fixed (soft_w_lik), so that what moves is the per-sample
# gradient, not only the softmax of the log-probabilities -- and the prior's parameters in the forward LOGPROBS_Z as well.
SOFT_SHOWS_IN = dict(tau=("W_LIK",), bge_alpha_mu=("LOGPROBS_Z", "W_LIK"), bge_alpha_lambd=("LOGPROBS_Z", "W_LIK"), mean_obs=("LOGPROBS_Z", "W_LIK"),
                     beta_linear=("GRAD_Z",), scale_latent=("KXX",))


def bge_prior(d):
    """the off-default BGe prior of every marginal case: amu / (amu + 1) = 1/3, alpha_lambd - d - 1 = 4.5, a mean that differs per node"""
    return dict(bge_alpha_mu=0.5, bge_alpha_lambd=d + 2 + 3.5, mean_obs=(1.0 + 3.0 * np.cos(1.7 * np.arange(d))).astype(np.float32))


# ---- the acyclicity kernels: the path choice ------------------------------------------------------------------------------------------------
def acyc_paired(d, Sa, layout="legacy"):
    """engine.hip: dibs_engine_create, `paired` -- one Threefry call serves two chains: legacy layout, even Sa, Sa d d below 2^32"""
    return layout == "legacy" and Sa % 2 == 0 and Sa * d * d < 0xFFFFFFFF


def acyc_kernel(d, Sa, layout="legacy", hfw_max=112):
    """tu_acyc.hip: acyc_launch_power with acyc_use_bf16 / acyc_use_bfw at DIBS_PIPE_DEFAULT (the A/B pipes are not restated).
    hfw_max: DibsTuning::acyc_hfw_max (tuning.h; DIBS_ACYC_HFW_MAX, default 112: by DEFAULT the whole range 65 .. 112 runs k_acyc_hfw,
    and k_acyc_bfw is reached only with a smaller hfw_max)"""
    if d > 112:
        return "k_acycb"                                  # engine.hip: acyc_big; kernels_acyc_big.h: acycb_soft_graph in k_acycb_init / _out
    paired, NT = acyc_paired(d, Sa, layout), (d + 15) // 16
    if paired and 33 <= d <= 64:
        return f"k_acyc_hf<{str(d > 48).lower()},3>"
    if paired and 64 < d <= 112:
        return f"k_acyc_hfw<{max(NT, 5)}>" if d <= hfw_max else f"k_acyc_bfw<{max(NT, 5)}>"
    return f"k_acyc<{NT},{str(paired).lower()}>"


def acyc_family(name):
    return name.split("<")[0] + ("<unpaired>" if name.endswith(",false>") and name.startswith("k_acyc<") else "")


# ---- what a case reaches --------------------------------------------------------------------------------------------------------------------
# the draw loops that branch on tau == 1 (k_acyc_bf is left out: only DIBS_ACYC_BF16 selects it, an A/B switch).  kernels_nn.h has no
# function of its own for the paired draws of the f32 DenseNN kernel: they are the FAST instantiation nn_build_graph_tab<true> ...
DRAW_LOOPS = ("k_acyc", "k_acyc<unpaired>", "k_acyc_hf", "k_acyc_hfw", "k_acyc_bfw", "k_acycb", "k_lin_logprobs_pair", "k_lin_logprobs_hf",
              "nn_build_graph_tab<true>", "nn_grad_build_graph", "kernels_nn_f16.h", "kernels_nn_f16x.h",
              "lin_sample_g:k_lin_logprobs", "lin_sample_g:k_lin_grad", "lin_sample_g:k_ling", "lin_sample_g:k_nng", "lin_sample_g:k_bge_soft_mf",
              "lin_sample_g:k_bge_soft")
# ... and the epilogues that multiply by tau alpha g (1 - g): the six acyclicity kernels above (k_acyc_bf again left out) and
EPILOGUES = ("k_lin_grad", "k_ling_grad", "k_nn_grad", "k_nng_grad", "k_soft_combine")
REQUIRED = frozenset(DRAW_LOOPS + EPILOGUES)


def reaches(c):
    """the draw loops / epilogues of DRAW_LOOPS + EPILOGUES that one step of the case runs with soft graphs (so: on its tau path)"""
    d, N, S = c["d"], c["N"], c["S"]
    out = {acyc_family(acyc_kernel(d, c["Sa"], c["layout"], c["hfw_max"]))}
    if c["est"] != "reparam":
        return out
    if c["model"] == "bge":
        p = SS.soft_path(d, c["interv"])
        return out | {"lin_sample_g:" + p["kernel"], "k_soft_combine"}
    if c["model"] == "lingauss":
        k = A.lin_kernel(d, N, S, c["layout"])
        if k == "gram":
            return out | {"lin_sample_g:k_ling", "k_ling_grad"}
        out |= {"lin_sample_g:k_lin_grad", "k_lin_grad"}
        return out | {"k_lin_logprobs_pair" if k.startswith("pair<") else "k_lin_logprobs_hf" if k.startswith("hf<") else "lin_sample_g:k_lin_logprobs"}
    H = c["model_kw"]["nn_hidden"]
    k = A.nn_logprob_kernel(d, N, H[0], S, True, c["layout"]) if len(H) == 1 else "general"
    if k == "general":
        return out | {"lin_sample_g:k_nng", "k_nng_grad"}
    out |= {"nn_grad_build_graph", "k_nn_grad"}
    return out | {"kernels_nn_f16x.h" if k.startswith("hx") else "kernels_nn_f16.h" if k == "image" else "nn_build_graph_tab<true>"}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _case(group, kernel, model, d, *, N=None, M=2, S=2, Sa=2, est="score", tau=0.7, interv=False, layout="legacy", hfw_max=112, **model_kw):
    """kernel: what the row is meant to reach (tests/test_hparam_states_host.py holds it against `reaches` / the restated dispatch)"""
    N = N or (min(3 * d, 100) if d <= 112 else 3 * d)
    return dict(group=group, kernel=kernel, model=model, d=d, N=N, M=M, S=S, Sa=Sa, est=est, tau=tau, interv=interv, layout=layout, hfw_max=hfw_max,
                model_kw=model_kw)


def case_id(c):
    return (f"{c['group']}-{c['model']}-d{c['d']}-N{c['N']}-S{c['S']}-Sa{c['Sa']}-{c['est']}-tau{c['tau']}" + ("-interv" if c["interv"] else "")
            + ("-part" if c["layout"] != "legacy" else "") + (f"-hfw{c['hfw_max']}" if c["hfw_max"] != 112 else "")
            + ("-H" + "x".join(map(str, c["model_kw"]["nn_hidden"])) if c["model"] == "densenn" else "")
            + (f"-{c['family']}-tiny{int(c['tiny'])}" if "tiny" in c else ""))


def _acyc_rows():
    """marginal BGe, score estimator: the acyclicity kernels.  Sa = 4 below 113 variables (two pairs), 2 above."""
    rows = []
    for d in (5, 16, 20, 32, 33, 48, 49, 50, 64, 65, 80, 81, 112, 113, 130):
        for tau in TAUS if d in (20, 50, 80, 112, 130) else TAUS[:1]:
            rows.append(_case("acyc", acyc_family(acyc_kernel(d, 4)), "bge", d, Sa=4 if d <= 112 else 2, tau=tau))
    rows.append(_case("acyc", "k_acyc<unpaired>", "bge", 20, Sa=3))
    rows.append(_case("acyc", "k_acyc<unpaired>", "bge", 20, Sa=4, layout="partitionable"))
    # k_acyc_bfw: not the default anywhere (acyc_kernel) -- the engine is created with acyc_hfw_max = 80
    for d, tau in ((81, 0.7), (112, 0.7), (112, 2.0)):
        rows.append(_case("acyc", "k_acyc_bfw", "bge", d, Sa=4, tau=tau, hfw_max=80))
    return rows


def _bge_rows():
    """marginal BGe off its default prior: the hard-graph tiers of k_bge_chol / k_bge_chol_wide (12, 20, 50, 70, 130), with and without
    interventions (per-node N_j), and the soft-graph kernels (17, 49, 65, 88, 129) with tau = 0.7 on top"""
    rows = [_case("bge", "k_bge_chol" if d <= 112 else "k_bge_chol_wide", "bge", d, S=4 if d <= 70 else 2, interv=iv) for d in (12, 20, 50, 70, 130) for iv in (False, True)]
    for i, d in enumerate((17, 49, 65, 88, 129)):
        iv = i % 2 == 1
        # (5 d / 4 observations: the prior enters R as t I + (N amu / (N + amu)) xbar xbar^T, about 1/2 xbar xbar^T whatever N, beside N
        # observations' scatter -- with 3 d of them bge_alpha_mu moves the gradient W_LIK by 19.7 bounds at 49 variables, short of the 20 asked)
        rows.append(_case("soft", SS.soft_path(d, iv)["kernel"], "bge", d, N=d + d // 4, M=2, S=2, est="reparam", interv=iv))
    return rows


def _lin_rows():
    rows = []
    for d, N, kw in ((8, 20, {}), (50, 100, {}), (8, 20, dict(S=3)), (8, 20, dict(layout="partitionable")), (20, 129, {}), (100, 113, {})):
        for est in ("reparam", "score"):
            c = _case("lin", None, "lingauss", d, N=N, est=est, tau=0.7 if est == "reparam" else 2.0, interv=est == "score", **kw)
            rows.append(dict(c, kernel=A.lin_kernel(d, N, c["S"], c["layout"])))
    return rows


def _nn_rows():
    one = dict(nn_hidden=(5,), nn_activation="tanh", nn_bias=True)
    rows = []
    for d, N, kw in ((20, 40, one), (48, 40, one), (80, 40, one), (12, 30, dict(one, nn_hidden=(6, 4))), (8, 129, one)):
        for est in ("reparam", "score"):
            c = _case("nn", None, "densenn", d, N=N, est=est, tau=0.7 if est == "reparam" else 2.0, interv=est == "score", **kw)
            H = kw["nn_hidden"]
            rows.append(dict(c, kernel=A.nn_logprob_kernel(d, N, H[0], c["S"], est == "reparam") if len(H) == 1 else "general"))
    return rows


ACYC_CASES, BGE_CASES, LIN_CASES, NN_CASES = _acyc_rows(), _bge_rows(), _lin_rows(), _nn_rows()
SOFT_CASES = [c for c in BGE_CASES if c["group"] == "soft"]
ORACLE_CASES = ACYC_CASES + [c for c in BGE_CASES if c["group"] == "bge"] + LIN_CASES + NN_CASES     # against the C oracle
ALL_CASES = ORACLE_CASES + SOFT_CASES
SCORE_D = (12, 20, 50, 70, 130)          # score_graphs on the off-default BGe prior
LIN_SCORE_CASES = ((8, 20), (20, 129), (100, 113))   # joint_lin_score_given: (d, n_ho) on the LDS path, above 128 observations, on the Gram path


# ---- configuration, data, references ----------------------------------------------------------------------------------------------------------
def is_soft(c):
    """a case of the soft-graph BGe kernels: its reference is the torch-autograd oracle"""
    return c["model"] == "bge" and c["est"] == "reparam"


def moved(c):
    """{parameter: off-default value} of a case -- everything the case moves off make_config's defaults"""
    out = dict(COMMON, tau=c["tau"])
    if c["model"] == "bge":
        return dict(out, **bge_prior(c["d"]))
    return dict(out, scale_theta=3.0, **(LIN if c["model"] == "lingauss" else NN))


def config_kwargs(c, **override):
    """make_config's keywords of a case and its bge_mean_obs; override: parameters of `moved` put back (value None / the default)"""
    d = c["d"]
    hp = dict(moved(c), **override)
    mean_obs = hp.pop("mean_obs", None)
    kw = dict(n_vars=d, n_particles=c["M"], n_observations=c["N"], n_grad_mc_samples=c["S"], n_acyclicity_mc_samples=c["Sa"], grad_estimator_z=c["est"],
              rng_layout=c["layout"], has_interventions=bool(c["interv"]), edges_per_node=1 if d <= 5 else 2, **hp, **c["model_kw"])
    if c["model"] != "bge":
        kw.update(joint=True, likelihood=c["model"], score_function_baseline=0.001 if c["est"] == "score" else 0.0)
    return kw, mean_obs


def t_step(c):
    return T_MARGINAL if c["model"] == "bge" else T_JOINT


def data(c):
    """(x, mask): structured observations (obs_axis.structured_x), a 15 % intervention mask where the case has one.  A tiny case whose hit
    is a likelihood draw makes the hit edge i -> j matter: x_j += 1.5 x_i."""
    x = A.structured_x(c["d"], c["N"], seed=5)
    if c.get("draws") == "lik":
        _, (_, _, i, j) = TINY_HITS[c["family"]]
        x = x.copy()
        x[:, j] += 1.5 * x[:, i]
    return x, (A.random_mask(c["d"], c["N"], 0.15) if c["interv"] else None)


def engine_env(c):
    """tuning switches set before the engine of a case is created (tuning.h)"""
    return {} if c["hfw_max"] == 112 else {"DIBS_ACYC_HFW_MAX": str(c["hfw_max"])}


def c_step(oracle, c, **override):
    """one C-oracle step of the case at its t from freshly initialised float32-representable particles of PRNGKey(KEY):
    (state before, debug stages, state after).  override: see config_kwargs."""
    from dibs_amd._abi import make_config
    from oracle import prng
    kw, mean_obs = config_kwargs(c, **override)
    x, mask = data(c)
    before = oracle.new_state(make_config(**kw), prng.PRNGKey(KEY))   # (both oracle builds draw the same float32 values)
    for k in ("z", "theta"):
        if before[k] is not None:
            before[k] = before[k].astype(np.float32).astype(oracle.real)
    after = {k: (None if v is None else v.copy()) for k, v in before.items()}
    dbg = oracle.step(make_config(**kw), x, mask, after, t_step(c), debug=True, mean_obs=mean_obs)
    return before, dbg, after


_BUILT = {}


def built_case(c, oracle64):
    """the float64 C oracle's step of a case: computed once, shared between the tests, never written to"""
    cid = case_id(c)
    if cid not in _BUILT:
        before, dbg, after = c_step(oracle64, c)
        for a in list(before.values()) + list(after.values()) + list(dbg.values()):
            if a is not None:
                a.setflags(write=False)
        kw, mean_obs = config_kwargs(c)
        x, mask = data(c)
        _BUILT[cid] = dict(c, id=cid, cfg_kw=kw, mean_obs=mean_obs, x=x, mask=mask, before=before, dbg=dbg, after=after)
    return _BUILT[cid]


def autograd_step(c, state=None, **override):
    """the soft-graph BGe cases: one step of the torch-autograd oracle (float64) from float32-representable fresh particles of PRNGKey(KEY),
    or from state = (z, key): dict(before: z / v_z / key, logprobs_z, lik_terms, w_lik, grad_z, kxx, phi_z, after: z / key).  lik_terms
    [M, S, d, d]: per sample d log p(soft graph_s) / d scores (oracle.dibs_oracle.likelihood_sample_terms: autograd of the likelihood alone,
    the chain tau alpha g (1 - g) included); w_lik: their sum with the softmax of logprobs_z (soft_w_lik).  A case with `tiny` set draws its
    logistic noise with the lower limit FLT_MIN (logistic_minval_tiny, which the autograd oracle has no switch for)."""
    import torch
    from oracle import dibs_oracle as O, prng
    kw, mean_obs = config_kwargs(c, **override)
    x, mask = data(c)
    d, M = c["d"], c["M"]
    ocfg = O.Config(likelihood="bge", grad_estimator_z="reparam", n_grad_mc_samples=c["S"], n_acyclicity_mc_samples=c["Sa"], tau=kw["tau"],
                    beta_linear=kw.get("beta_linear", 1.0), scale_latent=kw.get("scale_latent", 1.0), rng_layout=c["layout"],
                    prior=O.GraphPrior("er", kw["edges_per_node"]),
                    bge=O.BGeParams(mean_obs=None if mean_obs is None else torch.as_tensor(mean_obs.astype(np.float64)), alpha_mu=kw.get("bge_alpha_mu", 1.0),
                                    alpha_lambd=kw.get("bge_alpha_lambd")))
    st = O.init_state(ocfg, prng.PRNGKey(KEY), M, d)
    st.z = torch.as_tensor(st.z.numpy().astype(np.float32).astype(np.float64))
    if state is not None:
        st.z, st.key = torch.as_tensor(np.asarray(state[0], np.float64)), np.array(state[1], np.uint32)
    xt = torch.as_tensor(x.astype(np.float64))
    it = torch.as_tensor((mask if mask is not None else np.zeros_like(x)).astype(np.float64))
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (thousands of small float64 operations: see large_states.autograd_step)
    logistic = prng.logistic
    if c.get("tiny"):
        prng.logistic = lambda key, shape, layout="legacy": logistic(key, shape, layout, minval=np.float32(1.17549435e-38))
    try:
        st2, aux = O.svgd_step(ocfg, st, xt, it, T_MARGINAL, return_aux=True)
        kz = SS.z_keys(st.key, M, c["layout"])[0]       # the keys svgd_step hands to the Z estimator
        terms = [O.likelihood_sample_terms(ocfg, "reparam", st.z[m], None, T_MARGINAL, kz[m], xt, it) for m in range(M)]
    finally:
        prng.logistic = logistic
        torch.set_num_threads(n_threads)
    lp = np.stack([a["logprobs"].numpy() for a in aux["lik_aux"]])
    assert np.allclose(lp, np.stack([t[0].numpy() for t in terms]), rtol=1e-12, atol=0), "likelihood_sample_terms: not the samples of the step"
    lik_terms = np.stack([t[2][0].numpy() for t in terms])
    return dict(before=dict(z=st.z.numpy(), v_z=st.v_z.numpy(), key=np.array(st.key, np.uint32)),
                logprobs_z=lp, lik_terms=lik_terms, w_lik=soft_w_lik(lik_terms, lp), dz_lik=aux["dz_lik"].numpy(), grad_z=(aux["dz_lik"] + aux["dz_prior"]).numpy(),
                kxx=aux["kxx"].numpy(), phi_z=aux["phi_z"].numpy(), after=dict(z=st2.z.numpy(), key=np.array(st2.key, np.uint32)))


def soft_w_lik(lik_terms, logprobs):
    """W_LIK [M, d, d] of the soft-graph BGe kernels for ANY log-probabilities [M, S]: sum_s softmax(logprobs)_s lik_terms_s.  The GPU
    test hands it the DEVICE's LOGPROBS_Z, as tests/test_gpu_soft_bge.py and tests/test_gpu_grad_weights.py do: two samples a few hundred
    apart in log-probability have weights that the LOGPROBS_Z bound itself lets move, and that error is LOGPROBS_Z's to answer for."""
    w = SS.softmax_weights(np.asarray(logprobs, np.float64).reshape(lik_terms.shape[:2]))
    return np.stack([SS.weighted_sum(lik_terms[m], w[m]) for m in range(lik_terms.shape[0])])


def reference_stages(c, ref_dbg, dev_dbg):
    """the reference's stages as the device's are held against them: a soft-graph BGe case's W_LIK with the device's own weights"""
    return dict(ref_dbg, w_lik=soft_w_lik(ref_dbg["lik_terms"], dev_dbg["logprobs_z"])) if is_soft(c) else ref_dbg


_SOFT = {}


def built_soft_case(c):
    cid = case_id(c)
    if cid not in _SOFT:
        kw, mean_obs = config_kwargs(c)
        x, mask = data(c)
        _SOFT[cid] = dict(c, id=cid, cfg_kw=kw, mean_obs=mean_obs, x=x, mask=mask, ref=autograd_step(c))
    return _SOFT[cid]


# ---- the hard-graph scorers -------------------------------------------------------------------------------------------------------------------
LIN_SCORE_BOUND = 2e-5      # test_score_graphs_along_n_ho (tests/test_gpu_obs_axis.py)


def dags(d, rng):
    """five graphs: the empty one, a complete DAG over a random order, three sparse DAGs"""
    order = rng.permutation(d)
    rank = np.empty(d, int)
    rank[order] = np.arange(d)
    up = rank[:, None] < rank[None, :]                       # i before j
    return np.stack([np.zeros((d, d), np.int32), up.astype(np.int32)] + [(up & (rng.random((d, d)) < p)).astype(np.int32) for p in (0.05, 0.2, 0.5)])


def bge_score_inputs(d, interv):
    """(case, configuration keywords, mean_obs, x, mask, graphs) of score_graphs on the data and prior of the BGe row of that size"""
    case = next(c for c in BGE_CASES if c["d"] == d and c["interv"] == interv and c["group"] == "bge")
    kw, mean_obs = config_kwargs(case)
    return (case, kw, mean_obs) + data(case) + (dags(d, np.random.default_rng(d)),)


def lin_score_inputs(d, n_ho):
    """(configuration keywords, x, mask, graphs, theta [5, d, d]) of joint_lin_score_given.  The log-likelihood of held-out data under
    freshly drawn weights dwarfs the weights' prior (-5e4 against a prior term that mean_edge moves by 1: 1.6e-5 of the score, below the
    bound), so the observations are scaled to a tenth and the weights drawn around mean_edge with a spread of 0.3: the prior of the edges
    present, which is where mean_edge and sig_edge enter, then is a share of the score that the bound resolves"""
    rng = np.random.default_rng(d)
    gs = dags(d, rng)
    th = (LIN["lin_mean_edge"] + 0.3 * rng.normal(size=(5, d, d))).astype(np.float32)
    x = (0.1 * A.structured_x(d, n_ho, seed=5)).astype(np.float32)
    kw = dict(n_vars=d, n_particles=1, n_observations=n_ho, joint=True, likelihood="lingauss", has_interventions=True, **LIN)
    return kw, x, A.random_mask(d, n_ho), gs, th


# ---- logistic_minval_tiny: a draw whose 23 uniform bits are all zero ------------------------------------------------------------------------
# With bits >> 9 == 0 the uniform is its lower limit: 2^-23 (eps = -15.94) by default, FLT_MIN (eps = -87.3) with logistic_minval_tiny.  On
# an edge with alpha s = 16 the soft graph is 0.51 under the one setting and e^-71 under the other.  Eight kernels hold their own copy of
# the limit (`ulo`, the tau == 1 path), the others call rng_logistic: one case per family, tau = 1 where the family has the fast path.
# The key of each case was found on the CPU with oracle/prng.py (`find_tiny_key`: state keys (TINY_K0, n), n = 0, 1, ...; one draw in 2^23
# has no bit set); tests/test_hparam_states_host.py re-derives the hit from the committed key.
TINY_K0 = 0x7E57
TINY_M, TINY_S = 4, 8
TINY_A = 16.0
# family -> kernel it reaches, shape, which draws (`acyc`: the Sa chains of the acyclicity term; `lik`: the S soft graphs of the Z pass)
TINY_FAMILIES = dict(
    k_acyc=dict(model="bge", d=20, est="score", draws="acyc"),
    k_acyc_hf=dict(model="bge", d=50, est="score", draws="acyc"),
    k_acyc_hfw=dict(model="bge", d=80, est="score", draws="acyc"),
    k_acyc_bfw=dict(model="bge", d=96, est="score", draws="acyc", hfw_max=80),
    k_lin_logprobs_hf=dict(model="lingauss", d=40, est="reparam", draws="lik"),
    kernels_nn_f16=dict(model="densenn", d=48, est="reparam", draws="lik", nn_hidden=(5,), nn_activation="tanh", nn_bias=True),
    k_bge_soft_mf=dict(model="bge", d=17, est="reparam", draws="lik"),
)
# found keys: n of (TINY_K0, n), and the hit -- particle m, sample / chain s, edge i -> j
TINY_HITS = dict(k_acyc=(474, (3, 1, 10, 16)), k_acyc_hf=(36, (0, 0, 44, 34)), k_acyc_hfw=(54, (3, 4, 77, 25)), k_acyc_bfw=(4, (3, 7, 55, 74)),
                 k_lin_logprobs_hf=(85, (2, 6, 3, 1)), kernels_nn_f16=(112, (3, 0, 22, 27)), k_bge_soft_mf=(479, (3, 1, 13, 6)))


def tiny_case(name, tiny):
    f = dict(TINY_FAMILIES[name])
    model, d, est, draws = f.pop("model"), f.pop("d"), f.pop("est"), f.pop("draws")
    lik = draws == "lik"
    c = _case("tiny", name, model, d, N=40, M=TINY_M, S=TINY_S if lik else 2, Sa=2 if lik else TINY_S, est=est, tau=1.0, **f)
    return dict(c, draws=draws, tiny=bool(tiny), family=name)


def draw_keys(c, key):
    """per particle, the key its `draws` come from, out of the loop-carry key of the step (svgd.py:226-267 / :673-721; dibs.py:430-431,
    595): the joint models split off the theta estimator's keys first, then the Z estimator's, then the prior's"""
    from oracle import prng
    M, lay = c["M"], c["layout"]
    key = np.asarray(key, np.uint32)
    if c["model"] != "bge":
        key = prng.split(key, M + 1, lay)[0]
    ks = prng.split(key, M + 1, lay)
    if c["draws"] == "lik":
        return np.stack([prng.split(k, 2, lay)[1] for k in ks[1:]])
    return prng.split(ks[0], M + 1, lay)[1:]


def zero_bit_draws(c, key):
    """[(m, s, i, j)] of the draws of the step whose 23 uniform bits are all zero"""
    from oracle import prng
    d, n = c["d"], (c["S"] if c["draws"] == "lik" else c["Sa"]) * c["d"] ** 2
    out = []
    for m, k in enumerate(draw_keys(c, key)):
        for e in np.flatnonzero((prng.random_bits(k, n, c["layout"]) >> np.uint32(9)) == 0):
            out.append((m, int(e) // (d * d), (int(e) // d) % d, int(e) % d))
    return out


def find_tiny_key(name, n_max=20000):
    """the first n for which the state key (TINY_K0, n) gives the case a zero-bits draw on an off-diagonal element"""
    c = tiny_case(name, False)
    for n in range(n_max):
        hits = [h for h in zero_bit_draws(c, (TINY_K0, n)) if h[2] != h[3]]
        if hits:
            return n, hits[0]
    return None


def tiny_state(c, oracle):
    """the state of a tiny case: z[..., 0] = I and z[m, j, i, 1] = the score of edge i -> j (soft_states.py), scores alpha s uniform in
    [-1, 1] but TINY_A on the hit edge of the hit particle; theta freshly initialised; the committed key"""
    from dibs_amd._abi import make_config
    from oracle import prng
    n, (m, s, i, j) = TINY_HITS[c["family"]]
    d, M = c["d"], c["M"]
    kw, _ = tiny_config(c)
    st = oracle.new_state(make_config(**kw), prng.PRNGKey(KEY))
    A_ = np.random.default_rng(d).uniform(-1.0, 1.0, size=(M, d, d))
    A_[m, i, j] = TINY_A
    scores = (A_ / 2.0).astype(np.float32)                      # alpha = 2 at the step index of either model
    z = np.zeros((M, d, d, 2), oracle.real)
    z[..., 0] = np.eye(d)
    z[..., 1] = scores.transpose(0, 2, 1)
    st.update(z=z, v_z=np.zeros_like(z), key=np.array([TINY_K0, n], np.uint32))
    if st["theta"] is not None:
        st["theta"] = st["theta"].astype(np.float32).astype(oracle.real)
    return st


def tiny_config(c):
    kw, mean_obs = config_kwargs(c)
    return dict(kw, logistic_minval_tiny=c["tiny"]), mean_obs


def tiny_step(oracle, c):
    """(state before, debug stages, state after) of one C-oracle step of a tiny case"""
    from dibs_amd._abi import make_config
    kw, mean_obs = tiny_config(c)
    x, mask = data(c)
    before = tiny_state(c, oracle)
    after = {k: (None if v is None else v.copy()) for k, v in before.items()}
    dbg = oracle.step(make_config(**kw), x, mask, after, t_step(c), debug=True, mean_obs=mean_obs)
    return before, dbg, after


def tiny_reference(c, oracle64):
    """(state before, stages, state after) of a tiny case from its reference: the float64 C oracle, or the torch-autograd oracle for the
    soft-graph BGe family (stages logprobs_z / grad_z / kxx / phi_z)"""
    if not (c["model"] == "bge" and c["est"] == "reparam"):
        return tiny_step(oracle64, c)
    st = tiny_state(c, oracle64)
    r = autograd_step(c, state=(st["z"], st["key"]))
    return dict(r["before"], baseline=np.zeros(c["M"])), r, r["after"]


TINY_CASES = [tiny_case(name, tiny) for name in TINY_FAMILIES for tiny in (False, True)]
_TINY = {}


def built_tiny_case(c, oracle64):
    """a tiny case with its reference step: computed once, shared, never written to"""
    cid = case_id(c)
    if cid not in _TINY:
        before, dbg, after = tiny_reference(c, oracle64)
        kw, mean_obs = tiny_config(c)
        x, mask = data(c)
        _TINY[cid] = dict(c, id=cid, cfg_kw=kw, mean_obs=mean_obs, x=x, mask=mask, before=before, dbg=dbg, after=after)
    return _TINY[cid]


def tiny_hit_value(c, dbg):
    """(stage, its value at the hit) -- W_ACYC[m, i, j] for the acyclicity draws, LOGPROBS_Z[m, s] for the likelihood's; relative to the
    stage's largest entry, as the bounds are"""
    _, (m, s, i, j) = TINY_HITS[c["family"]]
    if c["draws"] == "acyc":
        a = np.asarray(dbg["w_acyc"], np.float64).reshape(c["M"], c["d"], c["d"])
        return "W_ACYC", a[m, i, j]
    return "LOGPROBS_Z", np.asarray(dbg["logprobs_z"], np.float64).reshape(c["M"], c["S"])[m, s]


# ---- bounds: the project's own, by stage and size -------------------------------------------------------------------------------------------
STAGE_KEYS = dict(SCORES="scores", NODE_SCORES="node_scores", LOGPROBS_THETA="logprobs_th", LOGPROBS_Z="logprobs_z", GRAD_THETA="grad_theta",
                  W_LIK="w_lik", W_ACYC="w_acyc", GRAD_Z="grad_z", KXX="kxx", PHI_THETA="phi_theta", PHI_Z="phi_z")
# test_marginal_bge_reparam_estimator; LOGPROBS_Z: soft_states.lp_floor; W_LIK: soft_states.W_LIK_MAXNORM (tests/test_gpu_soft_bge.py)
SOFT_BOUNDS = dict(W_LIK=SS.W_LIK_MAXNORM, GRAD_Z=2e-3, PHI_Z=2e-3, KXX=1e-5)
MIN_SHARE = dict(z=0.45, theta=0.35)                      # conftest.assert_update_parity: half of transform_states.SIGNAL_SHARE, rounded down


def bounds(c):
    """stage -> max-norm relative bound: test_marginal_bge_step_stages for the marginal model, obs_axis.BOUNDS / BOUNDS_NN (those of
    test_joint_lingauss_step_stages / test_joint_densenn_step_stages) with W_ACYC, KXX and PHI_Z of the same tests for the joint ones"""
    d = c["d"]
    if is_soft(c):
        return dict(LOGPROBS_Z=SS.lp_floor(d), **SOFT_BOUNDS)
    if c["model"] == "bge":
        return dict(SCORES=2e-6, NODE_SCORES=1e-4 if d <= 50 else (5e-4 if d <= 112 else 1e-3), LOGPROBS_Z=2e-5 if d <= 112 else 5e-5, W_LIK=2e-3,
                    W_ACYC=1e-5, GRAD_Z=1e-4, KXX=1e-5, PHI_Z=1e-4)
    b = A.BOUNDS_NN if c["model"] == "densenn" else A.BOUNDS
    return dict({s: b[s] for s in ("LOGPROBS_THETA", "LOGPROBS_Z", "GRAD_THETA", "W_LIK", "GRAD_Z", "PHI_THETA")}, SCORES=2e-6, W_ACYC=1e-5, KXX=1e-5, PHI_Z=1e-4)


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a[:b.size] - b).max() / max(np.abs(b).max(), 1e-300))


def stage_errors(c, dbg, ref_dbg):
    """max-norm relative error of every stage of bounds(c) of one implementation's debug stages against the reference's"""
    return {s: rel(dbg[STAGE_KEYS[s]], ref_dbg[STAGE_KEYS[s]]) for s in bounds(c)}


def phi_overflows(ref_dbg):
    """test_marginal_bge_step_stages: from about 128 variables on phi^2 of the dense early soft graphs leaves float32 in RMSprop's second
    moment -- the comparison then ends with phi"""
    return 0.1 * float(np.abs(ref_dbg["phi_z"]).max()) ** 2 > 1e38
