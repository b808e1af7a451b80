"""Joint-model states with a KNOWN softmax-weight profile per particle, and the cases the gradient-kernel tests run on them.  A plain
module, imported by the tests like bge_states.py and large_states.py (no fixtures, no pytest hooks).

Every joint step ends in sum_s w_s g_s over the S Monte-Carlo samples of a particle, w = softmax(log-probabilities).  The gradient kernels
(k_lin_grad, k_ling_grad, k_nn_grad, k_nng_grad) differentiate a sample when its float32 weight is at least 2^-30 and deal those samples
round-robin to NS blocks (kernels_joint.h: GradSplit).  A fresh state has one weighted sample per particle, a state with a huge observation
noise has all of them; here the number of samples above the cut -- and how many lie below it, or underflow -- is CHOSEN per particle:

  z      k = d, V = I, U = the score matrix: +-L_SAT on the edges / non-edges of one base DAG G* (alpha L_SAT = 120: their probabilities are
         exactly 1 and 0 in float32, every sample carries G*), and logit(p_r) / alpha on a few FREE edges into distinct child nodes
  theta  the parameters of free edge r are tuned on the float64 oracle so that adding the edge changes log p(theta, D | G) by delta_r.  The
         children are distinct and the likelihood factorises over nodes, so a hard sample with the free edges B has log-probability
         base + sum_{r in B} delta_r EXACTLY: with delta_r = -c 2^r the weights are the geometric ladder exp(-c n), n the number spelt by
         the sample's bits; one edge with delta = -45 puts samples below the cut, one with delta = -160 makes them zero in float32.
  search which bits a sample has follows from the PRNG key and p_r alone (oracle/prng.py reproduces the device's streams bit for bit), so
         c, the p_r and the edge roles are searched on the CPU until the particle has the asked number of samples above the cut, at least
         8 below it that are non-zero, at least 2 that are zero, and none within a factor MARGIN of the cut.  The C oracle's step on the
         finished state has the last word (`profile`): what the tests use is measured there, not simulated.

The theta estimator and the Z estimator draw from different keys: each has its own profile.  The Z score estimator samples hard graphs
too and is searched to its own targets; the Z reparam estimator's soft graphs are continuous (g = sigmoid(logistic + logit p)), its
profile is what the state gives: the search only insists on the margin and on the samples below the cut, and the class is read off the
oracle's step like every other.  The `straddle` profile instead places two free edges AT the cut: samples with just one of them weigh 1.25 x and 1 / 1.25 x 2^-30.

tests/test_weight_states_host.py asserts all of this on the oracles alone; tests/test_gpu_grad_weights.py and the chains modules run the
states on the device."""
import numpy as np

CUT = 2.0 ** -30          # GRAD_W_MIN (kernels_joint.h)
MARGIN = 4.0              # outside the straddle profile no weight lies within this factor of the cut (at least: margin_for)
T_STEP = 400              # alpha = alpha_linear t = 0.05 * 400 = 20
L_SAT = 6.0
D_BELOW, D_ZERO = -45.0, -160.0
CLASSES = ("1", "2", "mid", "ns", "ns+1", "many", "flat")


def classify(nnz, S, ns):
    """the class of a participation count (`between`: ns + 2 .. 2 ns, asked for by no case)"""
    if nnz == S:
        return "flat"
    if nnz <= 2:
        return str(nnz)
    if nnz < ns:
        return "mid"
    if nnz == ns:
        return "ns"
    if nnz == ns + 1:
        return "ns+1"
    return "many" if nnz > 2 * ns else "between"


def weights32(logprobs):
    """float32 softmax weights of log-probabilities [..., S], evaluated in float64 as the kernels do (grad_softmax_stats)"""
    lp = np.asarray(logprobs, np.float64)
    w = np.exp(lp - lp.max(-1, keepdims=True))
    return (w / w.sum(-1, keepdims=True)).astype(np.float32)


def margin_for(max_abs_logprob):
    """the factor around the cut that a case keeps free of weights: MARGIN, or more where the 2e-5 (max-norm relative) bound of the
    LOGPROBS stage is more than that in the weights -- two log-probabilities may each move by the bound"""
    return max(MARGIN, float(np.exp(2 * 2e-5 * max_abs_logprob)))


def weight_stats(w, margin=MARGIN):
    """what the tests ask of one particle's weights [S]"""
    w = np.asarray(w, np.float32)
    near = (w > 0) & (w >= np.float32(CUT / margin)) & (w < np.float32(CUT * margin))
    return dict(nnz=int((w >= np.float32(CUT)).sum()), below=int(((w > 0) & (w < np.float32(CUT))).sum()), zero=int((w == 0).sum()),
                near=int(near.sum()), above_close=int(((w > np.float32(CUT)) & (w <= np.float32(1.5 * CUT))).sum()),
                below_close=int(((w >= np.float32(CUT / 1.5)) & (w < np.float32(CUT))).sum()))


def _ok(st, S, ns, target):
    """does a particle's weight statistics meet `target` (a class, `straddle`, or None: any class) and the conditions every profile has"""
    if target == "straddle":
        return st["above_close"] >= 2 and st["below_close"] >= 2 and st["below"] >= 8 and st["zero"] >= 2
    if st["near"]:
        return False
    if st["nnz"] < S and (st["below"] < 8 or st["zero"] < 2):
        return False
    return target is None or classify(st["nnz"], S, ns) in ((target,) if isinstance(target, str) else target)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _case(kernel, model, d, S, est, th, z=None, *, M=None, N=40, interv=None, gram=False, ns=8, seed=0, key_seed=0, z_margin=True, z_free=False, **model_kw):
    """th / z: what is asked of every particle's theta / Z estimator -- a class, a tuple of admissible classes, or None: what the state
    gives (z = None: that for every particle).  z_margin=False: the Z estimator's weights may lie near the cut (see GRAD_CASES); z_free: nothing at all is asked of the Z profile"""
    M = M or len(th)
    z = (None,) * M if z is None else z
    assert len(th) == M and len(z) == M
    return dict(kernel=kernel, model=model, d=d, S=S, est=est, t_th=tuple(th), t_z=tuple(z), M=M, N=N, interv=interv,
                gram=gram, ns=ns, seed=seed, key_seed=key_seed, z_margin=z_margin, z_free=z_free, model_kw=model_kw)


def case_id(c):
    return (f"{c['kernel']}-{c['model']}-d{c['d']}-S{c['S']}-M{c['M']}-N{c['N']}-{c['est']}" + ("-interv" if c["interv"] else "")
            + ("-gram" if c["gram"] else "") + (f"-s{c['seed']}" if c["seed"] else "") + (f"-k{c['key_seed']}" if c["key_seed"] else "")
            + (f"-a{c['model_kw']['alpha_linear']}" if "alpha_linear" in c["model_kw"] else ""))


_SIX = ("1", "2", "mid", "ns", "ns+1", "many")
_SIX_Z = ("2", "1", "mid", "ns+1", "ns", "many")         # for the Z score estimator: another class where the same ladder can give one
_SIX_B = ("flat", "straddle", "mid", "ns", "many", "2")
_SIX_BZ = ("flat", None, "mid", "ns+1", "many", "1")     # (beside the theta straddle the Z estimator's weights sit near the cut too: nothing asked)
_SIX_NN = ("1", "2", "mid", "ns", "ns+1", "mid")         # (reparam with NS = 16: soft graphs crowd the cut when > 32 of 64 samples are kept in theta)
_ABOVE = ("ns+1", "between", "many")
NN5 = dict(nn_hidden=(5,), nn_sig_param=0.4)              # sig_param 0.4: log N(0; 0.4) = -0.003, a weight row near zero costs nothing
GRAD_CASES = (
    # k_lin_grad (GRAD_NS = 8)
    _case("k_lin_grad", "lingauss", 8, 64, "reparam", _SIX),
    _case("k_lin_grad", "lingauss", 8, 64, "score", _SIX_B, _SIX_BZ),
    _case("k_lin_grad", "lingauss", 20, 64, "reparam", _SIX_B, interv=0.1),
    _case("k_lin_grad", "lingauss", 20, 64, "score", _SIX, _SIX_Z, interv=0.1),
    _case("k_lin_grad", "lingauss", 50, 48, "reparam", _SIX),
    _case("k_lin_grad", "lingauss", 50, 48, "score", _SIX_B, _SIX_BZ),
    _case("k_lin_grad", "lingauss", 72, 24, "reparam", ("1", "mid", "ns+1")),      # two row tiles per wave; S = 24: at most 14 above the cut
    _case("k_lin_grad", "lingauss", 72, 24, "score", ("2", "ns", "straddle"), ("1", "ns+1", None)),
    # a full GRAD_WCH chunk.  (256 soft-graph samples spread over ~60 units of log-weight do not leave a window of 2 log 4 around the cut
    #  empty in any state the search has seen: the reparam Z profile of this case is taken with weights near the cut, and the GPU test
    #  takes its membership from the device's log-probabilities as everywhere)
    _case("k_lin_grad", "lingauss", 8, 256, "reparam", _SIX_B, z_margin=False),
    _case("k_lin_grad", "lingauss", 8, 256, "score", _SIX, _SIX_Z),
    # k_ling_grad: the Gram path, forced (the sizes fit the LDS-resident kernels)
    _case("k_ling_grad", "lingauss", 8, 64, "reparam", _SIX_B, gram=True),
    _case("k_ling_grad", "lingauss", 8, 64, "score", _SIX, _SIX_Z, gram=True),
    _case("k_ling_grad", "lingauss", 20, 64, "reparam", _SIX, gram=True),
    _case("k_ling_grad", "lingauss", 20, 64, "score", _SIX_B, _SIX_BZ, gram=True),
    _case("k_ling_grad", "lingauss", 8, 64, "reparam", _SIX, N=300, gram=True),
    # (N = 300: a flat ladder would put the free edges at the parabola's vertex, where x_i^T r_j cancels -- flat is asked at N = 40)
    _case("k_ling_grad", "lingauss", 8, 64, "score", ("1",) + _SIX_B[1:], ("2",) + _SIX_BZ[1:], N=300, gram=True, interv=0.1),
    # k_nn_grad (GRAD_NS_NN = 16: `many` is more than 32 samples)
    _case("k_nn_grad", "densenn", 8, 64, "reparam", _SIX_NN, ns=16, nn_activation="relu", nn_bias=True, **NN5),
    _case("k_nn_grad", "densenn", 8, 64, "score", _SIX_B, _SIX_BZ, ns=16, nn_activation="relu", nn_bias=True, **NN5),
    _case("k_nn_grad", "densenn", 20, 48, "reparam", _SIX_NN, ns=16, interv=0.1, nn_activation="tanh", nn_bias=False, **NN5),
    # (S = 48: more than 2 NS = 32 above the cut beside 8 below and 2 zeros leaves 5 counts -- `many` is asked at S = 64 only)
    _case("k_nn_grad", "densenn", 20, 48, "score", _SIX[:5] + (("between", "many"),), _SIX_Z[:5] + (("between", "many"),), ns=16, interv=0.1,
          nn_activation="tanh", nn_bias=False, **NN5),
    _case("k_nn_grad", "densenn", 100, 24, "score", ("2", "mid"), ("1", "mid"), N=100, ns=16, nn_activation="relu", nn_bias=True, **NN5),   # the 8-wave instantiation
    # (reparam at this size: no state the search has seen keeps the soft-graph weights out of the margin -- e^5.8 at max |log p| = 1.5e5 --
    #  so the Z profile is taken without it, membership from the device as at S = 256)
    _case("k_nn_grad", "densenn", 100, 24, "reparam", ("2", "mid"), N=100, ns=16, z_margin=False, nn_activation="relu", nn_bias=True, **NN5),
    # more (particle, share) items than resident blocks: every sample of 40 particles weighted, 640 items -- a persistent block walks several
    # and stages x again after a theta item has borrowed its LDS (tests/test_gpu_grad_weights.py checks the count against the device).
    # The reparam engine is there for its theta pass (flat whatever Z does): the soft graphs of 40 flat particles leave some Z profiles with
    # one to seven weights below the cut, neither flat nor with the eight every other profile has -- nothing is asked of them (z_free).
    _case("k_nn_grad", "densenn", 8, 32, "reparam", ("flat",) * 40, ns=16, z_margin=False, z_free=True, nn_activation="relu", nn_bias=True, **NN5),
    _case("k_nn_grad", "densenn", 8, 32, "score", ("flat",) * 40, ("flat",) * 40, ns=16, nn_activation="relu", nn_bias=True, **NN5),
    # k_nng_grad: two hidden layers, the general stack (GRAD_NS = 8)
    _case("k_nng_grad", "densenn", 12, 40, "reparam", _SIX_B, nn_hidden=(6, 4), nn_sig_param=0.4),
    _case("k_nng_grad", "densenn", 12, 40, "score", _SIX, _SIX_Z, nn_hidden=(6, 4), nn_sig_param=0.4),
)
# The chains engines (C = 3 chains of M = 4 in one launch): chain 0 has one weighted sample everywhere, chain 1 two .. NS - 1, chain 2 more
# than NS.  A chain draws from its OWN key (split(key_c, M + 1)), so every chain is a state of its own: one data set and base graph (seed),
# three keys (key_seed).  The reparam Z estimator takes what the state gives.
_CH_TH = (("1",) * 4, ("2", "mid", "mid", "2"), ("ns+1", "many", "many", "ns+1"))
_CH_Z = (("1",) * 4, (("2", "mid"),) * 4, (_ABOVE,) * 4)


def _chain(model, d, S, est, above=_CH_TH[2], **kw):
    th = _CH_TH[:2] + (above,)
    return tuple(_case("chains", model, d, S, est, th[c], _CH_Z[c] if est == "score" else None, seed=1, key_seed=c, **kw) for c in range(3))


def _chain_data(above=_CH_TH[2], interv=(None, None, None), **kw):
    """three chains with a data set each (seed), LinearGaussian score engines"""
    th = _CH_TH[:2] + (above,)
    return tuple(_case("chains", "lingauss", 8, 64, "score", th[c], _CH_Z[c], seed=1 + c, interv=interv[c], **kw) for c in range(3))


CHAIN_CASES = dict(
    lingauss_reparam=_chain("lingauss", 8, 64, "reparam"),
    lingauss_score=_chain("lingauss", 8, 64, "score"),
    densenn=_chain("densenn", 8, 64, "score", ns=16, nn_activation="relu", nn_bias=True, **NN5),
    densenn_deep=_chain("densenn", 12, 40, "score", nn_hidden=(6, 4), nn_sig_param=0.4),
    # per-chain data (sample_joint_batch): a data set per chain, chain 1 with interventions
    data_lingauss=_chain_data(interv=(None, 0.1, None)),
    # ... and the Gram path at N = 300 (forced: d = 8 fits the LDS-resident kernels).  The small rungs of a `many` ladder lie above the
    # vertex of the free edges' parabolas at N = 300: chain 2 is asked for any count above NS
    data_gram_n300=_chain_data(above=(_ABOVE,) * 4, N=300, gram=True),
)
# per-chain hyper-parameters (sample_joint_sweep): shared data, alpha_linear and h_theta of chain c.  alpha enters the edge probabilities, so
# every chain's state is built with its own (alpha L_SAT >= 120 still saturates G*); h_theta only enters the kernel matrix.
SWEEP_HPS = (dict(alpha_linear=0.05, h_theta=500.0), dict(alpha_linear=0.06, h_theta=200.0), dict(alpha_linear=0.08, h_theta=50.0))
CHAIN_CASES["sweep_lingauss"] = tuple(
    _case("chains", "lingauss", 8, 64, "score", _CH_TH[c], _CH_Z[c], seed=1, key_seed=c, **SWEEP_HPS[c]) for c in range(3))


# ---- construction -----------------------------------------------------------------------------------------------------------------------
def _base_dag(d, rng):
    """G*: nodes in topological order, one or two parents for every node from 2 on (node 1 keeps 0 -> 1 for a free edge)"""
    g = np.zeros((d, d), np.int32)
    for j in range(2, d):
        for i in rng.choice(j, size=1 + int(j >= 3 and rng.random() < 0.5), replace=False):
            g[i, j] = 1
    return g


def _free_edges(g, rng, k_max=7):
    """up to k_max edges (i, j), i < j, absent from G*, into DISTINCT children"""
    d = g.shape[0]
    out = []
    for j in rng.permutation(np.arange(1, d)):
        cand = [i for i in range(j) if not g[i, j]]
        if cand and len(out) < k_max:
            out.append((int(rng.choice(cand)), int(j)))
    return out


def _data(c, rng):
    d, N = c["d"], c["N"]
    x = rng.normal(size=(N, d)).astype(np.float32)
    w = np.triu((rng.random((d, d)) < 2.0 / d) * rng.normal(size=(d, d)), 1)
    for j in range(d):   # some structure: upper-triangular linear mechanism
        x[:, j] += (x[:, :j] @ w[:j, j]).astype(np.float32)
    mask = (rng.random((N, d)) < c["interv"]).astype(np.int32) if c["interv"] else None
    return x, mask


def _edge_uniforms(ocfg, keys, est, S, d, edges):
    """[M, S, K] the uniforms that decide the free edges' bits in a hard-graph estimator (theta: the particle key itself; score: subk_)"""
    from oracle import prng
    ii, jj = [e[0] for e in edges], [e[1] for e in edges]
    out = []
    for k in keys:
        if est != "theta":
            k = prng.split(k, 2, ocfg.rng_layout)[1]
        out.append(prng.uniform(k, (S, d, d), layout=ocfg.rng_layout)[:, ii, jj])
    return np.stack(out)


def _p32(score32, alpha):
    """the float32 edge probability both oracles compare the uniforms with"""
    return np.float32(1.0 / (1.0 + np.exp(-np.float64(alpha) * np.float64(score32))))


def _candidates(rng, K, target):
    """(delta [K], p [K]) proposals for a particle with K free edges"""
    if target == "flat":
        while True:
            c = float(np.exp(rng.uniform(np.log(0.01), np.log(0.05))))
            yield -c * 2.0 ** np.arange(K), rng.choice([0.3, 0.5, 0.7], K)
    while True:
        kl = K - 2                                              # ladder edges; then the `below` and the `zero` edge
        c = float(np.exp(rng.uniform(np.log(0.05), np.log(30.0))))
        delta = np.concatenate([-c * 2.0 ** np.arange(kl), [D_BELOW, D_ZERO]])
        p = np.concatenate([rng.choice([0.2, 0.35, 0.5, 0.65, 0.8], kl), rng.choice([0.08, 0.15, 0.25], 2)])
        if target == "straddle":                                # the first two ladder edges sit AT the cut instead (set in `_simulate`)
            delta[:2] = np.nan
            p[:2] = 0.3
        yield delta, p


def _simulate(u, delta, p32):
    """log-weights [S] of a hard-graph estimator whose free-edge uniforms are u [S, K]; a straddle proposal (delta[:2] NaN) is completed:
    a sample with only edge 0 weighs 1.25 CUT, with only edge 1 CUT / 1.25 (the normaliser is the number of samples with no free edge)"""
    bits = u < p32[None, :]
    delta = delta.copy()
    if np.isnan(delta[0]):
        n0 = max(int((~bits.any(1)).sum()), 1)
        delta[0], delta[1] = np.log(1.25 * CUT * n0), np.log(CUT * n0 / 1.25)
    return bits @ delta, delta


def lin_edge_ratio(x, mask, g1, theta, edge):
    """LinearGaussian, graph g1 with the free edge (i, j): |x_i^T r_j| / (|x_i| |r_j|) over the observations that count for node j, r_j the
    node's residual -- the free edge's gradient is -theta + x_i^T r_j / obs_noise, and a float32 x_i^T r_j is exact to ~1e-6 |x_i| |r_j|"""
    (i, j), d = edge, x.shape[1]
    x = np.asarray(x, np.float64)
    keep = np.ones(len(x), bool) if mask is None else np.asarray(mask)[:, j] == 0
    r = (x[:, j] - x @ (g1 * np.asarray(theta, np.float64).reshape(d, d))[:, j])[keep]
    return float(abs(x[keep, i] @ r) / (np.linalg.norm(x[keep, i]) * np.linalg.norm(r)))


def _tune(oracle, cfg1, kw, c, x, mask, g0, lp0, edge, theta, target, flat):
    """set the parameters of free edge (i, j) in theta [P] (in place, float32 values) so that log p(G* + edge) - log p(G*) = target; lp0 =
    log p(G*), which the edge's parameters do not enter.  Returns the delta reached (None: out of reach).  flat: a target above the
    parabola's vertex is moved to 0.3 below it (still flat, and the edge's gradient stays away from its zero at the vertex)."""
    d, (i, j) = c["d"], edge
    g1 = g0.copy()
    g1[i, j] = 1

    def delta(th):
        return float(oracle.score_graphs(cfg1, x, mask, g1[None], th[None])[0] - lp0)

    if c["model"] == "lingauss":   # delta is the parabola a v^2 + b v + c0 in v = theta[i, j]: three evaluations, the root on one side
        e = i * d + j
        vals = []
        for v in (0.0, 1.0, -1.0):
            theta[e] = v
            vals.append(delta(theta))
        c0, a, b = vals[0], 0.5 * (vals[1] + vals[2]) - vals[0], 0.5 * (vals[1] - vals[2])
        for shift in (0.3, 0.6, 1.2, 2.4) if flat else (0.0,):
            tgt = min(target, c0 - b * b / (4 * a) - shift) if flat else target
            disc = b * b - 4 * a * (c0 - tgt)
            if not (a < 0 and disc > 0):
                return None
            roots = ((-b - np.sqrt(disc)) / (2 * a), (-b + np.sqrt(disc)) / (2 * a))
            theta[e] = np.float32(min(roots, key=abs))   # (the root nearer 0: between 0 and the vertex for a target above delta(0))
            if lin_edge_ratio(x, mask, g1, theta, edge) >= 2e-2:
                break
        else:
            return None
    else:                          # DenseNN: the scale of the row W1[j, i, :] (theta leaf 0 is [d, d, H1]); bisection from 0 outwards
        H = c["model_kw"]["nn_hidden"][0]
        sl = slice((j * d + i) * H, (j * d + i + 1) * H)
        rng = np.random.default_rng([i, j, int(abs(target) * 1000)])
        for attempt in range(20):   # (another direction when a hidden unit's x_i^T dpre is a cancellation: nn_edge_ratios)
            row = theta[sl].copy() if attempt == 0 else rng.standard_normal(H)
            row /= np.abs(row).max()

            def f(lam):
                theta[sl] = (lam * row).astype(np.float32)
                return delta(theta) - target

            if f(0.0) <= 0:
                return None
            hi = 0.25
            while f(hi) > 0:
                hi *= 2
                if hi > 1e3:
                    return None
            lo = 0.0
            for _ in range(24):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
            f(lo)
            if nn_edge_ratios(kw, x, mask, g1, theta, edge).min(initial=1.0) >= 2e-2:
                break
        else:
            return None
    return delta(theta)


_BUILT = {}


def build(c, oracle):
    """The state of a case: a dict with cfg_kw, x, mask, z, theta, key, t, the base graph `g0`, the free edges and, from the C oracle's
    step on the finished state, `profile` = dict(theta=[per-particle weight_stats], z=[...]) and the oracle's stages `dbg`.  `oracle`: the
    float64 COracle.  Arrays are shared between callers and read-only."""
    from dibs_amd._abi import make_config
    from oracle import dibs_oracle as O, prng
    cid = case_id(c)
    if cid in _BUILT:
        return _BUILT[cid]
    d, S, M, ns = c["d"], c["S"], c["M"], c["ns"]
    rng = np.random.default_rng(1000 * d + S + 7 * c["seed"])
    x, mask = _data(c, rng)
    kw = dict(n_vars=d, n_particles=M, n_observations=c["N"], n_grad_mc_samples=S, n_acyclicity_mc_samples=2, joint=True,
              likelihood=c["model"], grad_estimator_z=c["est"], has_interventions=mask is not None, **c["model_kw"])
    cfg = make_config(**kw)
    cfg1 = make_config(**dict(kw, n_particles=1))
    alpha = cfg.alpha_linear * T_STEP
    st = oracle.new_state(cfg, prng.PRNGKey(11 + c["seed"] + 100 * c["key_seed"]))
    theta = np.asarray(st["theta"], np.float32).astype(np.float64)
    key = np.array(st["key"], np.uint32)
    g0 = _base_dag(d, rng)
    edges = _free_edges(g0, rng)
    K = len(edges)
    assert K >= 5, K
    ocfg = O.Config(joint=True, likelihood=c["model"])
    kth, kz = O.estimator_keys(ocfg, key, M)
    u_th = _edge_uniforms(ocfg, kth, "theta", S, d, edges)
    u_z = _edge_uniforms(ocfg, kz, "score", S, d, edges) if c["est"] == "score" else None
    score = np.where(g0 != 0, L_SAT, -L_SAT).astype(np.float32)
    np.fill_diagonal(score, 0.0)
    z = np.zeros((M, d, d, 2), np.float64)
    z[..., 1] = np.eye(d)
    z[..., 0] = score
    lp0 = oracle.score_graphs(cfg1, x, mask, np.repeat(g0[None], M, 0), theta)   # (the free edges' parameters do not enter)
    margin = margin_for(np.abs(lp0).max())
    gens = [_candidates(np.random.default_rng([d, S, m, c["seed"]] + ([c["key_seed"]] if c["key_seed"] else [])), K, c["t_th"][m]) for m in range(M)]
    deltas = np.zeros((M, K))
    todo, rounds, prof, dbg, tunes = list(range(M)), 0, None, None, 0

    def _ok_z(stz, m):   # (beside a theta straddle the Z estimator's weights sit near the cut too: no margin asked there)
        if c["z_free"]:
            return True
        if c["t_th"][m] == "straddle" or not c["z_margin"]:
            return stz["nnz"] == S or (stz["below"] >= 8 and stz["zero"] >= 2)
        return _ok(stz, S, ns, c["t_z"][m])

    while todo:
        rounds += 1
        assert rounds <= (300 if d <= 20 else 40), (cid, todo)
        for m in todo:
            for trial in range(200000):
                delta, p = next(gens[m])
                sc32 = (np.log(p / (1 - p)) / alpha).astype(np.float32)
                p32 = _p32(sc32, alpha)
                lw, delta = _simulate(u_th[m], delta, p32)
                if not _ok(weight_stats(weights32(lw), margin), S, ns, c["t_th"][m]):
                    continue
                if u_z is not None:
                    lwz, _ = _simulate(u_z[m], delta, p32)
                    if not _ok_z(weight_stats(weights32(lwz), margin), m):
                        continue
                th_m, flat = theta[m].copy(), c["t_th"][m] == "flat"
                tunes += 1
                assert tunes <= 400 * M, (cid, m, "the free edges cannot be tuned")
                got = [_tune(oracle, cfg1, kw, c, x, mask, g0, lp0[m], edges[r], th_m, delta[r], flat) for r in range(K)]
                if any(v is None or (abs(v - t_) > 1e-3 and not flat) for v, t_ in zip(got, delta)):
                    continue
                theta[m], deltas[m] = th_m, got
                for r, (i, j) in enumerate(edges):
                    z[m, i, j, 0] = sc32[r]
                break
            else:
                raise AssertionError((cid, m, "no candidate"))
        # the last word: the oracle's own step on the state
        stt = dict(z=z.copy(), v_z=np.zeros_like(z), theta=theta.copy(), v_theta=np.zeros_like(theta), key=key.copy(), baseline=np.zeros(M))
        dbg = oracle.step(cfg, x, mask, stt, T_STEP, debug=True)
        margin = margin_for(max(np.abs(dbg["logprobs_th"]).max(), np.abs(dbg["logprobs_z"]).max()))
        prof = dict(theta=[weight_stats(w, margin) for w in weights32(dbg["logprobs_th"])],
                    z=[weight_stats(w, margin) for w in weights32(dbg["logprobs_z"])])
        todo = []
        for m in range(M):
            if not (_ok(prof["theta"][m], S, ns, c["t_th"][m]) and _ok_z(prof["z"][m], m)):
                todo.append(m)
    out = dict(c, id=cid, cfg_kw=kw, x=x, mask=mask, z=z.astype(np.float32).astype(np.float64), theta=theta, key=key, t=T_STEP, g0=g0,
               edges=tuple(edges), deltas=deltas, profile=prof, margin=margin, dbg=dbg, after=stt, rounds=rounds)
    assert np.array_equal(out["z"], z)
    for a in (x, mask, out["z"], theta, key, g0, deltas):
        if a is not None:
            a.setflags(write=False)
    _BUILT[cid] = out
    return out


def fresh_state(b, rows=None):
    """the keyword arguments of Engine.set_state for the rows `rows` (default: all) of a built case"""
    r = slice(None) if rows is None else rows
    z, th = np.array(b["z"][r], np.float32), np.array(b["theta"][r], np.float32)
    return dict(z=z, v_z=np.zeros_like(z), theta=th, v_theta=np.zeros_like(th), key=b["key"].copy(), baseline=np.zeros(len(z), np.float32))


# ---- the reference that takes the weights as given -----------------------------------------------------------------------------------------
W_REF_MIN = 1e-20   # samples below this float64 weight are left out of the reference: eleven orders below the cut, they move no figure here


def oracle_config(b):
    """the autograd oracle's Config of a built case"""
    from oracle import dibs_oracle as O
    kw = b["cfg_kw"]
    nn = O.DenseNNParams(hidden_layers=tuple(kw.get("nn_hidden", (5,))), sig_param=kw.get("nn_sig_param", 1.0),
                         activation=kw.get("nn_activation", "relu"), bias=kw.get("nn_bias", True))
    return O.Config(joint=True, likelihood=b["model"], alpha_linear=kw.get("alpha_linear", 0.05), grad_estimator_z=b["est"], n_grad_mc_samples=b["S"], nn=nn)


def theta_leaves(b, m):
    """particle m's theta as the autograd oracle's list of leaves (the flat row is their concatenation)"""
    return _leaves(b["model"], b["d"], b["cfg_kw"], b["theta"][m])


def nn_edge_ratios(kw, x, mask, g1, theta, edge):
    """DenseNN, graph g1 with the free edge (i, j): the gradient of W1[j, i, h] is -W / sig^2 + x_i^T dpre_h, dpre the back-propagated signal at node
    j's first pre-activations.  Returns |x_i^T dpre_h| / (|x_i| |dpre_h|) for the hidden units h with a signal (a unit that relu switches
    off for every observation has none: its gradient is the prior's alone) -- what |x_i^T r_j| / (|x_i| |r_j|) is for LinearGaussian."""
    import torch
    from oracle import dibs_oracle as O
    (i, j), d = edge, x.shape[1]
    leaves = _leaves("densenn", d, kw, theta)
    stride = 2 if kw.get("nn_bias", True) else 1
    act = O._ACT[kw.get("nn_activation", "relu")]
    xt = torch.as_tensor(np.asarray(x, np.float64))
    pre = (xt * torch.as_tensor(np.asarray(g1[:, j], np.float64))) @ leaves[0][j]
    if stride == 2:
        pre = pre + leaves[1][j]
    pre.requires_grad_(True)
    h = pre
    for li in range(1, len(leaves) // stride):
        h = act(h) @ leaves[li * stride][j]
        if stride == 2:
            h = h + leaves[li * stride + 1][j]
    ll = -0.5 * (xt[:, j] - h[:, 0]) ** 2 / kw.get("nn_obs_noise", 0.1)
    if mask is not None:
        ll = ll * torch.as_tensor(1.0 - np.asarray(mask[:, j], np.float64))
    (dpre,) = torch.autograd.grad(ll.sum(), pre)
    dpre, xi = dpre.numpy(), np.asarray(x[:, i], np.float64)
    nrm = np.linalg.norm(dpre, axis=0)
    on = nrm > 0
    return np.abs(xi @ dpre[:, on]) / (np.linalg.norm(xi) * nrm[on])


def _leaves(model, d, kw, th):
    import torch
    th = np.asarray(th)
    if model == "lingauss":
        return [torch.as_tensor(th.reshape(d, d).copy())]
    sizes = [d] + list(kw["nn_hidden"]) + [1]
    out, o = [], 0
    for li in range(len(sizes) - 1):
        shapes = [(d, sizes[li], sizes[li + 1])] + ([(d, sizes[li + 1])] if kw.get("nn_bias", True) else [])
        for shp in shapes:
            n = int(np.prod(shp))
            out.append(torch.as_tensor(th[o:o + n].reshape(shp).copy()))
            o += n
    assert o == th.size
    return out


def sample_terms(b):
    """Per estimator ('theta', 'z') and particle: (samples, terms [n, P or d d]) -- the per-sample terms g_s of the autograd oracle
    (likelihood_sample_terms) for every sample whose ORACLE weight is at least W_REF_MIN, flattened like GRAD_THETA / W_LIK.  Computed once
    per case and shared; which of them are kept, and with which weights, is the caller's business."""
    import torch
    from oracle import dibs_oracle as O
    if "terms" in b:
        return b["terms"]
    ocfg = oracle_config(b)
    kth, kz = O.estimator_keys(ocfg, b["key"], b["M"])
    x = torch.as_tensor(np.asarray(b["x"], np.float64))
    it = torch.zeros_like(x) if b["mask"] is None else torch.as_tensor(np.asarray(b["mask"], np.float64))
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (thousands of tiny float64 operations: a thread pool only waits for its slowest thread)
    try:
        out = dict(theta=[], z=[])
        for name, mode, keys, lps in (("theta", "theta", kth, b["dbg"]["logprobs_th"]), ("z", b["est"], kz, b["dbg"]["logprobs_z"])):
            for m in range(b["M"]):
                lp = np.asarray(lps[m], np.float64)
                w = np.exp(lp - lp.max())
                idx = np.flatnonzero(w / w.sum() >= W_REF_MIN)
                zt = torch.as_tensor(np.array(b["z"][m]))
                lp_o, _, terms = O.likelihood_sample_terms(ocfg, mode, zt, theta_leaves(b, m), b["t"], keys[m], x, it, samples=idx)
                # both oracles drew the same samples (a differing free-edge bit moves a log-probability by a rung of the ladder; the soft graphs
                # of the two agree to the last place of the float32 logistic, 1e-9 of the log-probability)
                assert np.abs(lp_o.numpy() - lp).max() <= 1e-8 * np.abs(lp).max(), (b["id"], name, m)
                out[name].append((idx, np.concatenate([tl.numpy().reshape(len(idx), -1) for tl in terms], axis=1)))
    finally:
        torch.set_num_threads(n_threads)
    b["terms"] = out
    return out


def free_coords(b, name):
    """flat indices into GRAD_THETA (name 'theta') / W_LIK ('z') of the free edges' coordinates"""
    d = b["d"]
    if name == "z" or b["model"] == "lingauss":
        return np.array([i * d + j for i, j in b["edges"]])
    H = b["cfg_kw"]["nn_hidden"][0]
    return np.concatenate([np.arange((j * d + i) * H, (j * d + i + 1) * H) for i, j in b["edges"]])


def weighted_sums(b, name, m, w32):
    """For particle m of estimator `name` and float32 weights w32 [S] (the caller's: the softmax of the DEVICE's log-probabilities):
    dict(kept = sum over w >= CUT of w_s g_s, abs = the same of w_s |g_s|, dropped = sum over 0 < w < CUT, nnz).  float64, sample order."""
    idx, g = sample_terms(b)[name][m]
    w = np.asarray(w32, np.float64)[idx]
    keep = np.asarray(w32, np.float32)[idx] >= np.float32(CUT)
    missing = np.setdiff1d(np.flatnonzero(np.asarray(w32, np.float32) >= np.float32(CUT)), idx)
    assert missing.size == 0, (b["id"], name, m, missing)   # a kept sample the reference left out: the device's weights are elsewhere
    return dict(kept=(w[keep, None] * g[keep]).sum(0), abs=(w[keep, None] * np.abs(g[keep])).sum(0),
                dropped=(w[~keep, None] * g[~keep]).sum(0), nnz=int(keep.sum()))


# ---- the chains engines on these states ---------------------------------------------------------------------------------------------------
def chains_run(bs, per_chain_data=False, hps=None):
    """One engine holding the built states bs (a chains engine for several, chain c = bs[c]; a standalone engine for one), set with
    set_state / the chains' keys: (GRAD_THETA, W_LIK after run(t, 1); the state after three further steps).  per_chain_data: every chain's
    own data set through set_data_problem; hps[c]: chain c's per-chain values (the standalone engine has them in its configuration)."""
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    C, M, t = len(bs), bs[0]["M"], bs[0]["t"]
    names = ("z", "v_z", "theta", "v_theta", "baseline")
    kw = dict(bs[0]["cfg_kw"])
    if C > 1:
        kw.update(n_chains=C, has_interventions=any(b["mask"] is not None for b in bs))
        for f in (hps[0] if hps else ()):
            kw.pop(f, None)
    e = Engine(make_config(**kw))
    try:
        states = [fresh_state(b) for b in bs]
        if C == 1:
            e.set_data(bs[0]["x"], bs[0]["mask"])
            e.set_state(**states[0])
        else:
            if per_chain_data or hps:
                for c, b in enumerate(bs):
                    e.set_data_problem(c, b["x"], b["mask"])
                    if hps:
                        e.set_chain_hparams(c, **hps[c])
            else:
                e.set_data(bs[0]["x"], bs[0]["mask"])
            e.init_particles_batch(np.stack([b["key"] for b in bs]))   # (a chains engine is initialised before it is given a state)
            e.set_state(**{k: np.concatenate([s_[k] for s_ in states]) for k in names})
            e.set_keys(np.stack([b["key"] for b in bs]))
        e.run(t, 1)
        grads = (e.read("GRAD_THETA").reshape(C * M, -1).copy(), e.read("W_LIK").reshape(C * M, -1).copy())
        e.run(t + 1, 3)
        return grads, e.get_state()
    finally:
        e.close()


def assert_chains_match_standalone(bs, per_chain_data=False, hps=None):
    """chain c of one launch against a standalone engine given the same rows, key, data and values: bit for bit"""
    M = bs[0]["M"]
    (gt, wl), cst = chains_run(bs, per_chain_data, hps)
    for c, b in enumerate(bs):
        sl = slice(M * c, M * (c + 1))
        (gt1, wl1), st = chains_run([b])
        assert np.isfinite(gt1).all() and np.isfinite(wl1).all() and np.abs(gt1).max() > 0 and np.abs(wl1).max() > 0, c
        assert np.array_equal(gt[sl], gt1) and np.array_equal(wl[sl], wl1), c
        for k in ("z", "v_z", "theta", "v_theta", "baseline"):
            assert np.isfinite(st[k]).all() and np.array_equal(cst[k][sl], st[k]), (c, k)
        assert np.array_equal(cst["key"][c], st["key"]), c
