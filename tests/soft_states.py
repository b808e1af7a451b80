"""Particle states that drive the soft-graph BGe kernels (grad_estimator_z = "reparam" of MarginalDiBS: k_bge_soft_mf, k_bge_soft,
k_soft_combine; dibs_amd/csrc/tu_bge_soft.hip) across the whole range of the parent weights p, a plain numpy reference of what they
compute, and the bookkeeping that says which kernel instantiation a case takes.  A plain module, imported by the tests like bge_states.py
and weight_states.py (no fixtures, no pytest hooks).

States.  z[M, d, d, 2] with n_dim = d: z[..., 0] = I and z[m, j, i, 1] = the score of edge i -> j, so the device's u_i . v_j IS the chosen
float32 score (one product with 1, the rest with 0).  One step at t = T_STEP = 2 with alpha_linear = 1: alpha = 2.  A profile is a target
A = alpha s per edge; saturation comes from large scores, so the float32 rounding of a score (6e-8 relative) stays out of the free edges.
The logistic noise is the engine's own draw, reproduced by oracle/prng.py; the soft graph of sample s is p = sigmoid(eps_s + A).

Which p is EXACTLY 0 or 1 on the device (kernels_joint.h: lin_sample_g; rng.h: rng_logistic with logistic_minval_tiny = 0):
  eps = logf(x / (1 - x)), x in [2^-23, 1 - 2^-23]                     =>  |eps| <= log(2^23 - 1) = 15.942
  p = 1 / (1 + expf(-(eps + A))) is 1.0f once expf(.) <= 2^-24          =>  eps + A >= 16.636: A >= 32.6 for every draw
  p is 0.0f once expf(-(eps + A)) overflows (argument above 88.7229); just below that 1 / (1 + e^y) is a subnormal, not 0
                                                                       =>  eps + A <= -88.73: A <= -104.7 for every draw
  (with logistic_minval_tiny = 1 eps reaches -87.3 and an exact 1 needs A >= 104; the cases here keep the default)
`saturated` uses |A| = 120.  The backbone of the other profiles has |A| = 40: its edges are exactly 1, its non-edges 1e-25 .. 1e-10.

Classes.  Every edge of a state belongs to one class, decided on the CPU from the reference's draws; with L = eps_s + A its logit,
  one    L > 16.636 (p = 1.0f)                tiny   -87.3 < L < log 1e-9            zero   L < -88.73 (p = 0.0f)
  small  log 1e-7 < L < log 1e-3              under  -87.3 < L < log 1e-20 (p^2 underflows in float32; p itself is a normal number)
  dense  log 9 < L < 16.636 (0.9 <= p < 1)    free   target A in [-3, 3]; p is whatever the draw makes of it
and `build` asserts for every sample that no entry is within a factor MARGIN = 4 of a boundary of its class (log 4 in L).  An edge whose
draws over the S samples spread too far for `small` / `dense` falls back to `tiny` / `one`.

Profiles: see PROFILES and `_targets`.  tests/test_soft_states_host.py holds everything said here against the reference alone;
tests/test_gpu_soft_bge.py runs the cases on the device."""
import math

import numpy as np

ALPHA_LINEAR, T_STEP, TAU = 1.0, 2, 1.0
ALPHA = ALPHA_LINEAR * T_STEP
A_BACK, A_SAT, A_UNDER = 40.0, 120.0, -68.0
MARGIN = 4.0
LM = math.log(MARGIN)
EPS_MAX = math.log(2.0 ** 23 - 1.0)
L_ONE, L_ZERO, L_NORMAL = 24 * math.log(2.0), -88.73, -87.3    # p = 1.0f above / p = 0.0f below / p a normal float32 above
CLASSES = ("diag", "one", "tiny", "zero", "small", "under", "dense", "free")
DIAG, ONE, TINY, ZERO, SMALL, UNDER, DENSE, FREE = range(8)
RANGE = {ONE: (L_ONE, np.inf), TINY: (L_NORMAL, math.log(1e-9)), ZERO: (-np.inf, L_ZERO), SMALL: (math.log(1e-7), math.log(1e-3)),
         UNDER: (L_NORMAL, math.log(1e-20)), DENSE: (math.log(9.0), L_ONE), FREE: (-3.0 - EPS_MAX - 0.01, 3.0 + EPS_MAX + 0.01)}
ENTRY_CLASSES = (FREE, SMALL, DENSE)     # the classes whose W_LIK entries are compared one by one, relative to their own size
PROFILES = ("mixed", "small_p", "saturated", "dense", "collinear", "few_obs")
COLLINEAR_RATIO = (1e-4, 1e-3)           # s / R_jj of the near-collinear children
COLLINEAR_TARGET = 3e-4


# ---- path bookkeeping -------------------------------------------------------------------------------------------------------------------
LDS = 160 * 1024


def soft_tri(d):
    """joint_launch.h: bge_soft_tri"""
    return d * (d + 1) // 2


def soft_wave_bytes(d):
    """joint_launch.h: bge_soft_wave_bytes -- L tri | U tri | p, y, w, dinv [128]"""
    return ((2 * soft_tri(d) + 4 * 128) * 4 + 15) & ~15


def soft_shared_bytes(d, r_in_lds):
    """joint_launch.h: bge_soft_shared_bytes -- R (when LDS-resident) | red[4] + pad"""
    return (((d * d if r_in_lds else 0) * 4 + 15) & ~15) + 256


def soft_waves(d, r_in_lds):
    """joint_launch.h: bge_soft_waves -- waves of k_bge_soft that fit 160 KiB - 1 KiB, at most 4; 0: not even one"""
    shared = soft_shared_bytes(d, r_in_lds)
    if shared + soft_wave_bytes(d) > LDS - 1024:
        return 0
    return min((LDS - 1024 - shared) // soft_wave_bytes(d), 4)


def soft_rl(d, n_mats):
    """tu_bge_soft.hip: bge_soft_launch, `rl` (65 .. 128) -- one matrix for all nodes AND keeping it in LDS costs no wave"""
    return n_mats == 1 and soft_waves(d, True) >= min(soft_waves(d, False), 4)


def soft_path(d, interv):
    """tu_bge_soft.hip: bge_soft_launch -- the kernel instantiation of a case.  engine_data.hip: n_mats = d with an intervention mask that has
    a non-zero entry, 1 otherwise."""
    n_mats = d if interv else 1
    if d > 128:
        return dict(kernel="k_bge_soft", name="k_bge_soft<false,4,GLOB>", NB=None, RL=False, RPL=4, GLOB=True, n_mats=n_mats)
    if d <= 64:
        nb, rl = min((d + 15) // 16, 4), n_mats == 1
        return dict(kernel="k_bge_soft_mf", name=f"k_bge_soft_mf<{nb},{str(rl).lower()},3>", NB=nb, RL=rl, RPL=1, GLOB=False, n_mats=n_mats)
    rl = soft_rl(d, n_mats)
    return dict(kernel="k_bge_soft", name=f"k_bge_soft<{str(rl).lower()},2>", NB=None, RL=rl, RPL=2, GLOB=False, n_mats=n_mats)


def rl_boundary():
    """(last d with rl, first d without) in 65 .. 128 without interventions, or None when one side is empty"""
    with_rl = [d for d in range(65, 129) if soft_rl(d, 1)]
    without = [d for d in range(65, 129) if not soft_rl(d, 1)]
    return (max(d for d in with_rl if d < min(without)), min(without)) if with_rl and without else None


def required_paths():
    """every path of bge_soft_launch, per RL value where both exist"""
    req = {(f"k_bge_soft_mf<{nb}", rl) for nb in (1, 2, 3, 4) for rl in (True, False)}
    req |= {("k_bge_soft<2>", False), ("k_bge_soft<GLOB>", False)}
    if any(soft_rl(d, 1) for d in range(65, 129)):
        req.add(("k_bge_soft<2>", True))
    return req


def path_key(p):
    if p["GLOB"]:
        return ("k_bge_soft<GLOB>", False)
    return (f"k_bge_soft_mf<{p['NB']}", p["RL"]) if p["kernel"] == "k_bge_soft_mf" else ("k_bge_soft<2>", p["RL"])


# ---- the case table (derived from the bookkeeping) ------------------------------------------------------------------------------------------
def _case(profile, d, M, S, interv=False, N=None, seed=0):
    N = N or (3 * d if profile == "dense" else (100 if d <= 64 else 200))
    return dict(profile=profile, d=d, M=M, S=S, interv=interv, N=N, seed=seed)


def case_id(c):
    return f"{c['profile']}-d{c['d']}-M{c['M']}-S{c['S']}-N{c['N']}" + ("-interv" if c["interv"] else "")


def _shape(k, d):
    """(M, S) of the k-th case of a size: S cycles through 1, 3, 4; two particles where the reference is cheap"""
    S = (4, 3, 1)[k % 3]
    return (2 if d <= 33 and S > 1 else 1), S


def _table():
    rb = rl_boundary()
    sizes = [5, 16, 17, 32, 33, 48, 49, 64, 65] + (list(rb) if rb else []) + [128, 129]
    out, k = [], 0
    for d in sorted(set(sizes)):
        for interv in (False, True):
            M, S = _shape(k, d)
            out.append(_case("mixed", d, M, S, interv))
            k += 1
    out.append(_case("mixed", 160, 1, 1, True))      # (one sample: the reference costs 2 s per sample at this size)
    few = {17: (1, 2, 5), 49: (2,), 64: (5,), 65: (1,), 129: (2,)}
    for d in (17, 49, 64, 65, 129):
        for prof in ("small_p", "saturated", "dense", "collinear"):
            M, S = _shape(k, d)
            out.append(_case(prof, d, M, S))
            k += 1
        for N in few[d]:
            M, S = _shape(k, d)
            out.append(_case("few_obs", d, M, S, N=N))
            k += 1
    out.append(_case("mixed", 17, 1, 128, seed=1))   # k_soft_combine's weight loop
    return tuple(out)


CASES = _table()
HOST_PIN_CASES = tuple(c for c in CASES if c["d"] <= 33 and c["S"] <= 4) + tuple(c for c in CASES if c["d"] == 65 and c["profile"] == "mixed" and not c["interv"])


# ---- construction ---------------------------------------------------------------------------------------------------------------------------
def _backbone(d, rng, last=None):
    """G* (g[i, j] = 1: i -> j), a DAG over a random order; the node at position q has nsat[q] parents among its predecessors: d - 2 at the
    last position, d // 2 at the one before (which is no parent of the last), none at the third from the end, one at position 1.  last: the
    number at the last position instead of d - 2.  Returns (g, order)."""
    order = rng.permutation(d)
    g = np.zeros((d, d), np.int32)
    for q in range(1, d):
        n = min(q, int(rng.choice([0, 1, 1, 2, 2, 3])))
        pool = order[:q]
        if q == d - 1:
            n, pool = min(d - 2 if last is None else last, q - 1), order[:q - 1]
        elif q == d - 2:
            n = min(d // 2, q)
        elif q == d - 3:
            n = 0
        elif q == 1:
            n = 1
        g[rng.choice(pool, size=n, replace=False), order[q]] = 1
    return g, order


def _data(g, order, N, rng, collinear=()):
    """observations of a linear SEM on G*, float32.  collinear: the noise has standard deviation 20 instead of 1 (R_jj ~ 400 N beside the
    prior's 0.5 I), and the children named are a unit-norm combination of their parents plus noise whose size is set by bisection so that
    the Schur complement s = R_jj - b^T R_pa^-1 b is COLLINEAR_TARGET R_jj"""
    d = g.shape[0]
    x = np.zeros((N, d))
    scale = 20.0 if collinear else 1.0
    for j in order:
        pa = np.flatnonzero(g[:, j])
        e = rng.normal(size=N)
        w = rng.uniform(0.3, 0.8, size=pa.size) * rng.choice([-1.0, 1.0], size=pa.size) / math.sqrt(max(pa.size, 1))
        if j in collinear:
            lin = x[:, pa] @ (w / np.linalg.norm(w))

            def ratio(sig):
                xx = np.concatenate([x[:, pa], (lin + sig * e)[:, None]], 1).astype(np.float32).astype(np.float64)
                R = bge_stats(xx, None)[0][0]
                return (R[-1, -1] - R[-1, :-1] @ np.linalg.solve(R[:-1, :-1], R[:-1, -1])) / R[-1, -1]

            lo, hi = 1e-4, 10.0
            assert ratio(lo) < COLLINEAR_TARGET < ratio(hi), (ratio(lo), ratio(hi))
            for _ in range(40):
                mid = math.sqrt(lo * hi)
                lo, hi = (mid, hi) if ratio(mid) < COLLINEAR_TARGET else (lo, mid)
            x[:, j] = lin + lo * e
        else:
            x[:, j] = x[:, pa] @ w + scale * e
    return x.astype(np.float32)


def _fit(eps_e, lo, hi):
    """a target A with lo + log 4 < eps_s + A < hi - log 4 for every sample's draw eps_e [S] (the middle of the interval), or None"""
    a_lo, a_hi = lo + LM + 0.05 - eps_e.min(), hi - LM - 0.05 - eps_e.max()
    return 0.5 * (a_lo + a_hi) if a_lo < a_hi else None


def _targets(profile, d, g, order, eps, rng, collinear=(), extra=()):
    """(A [d, d], cls [d, d]) of one particle: targets alpha s per edge and the class of every edge.  eps [S, d, d]: the particle's draws; extra: further tested columns."""
    A = np.where(g != 0, A_BACK, -A_BACK).astype(np.float64)
    cls = np.where(g != 0, ONE, TINY)
    if profile == "saturated":
        A, cls = np.where(g != 0, A_SAT, -A_SAT).astype(np.float64), np.where(g != 0, ONE, ZERO)
    elif profile == "dense":
        for i in range(d):
            for j in range(d):
                a = _fit(eps[:, i, j], *RANGE[DENSE]) if i != j else None
                A[i, j], cls[i, j] = (a, DENSE) if a is not None else (A_BACK, ONE)
    else:
        # tested columns: the structural ones (d - 2, d // 2, 0 and 1 backbone parents) and up to three more
        struct = [int(order[q]) for q in (d - 1, d - 2, d - 3, 1) if q >= 1]
        tested = list(dict.fromkeys(struct + [int(j) for j in rng.permutation(order[1:])[:3]] + list(extra)))
        used = set()
        for k, j in enumerate(tested):
            cand =[i for i in range(d) if i != j and not g[i, j] and i not in collinear]
            if profile == "small_p" and k % 2 == 1:    # every non-backbone parent small; the first such column below 1e-20
                for i in cand:
                    a = _fit(eps[:, i, j], *RANGE[SMALL])
                    if k == 1:
                        A[i, j], cls[i, j] = A_UNDER, UNDER
                    elif a is not None:
                        A[i, j], cls[i, j] = a, SMALL
                continue
            n = min(len(cand), int(rng.integers(1, 3)) if j in collinear else int(rng.integers(3, 7)))
            tg = rng.permutation(np.linspace(-3.0, 3.0, n)) if n >= 3 else rng.uniform(-3.0, 3.0, size=n)   # spread over [-3, 3]
            src = sorted(rng.permutation(cand).tolist(), key=lambda i: i in used)[:n]     # (sources that have no free edge yet first)
            used.update(src)
            for i, a in zip(src, tg):
                A[i, j], cls[i, j] = a, FREE
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(cls, DIAG)
    return A, cls


def z_keys(key, M, layout="legacy"):
    """per particle, the key the reparam estimator draws its logistic noise from: svgd.py:226-267 (split(key, M + 1)[1 + m]) and
    dibs.py:430-431 (subk_ of its split) -- lin_mode_key on the device"""
    from oracle import prng
    ks = prng.split(np.asarray(key, np.uint32), M + 1, layout)
    return ks[1:], np.stack([prng.split(k, 2, layout)[1] for k in ks[1:]])


def logits(b):
    """L = eps + alpha s [M, S, d, d] (float64 of the float32 values)"""
    return b["eps"].astype(np.float64) + ALPHA * b["scores"][:, None].astype(np.float64)


def device_p32(b):
    """the soft graphs as the device draws them: float32 arithmetic of lin_sample_g on the reference's draws [M, S, d, d]"""
    with np.errstate(over="ignore"):
        y = -(np.float32(TAU) * (b["eps"] + np.float32(ALPHA) * b["scores"][:, None]))
        p = np.float32(1.0) / (np.float32(1.0) + np.exp(y, dtype=np.float32))
    p[:, :, np.arange(b["d"]), np.arange(b["d"])] = 0.0
    return p


_BUILT = {}
MAX_KEY_TRIES = 40
W2_MIN = 0.05


def _build_once(c, key_seed):
    from dibs_amd._abi import make_config  # noqa: F401  (the configuration keywords below are make_config's)
    from oracle import prng
    d, M, S, N = c["d"], c["M"], c["S"], c["N"]
    rng = np.random.default_rng([d, S, M, c["seed"], PROFILES.index(c["profile"]), int(c["interv"]), N])
    g, order = _backbone(d, rng, d - 3 if c["profile"] == "collinear" else None)   # (collinear: one non-parent left for a free edge)
    coll = tuple(int(order[q]) for q in (d - 1, d - 2)) if c["profile"] == "collinear" else ()
    x = _data(g, order, N, rng, coll)
    mask, ja = None, None
    if c["interv"]:
        ja = int(order[d // 3])
        mask = (rng.random((N, d)) < 0.15).astype(np.int32)
        mask[:, ja] = 1                       # intervened in every observation: N_j = 0
    key = np.array([c["seed"] + 11 + 1000 * key_seed, d], np.uint32)
    kz, ksub = z_keys(key, M)
    eps = np.stack([prng.logistic(ksub[m], (S, d, d)) for m in range(M)])
    A, cls = zip(*[_targets(c["profile"], d, g, order, eps[m], rng, coll, () if ja is None else (ja,)) for m in range(M)])
    scores = (np.stack(A) / ALPHA).astype(np.float32)
    z = np.zeros((M, d, d, 2), np.float64)
    z[..., 0] = np.eye(d)
    z[..., 1] = scores.transpose(0, 2, 1)
    R, Nj = bge_stats(x.astype(np.float64), mask)
    kw = dict(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=2, alpha_linear=ALPHA_LINEAR,
              grad_estimator_z="reparam", has_interventions=mask is not None, edges_per_node=1 if d <= 5 else 2)
    b = dict(c, id=case_id(c), cfg_kw=kw, x=x, mask=mask, all_intervened=ja, z=z, key=key, kz=kz, eps=eps, scores=scores, cls=np.stack(cls),
             g0=g, order=order, collinear=coll, R=R, Nj=Nj, t=T_STEP, path=soft_path(d, c["interv"]), key_seed=key_seed)
    # membership: every entry inside its class, a factor MARGIN from the boundaries, in every sample
    L = logits(b)
    for k, (lo, hi) in RANGE.items():
        sel = np.broadcast_to((b["cls"] == k)[:, None], L.shape)
        m_ = 0.0 if k == FREE else LM
        assert (L[sel] > lo + m_).all() and (L[sel] < hi - m_).all(), (b["id"], CLASSES[k], L[sel].min(initial=0), L[sel].max(initial=0))
    return b


def build(c):
    """The state of a case: configuration keywords, data, particles, key, the draws `eps`, the class of every edge, R / N_j, the float64 and
    float32 runs of the reference (`ref64`, `ref32`: dicts of logprobs [M, S] and dscore [M, S, d, d]) and the path.  The loop-carry key
    is searched (at most MAX_KEY_TRIES keys) until every particle's second-largest softmax weight is at least W2_MIN.  Arrays are shared
    between callers and read-only."""
    cid = case_id(c)
    if cid in _BUILT:
        return _BUILT[cid]
    for key_seed in range(MAX_KEY_TRIES):
        b = _build_once(c, key_seed)
        b["ref64"] = soft_reference(b, np.float64)
        if (c["S"] == 1 or second_weight(b["ref64"]["logprobs"]).min() >= W2_MIN) and free_edges_carry_signal(b):
            break
    else:
        raise AssertionError((cid, "no key with a second-largest softmax weight of", W2_MIN))
    b["ref32"] = soft_reference(b, np.float32)
    for a in (b["x"], b["mask"], b["z"], b["key"], b["eps"], b["scores"], b["cls"], b["R"], *b["ref64"].values(), *b["ref32"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _BUILT[cid] = b
    return b


def free_edges_carry_signal(b):
    """every column with at least three free edges (but the one of a node without observations: exactly 0) has at least three of them
    with |dscore| >= 1e-3 of the particle's largest in some sample"""
    for m in range(b["M"]):
        ds = np.abs(b["ref64"]["dscore"][m]).max(0)
        free = b["cls"][m] == FREE
        for j in np.flatnonzero(free.sum(0) >= 3):
            if j != b["all_intervened"] and (free[:, j] & (ds[:, j] >= 1e-3 * ds.max())).sum() < 3:
                return False
    return True


def fresh_state(b):
    z = np.array(b["z"], np.float32)
    return dict(z=z, v_z=np.zeros_like(z), key=b["key"].copy(), baseline=np.zeros(b["M"], np.float32))


def softmax_weights(logprobs):
    """float64 softmax over the last axis"""
    lp = np.asarray(logprobs, np.float64)
    w = np.exp(lp - lp.max(-1, keepdims=True))
    return w / w.sum(-1, keepdims=True)


def second_weight(logprobs):
    """the second-largest softmax weight per particle"""
    return np.sort(softmax_weights(logprobs), axis=-1)[..., -2]


# ---- the reference: a plain evaluation of the reference's own formula ---------------------------------------------------------------------
def bge_stats(x, mask, alpha_mu=1.0):
    """linearGaussian.py:63-100 -- (R [n_mats, d, d], N_j [d]) in float64: one matrix without interventions, one per node with (node j's from
    the observations in which it is not intervened; the identity, never used, where there is none)"""
    x = np.asarray(x, np.float64)
    N, d = x.shape
    t = alpha_mu * ((d + 2) - d - 1) / (alpha_mu + 1)

    def one(keep):
        n = keep.sum()
        if n == 0:
            return np.eye(d)
        xk = x * keep[:, None]
        xb = xk.sum(0, keepdims=True) / n
        xc = (xk - xb) * keep[:, None]
        return t * np.eye(d) + xc.T @ xc + (n * alpha_mu / (n + alpha_mu)) * (xb.T @ xb)

    if mask is None or not np.asarray(mask).any():
        return one(np.ones(N))[None], np.full(d, float(N))
    keep = 1.0 - np.asarray(mask, np.float64)
    return np.stack([one(keep[:, j]) for j in range(d)]), keep.sum(0)


def _digamma(x):
    """digamma of a positive float64 (recurrence to x >= 10, then the asymptotic series)"""
    acc = 0.0
    while x < 10.0:
        acc -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    return acc + math.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f / 132))))


_lgamma_v, _digamma_v = np.vectorize(math.lgamma), np.vectorize(_digamma)


def gamma_args(b, l):
    """the arguments of lgamma / digamma of a node with N_j observations and parent weight sum l: a1 = (N_j + alpha_lambd - d + l + 1) / 2,
    a2 = (alpha_lambd - d + l + 1) / 2 with alpha_lambd = d + 2"""
    return 0.5 * (np.asarray(b["Nj"]) + 3.0 + l), 0.5 * (3.0 + np.asarray(l))


def soft_sample(b, p, dtype, want_grad=True):
    """linearGaussian.py:63-170 on the real-valued parent vectors p[:, j] (func.py:128-145: the masked matrix is outer(p, p) R + (1 -
    outer(p, p)) I) in arithmetic of `dtype`, and its derivative: (log-probability, dl [d, d] with dl[i, j] = d log p / d p_ij, s [d] =
    det(M_all) / det(M_pa) per node).  numpy.linalg on the masked matrices: log-determinants by slogdet, d logdet M / d p_i = 2 ((M^-1 o
    (R - I)) p)_i by the explicit inverse."""
    d = b["d"]
    R = np.asarray(b["R"], np.float64).astype(dtype)          # (the device is handed float32 R computed in double: the float32 run rounds it)
    I = np.eye(d, dtype=dtype)
    one = dtype(1.0)
    P = np.ascontiguousarray(p.T.astype(dtype))                # P[j] = parent vector of node j
    Pall = P.copy()
    Pall[np.arange(d), np.arange(d)] = one
    l = P.sum(1)
    Nj = np.asarray(b["Nj"], np.float64)
    c = (Nj + 2.0).astype(dtype) + l                           # N + alpha_lambd - d + l
    a1, a2 = gamma_args(b, l.astype(np.float64))
    log_t, am = math.log(0.5), 1.0
    gam = (0.5 * (math.log(am) - np.log(Nj + am)) + _lgamma_v(a1) - _lgamma_v(a2) - 0.5 * Nj * math.log(math.pi)).astype(dtype) \
        + dtype(0.5) * (dtype(3.0) + dtype(2.0) * l) * dtype(log_t)
    dgam = (0.5 * _digamma_v(a1) - 0.5 * _digamma_v(a2) + log_t).astype(dtype)
    out = []
    for Pm in (P, Pall):
        outer = Pm[:, :, None] * Pm[:, None, :]
        Mm = outer * R + (one - outer) * I
        sign, ld = np.linalg.slogdet(Mm)
        h = None
        if want_grad:
            h = np.einsum("jib,jb->ji", np.linalg.inv(Mm) * (R - I), Pm)
        out.append((sign, ld.astype(dtype), h))
    (sg_pa, ld_pa, h_pa), (sg_all, ld_all, h_all) = out
    have = Nj > 0                                              # linearGaussian.py:118: a node without observations scores 0
    lj = np.where(have, gam + dtype(0.5) * c * ld_pa - dtype(0.5) * (c + one) * ld_all, dtype(0.0))
    s = np.where((sg_pa > 0) & (sg_all > 0), np.exp(ld_all.astype(np.float64) - ld_pa.astype(np.float64)), -1.0)
    dl = None
    if want_grad:
        dlj = (dgam + dtype(0.5) * ld_pa - dtype(0.5) * ld_all)[:, None] + c[:, None] * h_pa - (c + one)[:, None] * h_all
        dl = np.where(have[:, None], dlj, dtype(0.0)).T.astype(dtype)     # [i, j]
        np.fill_diagonal(dl, 0.0)
    return lj.sum(dtype=dtype), dl, s


def soft_reference(b, dtype):
    """The reparam estimator's samples of every particle in arithmetic of `dtype` (float64: the reference; float32: the yardstick):
    dict(logprobs [M, S], dscore [M, S, d, d] = d log p(soft graph_s) / d scores, s [M, S, d] Schur complements, l [M, S, d]).
    The soft graph is sigmoid(tau (eps + alpha score)) of the float32 draws and scores; the chain to the scores is tau alpha p (1 - p)."""
    d, M, S = b["d"], b["M"], b["S"]
    lp, ds, ss, ll = np.zeros((M, S), dtype), np.zeros((M, S, d, d), dtype), np.zeros((M, S, d)), np.zeros((M, S, d))
    one = dtype(1.0)
    with np.errstate(over="ignore", under="ignore"):
        for m in range(M):
            for s in range(S):
                arg = dtype(TAU) * (b["eps"][m, s].astype(dtype) + dtype(ALPHA) * b["scores"][m].astype(dtype))
                p = one / (one + np.exp(-arg))
                np.fill_diagonal(p, 0.0)
                lp[m, s], dl, ss[m, s] = soft_sample(b, p, dtype)
                ds[m, s] = dl * (dtype(TAU) * dtype(ALPHA)) * p * (one - p)
                ll[m, s] = p.sum(0)
    return dict(logprobs=lp, dscore=ds, s=ss, l=ll)


def weighted_sum(dscore, w):
    """sum_s w_s dscore_s for any weight vector (float64, sample order), as oracle.dibs_oracle.weighted_sample_sum"""
    return (np.asarray(w, np.float64)[:, None, None] * np.asarray(dscore, np.float64)).sum(0)


def limit_graph(b):
    """the graph of the positive scores [M, d, d] (dibs.py:84-99)"""
    return (np.asarray(b["scores"]) > 0).astype(np.int32)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------
def lp_floor(d):
    """the LOGPROBS_Z bound of test_marginal_bge_reparam_estimator (tests/test_gpu_parity.py)"""
    return 5e-5 if d < 50 else 3e-4


W_LIK_MAXNORM = 2e-3     # conftest.stage_err: W_LIK
# The floor of the entry-wise W_LIK comparison: |dev_e - ref_e| <= C_SUM sum_s w_s |dscore_se| (the forward-error form of the sum).
# C_SUM from the float32 run of the reference, measured on the CPU before any device run (tests/test_soft_states_host.py prints it per
# case; profiles/soft_bge_errors.txt): over the 55 (case, entry class) cells the worst |f32 - f64| / sum_s w_s |dscore_s| has median
# 4.7e-5, 90th percentile 5.6e-4 and maximum 8.65e-4 (the `dense` cells: the float32 rounding of p near 1 in p (1 - p); elsewhere the
# reference's c h_pa - (c + 1) h_all cancels inside one sample: up to 4e-4).  1e-3 is the next round figure above all of them.
C_SUM = 1e-3


def reference_sums(b, w):
    """for weights w [M, S]: (sum_s w_s dscore_s of the float64 run, the same of the float32 run, sum_s w_s |dscore_s| of the float64 run),
    each [M, d, d]"""
    r64, r32 = b["ref64"]["dscore"], b["ref32"]["dscore"]
    M = b["M"]
    return (np.stack([weighted_sum(r64[m], w[m]) for m in range(M)]), np.stack([weighted_sum(r32[m], w[m]) for m in range(M)]),
            np.stack([weighted_sum(np.abs(r64[m]), w[m]) for m in range(M)]))


def yardstick(b):
    """the float32 run of the reference against the float64 run, both summed with the float64 run's own softmax weights:
    dict(lp: LOGPROBS max-norm relative, w_max: W_LIK max-norm relative (0 where the sum itself is below 1e-30), entry: entry_errors)"""
    W64, W32, absw = reference_sums(b, softmax_weights(b["ref64"]["logprobs"]))
    return dict(lp=rel(b["ref32"]["logprobs"], b["ref64"]["logprobs"]), w_max=rel(W32, W64) if np.abs(W64).max() > 1e-30 else 0.0,
                entry=entry_errors(b, W32, W64, absw))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def entry_errors(b, got, ref, absw):
    """per particle-stacked W_LIK `got` / `ref` [M, d, d] and absw = sum_s w_s |dscore_s|: {class name: (count, worst |got - ref| / |ref|,
    worst |got - ref| / absw)} over the entries of the entry classes with a reference value above 1e-30"""
    out = {}
    for k in ENTRY_CLASSES:
        sel = (b["cls"] == k) & (np.abs(ref) > 1e-30)
        if sel.any():
            e = np.abs(np.asarray(got, np.float64) - ref)[sel]
            out[CLASSES[k]] = (int(sel.sum()), float((e / np.abs(ref[sel])).max()), float((e / absw[sel]).max()))
    return out
