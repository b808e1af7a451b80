"""The observation axis N of the joint models: a plain-Python restatement of the launchers' path choice, and the case tables built on it.
A plain module, imported by the tests like large_states.py and weight_states.py (no fixtures, no pytest hooks).

N decides which kernel runs and how many 16-row tiles of x it walks:

  LinearGaussian  paired kernels (k_lin_logprobs_pair / k_lin_logprobs_hf) up to 128 observations, the unpaired k_lin_logprobs<NT> above, on
                  the LDS-resident path until x, the operand and the residuals of k_lin_grad<NT> no longer fit LDS (`lin_cut`); then the Gram
                  path of kernels_lin_gram.h.
  DenseNN         the tuned one-hidden-layer kernels up to 128 observations (register-operand f16 kernels with a 7-tile x image up to 112
                  observations and an 8-tile image above, the image variant, or the f32 kernel), the general kernels beyond.
  row tiles       nrt = ceil(N / 16): one tile, a ragged last tile, an exactly full last tile, the eighth tile (113 .. 128).

tests/test_obs_axis_host.py holds the table against this restatement (every case in exactly one class, every class visited) and the
reference against itself (float32 C oracle within the stage bounds of the float64 one; the autograd oracle on the intervention edges);
tests/test_gpu_obs_axis.py runs the cases on the device, and its path probe holds `lin_cut` against what the engine really does."""
import numpy as np

LDS = 160 * 1024
T_STEP = 2
M, S, SA = 2, 8, 2
KEY = 3

# the stage bounds of test_joint_lingauss_step_stages / test_joint_densenn_step_stages (tests/test_gpu_parity.py); max-norm relative
BOUNDS = dict(LOGPROBS_THETA=2e-5, LOGPROBS_Z=2e-5, GRAD_THETA=5e-4, W_LIK=2e-3, GRAD_Z=1e-4, PHI_THETA=2e-3, theta=1e-4, z=1e-4)
BOUNDS_NN = dict(BOUNDS, z=5e-4)
# stage -> key of COracle.step's debug dict
STAGE_KEYS = dict(LOGPROBS_THETA="logprobs_th", LOGPROBS_Z="logprobs_z", GRAD_THETA="grad_theta", W_LIK="w_lik", GRAD_Z="grad_z",
                  PHI_THETA="phi_theta")
# The one admissible widening: where the float32 C oracle is itself more than a quarter of a bound off the float64 one, the case's bound
# is 4 x that error.  {case id: {stage: measured float32-oracle error}}, filled from tests/test_obs_axis_host.py (which asserts that every
# case missing here stays within a quarter of the bounds) and kept in profiles/obs_axis_errors.txt.  Measured: no case needs it -- the
# float32 oracle's worst use of a bound is 0.65 of the quarter (z of a score-estimator case, 1.6e-5 of 2.5e-5).
WIDENED = {}


def bound(case, stage):
    b = (BOUNDS_NN if case["model"] == "densenn" else BOUNDS)[stage]
    w = WIDENED.get(case_id(case), {}).get(stage)
    return b if w is None else max(b, 4.0 * w)


# ---- LinearGaussian: the path choice -----------------------------------------------------------------------------------------------------
def lin_lds_bytes(d, N, NT, with_res):
    """kernels_joint.h: lin_geom / lin_lds_bytes -- X[np][ldx] | WG[kp][ldw] | (gradient kernel) RS[np][ldw], + 64 doubles"""
    kp, np_, ld = (d + 3) & ~3, (N + 15) & ~15, 16 * NT + 2
    f = np_ * ld + kp * ld + (np_ * ld if with_res else 0)
    return ((f * 4 + 15) & ~15) + 64 * 8


def joint_lin_fast_path(d, N, force_gram=False):
    """tu_lin.hip: joint_lin_fast_path -- !force_gram && d <= 112 && lin_lds_bytes(d, N, ceil(d / 16), true) <= 160 KiB - 2 KiB"""
    return (not force_gram) and d <= 112 and lin_lds_bytes(d, N, (d + 15) // 16, True) <= LDS - 2048


def lin_paired(d, N, S, layout="legacy"):
    """lin_launch.h: lin_logprobs, `paired` -- legacy PRNG layout, even S, S d d below 2^32, N <= 128"""
    return layout == "legacy" and S % 2 == 0 and S * d * d < 0xFFFFFFFF and N <= 128


def lin_kernel(d, N, S, layout="legacy", lin_f32=False):
    """lin_launch.h: lin_all_logprobs / lin_logprobs -- which log-probability kernel a step launches, in either form of the data
    (lin_f32: DIBS_LIN_F32, the `!jl.lin_f32` of use_bf)"""
    if not joint_lin_fast_path(d, N):
        return "gram"
    NT = (d + 15) // 16
    if not lin_paired(d, N, S, layout):
        return f"unpaired<{NT}>"
    if NT <= 4 and d > 32 and not lin_f32:      # use_bf: lin_launch_hf
        if d <= 48:
            return "hf<5,false>"
        return "hf<5,true>" if (d * d + 511) // 512 <= 5 else "hf<8,true>"
    epq = (d * d + 255) // 256                  # lin_launch_pair: EPQ by NT; NT = 4 alone has two
    if NT <= 2:
        return f"pair<{NT},4>"
    if NT == 3:
        return "pair<3,10>"
    if NT == 4:
        return f"pair<4,{10 if epq <= 10 else 16}>"
    return f"pair<{NT},0>"


def lin_cut(d):
    """the largest N on the LDS-resident path (joint_lin_fast_path is monotone in N: np = ceil16(N) only grows)"""
    assert joint_lin_fast_path(d, 1)
    n = 1
    while joint_lin_fast_path(d, n + 1):
        n += 1
    return n


def row_tiles(N):
    """kernels_joint.h: lin_pred_tiles, nrt = g.np >> 4 -- (tiles, class of the last one)"""
    nrt = (N + 15) >> 4
    return nrt, ("one" if nrt == 1 else "full" if N % 16 == 0 else "ragged")


# ---- DenseNN: the path choice ------------------------------------------------------------------------------------------------------------
NN_HC, NN_SLR = 8, 128   # kernels_nn.h


def _geom(d, N, NT):
    return (d + 3) & ~3, (N + 15) & ~15, 16 * NT + 2   # kp, np, ldx = ldw (kernels_joint.h: lin_geom)


def nn_lds_bytes_logprobs(d, N, NT, H):
    """kernels_nn.h: nn_lds_bytes + nn_lds_bytes_logprobs -- X[np][ldx] | GS[d d] | TR[max(kp, np)][ldw] | red | b1, W2, b2"""
    kp, np_, ld = _geom(d, N, NT)
    f = np_ * ld + d * d + max(kp, np_) * ld
    return ((f * 4 + 15) & ~15) + 64 * 8 + (((2 * d * H + d) * 4 + 15) & ~15)


def nn_grad_lds_bytes(d, N, NT, hcs):
    """kernels_nn.h: nn_grad_lds_floats / nn_grad_lds_bytes -- X | GS | SL[hcs][128][16] | CS[8][16] | CS2[hcs][2][8][16] | red"""
    kp, np_, ld = _geom(d, N, NT)
    f = np_ * ld + d * d + hcs * NN_SLR * 16 + 8 * 16 + hcs * 2 * 8 * 16
    return ((f * 4 + 15) & ~15) + 64 * 8


def nn_grad_hcs(d, N, NT, H):
    """kernels_nn.h: nn_grad_hcs -- hidden units per group that registers (8) and LDS (160 KiB - 2 KiB) hold; 0: does not fit"""
    hcs = min(H, NN_HC)
    while hcs > 0 and nn_grad_lds_bytes(d, N, NT, hcs) > LDS - 2048:
        hcs -= 1
    return hcs


def joint_nn_fast_path(d, N, H, n_hidden=1):
    """tu_nn.hip: joint_nn_fast_path"""
    NT = (d + 15) // 16
    return (n_hidden == 1 and 1 <= H <= 64 and N <= 128 and d <= 112 and nn_grad_hcs(d, N, NT, H) > 0
            and nn_lds_bytes_logprobs(d, N, NT, H) <= LDS - 512)


def nhf_lds_bytes(d, NT, H, soft):
    """kernels_nn_f16.h: nhf_lds_bytes -- the image variant: x image | two graphs | leaves"""
    nks, dp2, dp4 = (NT + 1) // 2, (d + 1) & ~1, (d + 3) & ~3
    img = 2 * NT * (32 * nks * 32 + 32)
    graphs = 2 * ((d * (dp2 // 2) * (8 if soft else 4) + 15) & ~15)
    return img + graphs + (2 * H + 1) * dp4 * 4 + 64 * 8 + 64


def nhx_ntn(N):
    """kernels_nn_f16x.h: nhx_ntn -- observation tiles of the x^T image of the instantiation that runs"""
    return 7 if N <= 112 else 8


def nhx_lds_bytes(d, NT, N, H, soft):
    """kernels_nn_f16x.h: nhx_img_bytes + nhx_graph_bytes + nhx_lds_bytes -- the register-operand kernels"""
    dp4 = (d + 3) & ~3
    img = 2 * nhx_ntn(N) * (32 * ((NT + 1) // 2) * 32 + 32)
    graphs = 2 * d * dp4 * 4 if soft else 2 * dp4 * 16
    return img + graphs + (2 * H + 1) * dp4 * 4 + 64 * 8 + 64


def nn_logprob_kernel(d, N, H, S, soft, layout="legacy"):
    """tu_nn.hip: joint_nn_dispatch / joint_nn_launch / joint_nn_logprobs_hf -- the log-probability kernel of one estimator pass
    (soft: the Z pass of the reparam estimator samples soft graphs; the theta pass and the score estimator hard ones)"""
    if not joint_nn_fast_path(d, N, H):
        return "general"
    NT = (d + 15) // 16
    paired = layout == "legacy" and S % 2 == 0 and S * d * d < 0xFFFFFFFF
    if NT >= 3 and paired and N <= 128:
        if NT >= 5 and nhx_lds_bytes(d, NT, N, H, soft) <= LDS - 512:
            return f"hx{nhx_ntn(N)}"                  # NHX_PICK(7) / NHX_PICK(8)
        if nhf_lds_bytes(d, NT, H, soft) <= LDS - 512:
            return "image"
    return "f32x16" if nn_lds_bytes_logprobs(d, N, NT, H) > 80 * 1024 else "f32x4"   # NN_LP_LAUNCH(16 / 4 waves)


def nn_grad_wide(d, N, H):
    """tu_nn.hip: joint_nn_launch, `wide` -- k_nn_grad with 8 waves, one block per CU"""
    NT = (d + 15) // 16
    return nn_grad_lds_bytes(d, N, NT, nn_grad_hcs(d, N, NT, H)) > 80 * 1024


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _case(model, d, N, *, S=S, est="reparam", interv=None, layout="legacy", edge=None, **model_kw):
    return dict(model=model, d=d, N=N, S=S, est=est, interv=interv, layout=layout, edge=edge, model_kw=model_kw)


def case_id(c):
    return (f"{c['model']}-d{c['d']}-N{c['N']}-S{c['S']}-{c['est']}" + ("-interv" if c["interv"] else "") + (f"-{c['edge']}" if c["edge"] else "")
            + ("-part" if c["layout"] != "legacy" else ""))


def classify(c):
    """the path / tile class of a case: exactly one tuple"""
    d, N = c["d"], c["N"]
    if c["model"] == "lingauss":
        return ("lingauss", lin_kernel(d, N, c["S"], c["layout"])) + row_tiles(N)
    H = c["model_kw"]["nn_hidden"][0]
    soft = c["est"] == "reparam"
    return ("densenn", nn_logprob_kernel(d, N, H, c["S"], False, c["layout"]), nn_logprob_kernel(d, N, H, c["S"], soft, c["layout"]),
            "wide" if joint_nn_fast_path(d, N, H) and nn_grad_wide(d, N, H) else "narrow") + row_tiles(N)


def _alternate(cases):
    """reparam / score alternate along the table; interventions (10 % mask) on about half of the cases, out of step with the estimator"""
    out = []
    for i, c in enumerate(cases):
        out.append(dict(c, est="reparam" if i % 2 == 0 else "score", interv=0.1 if (i // 2) % 2 == 0 else None))
    return out


# d -> N values (`cut` = lin_cut(d)); kernel family of the paired window in the comment
def _lin_table():
    cut = lin_cut
    rows = {
        8: (1, 16, 17, 128, 129, cut(8), cut(8) + 1),                       # pair<1,4>
        20: (1, 15, 16, 128, 129, cut(20), cut(20) + 1),                    # pair<2,4>
        40: (1, 16, 17, 112, 113, 128, 129, cut(40), cut(40) + 1),          # hf<5,false>
        50: (128, 129, cut(50)),                                            # hf<5,true>
        56: (16, 113, 128, 129, cut(56)),                                   # hf<8,true>
        64: (128, 129, cut(64), cut(64) + 1),                               # hf<8,true>, no padding column
        80: (17, 128, 129, cut(80), cut(80) + 1),                           # pair<5,0>
        100: (112, 113, 128),                                               # pair<7,0>; cut = 112: 113 .. 128 already take the Gram path
        112: (112, 113, 128),
    }
    cases = _alternate([_case("lingauss", d, N) for d, ns in rows.items() for N in ns])
    # odd S (the unpaired kernel below 128 too) at N = 128 and at the cut; the partitionable PRNG layout (never paired) at N = 128
    for i, d in enumerate(rows):
        for N in sorted({128, cut(d)}):
            cases.append(_case("lingauss", d, N, S=7, est="score" if i % 2 == 0 else "reparam", interv=0.1 if N == 128 else None))
        cases.append(_case("lingauss", d, 128, layout="partitionable", est="reparam" if i % 2 == 0 else "score", interv=0.1 if i % 2 else None))
    return cases


def _nn_hcs_edge(d, H):
    """(last N <= 128 with nn_grad_hcs > 0, first without) if the gradient kernel's LDS ends the fast path below 128 observations"""
    NT = (d + 15) // 16
    bad = [N for N in range(1, 129) if nn_grad_hcs(d, N, NT, H) == 0]
    return (bad[0] - 1, bad[0]) if bad else ()


def _nn_table():
    rows = (
        (20, dict(nn_hidden=(5,), nn_activation="relu", nn_bias=True), (1, 16, 17, 112, 113, 128, 129)),        # f32 kernel (NT = 2)
        (48, dict(nn_hidden=(5,), nn_activation="relu", nn_bias=True), (16, 112, 113, 128, 129)),              # the image variant
        (80, dict(nn_hidden=(5,), nn_activation="leakyrelu", nn_bias=False), (1, 16, 112, 113, 128, 129)),     # register-operand kernels
        (108, dict(nn_hidden=(5,), nn_activation="relu", nn_bias=True), (112, 113)),                           # last fast-path N and the first general one
        # the windows where the theta pass (hard graphs) takes the register-operand kernel and the Z pass of the reparam estimator (soft graphs:
        # + the graph bytes) does not: the image variant at d = 110, H = 7 (where k_nn_grad holds 6 of the 7 units at N = 112: groups 6 + 1),
        # the f32 kernel with 16 waves at d = 112.  (At d = 108, H = 5 both passes still fit: nhx_lds_bytes = 156 432 <= 160 KiB - 512.)
        (110, dict(nn_hidden=(7,), nn_activation="relu", nn_bias=True), (16, 112)),
        (112, dict(nn_hidden=(5,), nn_activation="tanh", nn_bias=True), (112, 113)),
    )
    cases = []
    for d, kw, ns in rows:
        ns = tuple(ns) + tuple(n for n in _nn_hcs_edge(d, kw["nn_hidden"][0]) if n not in ns)   # (empty for every d <= 112, H <= 64)
        cases += [_case("densenn", d, N, **kw) for N in ns]
    cases = _alternate(cases)
    for c in cases:     # the windows exist for soft graphs only: their cases run the reparam estimator
        if c["d"] >= 108:
            c["est"] = "reparam"
    return cases


def _edge_table():
    """intervention edges: a node intervened in every observation (its likelihood term is an empty sum; Gram count 0), an observation
    intervened on every node, a mask of ones except one entry per column"""
    cases = []
    for i, edge in enumerate(("node_always", "row_always", "one_left")):
        est = "reparam" if i % 2 == 0 else "score"
        cases.append(_case("lingauss", 20, 100, est=est, interv=1, edge=edge))
        cases.append(_case("lingauss", 20, lin_cut(20) + 1, est=est, interv=1, edge=edge))
        cases.append(_case("densenn", 20, 60, est=est, interv=1, edge=edge, nn_hidden=(5,), nn_activation="relu", nn_bias=True))
    return cases


LIN_CASES = _lin_table()
# DIBS_LIN_F32=1 keeps the f32 paired kernels at 33 <= d <= 64, which no case above reaches: NT 3 (epq 7), the last size of pair<4,10>
# (epq 10), the first of pair<4,16> (epq 11), and the operand exactly full (epq 16).  Not part of ALL_CASES: classify() restates the default
LIN_F32_CASES = _alternate([_case("lingauss", d, 40) for d in (40, 50, 51, 64)])
LIN_F32_KERNELS = ("pair<3,10>", "pair<4,10>", "pair<4,16>", "pair<4,16>")
NN_CASES = _nn_table()
EDGE_CASES = _edge_table()
ALL_CASES = LIN_CASES + NN_CASES + EDGE_CASES

# the paired classes that exist: NT = ceil(d / 16) and epq = ceil(d d / 256) are both functions of d (lin_launch.h instantiates these only)
LIN_PAIR_CLASSES = ("pair<1,4>", "pair<2,4>", "pair<3,10>", "pair<4,10>", "pair<4,16>", "pair<5,0>", "pair<6,0>", "pair<7,0>")
# every path / tile-count class that the table must visit (tests/test_obs_axis_host.py)
LIN_KERNELS = ("pair<1,4>", "pair<2,4>", "hf<5,false>", "hf<5,true>", "hf<8,true>", "pair<5,0>", "pair<7,0>", "gram",
               "unpaired<1>", "unpaired<2>", "unpaired<3>", "unpaired<4>", "unpaired<5>", "unpaired<7>")
NN_KERNELS = (("f32x4", "f32x4"), ("image", "image"), ("hx7", "hx7"), ("hx8", "hx8"), ("general", "general"), ("hx7", "image"), ("hx7", "f32x16"))   # (theta pass, Z pass)

SCORE_D = (20, 40, 80)
CHAIN_CASES = ((20, 16), (20, 129), (20, "cut"), (40, 128), (40, 129), (56, "cut"))
PROBE_D = (20, 40, 100)


def score_n_ho(d):
    return (1, 16, 128, 129, lin_cut(d), lin_cut(d) + 1)


# ---- data, configuration, state ---------------------------------------------------------------------------------------------------------
_DATA, _BUILT = {}, {}


def structured_x(d, N, seed=3):
    """test_joint_lingauss_gram_path: random x with some structure (lower-triangular mechanism); shared and read-only"""
    if (d, N, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        wts = (rng.random((d, d)) < 2.0 / d) * rng.normal(size=(d, d))
        x = rng.normal(size=(N, d)).astype(np.float32)
        for j in range(d):
            x[:, j] += (x[:, :j] @ np.tril(wts.T, -1)[j, :j]).astype(np.float32)
        x.setflags(write=False)
        _DATA[(d, N, seed)] = x
    return _DATA[(d, N, seed)]


def random_mask(d, N, share=0.1):
    mask = (np.random.default_rng(1000 * d + N).random((N, d)) < share).astype(np.int32)
    mask.setflags(write=False)
    return mask


def make_mask(c):
    d, N = c["d"], c["N"]
    if c["edge"] == "node_always":
        mask = np.zeros((N, d), np.int32)
        mask[:, d // 2] = 1
    elif c["edge"] == "row_always":
        mask = np.zeros((N, d), np.int32)
        mask[N // 3, :] = 1
    elif c["edge"] == "one_left":
        mask = np.ones((N, d), np.int32)
        mask[(7 * np.arange(d) + 3) % N, np.arange(d)] = 0
    elif c["interv"]:
        return random_mask(d, N, c["interv"])
    else:
        return None
    mask.setflags(write=False)
    return mask


def config_kwargs(c):
    return dict(n_vars=c["d"], n_particles=M, n_observations=c["N"], joint=True, likelihood=c["model"], grad_estimator_z=c["est"],
                n_grad_mc_samples=c["S"], n_acyclicity_mc_samples=SA, has_interventions=bool(c["interv"]), rng_layout=c["layout"],
                score_function_baseline=0.001 if c["est"] == "score" else 0.0, **c["model_kw"])


def built_case(c, oracle64):
    """x, mask, configuration keywords, the float32-representable start state and the float64 oracle's step on it at T_STEP (debug
    stages and the state after): computed once per case, shared between the tests, never written to"""
    from dibs_amd._abi import make_config
    cid = case_id(c)
    if cid not in _BUILT:
        x, mask, kw = structured_x(c["d"], c["N"]), make_mask(c), config_kwargs(c)
        before = start_state(oracle64, kw)
        after = {k: (None if v is None else v.copy()) for k, v in before.items()}
        dbg = oracle64.step(make_config(**kw), x, mask, after, T_STEP, debug=True)
        for a in list(before.values()) + list(after.values()) + list(dbg.values()):
            if a is not None:
                a.setflags(write=False)
        _BUILT[cid] = dict(c, id=cid, x=x, mask=mask, cfg_kw=kw, before=before, after=after, dbg=dbg)
    return _BUILT[cid]


def start_state(oracle, kw):
    """freshly initialised particles of PRNGKey(KEY) (both oracle builds draw the same float32 values), in the oracle's precision"""
    from dibs_amd._abi import make_config
    from oracle import prng
    st = oracle.new_state(make_config(**kw), prng.PRNGKey(KEY))
    for k in ("z", "theta"):
        st[k] = st[k].astype(np.float32).astype(oracle.real)
    return st


def stage_errors(built, dbg, after):
    """max-norm relative error of every stage of BOUNDS against the float64 oracle's step of the case; keys_equal beside them"""
    def rel(a, b):
        a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
        return float(np.abs(a[:b.size] - b).max() / max(np.abs(b).max(), 1e-300))
    errs = {s: rel(dbg[k], built["dbg"][k]) for s, k in STAGE_KEYS.items()}
    errs["theta"] = rel(after["theta"], built["after"]["theta"])
    errs["z"] = rel(after["z"], built["after"]["z"])
    return errs, bool((np.asarray(after["key"]) == built["after"]["key"]).all())
