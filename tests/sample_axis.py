"""The Monte-Carlo sample axes S (n_grad_mc_samples) and Sa (n_acyclicity_mc_samples) past one pass of every sample loop: a plain-Python
restatement of the choices the kernels and launchers make from S and Sa, `classify` (the branches a case reaches) and the case table
derived from both.  A plain module, imported by the tests like obs_axis.py and hparam_states.py (no fixtures, no pytest hooks); what those
two already restate (acyc_kernel, lin_kernel, nn_logprob_kernel, the stage bounds, the oracle steps) is imported from them.

  S   particle_grad_block (kernels_tail.h): tail_nsplit = min(8, 1024 / S, d) parts of the node-score sum; the barrier-free softmax with
      TAIL_SU = 4 samples per lane up to 256 samples, the block-wide reductions above; a second trip of the part loop from 1025; parent
      sets staged in LDS or read from global memory.  k_bge_sample (kernels_bge.h): 64 lanes over S / 2 pairs or S samples.  The joint
      models: grad_softmax_stats<4> and k_soft_combine stride by 256, k_grad_plan by 64; the log-probability launchers cut S into blocks.
  Sa  k_acyc_reduce (kernels_acyc.h) adds the per-block partial sums in groups of 16 and a guarded tail; the grid of every acyclicity
      kernel is acyc_units blocks wide (one unit per block).

tests/test_sample_axis_host.py holds the table against the restatement and the reference against itself; tests/test_gpu_sample_axis.py
runs the cases on the device."""
import numpy as np

import hparam_states as H
import obs_axis as A

LDS = 160 * 1024
LIMIT = LDS - 2048            # engine.hip: LDS_LIMIT - 2048, the budget of k_bge_sample and of particle_grad_block
TAIL_NT, TAIL_SU = 1024, 4    # kernels_tail.h
BGE_SAMPLE_WAVES = 4          # kernels_bge.h
T_STEP = H.T_MARGINAL         # every case is one step at t = 2 (the joint rows too: alpha = 0.1 keeps their sample weights apart from one-hot)
MAX_CASES = 64             # the issue's cap is `about 60`


# ---- particle_grad_block: kernels_tail.h --------------------------------------------------------------------------------------------------
def tail_nsplit(S, d):
    """kernels_tail.h: tail_nsplit -- min(8, 1024 / S, d), at least 1"""
    return max(1, min(8, TAIL_NT // max(S, 1), d))


def tail_ldw(d):
    return ((d + 15) & ~15) + 2


def tail_union_bytes(d, S, lik, big=False):
    """kernels_tail.h: tail_union_bytes -- W [dp16][dp16 + 2] f32 UNION lp S f64 | lp2 nsplit S f64 | wt S f32"""
    w = 0 if big else ((d + 15) & ~15) * tail_ldw(d) * 4
    a = S * 8 * (1 + tail_nsplit(S, d)) + S * 4 if lik else 0
    return (max(w, a) + 15) & ~15


def tail_fixed_bytes(d, ldz, S, lik):
    """kernels_tail.h: tail_fixed_bytes -- + U, V [kp4][ldz] f32 each, colsum d f32, (score estimator) nzw S f32, nzi S i32"""
    return (tail_union_bytes(d, S, lik, ldz == 0) + (2 * ((d + 3) & ~3) * ldz + d) * 4 + (S * 8 if lik else 0) + 15) & ~15


def tail_ldz(d, k, S, lik, limit=LIMIT):
    """kernels_tail.h: tail_ldz -- k rounded up to 16, == 16 (mod 32) where that still fits"""
    kq = (k + 15) & ~15
    want = kq if kq & 16 else kq + 16
    return want if tail_fixed_bytes(d, want, S, lik) <= limit else kq


def tail_stage_cap(d, ldz, S, W, limit=LIMIT):
    """kernels_tail.h: tail_stage_cap -- samples with non-zero weight whose parent sets [d][W] u64 fit behind the fixed part"""
    fixed = tail_fixed_bytes(d, ldz, S, True)
    return 0 if fixed >= limit else min(S, (limit - fixed) // (d * W * 8))


def tail_lds_bytes(d, ldz, S, W, lik, stage_cap):
    return tail_fixed_bytes(d, ldz, S, lik) + (stage_cap * d * W * 8 if lik else 0)


def tail_w_tot(d, S, lik):
    """engine.hip: engine_alloc -- W, U, V of a particle do not fit one block's LDS (w_tot; k_backproject_big does phase C, ldz = 0)"""
    return tail_lds_bytes(d, tail_ldz(d, d, S, lik), S, (d + 63) // 64, lik, 0) > LIMIT


def stage_cap_of(d, S):
    """engine_step.hip: the stage_cap a score-estimator step of d variables (k = d) hands to the block"""
    ldz = 0 if tail_w_tot(d, S, True) else tail_ldz(d, d, S, True)
    return tail_stage_cap(d, ldz, S, (d + 63) // 64)


def tail_refused(d, S, lik):
    """engine.hip: dibs_engine_create -- "a particle's sample weights do not fit in LDS" (the n_vars half of the test, backproject_big_lds, is
    not restated: it does not depend on S)"""
    return tail_lds_bytes(d, 0, S, (d + 63) // 64, lik, 0) > LIMIT


# ---- k_bge_sample: kernels_bge.h, tu_bge.hip ------------------------------------------------------------------------------------------------
def bge_sample_wave_bytes(d, S, W):
    """kernels_bge.h: bge_sample_wave_bytes -- masks [S][W] u64 | thr [d] | lim [d] | loc [S]"""
    return (S * W * 8 + 2 * d * 4 + S * 4 + 15) & ~15


def bge_sample_lds_bytes(d, S, W):
    """tu_bge.hip: bge_sample_lds_bytes"""
    return BGE_SAMPLE_WAVES * bge_sample_wave_bytes(d, S, W)


def bge_sample_fast(d, S, W, layout="legacy"):
    """kernels_bge.h: bge_sample_fast -- legacy layout, even S, at most two mask words, 32-bit counters"""
    return layout == "legacy" and S % 2 == 0 and W <= 2 and S * d * d < 0xFFFFFFFF


def bge_refused(d, S):
    """engine.hip: dibs_engine_create -- "BGe: n_grad_mc_samples too large" """
    return bge_sample_lds_bytes(d, S, (d + 63) // 64) > LIMIT


def bge_s_max(d):
    """the largest even S that dibs_engine_create admits for the BGe score estimator (bge_sample_lds_bytes is monotone in S)"""
    S = 2
    while not bge_refused(d, S + 2):
        S += 2
    return S


def bge_sample_loop(d, S, layout="legacy"):
    """k_bge_sample: (form of the draw loop, its trips per lane); the queue-reservation loop makes ceil(S / 64) trips in every form"""
    W = (d + 63) // 64
    if bge_sample_fast(d, S, W, layout):
        return "fast", (S // 2 + 63) // 64
    if W > 2:
        return "words", (S + 63) // 64
    if S % 2 == 0:
        return "even", (S // 2 + 63) // 64
    return "odd", (S + 63) // 64


def second_trip_samples(d, S, layout="legacy"):
    """the sample indices that k_bge_sample's draw loop writes on a lane's second and later trips"""
    form, trips = bge_sample_loop(d, S, layout)
    if trips < 2:
        return []
    if form in ("fast", "even"):
        return [s for p in range(64, S // 2) for s in (p, p + S // 2)]
    return list(range(64, S))


# ---- the acyclicity term: engine.hip, kernels_acyc.h ---------------------------------------------------------------------------------------
def acyc_units(d, Sa, layout="legacy"):
    """engine.hip: engine_alloc -- a work unit is a pair of chains where one Threefry call serves both (H.acyc_paired), else one chain;
    every acyclicity block handles one unit"""
    return Sa // 2 if H.acyc_paired(d, Sa, layout) else Sa


def reduce_trips(nblk):
    """kernels_acyc.h: k_acyc_reduce -- groups of 16 partial sums (`q + 16 <= nblk`), then the guarded tail"""
    full, tail = divmod(nblk, 16)
    name = {0: "", 1: "full", 2: "two_full"}.get(full, "many_full")
    return (name + "+tail" if name and tail else name) or "tail"


# ---- the joint models' launchers: lin_launch.h, tu_nn.hip -------------------------------------------------------------------------------------
def lin_blocks(d, N, S, M, layout="legacy"):
    """lin_launch.h: lin_logprobs -- (units, units per block) of the log-probability launch: pairs and ppb, or samples and spb = 4"""
    k = A.lin_kernel(d, N, S, layout)
    if k == "gram":
        return S, 1
    if k.startswith("unpaired"):
        return S, 4
    use_bf = k.startswith("hf<")
    return S // 2, 8 if use_bf and (S // 2 // 8) * M >= 1024 else 4


def nn_blocks(d, N, H_, S, M, soft, layout="legacy"):
    """tu_nn.hip: joint_nn_logprobs_hf (ppb) / joint_nn_launch (spb)"""
    k = A.nn_logprob_kernel(d, N, H_, S, soft, layout)
    if k == "general":
        return S, 1
    if k.startswith("hx") or k == "image":
        hS = S // 2
        return hS, 4 if (hS // 4) * M >= 1024 else (2 if hS >= 2 else 1)
    return S, 4 if (S // 4) * M >= 1024 else 2


def ragged(units, per_block):
    return units % per_block != 0


def gram_gx(S, rows):
    """lin_launch.h, lin_all_logprobs: the global-operand Gram path (n_vars > 198) clamps its grid to min(S, 1024 / rows) blocks that loop over the samples"""
    return S if S < 1024 // rows else max(1024 // rows, 1)


def trips(n, stride):
    return (n + stride - 1) // stride


def _t(n):
    return str(n) if n <= 2 else "3+"


# ---- classify: the branches a case reaches ---------------------------------------------------------------------------------------------------
def softmax_form(S):
    return "wave_u<=1" if S <= 128 else "wave_u>=2" if S <= 64 * TAIL_SU else "block"


def classify(c, nnz=None):
    """the set of branch names one step of the case runs.  nnz: the largest count of samples with non-zero float32 weight over the particles
    (from the float64 oracle); without it a case whose stage_cap is below S is `stage_by_nnz`."""
    d, S, Sa, M = c["d"], c["S"], c["Sa"], c["M"]
    nblk = acyc_units(d, Sa, c["layout"])
    out = {"acyc:" + H.acyc_family(H.acyc_kernel(d, Sa, c["layout"], c["hfw_max"]))}
    if d <= 112:
        out |= {"reduce:" + reduce_trips(nblk), "acyc_grid>16" if nblk > 16 else "acyc_grid<=16"}
    else:
        out.add("acycb_nch>16" if M * Sa > 16 else "acycb_nch<=16")
    if c["model"] == "bge" and c["est"] == "score":
        form, n = bge_sample_loop(d, S, c["layout"])
        out |= {f"nsplit{tail_nsplit(S, d)}", "softmax:" + softmax_form(S), f"bge_sample:{form}:{_t(n)}", "bge_queue:" + _t(trips(S, 64))}
        if tail_nsplit(S, d) * S > TAIL_NT:
            out.add("idx_second_trip")
        if -(-d // tail_nsplit(S, d)) * (tail_nsplit(S, d) - 1) >= d:
            out.add("empty_last_part")
        cap = stage_cap_of(d, S)
        out.add("staged" if cap >= S else "stage_by_nnz" if nnz is None else "staged" if nnz <= cap else "unstaged")
    elif c["model"] == "bge":
        out.add("soft_combine:" + _t(trips(S, 256)))
    else:
        soft = c["est"] == "reparam"
        if c["model"] == "lingauss":
            k = A.lin_kernel(d, c["N"], S, c["layout"])
            u, pb = lin_blocks(d, c["N"], S, M, c["layout"])
        else:
            Hh = c["model_kw"]["nn_hidden"][0]
            k = A.nn_logprob_kernel(d, c["N"], Hh, S, soft, c["layout"])
            u, pb = nn_blocks(d, c["N"], Hh, S, M, soft, c["layout"])
        if k == "gram" and d > 198 and gram_gx(S, M) < S:
            out.add("gram_gx_clamped")
        out |= {f"{c['model']}:{k}", "softmax_stats:" + _t(trips(S, 256)), "grad_plan:" + ("<=4" if trips(S, 64) <= 4 else "5+" if trips(S, 64) < 9 else "9+"),
                "ragged_last_block" if ragged(u, pb) else "whole_blocks"}
    return out


# every branch name the table must reach (tests/test_sample_axis_host.py).  Left to the rest of the suite: reduce:full (Sa = 32, the default).
BRANCHES = frozenset(
    [f"nsplit{n}" for n in range(1, 9)] + ["softmax:wave_u<=1", "softmax:wave_u>=2", "softmax:block", "idx_second_trip", "empty_last_part", "staged", "unstaged"]
    + ["bge_sample:fast:1", "bge_sample:fast:2", "bge_sample:fast:3+", "bge_sample:even:1", "bge_sample:even:2", "bge_sample:even:3+", "bge_sample:odd:1", "bge_sample:odd:2", "bge_sample:odd:3+", "bge_sample:words:1",
       "bge_queue:1", "bge_queue:2", "bge_queue:3+"]
    + ["reduce:tail", "reduce:full+tail", "reduce:two_full", "reduce:two_full+tail", "acyc_grid>16", "acyc_grid<=16", "acycb_nch>16", "acycb_nch<=16"]
    + ["acyc:" + f for f in ("k_acyc", "k_acyc<unpaired>", "k_acyc_hf", "k_acyc_hfw", "k_acyc_bfw", "k_acycb")]
    + ["softmax_stats:2", "softmax_stats:3+", "grad_plan:5+", "grad_plan:9+", "ragged_last_block", "whole_blocks", "gram_gx_clamped", "soft_combine:1", "soft_combine:2"]
    + ["lingauss:pair<1,4>", "lingauss:unpaired<1>", "lingauss:gram", "densenn:f32x4"])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _case(group, kernel, model, d, *, engine="single", key=None, **kw):
    """H._case + engine: `single`, `batch` (two problems of a batched engine), `edge` (the edge-wise prior with the Erdos-Renyi table),
    `chains` (three chains), `f64`.  tau = 1 unless a row says otherwise.  key: PRNGKey of the start state (KEYS holds the chosen ones)."""
    kw.setdefault("tau", 1.0)
    c = dict(H._case(group, kernel, model, d, **kw), engine=engine)
    return dict(c, key=KEYS.get(case_id(c), H.KEY) if key is None else key)


def case_id(c):
    return H.case_id(c) + ("" if c["engine"] == "single" else "-" + c["engine"]) + (f"-M{c['M']}" if c["M"] != 2 else "")


# The start key of a row whose weighted sums must reach past a loop's first pass (weight_index_sets): the first PRNGKey n = 0, 1, ... under
# which the float64 oracle gives some particle a softmax weight >= 1e-3 on one of the row's indices (find_key);
# tests/test_sample_axis_host.py holds weights_reach under the committed key.  Rows not listed start from H.KEY, which already does.
KEYS = {
    "S-bge-d8-N6-S130-Sa2-score-tau1.0": 0, "S-bge-d8-N6-S258-Sa2-score-tau1.0": 8, "S-bge-d8-N6-S1025-Sa2-score-tau1.0": 0,
    "S-bge-d8-N6-S258-Sa2-score-tau1.0-part": 6, "S-bge-d8-N6-S130-Sa2-score-tau1.0-edge": 0, "S-bge-d8-N6-S258-Sa2-score-tau1.0-edge": 8,
    "S-lingauss-d8-N4-S258-Sa2-reparam-tau1.0": 143, "S-lingauss-d8-N4-S258-Sa2-score-tau1.0": 115, "S-lingauss-d8-N4-S514-Sa2-score-tau1.0": 1,
    "S-lingauss-d8-N4-S259-Sa2-score-tau1.0": 45, "S-densenn-d8-N4-S258-Sa2-reparam-tau1.0-H5": 26, "S-densenn-d8-N4-S258-Sa2-score-tau1.0-H5": 50,
    "S-densenn-d8-N4-S514-Sa2-score-tau1.0-H5": 2, "S-densenn-d8-N4-S262-Sa2-reparam-tau1.0-H5": 7, "S-densenn-d8-N4-S259-Sa2-score-tau1.0-H5": 44,
    "S-bge-d12-N6-S258-Sa34-score-tau1.0-f64": 1, "S-bge-d8-N6-S130-Sa2-score-tau1.0-batch": 0, "S-bge-d8-N6-S258-Sa2-score-tau1.0-batch": 8,
}

N_BGE = 6      # observations of the S rows: few, so that the softmax weights over hundreds of sampled graphs stay near-flat
S_NSPLIT = (128, 129, 130, 146, 147, 170, 171, 192, 204, 205, 256, 257, 258, 341, 342, 512, 513, 514, 1024, 1025, 1026)


def _bge_rows():
    r = [_case("S", "particle_grad_block", "bge", 8, N=N_BGE, S=S, M=3 if S == 341 else 2) for S in S_NSPLIT]
    r += [_case("S", "particle_grad_block", "bge", 8, N=N_BGE, S=127)]                                          # (odd S: 127, 129 .. 205, 257 .. 1025 -- every softmax form)
    r += [_case("S", "k_bge_sample even", "bge", 8, N=N_BGE, S=S, layout="partitionable") for S in (130, 258)]
    r += [_case("S", "particle_grad_block", "bge", 5, N=N_BGE, S=S) for S in (64, 258)]                        # nsplit clamped by d
    r += [_case("S", "particle_grad_block", "bge", 9, N=N_BGE, S=128)]                                          # jw = 2: parts 5 .. 7 empty
    r += [_case("S", "particle_grad_block", "bge", 8, N=N_BGE, S=bge_s_max(8))]       # (cap < S and flat weights: unstaged at 8 variables too)
    # parent sets read from global memory: S one above the first S whose stage_cap is below it (cap = S - 2), weights near-flat from two observations.
    # 112: the smallest such S of 65 .. 128 (W = 2; W, U, V in LDS); 193: W = 4, w_tot (k_backproject_big does phase C)
    r += [_case("S", "unstaged", "bge", d, N=2, S=first_unstageable_s(d) + 1) for d in (112, 193)]
    return r


def first_unstageable_s(d):
    """the smallest S whose stage_cap is below S: from there a particle whose weights are all non-zero reads its parent sets unstaged"""
    S = 2
    while stage_cap_of(d, S) >= S:
        S += 1
    return S


def _engine_rows():
    r = [_case("S", "k_particle_grad_" + e, "bge", 8, N=N_BGE, S=S, engine=e) for e in ("batch", "edge") for S in (130, 258)]
    r += [_case("S", "float64 engine", "bge", 12, N=N_BGE, S=258, Sa=34, engine="f64")]
    return r


def _joint_rows():
    nn = dict(nn_hidden=(5,), nn_activation="relu", nn_bias=True)
    r = []
    for model, kw in (("lingauss", {}), ("densenn", nn)):
        for S, est in ((258, "reparam"), (258, "score"), (514, "score"), (514, "reparam"), (262, "reparam"), (259, "score")):
            r.append(_case("S", "grad_softmax_stats", model, 8, N=N_JOINT, S=S, est=est, **kw))
    r.append(_case("S", "chains engine", "lingauss", 8, N=N_JOINT, S=258, est="reparam", engine="chains"))
    # the global-operand Gram path (n_vars > 198): S two above the gx clamp of two particles, every block loops over two samples or one
    r.append(_case("S", "k_ling_logprobs glob", "lingauss", GLOB_D, N=20, S=gram_gx(1 << 20, 2) + 2, est="reparam"))
    return r


GLOB_D = 199       # kernels_lin_gram.h: ops_glob != null from 199 variables on (k_ling_logprobs), from 142 in k_ling_grad


def _soft_rows():
    """soft-graph BGe through k_soft_combine (strides S by 256): the torch-autograd oracle, as tests/test_gpu_soft_bge.py"""
    return [_case("S", "k_soft_combine", "bge", SOFT_D, N=SOFT_D + SOFT_D // 4, S=S, est="reparam") for S in (130, 258)]


SOFT_D = 5         # (17 variables: 20 s of autograd at S = 258)


N_JOINT = 4


def _acyc_rows():
    r = [_case("Sa", "k_acyc", "bge", 20, Sa=Sa) for Sa in (34, 64, 66)]
    r += [_case("Sa", "k_acyc<unpaired>", "bge", 20, Sa=Sa) for Sa in (17, 33)]
    r += [_case("Sa", "k_acyc<unpaired>", "bge", 20, Sa=34, layout="partitionable")]
    r += [_case("Sa", "k_acyc_hf", "bge", 50, Sa=Sa, tau=tau) for Sa, tau in ((34, 1.0), (34, 0.7), (66, 1.0))]
    r += [_case("Sa", "k_acyc_hfw", "bge", 80, Sa=34), _case("Sa", "k_acyc_bfw", "bge", 96, Sa=34, hfw_max=80), _case("Sa", "k_acycb", "bge", 130, Sa=34)]
    r += [_case("Sa", "k_acyc_batch", "bge", 20, Sa=34, engine="batch")]
    return r


BGE_CASES, ENGINE_CASES, JOINT_CASES, ACYC_CASES, SOFT_CASES = _bge_rows(), _engine_rows(), _joint_rows(), _acyc_rows(), _soft_rows()
ALL_CASES = BGE_CASES + ENGINE_CASES + JOINT_CASES + ACYC_CASES + SOFT_CASES
ORACLE_CASES = [c for c in ALL_CASES if c["engine"] in ("single", "edge") and not H.is_soft(c)]          # one step, stage by stage against the float64 C oracle
BITWISE_CASES = [c for c in ALL_CASES if c["engine"] in ("batch", "chains")]         # bit for bit against standalone engines
F64_CASES = [c for c in ALL_CASES if c["engine"] == "f64"]

# ---- configuration, data, reference -------------------------------------------------------------------------------------------------------------
def config_kwargs(c):
    """H.config_kwargs (every hyper-parameter off its default) + the baseline's EMA for the marginal score rows: `baseline` = sm / S weighs
    every sample equally"""
    kw, mean_obs = H.config_kwargs(c)
    if c["model"] == "bge" and c["est"] == "score":
        kw["score_function_baseline"] = 0.001
    return kw, mean_obs


def c_step(oracle, c, key=None):
    """one C-oracle step of the case at T_STEP from freshly initialised float32-representable particles of PRNGKey(key):
    (state before, debug stages, state after)"""
    from dibs_amd._abi import make_config
    from oracle import prng
    kw, mean_obs = config_kwargs(c)
    x, mask = H.data(c)
    before = oracle.new_state(make_config(**kw), prng.PRNGKey(c["key"] if key is None else key))
    for k in ("z", "theta"):
        if before[k] is not None:
            before[k] = before[k].astype(np.float32).astype(oracle.real)
    after = {k: (None if v is None else v.copy()) for k, v in before.items()}
    dbg = oracle.step(make_config(**kw), x, mask, after, T_STEP, debug=True, mean_obs=mean_obs)
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
        x, mask = H.data(c)
        _BUILT[cid] = dict(c, id=cid, cfg_kw=kw, mean_obs=mean_obs, x=x, mask=mask, before=before, dbg=dbg, after=after)
    return _BUILT[cid]


def weights(dbg):
    """[M, S] softmax of the Z estimator's log-probabilities, in float64"""
    lp = np.asarray(dbg["logprobs_z"], np.float64)
    w = np.exp(lp - lp.max(1, keepdims=True))
    return w / w.sum(1, keepdims=True)


def nnz_of(dbg):
    """per particle, the samples whose weight is non-zero in float32 (what particle_grad_block visits)"""
    return (weights(dbg).astype(np.float32) != 0).sum(1)


def weight_index_sets(c):
    """the index sets on each of which some particle must carry a weight >= 1e-3 for the row's weighted sums to notice a loop that stops
    after its first pass: samples >= 256 above S = 256 (TAIL_SU slots / strides of 256), >= 1024 above 1024, k_bge_sample's later trips"""
    S, sets = c["S"], []
    if c["group"] != "S":
        return sets
    if S > 256:
        sets.append(range(256, S))
    if S > 1024:
        sets.append(range(1024, S))
    if c["model"] == "bge" and c["est"] == "score" and second_trip_samples(c["d"], S, c["layout"]):
        sets.append(second_trip_samples(c["d"], S, c["layout"]))
    return sets


def weights_reach(c, dbg):
    w = weights(dbg)
    return all(w[:, list(idx)].max() >= 1e-3 for idx in weight_index_sets(c))


def find_key(oracle64, c, n_max=400):
    """the first PRNGKey n under which weights_reach holds (the way H.find_tiny_key walks keys)"""
    for n in [H.KEY] + [n for n in range(n_max) if n != H.KEY]:
        if weights_reach(c, c_step(oracle64, c, key=n)[1]):
            return n
    return None


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------
# The one admissible widening (as obs_axis.WIDENED): where the float32 C oracle is itself more than a quarter of a bound off the float64
# one, the case's bound is 4 x that error.  {case id: {stage: measured float32-oracle error}}
WIDENED = {}


def bound(c, stage):
    b = H.bounds(c)[stage]
    w = WIDENED.get(case_id(c), {}).get(stage)
    return b if w is None else max(b, 4.0 * w)


def stage_errors(c, dbg, after, built):
    """H.stage_errors + the baseline after the step (relative to its largest entry; 0 where the reference's is 0 everywhere)"""
    errs = H.stage_errors(c, dbg, built["dbg"])
    ref = np.asarray(built["after"]["baseline"], np.float64)
    errs["baseline"] = H.rel(after["baseline"], ref) if np.abs(ref).max() > 0 else float(np.abs(np.asarray(after["baseline"], np.float64)).max())
    return errs


BASELINE_BOUND = 1e-5    # test_step_stages_off_the_defaults (tests/test_gpu_hparams.py), tests/test_gpu_obs_axis.py


# ---- the acyclicity term chain by chain -----------------------------------------------------------------------------------------------------------
def acyc_chain_terms(c, built, oracle64):
    """[M, Sa, d, d]: d h(G_s) / d scores of every chain, h = tr((I + G / d)^d) - d on the soft graph G_s = sigmoid(tau (eps_s + alpha
    scores)) without its diagonal (dibs.py:557-601); their mean over s is W_ACYC.  eps: the C oracle's float32 logistic draws."""
    d, Sa, M = c["d"], c["Sa"], c["M"]
    kw = built["cfg_kw"]
    alpha, tau = kw.get("alpha_linear", 1.0) * T_STEP, kw["tau"]
    keys = H.draw_keys(dict(c, draws="acyc"), built["before"]["key"])
    sc = np.asarray(built["dbg"]["scores"], np.float64)
    out = np.zeros((M, Sa, d, d))
    off = 1.0 - np.eye(d)
    for m in range(M):
        eps = oracle64.logistic(keys[m], Sa * d * d, {"legacy": 0, "partitionable": 1}[c["layout"]]).astype(np.float64).reshape(Sa, d, d)
        for s in range(Sa):
            G = off / (1.0 + np.exp(-tau * (eps[s] + alpha * sc[m])))
            P = np.linalg.matrix_power(np.eye(d) + G / d, d - 1)
            out[m, s] = P.T * tau * alpha * G * (1.0 - G)
    return out
