// What the engine's translation units share (engine.hip, engine_step.hip, engine_data.hip, engine_f64.hip, engine_comm.hip): the engine
// struct, error / allocation / timing helpers, and the declarations of the internals that cross files.  No __global__ definitions: a kernel
// header whose kernels are not templates is compiled into ONE unit (kernels_marginal.h, kernels_tail.h: engine_step.hip; exchange_ipc.h:
// engine_comm.hip -- dibs_allow_lds keys its table on a kernel's host address) and gives every other file its structs and LDS sizes only.
// (The block of kernels_tail.h is also compiled under k_particle_grad_batch in tu_batch.hip and k_particle_grad_edge in tu_tail_edge.hip.)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include <utility>

#include "../../include/dibs_hip.h"
#include "launch.h"
#include "step_plan.h"
#include <map>
#include <mutex>
#include <rccl/rccl.h>  // declarations only: librccl is bound at run time (dibs_rccl, engine_comm.hip), libdibs_hip.so does not link it
#include "kernels_tail.h"
#include "exchange_ipc.h"

#define LDS_LIMIT ((size_t)160 * 1024)
// profiling counters (dibs_engine_get_counters): [0] executed Cholesky flops, [1..4] phases of k_particle_grad (100 MHz ticks of block 0),
// [8..12] phases of k_edge_scores, [16..21] phases of k_phi_update, [24..] k_bge_chol
#define DIBS_N_COUNTERS 8192  // ([64 ..]: per-block (start, end) clock stamps of the kernel under investigation)
int fail(const std::string& m);  // (engine.hip: the message of dibs_last_error on this thread; returns 1)
#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e));              \
  } while (0)

// BGe statistics that do not depend on the graph (linearGaussian.py:78-94): R_j, N_j, the (j, l) table of log_gamma_term,
// and for the complement form of kernels_bge.h R_j^-1 and logdet R_j.  Computed once per data set on the host in double,
// uploaded as f32 / f64.  Owns its device buffers.
struct BgeStats {
  float *R = nullptr, *Rp = nullptr, *Qp = nullptr;  // Qp = Rp + n_mats (d+1)^2: ONE allocation (see bge_upload)
  double *gam = nullptr, *Nj = nullptr, *ldR = nullptr;
  int n_mats = 1;
  double alpha_lambd = 0, alpha_mu = 0, log_t = 0;
  void release() {
    void* ptrs[] = {R, Rp, gam, Nj, ldR};
    for (void* p_ : ptrs)
      if (p_) hipFree(p_);
    R = Rp = Qp = nullptr;
    gam = Nj = ldR = nullptr;
  }
  ~BgeStats() { release(); }
  BgeStats() = default;
  BgeStats(const BgeStats&) = delete;
  BgeStats& operator=(const BgeStats&) = delete;
  BgeParams params() const { return BgeParams{Rp, Qp, gam, Nj, ldR, alpha_lambd, n_mats}; }
};

// BDeu (DIBS_LIK_BDEU; kernels_bdeu.h, bdeu_score.h): one data set as k_bdeu_nodes reads it -- packed rows, per-node used-row bits and
// counts.  Owns its device buffers.
struct BdeuData {
  uint64_t *rows = nullptr, *used = nullptr;  // [KW][N], [d][NW]
  int32_t* nused = nullptr;                   // [d]
  int N = 0, NW = 0;
  void release() {
    void* ptrs[] = {rows, used, nused};
    for (void* p_ : ptrs)
      if (p_) hipFree(p_);
    rows = used = nullptr;
    nused = nullptr;
    N = NW = 0;
  }
  ~BdeuData() { release(); }
  BdeuData() = default;
  BdeuData(const BdeuData&) = delete;
  BdeuData& operator=(const BdeuData&) = delete;
};
// ... and what dibs_engine_set_arities fixes: the arities, the field layout of a packed row and log r_i
struct BdeuState {
  std::vector<int32_t> arities;
  std::vector<BdeuField> fields;
  int KW = 0;
  BdeuField* d_fields = nullptr;
  double* d_log_arity = nullptr;
  double log_ess = 0.0;
  BdeuData train, ho;  // the engine's data (dibs_engine_set_data); the last held-out set dibs_score_graphs scored against
  ~BdeuState() {
    if (d_fields) hipFree(d_fields);
    if (d_log_arity) hipFree(d_log_arity);
  }
};
inline bool lik_marginal(int likelihood) { return likelihood == DIBS_LIK_BGE || likelihood == DIBS_LIK_BDEU; }

// the float64 engine's device state (dibs_config.reserved_i[1] = 64; kernels_f64.h): loop carry, per-step buffers and the BGe statistics in
// double.  The parent sets and node scores go to the f32 engine's PARENT_MASKS / NODE_SCORES buffers (same layouts).
struct F64State {
  double *z = nullptr, *vz = nullptr, *baseline = nullptr, *scores = nullptr, *probs = nullptr, *w_lik = nullptr, *w_acyc = nullptr,
         *part = nullptr, *logprobs = nullptr, *gradz = nullptr, *kxx = nullptr, *phi = nullptr, *R = nullptr, *Nj = nullptr, *gam = nullptr;
  uint32_t* thr = nullptr;
  float* ltab = nullptr;  // [2^23] the acyclicity noise: logistic value of every f32 uniform (f64_logistic_table)
  double alpha_lambd = 0;
  int n_mats = 1;
  ~F64State() {
    void* ptrs[] = {z, vz, baseline, scores, probs, w_lik, w_acyc, part, logprobs, gradz, kxx, phi, R, Nj, gam, thr, ltab};
    for (void* p_ : ptrs)
      if (p_) hipFree(p_);
  }
};

struct dibs_engine {
  dibs_config cfg;
  F64State* f64 = nullptr;  // float64 engine (see F64State); null: the f32 engine
  DibsTuning tune;  // the environment switches (tuning.h), latched at creation
  int d, k, M, Mloc, m0, N, S, Sa, W;
  // batched engine (cfg.reserved_i[0] = n_problems = B > 1): B independent problems of M particles each; the device arrays hold Mloc = B * M
  // rows, problem-major (m0 = 0).  M stays the size of ONE problem, so every choice the standalone engine makes from its particle count
  // (acyclicity chain grouping, kernel-matrix algorithm) is made the same way here.  See step_multi.
  int B = 1;
  Key2* bcarry = nullptr;                             // [B] loop-carry keys, advanced on the device (k_batch_keys)
  Key2 *bkeys_lik = nullptr, *bkeys_prior = nullptr;  // [B * M] this step's per-particle keys
  // chains engine (cfg.reserved_i[2] = n_chains = C > 1): C chains of ONE joint model on ONE data set.  B = C and the rows are laid out as
  // a batched engine's (chain-major, M = one chain's particles); every hyper-parameter is shared, and so is the data ...  See step_multi.
  bool chains = false;
  Key2* bkeys_theta = nullptr;                        // [C * M] this step's keys of the theta estimator (k_chain_keys)
  // ... or, LinearGaussian only, every chain on a data set of its own (dibs_engine_set_data_problem for every chain; engine_data.hip): the
  // device copies live in the workspace (JointWork::n_chain_data), here is what the host keeps until every chain has its data
  struct ChainData {
    bool shared = false;            // dibs_engine_set_data was called: the chains share that data set
    std::vector<char> set;          // [C] chain c was given data (empty: dibs_engine_set_data_problem was never called)
    std::vector<LinGramHost> gram;  // [C] Gram path: the chains' matrices, stacked and uploaded when the last chain arrives; released by batch_hp_commit
  } cdata;
  // per-problem hyper-parameters (dibs_engine_set_problem_hparams): the host values, and the device table of what the kernels take from
  // them (ProblemHP, common.h), written ONCE by batch_hp_commit when the particles are initialised -- set_problem_hparams is refused from
  // then on.  hp_tier: the step's kernels read the table (n_vars, n_dim <= 64 and what else batch_hp_tier asks); otherwise only the
  // batch-only kernels do (kernel matrix, phi, keys) and the rest take the configuration's values as launch arguments, as before
  // Chains engines keep the same host values and the same table per CHAIN (dibs_engine_set_chain_hparams: h_theta as well, which a batched
  // engine leaves at the configuration's).  chain_hp_ok: the condition of hp_tier for a chains engine, what differing values need;
  // hp_tier of a chains engine is decided by batch_hp_commit: some chain's derived values differ from the configuration's (step_multi then
  // takes the table-reading launches, otherwise it is launch for launch what it always was).
  std::vector<dibs_chain_hparams> hp_host;
  ProblemHP* hp = nullptr;  // [B]
  bool hp_final = false, hp_tier = false, chain_hp_ok = false;
  // median-heuristic kernel bandwidth (cfg.reserved_i[3]: bit 0 latent, bit 1 theta).  The kernel matrices and phi
  // read h / h_theta from the table: a standalone engine on the rule owns a one-row table (B = 1) and launches the table-reading forms
  // with one run.  Every step: distance pass -> sqd_z / sqd_t, selection -> the rows of hp and bw, kernel matrices (launch_bandwidth)
  int median_rule = 0;
  float *sqd_z = nullptr, *sqd_t = nullptr;  // [Mloc][M] squared distances (float)tot of the last step, block-diagonal per run
  float* bw = nullptr;                       // [B][2] (h_latent, h_theta) the last step's kernel matrices used
  struct BatchStats {                                 // host copies of the stacked BGe statistics (padded to d matrices per problem)
    std::vector<float> Rp, Qp;
    std::vector<double> gam, Nj, ldR;
    std::vector<char> set;
    double alpha_lambd = 0;
  } bst;
  int64_t D, P, E, Ev;  // z elems / theta elems per particle, packed row stride [z | grad_z | theta | grad_theta], plane row stride [z | theta] (floats)
  int dpad, ldk, edge_kc, acyc_nt, acyc_units;  // acyc_units: acyclicity blocks per particle (engine_alloc)
  bool acyc_paired;                             // ... each a Threefry pair of chains (else a single chain)
  float sigz;
  hipStream_t stream;
  bool own_stream;
  // state
  float *z, *vz, *theta, *vtheta, *baseline, *baseline2;
  Key2 key;
  // data
  float* x;
  int32_t* mask;
  BgeStats bge;
  BdeuState* bdeu = nullptr;  // DIBS_LIK_BDEU (engine_alloc); `bge` then holds zero tables for the shared sampling launch, which are never scored
  float* soft_ds;  // [Mloc, S, d, d]  BGe reparam estimator: per-sample score-space gradients
  float* soft_tri = nullptr;  // ... beyond 128 variables: the waves' packed triangles (factor | inverse columns) in global scratch
  int soft_blocks = 0;        //     of this many persistent blocks (kernels_bge_soft.h, GLOB)
  bool has_data;
  // work
  float* w_tot;     // [Mloc][d][d] total score-space gradient when a particle's W, U, V do not fit in one block's LDS (kernels_tail.h)
  float* acyc_big;  // n_vars > 112: buffers of the global-memory matrix powers (kernels_acyc_big.h)
  float* eas;       // [Mloc][d][d] exp(-alpha s) of this step (k_edge_scores -> k_acyc_hf / k_acyc_hfw); n_vars <= 112 only
  float *scores, *probs, *w_lik, *acyc_part, *w_acyc, *logprobs_z, *logprobs_th, *pack, *kz, *kt, *phi_z, *phi_th;
  unsigned int* fork_flag = nullptr;  // [0] sequence number published by k_edge_scores_p's last block, [1] its block counter (flag fork)
  unsigned int fork_seq = 0;
  double* kpart = nullptr;  // tiled kernel matrix (kernels_kmat.h): partial squared distances [nsplit][Mloc][M]
  int kmat_ns_max = 0;     // 0: the direct kernel k_kmat; otherwise the largest nsplit kpart has room for
  unsigned int* kmat_ctr = nullptr;  // one counter per tile (units riding in k_particle_grad: the last unit of a tile writes the entries)
  float* ksum = nullptr;  // joint models: kz + kt, formed by the k_kmat launch of kt (the weight matrix of the SVGD transform as ONE scalar-loadable array)
  // edge-wise graph prior (DIBS_PRIOR_EDGEWISE, dibs_engine_set_edge_prior): log odds [d][d], diagonal 0, as the engine's precision has them
  // (float: k_particle_grad_edge; double: k64_grad); allocated by the first call
  float* edge_tab = nullptr;
  double* edge_tab64 = nullptr;
  bool edge_tab_set = false;
  std::vector<float> edge_host32;  // staging of the stream-ordered copy
  std::vector<double> edge_host64;
  uint32_t* thr;
  uint64_t* masks;
  BgeQueues bq;
  double* node_scores;
  unsigned long long* counters;
  JointWork jw;
  // profiling
  bool profiling;
  bool profiling_concurrent;  // set_profiling(2): keep the second stream while timing (the acyclicity kernel is timed on its own stream)
  hipEvent_t ev0, ev1;
  hipStream_t stream2;      // the acyclicity kernel (needs only the edge scores) runs beside sampling -> factorisation -> weights: its bf16 MFMAs
                            // overlap with their vector work.  Same arithmetic, same results; DIBS_NO_ACYC_STREAM2 keeps one stream.
  hipEvent_t ev_fork, ev_join, ev_k0, ev_k1;
  // round 5: the fork of a step without a record packet on the main stream -- the event IS the edge kernel's completion signal
  // (hipExtLaunchKernel stop event; scripts/probe/stream_hop.hip: 5.7 -> 2.2 us between k_edge_scores and k_bge_sample) -- and, optionally,
  // the join as a flag polled inside k_particle_grad instead of an event wait in front of it (DIBS_FLAG_JOIN=1)
  unsigned int* join_flag = nullptr;   // device word: sequence number stored by the second stream's last kernel of a step (k_join_flag)
  unsigned int* join_err = nullptr;    // pinned host word: raised by tail_join_wait when the flag did not arrive (checked after every chunk)
  unsigned int join_seq = 0;
  bool streams_concurrent = false;     // kernels of the two streams run side by side (probed at creation): the in-kernel join is safe
  // The in-kernel flags (fork: k_wait_flag, join: tail_join_wait) need the two streams to make progress side by side.  That is probed at
  // creation and holds for an engine alone on its GPU; a masked-down device, a second process that fills the machine or a serialising tool
  // can still starve the polled kernel.  The waits are bounded; a chunk that saw a time-out is REPEATED on events from a copy of its
  // loop carry taken at the chunk's start, and the engine stays on events from then on (dibs_engine_run, dibs_engine_run_sharded).
  bool flags_now = false;              // this chunk / call uses the flags (latch_flags)
  bool flags_off = false;              // a wait timed out once: events for the rest of the engine's life
  int flag_fallbacks = 0;              // chunks repeated on events (dibs_engine_flag_fallbacks)
  bool debug_drop_flag = false;        // tests: the next step that would publish the join flag does not (dibs_engine_debug_drop_next_flag)
  float* carry_bak = nullptr;          // [Mloc (2 D + 2 P + 1)] z | v_z | theta | v_theta | baseline at the start of the chunk
  Key2 key_bak;
  KmatPlace kmat_place = KmatPlace::PhaseB;  // where phase A planned this step's kernel matrices (plan_step, step_plan.h); step_update reads it
  bool kmat_ext;    // the slab of the next phase B was computed by dibs_engine_kmat_values on a stream of the caller (overlapped exchange)
  double t_ms[DIBS_K_COUNT];
  int64_t t_n[DIBS_K_COUNT];
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  bool has_mean_obs;
  std::vector<float> mean_obs;
  // dibs_score_graphs: statistics / device copies of the last (x_ho, mask_ho) scored against (held-out evaluators and mixture weights
  // call it repeatedly with the same data: svgd.py:110-113, 370-372)
  // in-engine exchange (dibs_engine_comm_init / dibs_engine_run_sharded): RCCL communicators of this rank -- comm[0] on the engine stream,
  // comm[1] on the side stream of the overlapped protocol -- and the buffers of that protocol
  ncclComm_t comm[2] = {nullptr, nullptr};
  int n_comms = 0;
  float *planes = nullptr, *vsend = nullptr;  // [2][M][Ev] values | gradients of all particles, [Mloc][Ev] this rank's new values
  hipStream_t side = nullptr;
  hipEvent_t ev_exported = nullptr, ev_vals = nullptr;
  bool vals_fresh = false;  // plane 0 (and the kernel slab computed from it) belongs to the engine's current particles
  bool loopback = false;    // comm_init(NULL): collectives skipped (per-rank timing on one GPU)
  IpcComm ipc;              // the exchange through mapped peer memory instead of RCCL (exchange_ipc.h; dibs_engine_comm_init_ipc)
  uint32_t* agree_dev = nullptr;  // [4 + 4 n_ranks] this rank's error word of a chunk (16 bytes) | all ranks' (run_sharded's agreement)
  uint32_t* agree_host = nullptr; // pinned mirror
  struct ScoreCache {
    std::vector<float> x;
    std::vector<int32_t> mask;
    bool has_mask = false, valid = false;
    BgeStats st;
    JointWork jw;
    ScoreCache() { memset(&jw, 0, sizeof jw); }
    ~ScoreCache() { joint_free(&jw); }
    bool matches(const float* x_, const int32_t* m_, size_t n) const {
      return valid && x.size() == n && has_mask == (m_ != nullptr) && memcmp(x.data(), x_, n * 4) == 0 && (!m_ || memcmp(mask.data(), m_, n * 4) == 0);
    }
    void remember(const float* x_, const int32_t* m_, size_t n) {
      x.assign(x_, x_ + n);
      has_mask = m_ != nullptr;
      if (m_) mask.assign(m_, m_ + n);
      valid = true;
    }
  } score_cache;
};

inline NNParams nn_params(const dibs_config& c) {
  NNParams p{c.nn_hidden[0], c.nn_activation, c.nn_bias, (float)c.nn_obs_noise, (float)c.nn_sig_param, c.nn_n_hidden, {}};
  for (int l = 0; l < c.nn_n_hidden && l < DIBS_MAX_HIDDEN_LAYERS; ++l) p.hidden[l] = c.nn_hidden[l];
  return p;
}

template <typename T>
static hipError_t dalloc(T** p, size_t n) {
  *p = nullptr;
  if (n == 0) return hipSuccess;
  hipError_t e = hipMalloc((void**)p, n * sizeof(T));
  if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(T));
  return e;
}

inline int need_batch(const dibs_engine* e) {
  if (!e) return fail("null engine");
  if (e->B <= 1) return fail("not a batched engine (dibs_config.reserved_i[0] = n_problems must be > 1)");
  return 0;
}
// chains engine: the entry points it has no form of
inline int refuse_chains(const dibs_engine* e, const char* what) {
  return e && e->chains ? fail(std::string("chains engine (n_chains > 1): ") + what + " is not supported") : 0;
}

// Erdos-Renyi graph prior: the edge probability of the configuration, and its log odds (0 for the other priors)
inline double er_edge_prob(const dibs_config& c) { return c.graph_prior_edges_per_node * c.n_vars / ((c.n_vars * (c.n_vars - 1)) / 2.0); }
inline double er_log_odds(const dibs_config& c) {
  if (c.graph_prior != DIBS_PRIOR_ER) return 0.0;
  const double p = er_edge_prob(c);
  return log(p) - log(1 - p);
}

// edge-wise graph prior: every entry point that evaluates the latent prior asks this first (never a zero prior in place of a missing table)
inline int need_edge_prior(const dibs_engine* e) {
  return e->cfg.graph_prior == DIBS_PRIOR_EDGEWISE && !e->edge_tab_set ? fail("dibs_engine_set_edge_prior has not been called") : 0;
}

// ---- profiling helpers -----------------------------------------------------------------------
struct KTimer {
  dibs_engine* e;
  int id;
  hipEvent_t a, b;
  hipStream_t st;
  KTimer(dibs_engine* e_, int id_, hipStream_t st_ = nullptr) : e(e_), id(id_), a(nullptr), b(nullptr), st(st_ ? st_ : e_->stream) {
    if (e->profiling) {
      hipEventCreate(&a);
      hipEventCreate(&b);
      hipEventRecord(a, st);
    }
  }
  ~KTimer() {
    if (e->profiling) {
      hipEventRecord(b, st);
      e->pending.push_back({id, {a, b}});
    }
  }
};

void drain_timers(dibs_engine* e);  // (engine.hip)

// device buffer that frees itself (error paths)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t n) { return dalloc(&p, n); }
};

// Fork / join of the second stream by events, as step_multi and step_f64 do it (step_local has its own: ForkKind / JoinKind, step_plan.h):
//   fork() -- the second stream's chain on s2 -- chain_done() -- the main stream's chain -- join() -- the first reader of the chain's results.
// Without a second stream s2 is the main stream and the calls do nothing; while per-kernel timing is on, chain_done() joins right away.
struct EventFork {
  dibs_engine* e;
  bool on, join_now;
  hipStream_t s2;
  explicit EventFork(dibs_engine* e_)
      : e(e_), on(e_->stream2 != nullptr), join_now(e_->profiling && !e_->profiling_concurrent), s2(on ? e_->stream2 : e_->stream) {}
  int fork() const {
    if (!on) return 0;
    HIP_OK(hipEventRecord(e->ev_fork, e->stream));
    HIP_OK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
    return 0;
  }
  int chain_done() const {
    if (!on) return 0;
    HIP_OK(hipEventRecord(e->ev_join, e->stream2));
    if (join_now) HIP_OK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    return 0;
  }
  int join() const {
    if (on && !join_now) HIP_OK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    return 0;
  }
};

// carry keys: the loop-carry key advances by one split(key, M+1) per estimator batch (svgd.py:245, 251 / 695, 699, 703);
// the host walks the chain (row 0), kernels derive row 1 + m.
inline Key2 next_carry(const dibs_engine* e, Key2 k) { return rng_split_row(k, (uint32_t)e->M + 1u, 0u, e->cfg.rng_layout); }

// where phase A writes its per-particle rows (indexed by GLOBAL particle id): packed rows [z | grad_z | theta | grad_theta] (stride E, the
// single-rank buffer and the one-collective protocol) or gradient rows [grad_z | grad_theta] (stride Ev, the overlapped protocol, where
// the values travel separately).
struct RowTarget {
  float* base;
  size_t stride, gz_off, th_off, gth_off;
  int copy_vals;
};
inline RowTarget packed_rows(const dibs_engine* e, float* pack) {
  return RowTarget{pack, (size_t)e->E, (size_t)e->D, (size_t)(2 * e->D), (size_t)(2 * e->D + e->P), 1};
}

// explicit per-particle keys of one evaluation (dibs_engine_eval_gradients): device arrays Key2[Mloc], one per estimator family
struct StepKeys {
  const Key2 *theta, *lik, *prior;
};
// (`terms` of step_local: TERMS_LIK, TERMS_PRIOR, TERMS_ALL -- step_plan.h)

// where phase B reads the rows of ALL particles: packed rows (stride E) or the two planes [values | gradients] of the overlapped protocol
// (one allocation, [2][M][Ev]: both planes share the row stride, the gradient plane starts M * Ev floats later)
struct RowSource {
  const float* base;
  size_t stride, z_off, gz_off, th_off, gth_off;
};
inline RowSource packed_source(const dibs_engine* e, const float* pack) {
  return RowSource{pack, (size_t)e->E, 0, (size_t)e->D, (size_t)(2 * e->D), (size_t)(2 * e->D + e->P)};
}
inline RowSource plane_source(const dibs_engine* e, const float* planes) {
  const size_t g = (size_t)e->M * e->Ev;
  return RowSource{planes, (size_t)e->Ev, 0, g, (size_t)e->D, g + (size_t)e->D};
}

// ---- engine.hip ----
int batch_hp_commit(dibs_engine* e);  // (first use of the per-problem table: derive, upload, freeze)
inline float latent_sigma(double latent_prior_std, int k) { return latent_prior_std > 0 ? (float)latent_prior_std : 1.0f / sqrtf((float)k); }
void latch_flags(dibs_engine* e);
unsigned int take_join_err(dibs_engine* e);
int join_failure(unsigned int code, const char* what);
// ---- engine_step.hip ----
int step_local(dibs_engine* e, int t, const RowTarget& rt, const StepKeys* xk = nullptr, int terms = TERMS_ALL, const float* zero_w = nullptr);
int step_update(dibs_engine* e, int t, const RowSource& rs, float* vals_send = nullptr);
int step_multi(dibs_engine* e, int t);  // (one step of a batched or a chains engine)
int carry_copy(dibs_engine* e, bool restore);
void launch_stream_probe(hipStream_t main_stream, hipStream_t second_stream, unsigned int* words);  // k_probe_wait / k_probe_set (engine_alloc)
// ---- tu_batch.hip: the table-reading launches of step_multi (n_vars, n_dim <= 64; dibs_engine::hp_tier) ----
void batch_launch_edge_scores(hipStream_t st, const float* z, float* scores, uint32_t* thr, float* probs, float* eas, const ProblemHP* hp, int pM,
                              int Mloc, int d, int k, int dpad, int ldk);
void batch_launch_tail(hipStream_t st, const TailArgs& ta, const ProblemHP* hp, int pM, int Mloc, size_t lds);
void batch_launch_acyc_power(const AcycLaunch& a, const ProblemHP* hp, int pM);
// ---- tu_tail_edge.hip: k_particle_grad with the table of an edge-wise graph prior in place of the Erdos-Renyi constant ----
void edge_launch_tail(hipStream_t st, const TailArgs& ta, const float* tab, int blocks, size_t lds);
// ---- tu_batch.hip: the chain-aware launches of step_multi (keys, block-diagonal kernel matrices) ----
void chains_launch_keys(hipStream_t st, Key2* carry, Key2* keys_theta, Key2* keys_lik, Key2* keys_prior, int C, int M, int layout);
void chains_launch_kmat(hipStream_t st, bool tiled, const float* x, size_t len, float* kout, int C, int M, float scale, float h, const float* kadd,
                        float* ksum, size_t lds_direct);
// ... and their table-reading forms (per-chain hyper-parameters, dibs_engine::hp_tier of a chains engine): the keys launch also forms this
// step's alpha and beta of every chain, the kernel matrices take chain p's h (theta_seg: h_theta) from the table
void chains_launch_keys_hp(hipStream_t st, Key2* carry, Key2* keys_theta, Key2* keys_lik, Key2* keys_prior, int C, int M, int layout, ProblemHP* hp,
                           int t);
void chains_launch_kmat_hp(hipStream_t st, bool tiled, const float* x, size_t len, float* kout, int C, int M, float scale, const ProblemHP* hp,
                           int theta_seg, const float* kadd, float* ksum, size_t lds_direct);
bool chains_hp_differ(const dibs_engine* e);  // (engine.hip: some chain's host values derive to other scalars than the configuration's)
// ---- tu_batch.hip: median-heuristic bandwidth -- squared distances of one segment of every run (grids of chains_launch_kmat), and the
// selection that writes h / h_theta of every run's table row and bw [C][2] (rule: dibs_config.reserved_i[3]) ----
void bandwidth_launch_sqdist(hipStream_t st, bool tiled, const float* x, size_t len, float* out, int C, int M, size_t lds_direct);
void bandwidth_launch_select(hipStream_t st, const float* sqd_z, const float* sqd_t, int rule, int C, int M, ProblemHP* hp, float* bw);
// ---- engine_data.hip: BDeu -- k_bdeu_nodes over `nprob` parent sets of `masks` against one packed data set ----
int bdeu_launch(dibs_engine* e, hipStream_t st, const BdeuData& data, const uint64_t* masks, double* node_scores, long long nprob, int S);
// ---- engine_f64.hip ----
int f64_alloc(dibs_engine* e);
int f64_init_particles(dibs_engine* e, Key2 isub);
int step_f64(dibs_engine* e, int t);
