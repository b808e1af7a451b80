// Host-side launchers of the kernel families that live in their own translation units (tu_*.hip): plain arguments, no templates over a
// kernel, so the engine's files (engine*.hip) neither see nor instantiate those kernels.  The joint models and the soft-graph BGe
// estimator: joint_launch.h (included below).
#pragma once
#include "common.h"
#include "kernels_kmat.h"
#include "kernels_bge.h"
#include "kernels_bdeu.h"
#include "tuning.h"

// kernels that may need more than the default 64 KiB of dynamic LDS: raises hipFuncAttributeMaxDynamicSharedMemorySize once per
// (device, kernel) and size increase (engine.hip; thread-safe -- engines on several devices / host threads share the table)
void dibs_allow_lds(const void* kernel, size_t bytes);
template <typename K>
inline void allow_lds(K kernel, size_t bytes) { dibs_allow_lds((const void*)kernel, bytes); }
int dibs_cu_count();  // (engine.hip: compute units of the current device)

// ---- tu_bge.hip --------------------------------------------------------------------------------------
// sampling + queueing (sample = false: parent sets given in `masks`); kf.z != null appends the kernel-matrix blocks
void bge_launch_sample(bool sample, hipStream_t stream, const uint32_t* thr, uint64_t* masks, double* node_scores, const BgeParams& bp,
                       Key2 carry, int m0, int M, int Mloc, int d, int S, int W, int layout, const BgeQueues& qs, const KmatFuse& kf);
size_t bge_sample_lds_bytes(int d, int S, int W);
void bge_launch_chol(hipStream_t stream, double* node_scores, const BgeParams& bp, const BgeQueues& qs, int d, int S,
                     unsigned long long* counters);
// batched engines (one launch for every problem; BgeParams::pM set, keys explicit): include/dibs_hip.h, n_problems
void bge_launch_sample_batch(hipStream_t stream, const uint32_t* thr, uint64_t* masks, double* node_scores, const BgeParams& bp, Key2 carry,
                             int Mloc, int d, int S, int W, int layout, const BgeQueues& qs);
void bge_launch_chol_batch(hipStream_t stream, double* node_scores, const BgeParams& bp, const BgeQueues& qs, int d, int S);
void bge_launch_sum_nodes(hipStream_t stream, const double* node_scores, float* out, int d, int S);

// ---- tu_bdeu.hip: BDeu node scores of the parent sets in `masks` (kernels_bdeu.h); the LDS plan's fields of `a` are filled in ---------
int bdeu_launch_nodes(hipStream_t stream, BdeuArgs a);

// ---- tu_acyc.hip -------------------------------------------------------------------------------------
struct AcycLaunch {
  hipStream_t stream;
  const float* scores;
  float* part;            // [Mloc][units][d*d] partial sums of the blocks (one unit each)
  float* w_acyc;          // [Mloc][d*d] mean over the chains (k_acyc_reduce, same stream)
  float* big;             // n_vars > 112: acyc_big_elems() floats (matrix powers through global memory); null otherwise
  Key2 carry;
  int m0, M, Mloc, d, Sa, units;  // units = blocks per particle: Sa / 2 Threefry pairs of chains (paired), else Sa chains
  bool paired;
  float alpha, tau;
  int layout, tiny;
  hipEvent_t ev_start, ev_stop;  // profiling: kernel-level start / stop time stamps of the matrix-power kernel (see acyc_power_takes_events); else null
  const float* eas;       // [Mloc][d*d] exp(-alpha scores) (k_edge_scores), read by k_acyc_hf when tau == 1; may be null (then it is evaluated in place)
  int pipe = DIBS_PIPE_DEFAULT, hfw_max = 112;  // the engine's DibsTuning::acyc_pipe / acyc_hfw_max
};
// true: acyc_launch_power is ONE kernel and stamps a.ev_start / a.ev_stop around it (hipExtLaunchKernelGGL: the kernel's own start and
// end as the profiler sees them, without the dispatch latency an event pair recorded around the launch includes)
bool acyc_power_takes_events(const AcycLaunch& a);
void acyc_launch_power(const AcycLaunch& a);   // matrix powers -> per-block partial sums (n_vars > 112: everything, straight into w_acyc)
void acyc_launch_reduce(const AcycLaunch& a);  // partial sums -> w_acyc (same stream)
size_t acyc_big_elems(int Mloc, int d, int Sa);

// ---- tu_f64.hip: the float64 engine (kernels_f64.h; include/dibs_hip.h, dibs_config.reserved_i[1] = 64) -----------------------------
// Everything one step of the f64 engine reads and writes; the per-step fields (alpha .. carry_prior) are set by engine_f64.hip::step_f64.
struct F64Args {
  int d, k, M, S, Sa, dpad, L, tiny, prior, opt, n_mats;
  int64_t D;
  double alpha, beta, tau, er_c, inv_sig2, sfb, h, scale, step, alpha_lambd;
  Key2 carry_lik, carry_prior;
  double *z, *vz, *baseline, *scores, *probs, *w_lik, *w_acyc, *part, *logprobs, *gradz, *kxx, *phi;
  uint32_t* thr;
  uint64_t* masks;       // [M][d][S] (one word per parent set: n_vars <= 64)
  double* node_scores;   // [M][d][S]
  const double *R, *Nj, *gam;  // BGe statistics in double: R [n_mats][d][d], N_j [d], log_gamma_term [d][d + 1]
  const float* ltab;           // [2^23] logistic value of the f32 uniform (bits >> 9) (engine_f64.hip: f64_logistic_table)
  const double* prior_tab;     // [d][d] DIBS_PRIOR_EDGEWISE: log odds of edge i -> j, diagonal 0 (dibs_engine_set_edge_prior); else null
};
__host__ __device__ inline size_t f64_bge_wave_bytes(int d) { return (size_t)d * 64 * 8 + 64 * 4; }
__host__ __device__ inline size_t f64_acyc_lds_bytes(int dpad) { return (size_t)3 * dpad * (dpad + 1) * 8; }
void f64_launch_edge(hipStream_t st, const F64Args& a);
void f64_launch_bge(hipStream_t st, const F64Args& a);
void f64_launch_weights(hipStream_t st, const F64Args& a);
void f64_launch_acyc(hipStream_t st, const F64Args& a);
void f64_launch_acyc_reduce(hipStream_t st, const F64Args& a);
void f64_launch_grad(hipStream_t st, const F64Args& a);
void f64_launch_kmat(hipStream_t st, const F64Args& a);
void f64_launch_phi(hipStream_t st, const F64Args& a);
void f64_launch_update(hipStream_t st, const F64Args& a);

#include "joint_launch.h"
