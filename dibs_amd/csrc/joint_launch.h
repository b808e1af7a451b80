// Host side of the joint models (tu_lin.hip: LinearGaussian, tu_nn.hip: DenseNonlinearGaussian) and of the soft-graph BGe estimator
// (tu_bge_soft.hip): the structs and sizes the engine's files need and the plain declarations of the launchers.  No __global__, no
// __device__ function, no template over a kernel -- included by launch.h.
#pragma once
#include "common.h"
#include "../../include/dibs_hip.h"
#include <vector>

enum { LIN_MODE_THETA = 0, LIN_MODE_Z_SCORE = 1, LIN_MODE_Z_REPARAM = 2, LIN_MODE_GIVEN = 3 };

#define GRAD_NS 8   // (16 measured: config 3 at step 1 500 281 us against 271, at step 5 54 against 49)
#define GRAD_NS_NN 16  // DenseNonlinearGaussian: a sample's gradient takes ~0.7 ms of a block -- finer shares balance the CUs better
struct GradSplit {
  float* part;         // [jobs][GRAD_NS][stride] partial sums
  unsigned int* ctr;   // [jobs] arrivals (zero between launches: the last block resets it)
  size_t stride;
};

// work list of a persistent gradient kernel (k_grad_plan, kernels_nn.h): per job the softmax statistics of its samples, and the (job, share)
// items that have at least one weighted sample
struct GradPlan {
  double* stats;        // [jobs][4]: maximum, sum of exponentials, sum of the log-probabilities, number of weighted samples
  unsigned int* items;  // [<= jobs * shares]: job * 64 + share
  unsigned int* ctr;    // [0]: number of items, [1]: next item to take  (this launch's pair of the two the workspace keeps)
  unsigned int* ctr_next;  // the other pair: zeroed by this launch's plan kernel for the next launch (no memset launch between the steps)
};

// Per-chain data of a chains engine (include/dibs_hip.h, CHAINS ENGINE: dibs_engine_set_data_problem for every chain; LinearGaussian only):
// what the per-chain kernels of tu_lin_chains.hip take instead of one data set's pointers.  A block serves one particle row m, so its chain
// c = m / M is block-uniform and chain c's slice is a scalar offset.
struct LinChainData {
  const float* x;        // [C][N][d]
  const int32_t* mask;   // [C][N][d]
  const int* any_mask;   // [C] chain c has interventions (the any_mask argument of its standalone engine's launches)
  const double* gram;    // Gram path: [C][n_gram][d][d] ...
  const double* ncnt;    // ... and [C][d]
  int M;                 // one chain's particles
  // per-chain hyper-parameters (dibs_engine_set_chain_hparams): the engine's device table [C]; the kernels take this step's alpha (written
  // by the keys launch of the step) and the baseline rate of the block's chain from row c
  const ProblemHP* hp;
};

struct JointWork {
  float* x;        // [N, d] device copy  (per-chain data: [C][N][d], and so is mask)
  int32_t* mask;   // [N, d]
  float* wsm;      // [Mloc, S] softmax weights scratch
  float* ln_tab;   // [Mloc, d, d] DenseNN: per-particle first-layer prior table (kernels_nn.h), else null
  float* w1t;      // [Mloc, H, d, d] DenseNN fast path: first-layer weights re-laid out per hidden unit, W1T[h][a][j] = W1[j][a][h]
  size_t w1t_floats;
  int any_mask;
  double* gram;    // LinearGaussian Gram path (kernels_lin_gram.h): C^(j) [n_gram][d][d], observations not intervened on j
  double* ncnt;    // [d] their count
  int n_gram;      // 1 without interventions, else d; 0: not built
  // chains engine with per-chain data (joint_chain_data_*): n_chain_data = C (0: one shared data set), chain_rows = one chain's particles;
  // x, mask are [C][N][d], gram [C][n_gram][d][d], ncnt [C][d] (n_gram = d as soon as ONE chain has interventions: a mask-free chain's
  // single matrix is repeated d times -- the same doubles in the same order of summation as its standalone engine reads from one copy)
  int n_chain_data, chain_rows;
  int* any_mask_c;  // [C] device
  const ProblemHP* chain_hp;  // LinChainData::hp: the engine's per-chain table, set when it is made final (batch_hp_commit)
  void* nhf_w1s;   // DenseNN, f16 matrix pipe (kernels_nn_f16.h): scaled first-layer weights per column pair (float2) [Mloc][H][d][ceil(d/2)]
  void* nhf_w1p;   // ... and their packed f16 pieces {h pair, m pair} (uint2), same shape
  int* nhf_ew;     // [Mloc] exponent of the per-particle scale
  size_t nhf_pairs;  // allocated pairs (0: not allocated)
  void *nhx_w1s, *nhx_w1p;  // the same per a-QUAD and node (float4 / uint4) [Mloc][H][ceil(d/4)][d]: k_nn_logprobs_hx (kernels_nn_f16x.h)
  size_t nhx_quads;
  // which table set belongs to the CURRENT theta: both are cleared by the theta pass (first estimator of a step) and set by whichever variant
  // builds its tables, so that an estimator pass that takes the other variant than the theta pass did (the LDS size depends on soft / hard
  // graphs) builds its own instead of reading stale or uninitialised tables
  bool nhf_valid, nhx_valid;
  float* nng_scratch;         // general DenseNN path (kernels_nn_generic.h): activation records, grown on first use
  size_t nng_scratch_floats;
  // general paths beyond the LDS capacity (LinearGaussian Gram kernels: n_vars > 141 / 198, DenseNN general kernels: n_vars > 198): the
  // sampled graph (and the masked weights) of a block live here instead of in LDS; grown on first use
  float* gs_scratch;
  size_t gs_scratch_floats;
  // gradient kernels with several blocks per (particle, estimator) (GradSplit): partial sums and arrival counters, grown on first use
  float* gpart;
  size_t gpart_floats;
  unsigned int* gctr;
  size_t gctr_n;
  GradPlan gplan;     // persistent gradient kernels: statistics + item list, grown on first use
  size_t gplan_jobs, gplan_items;
  unsigned int gplan_gen;  // launches so far: the counter pair in use alternates
};

struct JointLaunch {
  hipStream_t stream;
  const float* z;
  const float* theta;
  const float* scores;
  const uint32_t* thr;
  float* w_lik;
  float* logprobs_z;
  float* logprobs_th;
  const float* baseline;
  float* baseline_out;
  float* pack;
  size_t pack_stride, theta_off, gtheta_off;
  int copy_theta;  // 1: packed rows carry a copy of theta at theta_off; 0: gradient rows only
  int m0, M, Mloc, d, N, S;
  float alpha, tau;
  int layout, tiny, est_z;
  double sf_baseline;
  float obs_noise, mean_edge, sig_edge;
  int lin_f32 = 0, nn_f32 = 0;  // the engine's DibsTuning (tuning.h): keep the f32-MFMA log-probability kernels (A/B runs)
  // chains engine (include/dibs_hip.h, n_chains): the particle count the launchers size their blocks from (samples per block, blocks per
  // particle) is one chain's, so that a chain is launched as its standalone engine would launch it; 0: Mloc
  int M_choice = 0;
  int choice_rows() const { return M_choice > 0 ? M_choice : Mloc; }
};

struct NNParams {
  int H, act, bias;  // H = width of the first hidden layer (the tuned one-hidden-layer kernels of kernels_nn.h)
  float obs_noise, sig_param;
  int n_hidden, hidden[DIBS_MAX_HIDDEN_LAYERS];
};

struct BgeSoftParams {
  const float* R;     // [n_mats, d, d]
  const double* Nj;   // [d]
  double alpha_lambd, alpha_mu, log_t;
  int n_mats;
};
__host__ __device__ inline int bge_soft_tri(int d) { return d * (d + 1) / 2; }
__host__ __device__ inline size_t bge_soft_wave_bytes(int d) {
  // L tri | U tri | p[128] | y[128] | w[128] | dinv[128]
  return (((size_t)2 * bge_soft_tri(d) + 4 * 128) * 4 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t bge_soft_shared_bytes(int d, bool r_in_lds) {
  return ((((size_t)d * d * (r_in_lds ? 1 : 0)) * 4 + 15) & ~(size_t)15) + 256;  // Rs | red[4] (+ pad)
}
__host__ __device__ inline int bge_soft_waves(int d, bool r_in_lds) {
  const size_t shared = bge_soft_shared_bytes(d, r_in_lds);
  if (shared + bge_soft_wave_bytes(d) > (size_t)160 * 1024 - 1024) return 0;
  const int nw = (int)(((size_t)160 * 1024 - 1024 - shared) / bge_soft_wave_bytes(d));
  return nw > 4 ? 4 : nw;
}

// ---- tu_lin.hip: the workspace, and JointDiBS + LinearGaussian --------------------------------------
int joint_alloc(JointWork* w, int Mloc, int d, int N, int S);
void joint_free(JointWork* w);
int joint_set_data(JointWork* w, const float* x, const int32_t* mask, int N, int d);
// scratch areas of the workspace, grown on first use; nullptr / false: hipMalloc failed.  (Called by tu_lin.hip and tu_nn.hip only: hidden,
// the library's exported symbols stay what they were when these were inline)
__attribute__((visibility("hidden"))) float* joint_gs_scratch(JointWork* w, size_t floats);
// partial-sum area of the split gradient kernels: `jobs` (particle, estimator) pairs x `ns` blocks x `stride` floats; counters zeroed once
__attribute__((visibility("hidden"))) bool joint_grad_split(JointWork* w, size_t jobs, size_t stride, GradSplit* out, int ns = GRAD_NS);
__attribute__((visibility("hidden"))) bool joint_grad_plan(JointWork* w, size_t jobs, int ns, GradPlan* out);
// true: x fits the LDS-resident MFMA kernels; false: the Gram-matrix path of kernels_lin_gram.h runs (joint_lin_set_gram builds C)
bool joint_lin_fast_path(int d, int N, bool force_gram);
int joint_lin_set_gram(JointWork* w, const float* x, const int32_t* mask, int N, int d);
// per-chain data (chains engine): the [C][N][d] arrays allocated once, one chain's slice uploaded, and the Gram matrices of all chains
// (their host copies, as joint_lin_gram_host built them per chain) stacked and uploaded.  Non-zero: hipMalloc / copy failed
int joint_chain_data_alloc(JointWork* w, int C, int rows_per_chain, int N, int d);
int joint_chain_data_set(JointWork* w, int c, const float* x, const int32_t* mask, int N, int d);
struct LinGramHost {  // one data set's Gram matrices on the host (joint_lin_gram_host): C [n_gram][d][d], cnt [d]
  std::vector<double> C, cnt;
  int n_gram = 0;
};
void joint_lin_gram_host(LinGramHost* g, const float* x, const int32_t* mask, int N, int d);
int joint_chain_gram_commit(JointWork* w, int d, const std::vector<LinGramHost>& chains);
LinChainData joint_chain_data(const JointWork& w);
// (the launchers return non-zero when a scratch area cannot be allocated: nothing was launched from that point on; lin_launch.h)
int joint_lin_all_logprobs(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z);
int joint_lin_all_grads(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z);
// log p(theta_i, D | g_i) of n given (graph, parameter) pairs (held-out scoring; dibs_score_graphs)
int joint_lin_score_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, float obs_noise,
                          float mean_edge, float sig_edge, hipStream_t stream);

// ---- tu_lin_chains.hip: the per-chain forms of the six LinearGaussian kernel families (LinChainData) -----
// The launch text of tu_lin.hip (lin_launch.h) compiled a second time: what joint_lin_all_logprobs / joint_lin_all_grads call for an engine
// with per-chain data (JointWork::n_chain_data), and nothing else calls
__attribute__((visibility("hidden"))) int lin_all_logprobs_chains(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z);
__attribute__((visibility("hidden"))) int lin_all_grads_chains(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z);

// ---- tu_nn.hip: JointDiBS + DenseNonlinearGaussian ---------------------------------------------------
// true: the tuned one-hidden-layer kernels of kernels_nn.h apply; false: the general path of kernels_nn_generic.h runs
bool joint_nn_fast_path(int d, int N, const NNParams& np_);
int joint_nn_dispatch(JointWork* w, const JointLaunch& jl, Key2 carry, int mode, const NNParams& np_, size_t P);
int joint_nn_score_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, const NNParams& np_,
                         size_t P, hipStream_t stream);
// theta = stax initialisation stream of sample_parameters (nonlinearGaussian.py:155-186)
void joint_nn_init_theta(float* theta, size_t P, Key2 key, int m0, int Mloc, int M, int d, const NNParams& np_, int layout, hipStream_t stream);

// ---- tu_bge_soft.hip: MarginalDiBS + BGe, reparameterised estimator ---------------------------------
// both launches of the estimator: per-sample soft-graph scores + gradients, then the softmax-weighted combination
void bge_soft_launch(const BgeSoftParams& sp, const float* scores, Key2 carry, int m0, int M, int Mloc, int d, int S, float alpha,
                     float tau, int layout, int tiny, float* soft_ds, float* logprobs, float* w_lik, hipStream_t stream, float* tri_glob,
                     int glob_blocks);
