// Launch code of the JointDiBS + LinearGaussian kernels (kernels_lin.h, kernels_lin_gram.h): ONE text for both forms of the kernels, as
// the kernels themselves are.  Included after the kernel headers by tu_lin.hip (one data set for every block) and by tu_lin_chains.hip
// (per-chain data, the kernels k_..._chains), and by nothing else.  Each unit gets the two entry points LIN_K(lin_all_logprobs) and
// LIN_K(lin_all_grads); the public joint_lin_all_logprobs / joint_lin_all_grads of tu_lin.hip call one or the other (JointWork::n_chain_data),
// so a chains launch gets the grid, the LDS size, the per-block counts and the instantiation its standalone engine would get -- from the
// same lines.  Kernels are named through LIN_K(...), and the data arguments are spelled by the call-side counterparts of the parameter
// macros: LIN_DATA_ARGS / LIN_ANY_ARG for LIN_DATA_PARAMS / LIN_ANY_PARAM, LING_DATA_ARGS / LING_CNT_ARG for LING_DATA_PARAMS / LING_CNT_PARAM.
#pragma once
#if !defined(DIBS_TU_LIN) && !defined(DIBS_TU_LIN_CHAINS)
#error "lin_launch.h launches the kernels of kernels_lin.h / kernels_lin_gram.h: it is compiled in tu_lin.hip and tu_lin_chains.hip only"
#endif
#include "kernels_lin.h"
#include "kernels_lin_gram.h"
#include <type_traits>

// `dat`, the data of a launch: the workspace itself, or the LinChainData built from it once per entry point
#ifdef DIBS_TU_LIN_CHAINS
using LinData = LinChainData;
static inline LinData lin_data(const JointWork& w) { return joint_chain_data(w); }
#define LIN_DATA_ARGS dat
#define LIN_ANY_ARG
#define LING_DATA_ARGS dat
#define LING_CNT_ARG
#define LIN_ENTRY  // (declared in joint_launch.h)
#else
using LinData = JointWork;
static inline const LinData& lin_data(const JointWork& w) { return w; }
#define LIN_DATA_ARGS dat.x, dat.mask
#define LIN_ANY_ARG , dat.any_mask
#define LING_DATA_ARGS dat.gram
#define LING_CNT_ARG , dat.ncnt
#define LIN_ENTRY static
#endif

// ---- the instantiations: NT = ceil(d / 16) tiles of 16 variables, 1 ... 7 (joint_lin_fast_path: d <= 112) -----------------------------------
constexpr int LIN_TILE = 16;
// f(std::integral_constant<int, NT>{}) for the NT of d: log-probabilities, gradients and the held-out scorer
template <typename F>
static int lin_nt_dispatch(int d, F&& f) {
  switch ((d + LIN_TILE - 1) / LIN_TILE) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 7>{});
  }
}
// k_lin_logprobs_pair<NT, EPQ> keeps EPQ operand elements per thread (256 threads; 0: no register-resident operand), so EPQ has to cover
// d * d <= 256 * EPQ.  Both NT and epq = ceil(d * d / 256) are functions of d, so only these (NT, EPQ) can be launched:
//   <1,4> <2,4> <3,10> <4,10> <4,16> <5,0> <6,0> <7,0>
// lin_launch_pair() selects among them; the range of epq over the d of one NT is checked here, so that another class limit or tile width
// fails to compile instead of dropping operand elements.
constexpr int lin_epq(int d) { return (d * d + 255) / 256; }
constexpr int lin_epq_min(int nt) {
  int lo = lin_epq(LIN_TILE * nt);
  for (int d = LIN_TILE * (nt - 1) + 1; d <= LIN_TILE * nt; ++d) lo = lin_epq(d) < lo ? lin_epq(d) : lo;
  return lo;
}
constexpr int lin_epq_max(int nt) {
  int hi = 0;
  for (int d = LIN_TILE * (nt - 1) + 1; d <= LIN_TILE * nt; ++d) hi = lin_epq(d) > hi ? lin_epq(d) : hi;
  return hi;
}
static_assert(lin_epq_max(1) <= 4 && lin_epq_max(2) <= 4, "NT <= 2 launches k_lin_logprobs_pair<NT, 4>");
static_assert(lin_epq_min(3) >= 5 && lin_epq_max(3) <= 10, "NT == 3 launches k_lin_logprobs_pair<3, 10>");
static_assert(lin_epq_min(4) == 10 && lin_epq_max(4) == 16, "NT == 4 launches k_lin_logprobs_pair<4, 10> or <4, 16>");

// ---- one launch per kernel family --------------------------------------------------------------------------------------------------------
// the three log-probability families of kernels_lin.h take one argument list (per: samples / pairs per block)
template <typename K>
static void lin_launch_lp(K kernel, dim3 grid, int threads, size_t lds, const LinData& dat, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                          int per) {
  allow_lds(kernel, lds);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, jl.stream, LIN_DATA_ARGS, jl.theta, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.d,
                     jl.N, jl.S, per, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge LIN_ANY_ARG);
}
template <int NT>
static void lin_launch_unpaired(dim3 grid, const LinData& dat, const JointLaunch& jl, float* lp, Key2 carry, int mode, int spb) {
  lin_launch_lp(LIN_K(k_lin_logprobs)<NT>, grid, 256, lin_lds_bytes(jl.d, jl.N, NT, false), dat, jl, lp, carry, mode, spb);
}
template <int NT>
static void lin_launch_pair(dim3 grid, const LinData& dat, const JointLaunch& jl, float* lp, Key2 carry, int mode, int ppb) {
  const size_t lds = lin_lds_bytes_pair(jl.d, NT);
  [[maybe_unused]] const int epq = lin_epq(jl.d);
  if constexpr (NT <= 2) lin_launch_lp(LIN_K(k_lin_logprobs_pair)<NT, 4>, grid, 256, lds, dat, jl, lp, carry, mode, ppb);
  else if constexpr (NT == 3) lin_launch_lp(LIN_K(k_lin_logprobs_pair)<NT, 10>, grid, 256, lds, dat, jl, lp, carry, mode, ppb);
  else if constexpr (NT == 4) {
    if (epq <= 10) lin_launch_lp(LIN_K(k_lin_logprobs_pair)<NT, 10>, grid, 256, lds, dat, jl, lp, carry, mode, ppb);
    else lin_launch_lp(LIN_K(k_lin_logprobs_pair)<NT, 16>, grid, 256, lds, dat, jl, lp, carry, mode, ppb);
  } else lin_launch_lp(LIN_K(k_lin_logprobs_pair)<NT, 0>, grid, 256, lds, dat, jl, lp, carry, mode, ppb);
}
// split-f16 operands, 33 <= d <= 64, eight waves: <elements per thread, four pieces, waves>
static void lin_launch_hf(dim3 grid, const LinData& dat, const JointLaunch& jl, float* lp, Key2 carry, int mode, int ppb) {
  const size_t lds = 2 * AHF_IMG_BYTES + 256;
  const int epq8 = (jl.d * jl.d + 511) / 512;
  if (jl.d <= 48) lin_launch_lp(LIN_K(k_lin_logprobs_hf)<5, false, 8>, grid, 64 * 8, lds, dat, jl, lp, carry, mode, ppb);
  else if (epq8 <= 5) lin_launch_lp(LIN_K(k_lin_logprobs_hf)<5, true, 8>, grid, 64 * 8, lds, dat, jl, lp, carry, mode, ppb);
  else lin_launch_lp(LIN_K(k_lin_logprobs_hf)<8, true, 8>, grid, 64 * 8, lds, dat, jl, lp, carry, mode, ppb);
}
template <int NT>
static void lin_launch_grad(const LinData& dat, const JointLaunch& jl, const LinGradJob& jt, const LinGradJob& jz, const GradSplit& gs) {
  const size_t lds = lin_lds_bytes(jl.d, jl.N, NT, true);
  allow_lds(LIN_K(k_lin_grad)<NT>, lds);
  hipLaunchKernelGGL(LIN_K(k_lin_grad)<NT>, dim3(jl.Mloc, 2, GRAD_NS), dim3(256), lds, jl.stream, LIN_DATA_ARGS, jl.theta, jl.scores, jl.thr, jt, jz,
                     jl.baseline, jl.m0, jl.M, jl.d, jl.N, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge,
                     jl.sf_baseline LIN_ANY_ARG, gs);
}
static void ling_launch_logprobs(dim3 grid, size_t lds, const LinData& dat, int ng, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                                 float* ops_glob) {
  allow_lds(LIN_K(k_ling_logprobs), lds);
  hipLaunchKernelGGL(LIN_K(k_ling_logprobs), grid, dim3(256), lds, jl.stream, LING_DATA_ARGS LING_CNT_ARG, ng, jl.theta, jl.scores, jl.thr, lp, carry,
                     mode, jl.m0, jl.M, jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge, ops_glob);
}
static void ling_launch_grad(size_t lds, const LinData& dat, int ng, const JointLaunch& jl, const LinGradJob& jt, const LinGradJob& jz, float* ops_glob,
                             const GradSplit& gs) {
  allow_lds(LIN_K(k_ling_grad), lds);
  hipLaunchKernelGGL(LIN_K(k_ling_grad), dim3(jl.Mloc, 2, GRAD_NS), dim3(256), lds, jl.stream, LING_DATA_ARGS, ng, jl.theta, jl.scores, jl.thr, jt, jz,
                     jl.baseline, jl.m0, jl.M, jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge,
                     jl.sf_baseline, ops_glob, gs);
}

// ---- launch shapes -----------------------------------------------------------------------------------------------------------------------
static size_t ling_lds(int d, int n_gram, bool grad) {
  const size_t dd = (size_t)d * d;
  return (n_gram == 1 ? dd * 8 : 0) + (((grad ? 2 : 1) * dd * 4 + 15) & ~(size_t)15) + 128;
}
// Launch shape of the Gram kernels for `blocks` blocks.
//   glob     the operands of a block (masked weights; for the gradient kernel the graph as well) are beyond the LDS capacity and live in
//            global scratch (n_vars > 198 for the log-probabilities, > 141 for the gradients): `scratch` floats, 0 otherwise
//   ng       the n_gram argument: a single matrix stays in LDS only while it fits beside the operands (d <= 101 for the gradient kernel);
//            beyond that it is read through the caches (-1).  (Found by tests/tools/gpu_fuzz.py: d = 112 with 500 observations failed to
//            launch.)
struct LingShape {
  bool glob;
  int ng;
  size_t lds, scratch;
};
static LingShape ling_shape(int d, int n_gram, bool grad, size_t blocks) {
  const bool glob = ling_lds(d, -1, grad) > (size_t)160 * 1024 - 1024;
  const int ng = n_gram == 1 && (glob || ling_lds(d, 1, grad) > (size_t)160 * 1024) ? -1 : n_gram;
  return LingShape{glob, ng, glob ? 256 : ling_lds(d, ng, grad), glob ? blocks * (grad ? 2 : 1) * d * d : 0};
}
// the two jobs of a gradient launch: the theta estimator into the packed rows, the Z estimator into w_lik
struct LinGradJobs {
  LinGradJob jt, jz;
};
static LinGradJobs lin_grad_jobs(const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  return LinGradJobs{{jl.logprobs_th, jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.gtheta_off, jl.pack_stride,
                      jl.copy_theta ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.theta_off : nullptr, nullptr, carry_theta, LIN_MODE_THETA},
                     {jl.logprobs_z, jl.w_lik, (size_t)jl.d * jl.d, nullptr, jl.baseline_out, carry_z,
                      jl.est_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM}};
}

// ---- LDS-resident path: one estimator's log-probabilities ----------------------------------------------------------------------------------
template <int NT>
static void lin_logprobs(const LinData& dat, const JointLaunch& jl, Key2 carry, int mode) {
  const int spb = 4;
  float* lp = mode == LIN_MODE_THETA ? jl.logprobs_th : jl.logprobs_z;
  const bool paired = jl.layout == 0 && (jl.S & 1) == 0 && (uint64_t)jl.S * jl.d * jl.d < 0xFFFFFFFFull && jl.N <= 128;
  if (!paired) return lin_launch_unpaired<NT>(dim3((jl.S + spb - 1) / spb, jl.Mloc), dat, jl, lp, carry, mode, spb);
  const bool use_bf = NT <= 4 && jl.d > 32 && !jl.lin_f32;  // (lin_f32: tuning.h, the f32-MFMA kernel at 33 <= d <= 64 for A/B runs)
  // pairs per block: the block's prologue (x fragments, operand factors, zeroed images) is ~a third of a pair's work; 8 pairs when that
  // still leaves two full rounds of blocks (config 3: 1 914 -> 1 964 steps/s; 16 pairs: 1 856)
  const int ppb = (use_bf && (jl.S / 2 / 8) * jl.choice_rows() >= 1024) ? 8 : 4;
  const dim3 grid((jl.S / 2 + ppb - 1) / ppb, jl.Mloc);
  if (use_bf) lin_launch_hf(grid, dat, jl, lp, carry, mode, ppb);
  else lin_launch_pair<NT>(grid, dat, jl, lp, carry, mode, ppb);
}

// ---- the entry points --------------------------------------------------------------------------------------------------------------------
// (non-zero: a scratch area could not be allocated, nothing was launched from that point on)
// log p(theta, D | G_s) for the samples of the theta estimator and of the Z estimator (two launches)
LIN_ENTRY int LIN_K(lin_all_logprobs)(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  const LinData& dat = lin_data(*w);
  const int mz = jl.est_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM;
  if (w->n_gram) {  // Gram-matrix path (x does not fit LDS)
    // (global operands: a bounded number of blocks per particle loop over the samples, each with its own d x d scratch)
    const int rows = jl.choice_rows(), gxg = jl.S < 1024 / rows ? jl.S : (1024 / rows > 1 ? 1024 / rows : 1);
    const LingShape sh = ling_shape(jl.d, w->n_gram, false, (size_t)gxg * jl.Mloc);
    const dim3 grid(sh.glob ? gxg : jl.S, jl.Mloc);
    float* gs = sh.glob ? joint_gs_scratch(w, sh.scratch) : nullptr;
    if (sh.glob && !gs) return 1;
    ling_launch_logprobs(grid, sh.lds, dat, sh.ng, jl, jl.logprobs_th, carry_theta, LIN_MODE_THETA, gs);
    ling_launch_logprobs(grid, sh.lds, dat, sh.ng, jl, jl.logprobs_z, carry_z, mz, gs);
    return 0;
  }
  return lin_nt_dispatch(jl.d, [&](auto nt) {
    lin_logprobs<decltype(nt)::value>(dat, jl, carry_theta, LIN_MODE_THETA);
    lin_logprobs<decltype(nt)::value>(dat, jl, carry_z, mz);
    return 0;
  });
}
// both softmax-weighted gradients in one launch
LIN_ENTRY int LIN_K(lin_all_grads)(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  const LinData& dat = lin_data(*w);
  const LinGradJobs j = lin_grad_jobs(jl, carry_theta, carry_z);
  GradSplit gsp;
  if (w->n_gram) {
    const LingShape sh = ling_shape(jl.d, w->n_gram, true, (size_t)GRAD_NS * 2 * jl.Mloc);
    float* gs = sh.glob ? joint_gs_scratch(w, sh.scratch) : nullptr;
    if (sh.glob && !gs) return 1;
    if (!joint_grad_split(w, (size_t)jl.Mloc * 2, (size_t)jl.d * jl.d, &gsp)) return 1;
    ling_launch_grad(sh.lds, dat, sh.ng, jl, j.jt, j.jz, gs, gsp);
    return 0;
  }
  return lin_nt_dispatch(jl.d, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if (!joint_grad_split(w, (size_t)jl.Mloc * 2, (size_t)((NT + 3) / 4) * NT * 4 * 256, &gsp)) return 1;
    lin_launch_grad<NT>(dat, jl, j.jt, j.jz, gsp);
    return 0;
  });
}
