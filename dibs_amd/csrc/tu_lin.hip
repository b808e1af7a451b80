// translation unit: the joint models' workspace (JointWork: allocation, data, scratch areas) and the JointDiBS + LinearGaussian kernels
// with their launchers (kernels_lin.h, kernels_lin_gram.h).  The launchers hand a chains engine with per-chain data (JointWork::n_chain_data)
// to the per-chain kernels of tu_lin_chains.hip, with the launch shape they chose for the shared-data kernel.
#define DIBS_TU_LIN
#include "launch.h"
#include "kernels_lin.h"
#include "kernels_lin_gram.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

bool joint_lin_fast_path(int d, int N, bool force_gram) {
  // (the MFMA kernels are instantiated for up to 7 tiles of 16 variables; force_gram: DibsTuning::lin_gram)
  // (2 KiB below the capacity: the gradient kernel has a little static LDS of its own)
  return !force_gram && d <= 112 && lin_lds_bytes(d, N, (d + 15) / 16, true) <= (size_t)160 * 1024 - 2048;
}

void joint_lin_gram_host(LinGramHost* g, const float* x, const int32_t* mask, int N, int d) {
  bool any = false;
  if (mask)
    for (size_t i = 0; i < (size_t)N * d; ++i) any |= mask[i] != 0;
  const int ng = any ? d : 1;
  std::vector<double>&C = g->C, &cnt = g->cnt;
  C.assign((size_t)ng * d * d, 0.0);
  cnt.assign(d, 0.0);
  for (int jm = 0; jm < ng; ++jm)
    for (int n = 0; n < N; ++n) {
      if (any && mask[(size_t)n * d + jm]) continue;
      const float* xr = x + (size_t)n * d;
      double* Cj = C.data() + (size_t)jm * d * d;
      for (int a = 0; a < d; ++a) {
        const double xa = xr[a];
        for (int b = 0; b < d; ++b) Cj[(size_t)a * d + b] += xa * (double)xr[b];
      }
    }
  for (int j = 0; j < d; ++j)
    for (int n = 0; n < N; ++n) cnt[j] += (any && mask[(size_t)n * d + j]) ? 0.0 : 1.0;
  g->n_gram = ng;
}
static int gram_upload(JointWork* w, const std::vector<double>& C, const std::vector<double>& cnt, int ng) {
  if (w->gram) hipFree(w->gram);
  if (w->ncnt) hipFree(w->ncnt);
  w->gram = nullptr;
  w->ncnt = nullptr;
  w->n_gram = 0;
  if (hipMalloc((void**)&w->gram, C.size() * 8) != hipSuccess) return 1;
  if (hipMalloc((void**)&w->ncnt, cnt.size() * 8) != hipSuccess) return 1;
  if (hipMemcpy(w->gram, C.data(), C.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return 1;
  if (hipMemcpy(w->ncnt, cnt.data(), cnt.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return 1;
  w->n_gram = ng;
  return 0;
}
int joint_lin_set_gram(JointWork* w, const float* x, const int32_t* mask, int N, int d) {
  LinGramHost g;
  joint_lin_gram_host(&g, x, mask, N, d);
  return gram_upload(w, g.C, g.cnt, g.n_gram);
}
// chains engine, per-chain data: every chain's matrices stacked [C][ng][d][d], ng = d as soon as one chain has interventions -- a chain
// without them then carries its single matrix d times (the doubles its standalone engine reads from one copy, summed in the same order)
int joint_chain_gram_commit(JointWork* w, int d, const std::vector<LinGramHost>& chains) {
  int ng = 1;
  for (const LinGramHost& g : chains) ng = g.n_gram > ng ? g.n_gram : ng;
  const size_t dd = (size_t)d * d;
  std::vector<double> C(chains.size() * ng * dd), cnt(chains.size() * (size_t)d);
  for (size_t c = 0; c < chains.size(); ++c) {
    const LinGramHost& g = chains[c];
    for (int j = 0; j < ng; ++j) memcpy(&C[(c * ng + j) * dd], &g.C[(g.n_gram > 1 ? (size_t)j : 0) * dd], dd * 8);
    memcpy(&cnt[c * d], g.cnt.data(), (size_t)d * 8);
  }
  return gram_upload(w, C, cnt, ng);
}
int joint_chain_data_alloc(JointWork* w, int C, int rows_per_chain, int N, int d) {
  const size_t n = (size_t)C * N * d;
  if (w->x) hipFree(w->x);
  if (w->mask) hipFree(w->mask);
  if (w->any_mask_c) hipFree(w->any_mask_c);
  w->x = nullptr;
  w->mask = nullptr;
  w->any_mask_c = nullptr;
  w->n_chain_data = 0;
  const bool ok = hipMalloc((void**)&w->x, n * 4) == hipSuccess && hipMalloc((void**)&w->mask, n * 4) == hipSuccess &&
                  hipMalloc((void**)&w->any_mask_c, (size_t)C * 4) == hipSuccess && hipMemset(w->x, 0, n * 4) == hipSuccess &&
                  hipMemset(w->mask, 0, n * 4) == hipSuccess && hipMemset(w->any_mask_c, 0, (size_t)C * 4) == hipSuccess;
  if (!ok) {  // (nothing half-allocated stays behind: the workspace is without data, as before the call)
    if (w->x) hipFree(w->x);
    if (w->mask) hipFree(w->mask);
    if (w->any_mask_c) hipFree(w->any_mask_c);
    w->x = nullptr;
    w->mask = nullptr;
    w->any_mask_c = nullptr;
    return 1;
  }
  w->n_chain_data = C;
  w->chain_rows = rows_per_chain;
  w->any_mask = 0;
  return 0;
}
int joint_chain_data_set(JointWork* w, int c, const float* x, const int32_t* mask, int N, int d) {
  const size_t n = (size_t)N * d;
  int any = 0;
  if (mask)
    for (size_t i = 0; i < n; ++i) any |= mask[i] != 0;
  if (hipMemcpy(w->x + c * n, x, n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  if (mask ? hipMemcpy(w->mask + c * n, mask, n * 4, hipMemcpyHostToDevice) != hipSuccess : hipMemset(w->mask + c * n, 0, n * 4) != hipSuccess) return 1;
  if (hipMemcpy(w->any_mask_c + c, &any, 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  return 0;
}
LinChainData joint_chain_data(const JointWork& w) { return LinChainData{w.x, w.mask, w.any_mask_c, w.gram, w.ncnt, w.chain_rows, w.chain_hp}; }

static size_t ling_lds(int d, int n_gram, bool grad) {
  const size_t dd = (size_t)d * d;
  return (n_gram == 1 ? dd * 8 : 0) + (((grad ? 2 : 1) * dd * 4 + 15) & ~(size_t)15) + 128;
}
// the operands of a block (masked weights; for the gradient kernel the graph as well) beyond the LDS capacity: global scratch
// (n_vars > 198 for the log-probabilities, > 141 for the gradients)
static bool ling_ops_global(int d, bool grad) { return ling_lds(d, -1, grad) > (size_t)160 * 1024 - 1024; }
// the n_gram argument of the Gram kernels: a single matrix stays in LDS only while it fits beside the operands (d <= 101 for the gradient
// kernel); beyond that it is read through the caches (-1).  (Found by tests/tools/gpu_fuzz.py: d = 112 with 500 observations failed to launch.)
static int ling_ngram_arg(int d, int n_gram, bool grad) {
  return (n_gram == 1 && ling_lds(d, 1, grad) > (size_t)160 * 1024) ? -1 : n_gram;
}
int joint_alloc(JointWork* w, int Mloc, int d, int N, int S) {
  (void)N;
  *w = JointWork{};
  if (hipMalloc((void**)&w->wsm, (size_t)Mloc * S * 4) != hipSuccess) return 1;
  if (hipMalloc((void**)&w->ln_tab, (size_t)Mloc * d * d * 4) != hipSuccess) return 1;
  return 0;
}
void joint_free(JointWork* w) {
  if (w->x) hipFree(w->x);
  if (w->mask) hipFree(w->mask);
  if (w->wsm) hipFree(w->wsm);
  if (w->ln_tab) hipFree(w->ln_tab);
  if (w->w1t) hipFree(w->w1t);
  if (w->nng_scratch) hipFree(w->nng_scratch);
  if (w->gs_scratch) hipFree(w->gs_scratch);
  if (w->gpart) hipFree(w->gpart);
  if (w->gctr) hipFree(w->gctr);
  if (w->gplan.stats) hipFree(w->gplan.stats);
  if (w->gplan.items) hipFree(w->gplan.items);
  if (w->gplan.ctr) hipFree(w->gplan.ctr);
  if (w->nhf_w1s) hipFree(w->nhf_w1s);
  if (w->nhf_w1p) hipFree(w->nhf_w1p);
  if (w->nhf_ew) hipFree(w->nhf_ew);
  if (w->nhx_w1s) hipFree(w->nhx_w1s);
  if (w->nhx_w1p) hipFree(w->nhx_w1p);
  if (w->gram) hipFree(w->gram);
  if (w->ncnt) hipFree(w->ncnt);
  if (w->any_mask_c) hipFree(w->any_mask_c);
  *w = JointWork{};
}
float* joint_gs_scratch(JointWork* w, size_t floats) {
  if (w->gs_scratch_floats < floats) {
    if (w->gs_scratch) hipFree(w->gs_scratch);
    w->gs_scratch = nullptr;
    w->gs_scratch_floats = 0;
    if (hipMalloc((void**)&w->gs_scratch, floats * 4) != hipSuccess) return nullptr;
    w->gs_scratch_floats = floats;
  }
  return w->gs_scratch;
}
bool joint_grad_split(JointWork* w, size_t jobs, size_t stride, GradSplit* out, int ns) {
  const size_t need = jobs * (size_t)ns * stride;
  if (w->gpart_floats < need) {
    if (w->gpart) hipFree(w->gpart);
    w->gpart = nullptr;
    w->gpart_floats = 0;
    if (hipMalloc((void**)&w->gpart, need * 4) != hipSuccess) return false;
    w->gpart_floats = need;
  }
  if (w->gctr_n < jobs) {
    if (w->gctr) hipFree(w->gctr);
    w->gctr = nullptr;
    w->gctr_n = 0;
    if (hipMalloc((void**)&w->gctr, jobs * 4) != hipSuccess) return false;
    if (hipMemset(w->gctr, 0, jobs * 4) != hipSuccess) return false;
    if (hipDeviceSynchronize() != hipSuccess) return false;  // (the engine's streams do not wait for the null stream)
    w->gctr_n = jobs;
  }
  *out = GradSplit{w->gpart, w->gctr, stride};
  return true;
}
bool joint_grad_plan(JointWork* w, size_t jobs, int ns, GradPlan* out) {
  if (w->gplan_jobs < jobs || w->gplan_items < jobs * (size_t)ns) {
    if (w->gplan.stats) hipFree(w->gplan.stats);
    if (w->gplan.items) hipFree(w->gplan.items);
    if (w->gplan.ctr) hipFree(w->gplan.ctr);
    w->gplan = GradPlan{nullptr, nullptr, nullptr, nullptr};
    w->gplan_jobs = w->gplan_items = 0;
    if (hipMalloc((void**)&w->gplan.stats, jobs * 4 * sizeof(double)) != hipSuccess) return false;
    if (hipMalloc((void**)&w->gplan.items, jobs * (size_t)ns * 4) != hipSuccess) return false;
    if (hipMalloc((void**)&w->gplan.ctr, 16) != hipSuccess) return false;
    if (hipMemset(w->gplan.ctr, 0, 16) != hipSuccess) return false;
    if (hipDeviceSynchronize() != hipSuccess) return false;  // (the engine's streams do not wait for the null stream)
    w->gplan_jobs = jobs;
    w->gplan_items = jobs * (size_t)ns;
    w->gplan_gen = 0;
  }
  // two counter pairs: launch k uses pair k & 1 and its plan kernel zeroes the other one for launch k + 1 (launches of a workspace are
  // ordered in one stream)
  *out = w->gplan;
  out->ctr = w->gplan.ctr + 2 * (w->gplan_gen & 1u);
  out->ctr_next = w->gplan.ctr + 2 * ((w->gplan_gen + 1u) & 1u);
  ++w->gplan_gen;
  return true;
}
int joint_set_data(JointWork* w, const float* x, const int32_t* mask, int N, int d) {
  const size_t n = (size_t)N * d;
  if (w->x) hipFree(w->x);
  if (w->mask) hipFree(w->mask);
  // Gram matrices belong to the data set they were built from: the caller builds new ones (joint_lin_set_gram) when THIS data set takes the
  // Gram path.  (dibs_score_graphs keeps one workspace for held-out sets of any row count: a set on the LDS-resident path scored after one
  // on the Gram path was evaluated against the earlier set's matrices.)
  if (w->gram) hipFree(w->gram);
  if (w->ncnt) hipFree(w->ncnt);
  w->x = nullptr;
  w->mask = nullptr;
  w->gram = nullptr;
  w->ncnt = nullptr;
  w->n_gram = 0;
  if (hipMalloc((void**)&w->x, n * 4) != hipSuccess) return 1;
  if (hipMalloc((void**)&w->mask, n * 4) != hipSuccess) return 1;
  if (hipMemcpy(w->x, x, n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  w->any_mask = 0;
  if (mask) {
    for (size_t i = 0; i < n; ++i) w->any_mask |= mask[i] != 0;
    if (hipMemcpy(w->mask, mask, n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  } else if (hipMemset(w->mask, 0, n * 4) != hipSuccess) {
    return 1;
  }
  return 0;
}

template <int NT>
static int joint_lin_logprobs(JointWork* w, const JointLaunch& jl, Key2 carry, int mode) {
  const int spb = 4;
  const size_t lds1 = lin_lds_bytes(jl.d, jl.N, NT, false);
  if (!w->n_chain_data) allow_lds(k_lin_logprobs<NT>, lds1);  // (per-chain data: lin_chains_launch_* raise the limit of the kernels they launch)
  float* lp = mode == LIN_MODE_THETA ? jl.logprobs_th : jl.logprobs_z;
  const bool paired = jl.layout == 0 && (jl.S & 1) == 0 && (uint64_t)jl.S * jl.d * jl.d < 0xFFFFFFFFull && jl.N <= 128;
  if (paired) {
    const bool use_bf = NT <= 4 && jl.d > 32 && !jl.lin_f32;  // (lin_f32: tuning.h, the f32-MFMA kernel at 33 <= d <= 64 for A/B runs)
    // pairs per block: the block's prologue (x fragments, operand factors, zeroed images) is ~a third of a pair's work; 8 pairs when that
    // still leaves two full rounds of blocks (config 3: 1 914 -> 1 964 steps/s; 16 pairs: 1 856)
    const int ppb = (use_bf && (jl.S / 2 / 8) * jl.choice_rows() >= 1024) ? 8 : 4;
    const size_t ldsp = lin_lds_bytes_pair(jl.d, NT);
    const dim3 grid((jl.S / 2 + ppb - 1) / ppb, jl.Mloc);
    const int epq = (jl.d * jl.d + 255) / 256;
    if (use_bf) {
      const int ldsb = 2 * AHF_IMG_BYTES + 256;
      const int epq8 = (jl.d * jl.d + 511) / 512;
#define LIN_HF_LAUNCH(EPQ_, FOUR_, NW_)                                                                                                      \
      if (w->n_chain_data) {                                                                                                                 \
        lin_chains_launch_hf(EPQ_, FOUR_, grid, ldsb, joint_chain_data(*w), jl, lp, carry, mode, ppb);                                       \
      } else {                                                                                                                               \
        allow_lds(k_lin_logprobs_hf<EPQ_, FOUR_, NW_>, ldsb);                                                                                \
        hipLaunchKernelGGL((k_lin_logprobs_hf<EPQ_, FOUR_, NW_>), grid, dim3(64 * NW_), ldsb, jl.stream, w->x, w->mask, jl.theta, jl.scores, \
                           jl.thr, lp, carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S, ppb, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise,  \
                           jl.mean_edge, jl.sig_edge, w->any_mask);                                                                          \
      }
      if (jl.d <= 48) LIN_HF_LAUNCH(5, false, 8)
      else if (epq8 <= 5) LIN_HF_LAUNCH(5, true, 8)
      else LIN_HF_LAUNCH(8, true, 8)
#undef LIN_HF_LAUNCH
      return 0;
    }
#define LIN_PAIR_LAUNCH(EPQ_)                                                                                                      \
    if (w->n_chain_data) {                                                                                                         \
      lin_chains_launch_pair(NT, EPQ_, grid, ldsp, joint_chain_data(*w), jl, lp, carry, mode, ppb);                                \
    } else {                                                                                                                       \
      allow_lds(k_lin_logprobs_pair<NT, EPQ_>, ldsp);                                                                              \
      hipLaunchKernelGGL((k_lin_logprobs_pair<NT, EPQ_>), grid, dim3(256), ldsp, jl.stream, w->x, w->mask, jl.theta, jl.scores, jl.thr, lp,   \
                         carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S, ppb, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise,         \
                         jl.mean_edge, jl.sig_edge, w->any_mask);                                                                  \
    }
    if (NT <= 4 && epq <= 4) LIN_PAIR_LAUNCH(4)
    else if (NT <= 4 && epq <= 10) LIN_PAIR_LAUNCH(10)
    else if (NT <= 4) LIN_PAIR_LAUNCH(16)
    else LIN_PAIR_LAUNCH(0)
#undef LIN_PAIR_LAUNCH
  } else if (w->n_chain_data) {
    lin_chains_launch_logprobs(NT, dim3((jl.S + spb - 1) / spb, jl.Mloc), lds1, joint_chain_data(*w), jl, lp, carry, mode, spb);
  } else {
    hipLaunchKernelGGL(k_lin_logprobs<NT>, dim3((jl.S + spb - 1) / spb, jl.Mloc), dim3(256), lds1, jl.stream, w->x, w->mask, jl.theta,
                       jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S, spb, jl.alpha, jl.tau, jl.layout, jl.tiny,
                       jl.obs_noise, jl.mean_edge, jl.sig_edge, w->any_mask);
  }
  return 0;
}

template <int NT>
static int joint_lin_grads(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  const size_t lds2 = lin_lds_bytes(jl.d, jl.N, NT, true);
  if (!w->n_chain_data) allow_lds(k_lin_grad<NT>, lds2);
  const LinGradJob jt{jl.logprobs_th, jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.gtheta_off, jl.pack_stride,
                      jl.copy_theta ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.theta_off : nullptr, nullptr, carry_theta, LIN_MODE_THETA};
  const LinGradJob jz{jl.logprobs_z, jl.w_lik, (size_t)jl.d * jl.d, nullptr, jl.baseline_out, carry_z,
                      jl.est_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM};
  GradSplit gs;
  if (!joint_grad_split(w, (size_t)jl.Mloc * 2, (size_t)((NT + 3) / 4) * NT * 4 * 256, &gs)) return 1;
  if (w->n_chain_data) {
    lin_chains_launch_grad(NT, dim3(jl.Mloc, 2, GRAD_NS), lds2, joint_chain_data(*w), jl, jt, jz, gs);
    return 0;
  }
  hipLaunchKernelGGL(k_lin_grad<NT>, dim3(jl.Mloc, 2, GRAD_NS), dim3(256), lds2, jl.stream, w->x, w->mask, jl.theta, jl.scores, jl.thr, jt, jz,
                     jl.baseline, jl.m0, jl.M, jl.d, jl.N, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge,
                     jl.sig_edge, jl.sf_baseline, w->any_mask, gs);
  return 0;
}

#define LIN_NT_SWITCH(CALL_)                 \
  switch ((jl.d + 15) / 16) {                \
    case 1: return CALL_(1);                 \
    case 2: return CALL_(2);                 \
    case 3: return CALL_(3);                 \
    case 4: return CALL_(4);                 \
    case 5: return CALL_(5);                 \
    case 6: return CALL_(6);                 \
    default: return CALL_(7);                \
  }
// log p(theta, D | G_s) for the samples of the theta estimator and of the Z estimator (two launches)
int joint_lin_all_logprobs(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  const int mz = jl.est_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM;
  if (w->n_gram) {  // Gram-matrix path (x does not fit LDS)
    const bool glob = ling_ops_global(jl.d, false);
    const int ng = glob ? (w->n_gram == 1 ? -1 : w->n_gram) : ling_ngram_arg(jl.d, w->n_gram, false);
    const size_t lds = glob ? 256 : ling_lds(jl.d, ng, false);
    // (global operands: a bounded number of blocks per particle loop over the samples, each with its own d x d scratch)
    const int rows = jl.choice_rows(), gx = glob ? (jl.S < 1024 / rows ? jl.S : (1024 / rows > 1 ? 1024 / rows : 1)) : jl.S;
    float* gs = glob ? joint_gs_scratch(w, (size_t)gx * jl.Mloc * jl.d * jl.d) : nullptr;
    if (glob && !gs) return 1;
    if (w->n_chain_data) {
      const LinChainData cd = joint_chain_data(*w);
      ling_chains_launch_logprobs(dim3(gx, jl.Mloc), lds, cd, ng, jl, jl.logprobs_th, carry_theta, LIN_MODE_THETA, gs);
      ling_chains_launch_logprobs(dim3(gx, jl.Mloc), lds, cd, ng, jl, jl.logprobs_z, carry_z, mz, gs);
      return 0;
    }
    allow_lds(k_ling_logprobs, lds);
    hipLaunchKernelGGL(k_ling_logprobs, dim3(gx, jl.Mloc), dim3(256), lds, jl.stream, w->gram, w->ncnt, ng, jl.theta, jl.scores, jl.thr,
                       jl.logprobs_th, carry_theta, (int)LIN_MODE_THETA, jl.m0, jl.M, jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise,
                       jl.mean_edge, jl.sig_edge, gs);
    hipLaunchKernelGGL(k_ling_logprobs, dim3(gx, jl.Mloc), dim3(256), lds, jl.stream, w->gram, w->ncnt, ng, jl.theta, jl.scores, jl.thr,
                       jl.logprobs_z, carry_z, mz, jl.m0, jl.M, jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge,
                       jl.sig_edge, gs);
    return 0;
  }
#define LIN_CALL(NT_) (joint_lin_logprobs<NT_>(w, jl, carry_theta, LIN_MODE_THETA) || joint_lin_logprobs<NT_>(w, jl, carry_z, mz))
  LIN_NT_SWITCH(LIN_CALL)
#undef LIN_CALL
}
// both softmax-weighted gradients in one launch
int joint_lin_all_grads(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  if (w->n_gram) {
    const bool glob = ling_ops_global(jl.d, true);
    const int ng = glob ? (w->n_gram == 1 ? -1 : w->n_gram) : ling_ngram_arg(jl.d, w->n_gram, true);
    const size_t lds = glob ? 256 : ling_lds(jl.d, ng, true);
    float* gs = glob ? joint_gs_scratch(w, (size_t)GRAD_NS * 2 * jl.Mloc * 2 * jl.d * jl.d) : nullptr;
    if (glob && !gs) return 1;
    GradSplit gsp;
    if (!joint_grad_split(w, (size_t)jl.Mloc * 2, (size_t)jl.d * jl.d, &gsp)) return 1;
    if (!w->n_chain_data) allow_lds(k_ling_grad, lds);
    const LinGradJob jt{jl.logprobs_th, jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.gtheta_off, jl.pack_stride,
                        jl.copy_theta ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.theta_off : nullptr, nullptr, carry_theta, LIN_MODE_THETA};
    const LinGradJob jz{jl.logprobs_z, jl.w_lik, (size_t)jl.d * jl.d, nullptr, jl.baseline_out, carry_z,
                        jl.est_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM};
    if (w->n_chain_data) {
      ling_chains_launch_grad(dim3(jl.Mloc, 2, GRAD_NS), lds, joint_chain_data(*w), ng, jl, jt, jz, gs, gsp);
      return 0;
    }
    hipLaunchKernelGGL(k_ling_grad, dim3(jl.Mloc, 2, GRAD_NS), dim3(256), lds, jl.stream, w->gram, ng, jl.theta, jl.scores, jl.thr, jt, jz, jl.baseline,
                       jl.m0, jl.M, jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge, jl.sf_baseline, gs, gsp);
    return 0;
  }
#define LIN_CALL(NT_) joint_lin_grads<NT_>(w, jl, carry_theta, carry_z)
  LIN_NT_SWITCH(LIN_CALL)
#undef LIN_CALL
}
#undef LIN_NT_SWITCH

template <int NT>
static void launch_lin_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, float obs_noise,
                             float mean_edge, float sig_edge, hipStream_t stream) {
  const size_t lds = lin_lds_bytes(d, N, NT, false);
  allow_lds(k_lin_logprobs<NT>, lds);
  hipLaunchKernelGGL(k_lin_logprobs<NT>, dim3(1, n), dim3(256), lds, stream, jw.x, jw.mask, theta, (const float*)nullptr,
                     reinterpret_cast<const uint32_t*>(g), out, Key2{0, 0}, (int)LIN_MODE_GIVEN, 0, n, d, N, 1, 1, 0.f, 1.f, 0, 0,
                     obs_noise, mean_edge, sig_edge, jw.any_mask);
}
int joint_lin_score_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, float obs_noise,
                          float mean_edge, float sig_edge, hipStream_t stream) {
  if (jw.n_gram) {
    const bool glob = ling_ops_global(d, false);
    const int ng = glob ? (jw.n_gram == 1 ? -1 : jw.n_gram) : ling_ngram_arg(d, jw.n_gram, false);
    const size_t lds = glob ? 256 : ling_lds(d, ng, false);
    float* gs = glob ? joint_gs_scratch(const_cast<JointWork*>(&jw), (size_t)n * d * d) : nullptr;
    if (glob && !gs) return 1;
    allow_lds(k_ling_logprobs, lds);
    hipLaunchKernelGGL(k_ling_logprobs, dim3(1, n), dim3(256), lds, stream, jw.gram, jw.ncnt, ng, theta, (const float*)nullptr,
                       reinterpret_cast<const uint32_t*>(g), out, Key2{0, 0}, (int)LIN_MODE_GIVEN, 0, n, d, 1, 0.f, 1.f, 0, 0, obs_noise, mean_edge,
                       sig_edge, gs);
    return 0;
  }
  switch ((d + 15) / 16) {
    case 1: launch_lin_given<1>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    case 2: launch_lin_given<2>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    case 3: launch_lin_given<3>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    case 4: launch_lin_given<4>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    case 5: launch_lin_given<5>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    case 6: launch_lin_given<6>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
    default: launch_lin_given<7>(jw, theta, g, out, n, d, N, obs_noise, mean_edge, sig_edge, stream); break;
  }
  return 0;
}
