// translation unit: the joint models' workspace (JointWork: allocation, data, scratch areas) and the JointDiBS + LinearGaussian kernels
// (kernels_lin.h, kernels_lin_gram.h) with their launch text (lin_launch.h) in the form that has one data set for every block.  The two
// public launchers at the end hand a chains engine with per-chain data (JointWork::n_chain_data) to the same launch text as compiled in
// tu_lin_chains.hip.
#define DIBS_TU_LIN
#include "launch.h"
#include "kernels_lin.h"
#include "kernels_lin_gram.h"
#include "lin_launch.h"
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


// ---- the launchers (lin_launch.h) ---------------------------------------------------------------------------------------------------------
// The only two places that look at the form of the data: a chains engine with per-chain data takes the same launch text as compiled in
// tu_lin_chains.hip.  (Non-zero: a scratch area could not be allocated, nothing was launched from that point on.)
int joint_lin_all_logprobs(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  return w->n_chain_data ? lin_all_logprobs_chains(w, jl, carry_theta, carry_z) : lin_all_logprobs(w, jl, carry_theta, carry_z);
}
int joint_lin_all_grads(JointWork* w, const JointLaunch& jl, Key2 carry_theta, Key2 carry_z) {
  return w->n_chain_data ? lin_all_grads_chains(w, jl, carry_theta, carry_z) : lin_all_grads(w, jl, carry_theta, carry_z);
}

// held-out scoring (shared form only): one block per given (graph, parameter) pair, through the launch functions of a step
int joint_lin_score_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, float obs_noise,
                          float mean_edge, float sig_edge, hipStream_t stream) {
  JointLaunch jl{};
  jl.stream = stream;
  jl.theta = theta;
  jl.thr = reinterpret_cast<const uint32_t*>(g);
  jl.M = n, jl.d = d, jl.N = N, jl.S = 1;
  jl.tau = 1.f;
  jl.obs_noise = obs_noise, jl.mean_edge = mean_edge, jl.sig_edge = sig_edge;
  if (jw.n_gram) {
    const LingShape sh = ling_shape(d, jw.n_gram, false, n);
    float* gs = sh.glob ? joint_gs_scratch(const_cast<JointWork*>(&jw), sh.scratch) : nullptr;
    if (sh.glob && !gs) return 1;
    ling_launch_logprobs(dim3(1, n), sh.lds, jw, sh.ng, jl, out, Key2{0, 0}, LIN_MODE_GIVEN, gs);
    return 0;
  }
  return lin_nt_dispatch(d, [&](auto nt) {
    lin_launch_unpaired<decltype(nt)::value>(dim3(1, n), jw, jl, out, Key2{0, 0}, LIN_MODE_GIVEN, 1);
    return 0;
  });
}
