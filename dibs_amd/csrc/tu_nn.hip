// translation unit: the JointDiBS + DenseNonlinearGaussian kernels and their launchers -- the tuned one-hidden-layer kernels (kernels_nn.h, on the
// f16 matrix pipe kernels_nn_f16.h / kernels_nn_f16x.h) and the general path (kernels_nn_generic.h)
#define DIBS_TU_NN
#include "launch.h"
#include "kernels_nn.h"
#include "kernels_nn_generic.h"
#include "kernels_nn_f16.h"
#include "kernels_nn_f16x.h"

// first layer on the f16 matrix pipe (kernels_nn_f16.h): 33 <= d <= 112, Threefry-paired samples, tables allocated; DIBS_NN_F32=1 keeps
// the f32-MFMA kernel (A/B runs).  Returns false when the f32 kernel has to run.
template <int NT>
static bool joint_nn_logprobs_hf(JointWork* w, const JointLaunch& jl, Key2 carry, int mode, const NNParams& np_, size_t P, float* lp) {
  if constexpr (NT < 3) {
    return false;
  } else {
    const bool off = jl.nn_f32 != 0;  // (tuning.h)
    const bool paired = jl.layout == 0 && (jl.S & 1) == 0 && (uint64_t)jl.S * jl.d * jl.d < 0xFFFFFFFFull;
    const bool soft = mode == LIN_MODE_Z_REPARAM;
    const size_t lds = nhf_lds_bytes(jl.d, NT, np_.H, soft);
    if (mode == LIN_MODE_THETA) w->nhf_valid = w->nhx_valid = false;  // (theta moved since the last step)
    if (off || !paired || jl.N > 128 || !w->ln_tab) return false;
    const int hS = jl.S / 2, ppb = (hS / 4) * jl.choice_rows() >= 1024 ? 4 : (hS >= 2 ? 2 : 1);
    if (!w->nhf_ew && hipMalloc((void**)&w->nhf_ew, (size_t)jl.Mloc * 4) != hipSuccess) {
      (void)hipGetLastError();
      w->nhf_ew = nullptr;
      return false;
    }
    // d >= 65: the per-sample operand in REGISTERS against an x^T image (k_nn_logprobs_hx: no block barrier per hidden unit); below
    // the image variant (k_nn_logprobs_hf: smaller blocks, several per CU)
    if constexpr (NT >= 5) {
      const size_t ldsx = nhx_lds_bytes(jl.d, NT, jl.N, np_.H, soft);
      if (ldsx <= (size_t)160 * 1024 - 512) {
        const size_t quads = (size_t)jl.Mloc * np_.H * ((jl.d + 3) / 4) * jl.d;
        if (w->nhx_quads < quads) {
          if (w->nhx_w1s) hipFree(w->nhx_w1s);
          if (w->nhx_w1p) hipFree(w->nhx_w1p);
          w->nhx_w1s = w->nhx_w1p = nullptr;
          w->nhx_quads = 0;
          w->nhx_valid = false;
          if (hipMalloc(&w->nhx_w1s, quads * 16) != hipSuccess || hipMalloc(&w->nhx_w1p, quads * 16) != hipSuccess) {
            (void)hipGetLastError();
            return false;
          }
          w->nhx_quads = quads;
        }
        if (!w->nhx_valid) {  // theta is the same for both estimators of a step: the tables are built once per step and variant
          hipLaunchKernelGGL(k_nn_w1_exp, dim3(jl.Mloc), dim3(1024), 0, jl.stream, jl.theta, P, w->nhf_ew, jl.d, np_.H);
          allow_lds(k_nn_tables_hx, (size_t)256 * np_.H * 4);
          hipLaunchKernelGGL(k_nn_tables_hx, dim3((jl.d + 15) / 16, (jl.d + 15) / 16, jl.Mloc), dim3(256), (size_t)256 * np_.H * 4, jl.stream, jl.theta, P,
                             w->nhf_ew, (float4*)w->nhx_w1s, (uint4*)w->nhx_w1p, jl.d, np_.H);
          w->nhx_valid = true;
        }
#define NHX_LAUNCH(NTN_, ACT_, SOFT_)                                                                                                        \
        {                                                                                                                                    \
          allow_lds(k_nn_logprobs_hx<NT, NTN_, ACT_, SOFT_>, ldsx);                                                                          \
          hipLaunchKernelGGL((k_nn_logprobs_hx<NT, NTN_, ACT_, SOFT_>), dim3((hS + ppb - 1) / ppb, (jl.Mloc + 7) & ~7), dim3(64 * NT), ldsx,  \
                             jl.stream, w->x, w->mask, jl.theta, P, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.Mloc, jl.d, jl.N,    \
                             jl.S, ppb, jl.alpha, jl.tau, jl.layout, jl.tiny, np_, w->any_mask, w->ln_tab, (const float4*)w->nhx_w1s,        \
                             (const uint4*)w->nhx_w1p, w->nhf_ew);                                                                           \
        }
#define NHX_PICK(NTN_)                                                                                                                       \
        if (soft) {                                                                                                                          \
          if (np_.act == 0) NHX_LAUNCH(NTN_, 0, true) else NHX_LAUNCH(NTN_, -1, true)                                                         \
        } else {                                                                                                                             \
          if (np_.act == 0) NHX_LAUNCH(NTN_, 0, false) else NHX_LAUNCH(NTN_, -1, false)                                                       \
        }
        if (jl.N <= 112) { NHX_PICK(7) } else { NHX_PICK(8) }
#undef NHX_PICK
#undef NHX_LAUNCH
        return true;
      }
    }
    if (lds > (size_t)160 * 1024 - 512) return false;
    const size_t pairs = (size_t)jl.Mloc * np_.H * jl.d * (nhf_dp2(jl.d) / 2);
    if (w->nhf_pairs < pairs) {
      if (w->nhf_w1s) hipFree(w->nhf_w1s);
      if (w->nhf_w1p) hipFree(w->nhf_w1p);
      w->nhf_w1s = w->nhf_w1p = nullptr;
      w->nhf_pairs = 0;
      w->nhf_valid = false;
      if (hipMalloc(&w->nhf_w1s, pairs * 8) != hipSuccess || hipMalloc(&w->nhf_w1p, pairs * 8) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      w->nhf_pairs = pairs;
    }
    if (!w->nhf_valid) {  // (once per step and variant, see JointWork)
      hipLaunchKernelGGL(k_nn_w1_exp, dim3(jl.Mloc), dim3(1024), 0, jl.stream, jl.theta, P, w->nhf_ew, jl.d, np_.H);
      const int npr = jl.d * (nhf_dp2(jl.d) / 2);
      hipLaunchKernelGGL(k_nn_tables_hf, dim3((npr + 255) / 256, np_.H, jl.Mloc), dim3(256), 0, jl.stream, jl.theta, P, w->nhf_ew,
                         (float2*)w->nhf_w1s, (uint2*)w->nhf_w1p, jl.d, np_.H);
      w->nhf_valid = true;
    }
#define NHF_LAUNCH(ACT_, SOFT_)                                                                                                               \
    {                                                                                                                                         \
      allow_lds(k_nn_logprobs_hf<NT, ACT_, SOFT_>, lds);                                                                                      \
      hipLaunchKernelGGL((k_nn_logprobs_hf<NT, ACT_, SOFT_>), dim3((hS + ppb - 1) / ppb, (jl.Mloc + 7) & ~7), dim3(NHF_NTHR), lds, jl.stream, \
                         w->x, w->mask, jl.theta, P, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.Mloc, jl.d, jl.N, jl.S, ppb, jl.alpha, jl.tau, \
                         jl.layout, jl.tiny, np_, w->any_mask, w->ln_tab, (const float2*)w->nhf_w1s, (const uint2*)w->nhf_w1p, w->nhf_ew);    \
    }
    if (soft) {
      if (np_.act == 0) NHF_LAUNCH(0, true) else NHF_LAUNCH(-1, true)
    } else {
      if (np_.act == 0) NHF_LAUNCH(0, false) else NHF_LAUNCH(-1, false)
    }
#undef NHF_LAUNCH
    return true;
  }
}

template <int NT>
static int joint_nn_launch(JointWork* w, const JointLaunch& jl, Key2 carry, int mode, const NNParams& np_, size_t P) {
  // samples per block: the block's prologue (x and the small leaves into LDS, validity bits) is shared by them; 4 while that leaves at least
  // four rounds of blocks (config 5: spb 2 / 4 / 8 -> 51.2 / 53.0 / 53.1 steps/s)
  const int spb = (jl.S / 4) * jl.choice_rows() >= 1024 ? 4 : 2;
  const size_t lds1 = nn_lds_bytes_logprobs(jl.d, jl.N, NT, np_.H);
  float* lp = mode == LIN_MODE_THETA ? jl.logprobs_th : jl.logprobs_z;
  const size_t w1t_need = (size_t)jl.Mloc * np_.H * jl.d * jl.d;
  if (w->w1t_floats < w1t_need) {  // (first launch)
    if (w->w1t) hipFree(w->w1t);
    w->w1t = nullptr;
    w->w1t_floats = hipMalloc((void**)&w->w1t, w1t_need * 4) == hipSuccess ? w1t_need : 0;
    if (!w->w1t_floats) w->w1t = nullptr;
  }
  if (!w->w1t || !w->ln_tab) return 1;  // (k_nn_grad reads both)
  if (mode == LIN_MODE_THETA) {  // theta is the same for both estimators of a step: the tables are built once (theta runs first)
    allow_lds(k_nn_prior_table, (size_t)256 * np_.H * 4);
    hipLaunchKernelGGL(k_nn_prior_table, dim3((jl.d + 15) / 16, (jl.d + 15) / 16, jl.Mloc), dim3(256), (size_t)256 * np_.H * 4, jl.stream, jl.theta, P,
                       w->ln_tab, w->w1t, jl.d, np_.H, np_.sig_param);
  }
#define NN_LP_LAUNCH(NW_, ACT_)                                                                                                             \
  {                                                                                                                                         \
    allow_lds(k_nn_logprobs<NT, NW_, ACT_>, lds1);                                                                                          \
    hipLaunchKernelGGL((k_nn_logprobs<NT, NW_, ACT_>), dim3((jl.S + spb - 1) / spb, jl.Mloc), dim3(64 * NW_), lds1, jl.stream, w->x, w->mask,   \
                       jl.theta, P, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S, spb, jl.alpha, jl.tau, jl.layout,    \
                       jl.tiny, np_, w->any_mask, w->ln_tab, w->w1t);                                                                       \
  }
  if (joint_nn_logprobs_hf<NT>(w, jl, carry, mode, np_, P, lp)) {
    // (log-probs done on the f16 matrix pipe)
  } else if (lds1 > 80 * 1024) {  // one block per CU: run it with 16 waves
    if (np_.act == 0) NN_LP_LAUNCH(16, 0) else NN_LP_LAUNCH(16, -1)
  } else {
    if (np_.act == 0) NN_LP_LAUNCH(4, 0) else NN_LP_LAUNCH(4, -1)
  }
#undef NN_LP_LAUNCH
  float* out = mode == LIN_MODE_THETA ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.gtheta_off : jl.w_lik;
  const size_t ostride = mode == LIN_MODE_THETA ? jl.pack_stride : (size_t)jl.d * jl.d;
  float* tcopy = (mode == LIN_MODE_THETA && jl.copy_theta) ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.theta_off : nullptr;
  GradSplit gs;  // (several blocks per particle once many samples keep a non-zero weight: kernels_joint.h)
  // (partial row of a block: the first-layer gradient in thread layout + the small leaves for theta, d*d for Z; the shares per particle are
  //  cut back when GRAD_NS_NN rows per particle would exceed 4 GiB -- hidden widths in the dozens)
  const int hcs = nn_grad_hcs(jl.d, jl.N, NT, np_.H);  // (> 0: joint_nn_fast_path)
  const size_t lds2 = nn_grad_lds_bytes(jl.d, jl.N, NT, hcs);
  const bool wide = lds2 > 80 * 1024;  // one block per CU: 8 waves (see k_nn_grad)
  const int nthr = wide ? 512 : 256, nudm = wide ? 1 : 2;  // (k_nn_grad: NTHR, NUDM)
  const size_t row_theta = (size_t)NT * nudm * np_.H * 4 * nthr + (P - (size_t)jl.d * jl.d * np_.H);
  const size_t row = row_theta > (size_t)jl.d * jl.d ? row_theta : (size_t)jl.d * jl.d;
  int ns_nn = GRAD_NS_NN;
  while (ns_nn > 1 && (size_t)jl.choice_rows() * ns_nn * row * 4 > ((size_t)4 << 30)) ns_nn >>= 1;
  // (chains engine: the shares are one chain's, so that its sums are grouped as its standalone engine groups them; all chains' rows must fit)
  if (jl.M_choice > 0 && (size_t)jl.Mloc * ns_nn * row * 4 > ((size_t)4 << 30)) return 1;
  if (!joint_grad_split(w, (size_t)jl.Mloc, row, &gs, ns_nn)) return 1;
  GradPlan gp;
  if (!joint_grad_plan(w, (size_t)jl.Mloc, ns_nn, &gp)) return 1;
  hipLaunchKernelGGL(k_grad_plan, dim3(jl.Mloc), dim3(64), 0, jl.stream, lp, jl.S, ns_nn, gp);
  // persistent blocks: as many as are resident at once (one per CU when a block fills the LDS, else two), at most one per item
  const long max_items = (long)jl.Mloc * ns_nn;
  const int resident = dibs_cu_count() * (wide ? 1 : 2);
  const int nblk = (int)(max_items < resident ? max_items : resident);
#define NN_GRAD_LAUNCH(ACT_, NW_)                                                                                                              \
  {                                                                                                                                            \
    allow_lds(k_nn_grad<ACT_, NW_>, lds2);                                                                                                     \
    hipLaunchKernelGGL((k_nn_grad<ACT_, NW_>), dim3(nblk), dim3(64 * NW_), lds2, jl.stream, w->x, w->mask, jl.theta, P, jl.scores,               \
                       jl.thr, lp, out, ostride, tcopy, jl.baseline, mode == LIN_MODE_THETA ? (float*)nullptr : jl.baseline_out, carry, mode,    \
                       jl.m0, jl.M, jl.d, jl.N, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, np_, jl.sf_baseline, w->any_mask, gs,                \
                       w->w1t, w->ln_tab, NT, hcs, gp, ns_nn);                                                                               \
  }
  if (wide) {
    if (np_.act == 0) NN_GRAD_LAUNCH(0, 8) else NN_GRAD_LAUNCH(-1, 8)
  } else {
    if (np_.act == 0) NN_GRAD_LAUNCH(0, 4) else NN_GRAD_LAUNCH(-1, 4)
  }
#undef NN_GRAD_LAUNCH
  return 0;
}

#ifdef DIBS_NN_STAMPS
extern "C" void dibs_debug_nn_stamps(unsigned long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_stamps), sizeof(unsigned long long) * 128);
  if (reset) {
    unsigned long long z[128] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(g_nn_stamps), z, sizeof(z));
  }
}
#endif
bool joint_nn_fast_path(int d, int N, const NNParams& np_) {
  return np_.n_hidden == 1 && np_.H >= 1 && np_.H <= 64 && N <= 128 && d <= 112 && nn_grad_hcs(d, N, (d + 15) / 16, np_.H) > 0 &&
         nn_lds_bytes_logprobs(d, N, (d + 15) / 16, np_.H) <= (size_t)160 * 1024 - 512;
}

// scratch of the general path: grown on first use (activation records of the work items; see kernels_nn_generic.h)
static float* nng_scratch(JointWork* w, size_t floats) {
  if (w->nng_scratch_floats < floats) {
    if (w->nng_scratch) hipFree(w->nng_scratch);
    w->nng_scratch = nullptr;
    w->nng_scratch_floats = 0;
    if (hipMalloc((void**)&w->nng_scratch, floats * 4) != hipSuccess) return nullptr;
    w->nng_scratch_floats = floats;
  }
  return w->nng_scratch;
}

// blocks of the persistent log-prob kernel (each owns 256 * hsum floats of activation records)
static int nng_blocks(long work) { return (int)(work < 2048 ? work : 2048); }

static int joint_nng_launch(JointWork* w, const JointLaunch& jl, Key2 carry, int mode, const NNParams& np_) {
  const NNNet net = nn_net(jl.d, np_);
  size_t lds = (((size_t)jl.d * jl.d + 3) & ~(size_t)3) * 4 + 128;
  const int nb = nng_blocks((long)jl.S * jl.Mloc);
  // shares per particle of the gradient kernel (GradSplit): as many as keep its per-block activation records within 2 GiB and its partial
  // rows within 2 GiB
  int ns_g = GRAD_NS;
  const size_t rec = (size_t)2 * net.hsum * jl.d * jl.N, row = (size_t)net.P > (size_t)jl.d * jl.d ? (size_t)net.P : (size_t)jl.d * jl.d;
  const size_t crows = (size_t)jl.choice_rows();
  while (ns_g > 1 && (crows * ns_g * rec * 4 > ((size_t)2 << 30) || crows * ns_g * row * 4 > ((size_t)2 << 30))) ns_g >>= 1;
  // (chains engine: one chain's shares, as above)
  if (jl.M_choice > 0 && ((size_t)jl.Mloc * ns_g * rec * 4 > ((size_t)2 << 30) || (size_t)jl.Mloc * ns_g * row * 4 > ((size_t)2 << 30))) return 1;
  const size_t need1 = (size_t)nb * 256 * net.hsum, need2 = (size_t)jl.Mloc * ns_g * rec;
  float* scr = nng_scratch(w, need1 > need2 ? need1 : need2);
  if (!scr) return 1;
  float* gs = nullptr;  // (n_vars > 198: the sampled graph of a block does not fit LDS -- global scratch)
  if (lds > (size_t)160 * 1024 - 1024) {
    const size_t nblk = (size_t)jl.Mloc * ns_g;
    gs = joint_gs_scratch(w, ((size_t)nb > nblk ? (size_t)nb : nblk) * jl.d * jl.d);
    if (!gs) return 1;
    lds = 256;
  }
  GradSplit gsp;
  if (!joint_grad_split(w, (size_t)jl.Mloc, row, &gsp, ns_g)) return 1;
  float* lp = mode == LIN_MODE_THETA ? jl.logprobs_th : jl.logprobs_z;
  allow_lds(k_nng_logprobs, lds);
  allow_lds(k_nng_grad, lds);
  hipLaunchKernelGGL(k_nng_logprobs, dim3(nb), dim3(256), lds, jl.stream, w->x, w->mask, jl.theta, jl.scores, jl.thr, lp, carry, mode,
                     jl.m0, jl.M, jl.d, jl.N, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, np_, w->any_mask, scr, jl.Mloc, gs);
  float* out = mode == LIN_MODE_THETA ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.gtheta_off : jl.w_lik;
  const size_t ostride = mode == LIN_MODE_THETA ? jl.pack_stride : (size_t)jl.d * jl.d;
  float* tcopy = (mode == LIN_MODE_THETA && jl.copy_theta) ? jl.pack + (size_t)jl.m0 * jl.pack_stride + jl.theta_off : nullptr;
  hipLaunchKernelGGL(k_nng_grad, dim3(jl.Mloc, ns_g), dim3(256), lds, jl.stream, w->x, w->mask, jl.theta, jl.scores, jl.thr, lp, out, ostride, tcopy,
                     jl.baseline, mode == LIN_MODE_THETA ? (float*)nullptr : jl.baseline_out, carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S,
                     jl.alpha, jl.tau, jl.layout, jl.tiny, np_, jl.sf_baseline, w->any_mask, scr, gs, gsp);
  return 0;
}

int joint_nn_dispatch(JointWork* w, const JointLaunch& jl, Key2 carry, int mode, const NNParams& np_, size_t P) {
  if (!joint_nn_fast_path(jl.d, jl.N, np_)) {
    return joint_nng_launch(w, jl, carry, mode, np_);
  }
  switch ((jl.d + 15) / 16) {
    case 1: return joint_nn_launch<1>(w, jl, carry, mode, np_, P);
    case 2: return joint_nn_launch<2>(w, jl, carry, mode, np_, P);
    case 3: return joint_nn_launch<3>(w, jl, carry, mode, np_, P);
    case 4: return joint_nn_launch<4>(w, jl, carry, mode, np_, P);
    case 5: return joint_nn_launch<5>(w, jl, carry, mode, np_, P);
    case 6: return joint_nn_launch<6>(w, jl, carry, mode, np_, P);
    default: return joint_nn_launch<7>(w, jl, carry, mode, np_, P);
  }
}

template <int NT>
static void launch_nn_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N,
                            const NNParams& np_, size_t P, hipStream_t stream) {
  const size_t lds = nn_lds_bytes_logprobs(d, N, NT, np_.H);
  allow_lds(k_nn_logprobs<NT, 4>, lds);
  hipLaunchKernelGGL((k_nn_logprobs<NT, 4>), dim3(1, n), dim3(256), lds, stream, jw.x, jw.mask, theta, P, (const float*)nullptr,
                     reinterpret_cast<const uint32_t*>(g), out, Key2{0, 0}, (int)LIN_MODE_GIVEN, 0, n, d, N, 1, 1, 0.f, 1.f, 0, 0, np_,
                     jw.any_mask, (const float*)nullptr, (const float*)nullptr);
}
int joint_nn_score_given(const JointWork& jw, const float* theta, const int32_t* g, float* out, int n, int d, int N, const NNParams& np_,
                         size_t P, hipStream_t stream) {
  if (!joint_nn_fast_path(d, N, np_)) {
    const NNNet net = nn_net(d, np_);
    size_t lds = (((size_t)d * d + 3) & ~(size_t)3) * 4 + 128;
    const int nb = nng_blocks(n);
    float* scr = nng_scratch(const_cast<JointWork*>(&jw), (size_t)nb * 256 * net.hsum);
    if (!scr) return 1;
    float* gs = nullptr;
    if (lds > (size_t)160 * 1024 - 1024) {
      gs = joint_gs_scratch(const_cast<JointWork*>(&jw), (size_t)nb * d * d);
      if (!gs) return 1;
      lds = 256;
    }
    allow_lds(k_nng_logprobs, lds);
    hipLaunchKernelGGL(k_nng_logprobs, dim3(nb), dim3(256), lds, stream, jw.x, jw.mask, theta, (const float*)nullptr,
                       reinterpret_cast<const uint32_t*>(g), out, Key2{0, 0}, (int)LIN_MODE_GIVEN, 0, n, d, N, 1, 0.f, 1.f, 0, 0, np_, jw.any_mask, scr, n, gs);
    return 0;
  }
  switch ((d + 15) / 16) {
    case 1: launch_nn_given<1>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    case 2: launch_nn_given<2>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    case 3: launch_nn_given<3>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    case 4: launch_nn_given<4>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    case 5: launch_nn_given<5>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    case 6: launch_nn_given<6>(jw, theta, g, out, n, d, N, np_, P, stream); break;
    default: launch_nn_given<7>(jw, theta, g, out, n, d, N, np_, P, stream); break;
  }
  return 0;
}
void joint_nn_init_theta(float* theta, size_t P, Key2 key, int m0, int Mloc, int M, int d, const NNParams& np_, int layout, hipStream_t stream) {
  const int nt = Mloc * d;
  (void)P;
  hipLaunchKernelGGL(k_nng_init_theta, dim3((nt + 63) / 64), dim3(64), 0, stream, theta, key, m0, Mloc, M, d, np_, layout);
}
