// translation unit: the soft-graph BGe estimator (MarginalDiBS + BGe, grad_estimator_z = "reparam"): its kernels (kernels_bge_soft.h,
// kernels_bge_soft_mf.h) and their launcher
#define DIBS_TU_BGE_SOFT
#include "launch.h"
#include "kernels_bge_soft.h"
#include "kernels_bge_soft_mf.h"

// both launches of the estimator: per-sample soft-graph scores + gradients, then the softmax-weighted combination
void bge_soft_launch(const BgeSoftParams& sp, const float* scores, Key2 carry, int m0, int M, int Mloc, int d, int S, float alpha,
                     float tau, int layout, int tiny, float* soft_ds, float* logprobs, float* w_lik, hipStream_t stream, float* tri_glob,
                     int glob_blocks) {
  if (d > 128) {  // packed triangles in global scratch (tri_glob: glob_blocks * 4 waves * 2 * tri(d) floats), persistent blocks
    hipLaunchKernelGGL((k_bge_soft<false, 4, true>), dim3(glob_blocks), dim3(256), bge_soft_glob_lds_bytes(), stream, scores, sp, carry, m0, M, d, S,
                       alpha, tau, layout, tiny, soft_ds, logprobs, tri_glob, S * Mloc);
    hipLaunchKernelGGL(k_soft_combine, dim3(Mloc, (d * d + 255) / 256), dim3(256), (size_t)S * 4 + 16, stream, soft_ds, logprobs, w_lik, d, S);
    return;
  }
  const bool rl = sp.n_mats == 1 && bge_soft_waves(d, true) >= (bge_soft_waves(d, false) < 4 ? bge_soft_waves(d, false) : 4);
  const size_t lds = bge_soft_lds_bytes(d, rl);
#define SOFT_LAUNCH(RL_, RPL_)                                                                                                          \
  {                                                                                                                                     \
    allow_lds(k_bge_soft<RL_, RPL_>, lds);                                                                                              \
    hipLaunchKernelGGL((k_bge_soft<RL_, RPL_>), dim3(S, Mloc), dim3(256), lds, stream, scores, sp, carry, m0, M, d, S, alpha, tau, layout, \
                       tiny, soft_ds, logprobs, (float*)nullptr, 1);                                                                    \
  }
  if (d <= 64) {
    // blocked factorisation on the matrix pipe (kernels_bge_soft_mf.h)
    const bool rr = sp.n_mats == 1;
    const size_t l2 = bsm_lds_bytes(d, rr);
#define SOFTM(NB_, RL_, W_)                                                                                                             \
  {                                                                                                                                     \
    allow_lds(k_bge_soft_mf<NB_, RL_, W_>, l2);                                                                                         \
    hipLaunchKernelGGL((k_bge_soft_mf<NB_, RL_, W_>), dim3(S, Mloc), dim3(256), l2, stream, scores, sp, carry, m0, M, d, S, alpha, tau, layout, \
                       tiny, soft_ds, logprobs);                                                                                        \
  }
    // (three waves per SIMD: 165 registers, no scratch -- 4.6 ms against 5.4 at two)
    switch ((d + 15) / 16) {
      case 1: if (rr) SOFTM(1, true, 3) else SOFTM(1, false, 3) break;
      case 2: if (rr) SOFTM(2, true, 3) else SOFTM(2, false, 3) break;
      case 3: if (rr) SOFTM(3, true, 3) else SOFTM(3, false, 3) break;
      default: if (rr) SOFTM(4, true, 3) else SOFTM(4, false, 3) break;
    }
#undef SOFTM
  } else {
    if (rl) SOFT_LAUNCH(true, 2) else SOFT_LAUNCH(false, 2)
  }
#undef SOFT_LAUNCH
  hipLaunchKernelGGL(k_soft_combine, dim3(Mloc, (d * d + 255) / 256), dim3(256), (size_t)S * 4 + 16, stream, soft_ds, logprobs, w_lik, d, S);
}
