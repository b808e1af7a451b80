// translation unit: BGe sampling / factorisation kernels and their launchers (kernels_bge.h)
#define DIBS_TU_BGE
#include "launch.h"
#include <stdlib.h>

size_t bge_sample_lds_bytes(int d, int S, int W) { return BGE_SAMPLE_WAVES * bge_sample_wave_bytes(d, S, W); }

// grid of k_bge_sample: one wave per column of the Mloc * d, dealt from a flat index (kernels_bge.h, K2) -- 1 600 blocks at the headline
// size, none of their waves idle -- and the riders (kf.z: Mloc * ceil(M / KMAT_BT) kernel-matrix blocks) in a range of their own behind them
void bge_launch_sample(bool sample, hipStream_t stream, const uint32_t* thr, uint64_t* masks, double* node_scores, const BgeParams& bp,
                       Key2 carry, int m0, int M, int Mloc, int d, int S, int W, int layout, const BgeQueues& qs, const KmatFuse& kf_in) {
  constexpr int WV = BGE_SAMPLE_WAVES;
  size_t lds = bge_sample_lds_bytes(d, S, W);
  KmatFuse kf = kf_in;
  kf.nbx = (int)(((long long)Mloc * d + WV - 1) / WV);  // (first rider block: whatever the caller put there described the old 2-D grid)
  int extra = 0;
  if (kf.z) {
    const size_t kl = (size_t)kf.len * 4 + 64;
    lds = lds > kl ? lds : kl;
    extra = Mloc * ((kf.M + KMAT_BT - 1) / KMAT_BT);
  }
  const dim3 grid(kf.nbx + extra), block(64 * WV);
  // (instantiations by role: riders or none, the paired fast loop or the generic ones -- see the template's header)
#define SAMPLE_K(...)                                                                                                              \
  {                                                                                                                                \
    allow_lds((k_bge_sample<WV, __VA_ARGS__>), lds);                                                                               \
    hipLaunchKernelGGL((k_bge_sample<WV, __VA_ARGS__>), grid, block, lds, stream, thr, masks, node_scores, bp, carry, m0, M, Mloc, d, S, W, \
                       layout, qs, kf);                                                                                            \
  }
  const bool fast = bge_sample_fast(d, S, W, layout), riders = kf.z != nullptr;
  if (!sample) SAMPLE_K(false)
  else if (riders && fast) SAMPLE_K(true, false, true, true)
  else if (riders) SAMPLE_K(true, false, true, false)
  else if (fast) SAMPLE_K(true, false, false, true)
  else SAMPLE_K(true, false, false, false)
#undef SAMPLE_K
}

void bge_launch_chol(hipStream_t stream, double* node_scores, const BgeParams& bp, const BgeQueues& qs, int d, int S,
                     unsigned long long* counters) {
  if (d > 128) {  // three or four mask words: one problem per wave, everything in the last tier (k_bge_chol_wide)
    const size_t lw = BGE_WIDE_WAVES * bge_wide_wave_bytes(d);
    allow_lds(k_bge_chol_wide<false>, lw);
    hipLaunchKernelGGL(k_bge_chol_wide<false>, dim3(2048), dim3(64 * BGE_WIDE_WAVES), lw, stream, node_scores, bp, qs, d, (d + 63) / 64);
    return;
  }
  const bool w2 = d > 64;
  bool rl = bp.n_mats == 1;
  if (rl && bge_chol_lds_bytes(d, true) > (size_t)150 * 1024) rl = false;
  const size_t lds = bge_chol_lds_bytes(d, rl);
  const dim3 grid(512), block(256);  // (512 = the resident blocks at two waves per SIMD: R / Q are staged once per slot; 1024: +2 us)
#define CHOL(RL_, W2_)                                                                                                  \
  {                                                                                                                     \
    allow_lds(k_bge_chol<RL_, W2_>, lds);                                                                               \
    hipLaunchKernelGGL((k_bge_chol<RL_, W2_>), grid, block, lds, stream, node_scores, bp, qs, d, S, counters);                    \
  }
  if (rl && !w2) CHOL(true, false)
  else if (rl) CHOL(true, true)
  else if (!w2) CHOL(false, false)
  else CHOL(false, true)
#undef CHOL
}

// batched engines (BgeParams::pM particles per problem, statistics stacked problem-major): the BATCH instantiations, no kernel-matrix
// blocks, matrices read through the caches
void bge_launch_sample_batch(hipStream_t stream, const uint32_t* thr, uint64_t* masks, double* node_scores, const BgeParams& bp, Key2 carry,
                             int Mloc, int d, int S, int W, int layout, const BgeQueues& qs) {
  constexpr int WV = BGE_SAMPLE_WAVES;
  const size_t lds = bge_sample_lds_bytes(d, S, W);
  const KmatFuse kf{nullptr, nullptr, 0, 0, 0, 0.f, 0.f, nullptr, 0u};
  const dim3 grid((unsigned)(((long long)Mloc * d + WV - 1) / WV)), block(64 * WV);
  // (M = -1: explicit per-particle keys, see rng_explicit_row; a block may span two particles of different problems: the statistics row
  //  is taken per wave)
  if (bge_sample_fast(d, S, W, layout)) {
    allow_lds((k_bge_sample<WV, true, true, false, true>), lds);
    hipLaunchKernelGGL((k_bge_sample<WV, true, true, false, true>), grid, block, lds, stream, thr, masks, node_scores, bp, carry, 0, -1, Mloc, d, S, W,
                       layout, qs, kf);
  } else {
    allow_lds((k_bge_sample<WV, true, true, false, false>), lds);
    hipLaunchKernelGGL((k_bge_sample<WV, true, true, false, false>), grid, block, lds, stream, thr, masks, node_scores, bp, carry, 0, -1, Mloc, d, S, W,
                       layout, qs, kf);
  }
}

void bge_launch_chol_batch(hipStream_t stream, double* node_scores, const BgeParams& bp, const BgeQueues& qs, int d, int S) {
  if (d > 128) {
    const size_t lw = BGE_WIDE_WAVES * bge_wide_wave_bytes(d);
    allow_lds(k_bge_chol_wide<true>, lw);
    hipLaunchKernelGGL(k_bge_chol_wide<true>, dim3(2048), dim3(64 * BGE_WIDE_WAVES), lw, stream, node_scores, bp, qs, d, (d + 63) / 64);
    return;
  }
  const size_t lds = bge_chol_lds_bytes(d, false);
  unsigned long long* const none = nullptr;
  if (d > 64) {
    allow_lds(k_bge_chol<false, true, true>, lds);
    hipLaunchKernelGGL((k_bge_chol<false, true, true>), dim3(512), dim3(256), lds, stream, node_scores, bp, qs, d, S, none);
  } else {
    allow_lds(k_bge_chol<false, false, true>, lds);
    hipLaunchKernelGGL((k_bge_chol<false, false, true>), dim3(512), dim3(256), lds, stream, node_scores, bp, qs, d, S, none);
  }
}

void bge_launch_sum_nodes(hipStream_t stream, const double* node_scores, float* out, int d, int S) {
  hipLaunchKernelGGL(k_sum_nodes, dim3((S + 127) / 128), dim3(128), 0, stream, node_scores, out, d, S);
}
