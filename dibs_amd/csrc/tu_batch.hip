// translation unit: the table-reading kernels of the batched engine (include/dibs_hip.h, dibs_engine_set_problem_hparams; ProblemHP in
// common.h) and their launchers.  Each is the block of a standalone kernel under a __global__ that takes the scalar(s) of the block's problem
// from the per-problem table.  A unit of their own, so that the units of the standalone kernels compile what they compiled without them.
#define DIBS_TU_BATCH
#include "engine_impl.h"
#include "kernels_edge_p.h"
#include "kernels_acyc.h"
#include "kernels_acyc_bf16.h"
#include "kernels_acyc_f16.h"

// batched engines (include/dibs_hip.h, per-problem hyper-parameters): the same block with alpha of the particle's problem, row m / pM of
// the table (block-uniform: a scalar load); no fork flag
__global__ __launch_bounds__(1024) void k_edge_scores_p_batch(const float* __restrict__ z, float* __restrict__ scores, uint32_t* __restrict__ thr,
                                                              float* __restrict__ probs, float* __restrict__ eas,
                                                              const ProblemHP* __restrict__ hp, int pM, int d, int k, int dpad, int ldk) {
  edge_scores_p_block(z, scores, thr, probs, eas, hp[blockIdx.x / (unsigned)pM].alpha, d, k, dpad, ldk, nullptr, nullptr, 0u);
}


void batch_launch_edge_scores(hipStream_t st, const float* z, float* scores, uint32_t* thr, float* probs, float* eas, const ProblemHP* hp, int pM,
                              int Mloc, int d, int k, int dpad, int ldk) {
  const size_t lds = (size_t)2 * dpad * ldk * 4;
  dibs_allow_lds((const void*)k_edge_scores_p_batch, lds);
  hipLaunchKernelGGL(k_edge_scores_p_batch, dim3(Mloc), dim3(1024), lds, st, z, scores, thr, probs, eas, hp, pM, d, k, dpad, ldk);
}

void batch_launch_tail(hipStream_t st, const TailArgs& ta, const ProblemHP* hp, int pM, int Mloc, size_t lds) {
  dibs_allow_lds((const void*)k_particle_grad_batch, lds);
  hipLaunchKernelGGL(k_particle_grad_batch, dim3(Mloc), dim3(TAIL_NT), lds, st, ta, hp, pM);
}

// the matrix powers of acyc_launch_power (tu_acyc.hip) for n_vars <= 64 on the default or the f32 pipe: k_acyc_hf for 33 <= d <= 64 with
// paired chains, k_acyc<NT> otherwise; a.alpha is not read
template <int NT>
static void launch_nt_batch(const AcycLaunch& a, const ProblemHP* hp, int pM) {
  constexpr int DP = 16 * NT, LD = DP + 4;
  const size_t lds = (size_t)(3 * DP + 1) * LD * 4;
  const dim3 grid(a.nblk, a.Mloc);
  if (a.units != a.Sa) {
    dibs_allow_lds((const void*)k_acyc_batch<NT, true>, lds);
    hipLaunchKernelGGL((k_acyc_batch<NT, true>), grid, dim3(256), lds, a.stream, a.scores, a.part, a.carry, a.m0, a.M, a.d, a.Sa, a.cpb, hp, pM,
                       a.tau, a.layout, a.tiny, a.nblk);
  } else {
    dibs_allow_lds((const void*)k_acyc_batch<NT, false>, lds);
    hipLaunchKernelGGL((k_acyc_batch<NT, false>), grid, dim3(256), lds, a.stream, a.scores, a.part, a.carry, a.m0, a.M, a.d, a.Sa, a.cpb, hp, pM,
                       a.tau, a.layout, a.tiny, a.nblk);
  }
}
template <bool FOUR>
static void launch_hf_batch(const AcycLaunch& a, const ProblemHP* hp, int pM) {
  const size_t lds = (size_t)AHF_LDS_BYTES;
  dibs_allow_lds((const void*)k_acyc_hf_batch<FOUR, 3>, lds);
  hipLaunchKernelGGL((k_acyc_hf_batch<FOUR, 3>), dim3(a.nblk, (a.Mloc + 7) & ~7), dim3(256), lds, a.stream, a.scores, a.eas, a.part, a.carry, a.m0,
                     a.M, a.Mloc, a.d, a.Sa, a.cpb, hp, pM, a.tau, a.layout, a.tiny, a.nblk);
}
void batch_launch_acyc_power(const AcycLaunch& a, const ProblemHP* hp, int pM) {
  if (a.pipe != DIBS_PIPE_F32 && a.units != a.Sa && a.d >= 33) {  // (acyc_use_bf16 of tu_acyc.hip; the bf16 pipe never comes here)
    if (a.d > 48) launch_hf_batch<true>(a, hp, pM);
    else launch_hf_batch<false>(a, hp, pM);
    return;
  }
  switch ((a.d + 15) / 16) {
    case 1: launch_nt_batch<1>(a, hp, pM); break;
    case 2: launch_nt_batch<2>(a, hp, pM); break;
    case 3: launch_nt_batch<3>(a, hp, pM); break;
    default: launch_nt_batch<4>(a, hp, pM); break;
  }
}
