// The block of k_edge_scores_p (kernels_marginal.h: one block of 16 waves per particle, n_vars <= 64, k <= 64) as a device function whose
// alpha is a plain parameter: k_edge_scores_p (engine_step.hip) passes its launch argument, k_edge_scores_p_batch (tu_batch.hip) the value
// of the particle's problem.
#pragma once
#include "common.h"

__device__ __forceinline__ void edge_scores_p_block(const float* __restrict__ z, float* __restrict__ scores, uint32_t* __restrict__ thr,
                                                    float* __restrict__ probs, float* __restrict__ eas, float alpha, int d, int k,
                                                    int dpad, int ldk, unsigned int* __restrict__ done_ctr,
                                                    unsigned int* __restrict__ done_flag, unsigned int done_seq) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Us = smem;
  float* Vs = smem + (size_t)dpad * ldk;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float2* zm = reinterpret_cast<const float2*>(z + (size_t)m * d * k * 2);
  const int nt = dpad >> 4;
  float2 uv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = wave + 16 * r;
    const bool in = i < d && lane < k;
    uv[r] = zm[in ? i * k + lane : 0];
    if (!in) uv[r] = make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = wave + 16 * r;
    if (i < dpad) {
      if (lane < ldk) {  // (ldk < 64 for small k: the row ends before the wave does)
        Us[i * ldk + lane] = uv[r].x;
        Vs[i * ldk + lane] = uv[r].y;
      }
      if (64 + lane < ldk) {  // (row padding beyond the 64 latent columns a wave covers: ldk = kp + (2 - kp) mod 32 <= 98)
        Us[i * ldk + 64 + lane] = 0.f;
        Vs[i * ldk + 64 + lane] = 0.f;
      }
    }
  }
  __syncthreads();
  const int t = wave;
  if (t < nt * nt) {  // (wave-uniform)
    const int ti = t / nt, tj = t - ti * nt, kp = (k + 3) & ~3;
    const float* ua = Us + (size_t)(ti * 16 + (lane & 15)) * ldk + (lane >> 4);
    const float* vb = Vs + (size_t)(tj * 16 + (lane & 15)) * ldk + (lane >> 4);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 4) a = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[k0], vb[k0], a, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ti * 16 + (lane >> 4) * 4 + r, col = tj * 16 + (lane & 15);
      if (row < d && col < d) {
        const float s = a[r];
        const size_t o = ((size_t)m * d + row) * d + col;
        const double ex = exp(-(double)__fmul_rn(alpha, s));  // (the epilogue of k_edge_scores, operation for operation)
        const float pf = (float)(1.0 / (1.0 + ex));
        if (done_ctr) {  // (what the second stream reads goes out at agent scope: see below)
          __hip_atomic_store(scores + o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (eas) __hip_atomic_store(eas + o, (float)ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          scores[o] = s;
          if (eas) eas[o] = (float)ex;
        }
        if (thr) thr[o] = row == col ? 0u : (uint32_t)ceilf(pf * 8388608.0f);  // (null: the copy of the second stream, scores / eas only)
        if (probs) probs[o] = row == col ? 0.f : pf;
      }
    }
  }
  // done_ctr != null: the fork to the engine's second stream without an event (k_wait_flag there polls done_flag): scores / eas were stored at
  // agent scope (complete once the storing wave has waited for vmcnt(0): the barrier alone does not), every block counts itself, the last one
  // publishes the step's sequence number
  if (done_ctr) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0 && atomicAdd(done_ctr, 1u) == gridDim.x - 1u) {
      atomicExch(done_ctr, 0u);  // (the next launch of this kernel is behind this one in its stream)
      __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

