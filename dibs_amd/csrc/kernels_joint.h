// What the joint models' translation units (tu_lin.hip, tu_nn.hip) and the soft-graph BGe estimator (tu_bge_soft.hip) share on the device:
// graph sampling and keys of the estimators (lin_*), the LDS geometry of the x-resident MFMA kernels (LinGeom), and the pieces of the
// softmax-weighted gradient kernels (grad_*).  Templates and __device__ __forceinline__ functions only: no kernel is defined here.
#pragma once
#include "joint_launch.h"

#define GRAD_WCH 256  // weights are evaluated in chunks of this many samples (one double-precision exp per thread and chunk)
// A sample is differentiated when its softmax weight is at least 2^-30.  The oracle (as round 5's kernels) keeps every weight that is
// non-zero in float32, down to 1e-45; but a term w_s grad_s with w_s < 2^-30 is 64 times below the float32 resolution of the sum it is added to
// (the weights sum to 1; the samples' gradients are NOT of one magnitude -- a sample far down the weights has a parameter far from its optimum and
// the larger gradient.  Measured, profiles/grad_weight_errors.txt: on the constructed weight profiles of tests/weight_states.py everything the cut
// drops is at most 4.3e-8 of the sum; on the adversarial state -- theta at the ridge optimum, the kept samples' gradient rounding noise, every other
// sample a factor 4 below the cut -- it is 8e-3 of the sum, where the float32 oracle itself is 0.2 off the float64 one) -- the reference's own float32 logsumexp loses it the same way -- and
// late in a run of the LinearGaussian model such samples are the majority of the "weighted" ones: config 3 at step 1 500 has 12.4 samples per
// particle with a non-zero weight in the theta estimator (worst particle 54) and 4.2 (24) with a weight of at least 2^-30 -- k_lin_grad
// 271 -> 154 us; config 5 at step 300 keeps 16.2 of 16.7 (the weights of its saturated graphs really are spread): profiles/round6_late_breakdown.txt.
// "Takes part" is !(w < GRAD_W_MIN) in every kernel and in the count of grad_softmax_stats: a NaN weight (a non-finite log-probability) takes
// part and the particle's gradient is NaN, as in the reference -- never a silent zero.
#define GRAD_W_MIN 9.313225746154785e-10f

struct LinGeom {
  int d, N, kp, np, ldx, ldw;  // kp = ceil4(d), np = ceil16(N) (rows of x / res incl. zero padding)
};
__host__ __device__ inline LinGeom lin_geom(int d, int N, int NT) {
  LinGeom g;
  g.d = d;
  g.N = N;
  g.kp = (d + 3) & ~3;
  g.np = (N + 15) & ~15;
  const int dp = 16 * NT;
  g.ldx = dp + 2;  // x rows / res rows: (row * ld + k) bank pattern of the MFMA A/B fragment reads
  g.ldw = dp + 2;
  return g;
}
// LDS: X[np][ldx] | WG[kp][ldw] | (gradient kernel) RS[np][ldw]; theta is read from global (L2-resident, d*d floats per particle)
__host__ __device__ inline size_t lin_lds_bytes(int d, int N, int NT, bool with_res) {
  const LinGeom g = lin_geom(d, N, NT);
  size_t f = (size_t)g.np * g.ldx + (size_t)g.kp * g.ldw;
  if (with_res) f += (size_t)g.np * g.ldw;
  return ((f * 4 + 15) & ~(size_t)15) + 64 * 8;
}
// row stride of the per-sample operands of the Threefry-paired kernels (k_lin_logprobs_pair, k_nn_logprobs): == 16 mod 32
template <int NT>
__host__ __device__ constexpr int lin_ldw2() { return (NT & 1) ? 16 * NT : 16 * NT + 16; }

__device__ __forceinline__ float lin_logn(float v, float mu, float sig) {
  const float zt = (v - mu) / sig;
  return -0.5f * zt * zt - logf(sig) - 0.918938533204672742f;
}

// element (i, j) of sample s: hard Bernoulli graph (theta / score modes) or Gumbel-soft graph (reparam)
__device__ __forceinline__ float lin_sample_g(int mode, Key2 key, uint64_t nbits, uint64_t dd, int s, int i, int j, int d,
                                              const uint32_t* __restrict__ thr_m, const float* __restrict__ sc_m, float alpha,
                                              float tau, int layout, int tiny) {
  if (mode == LIN_MODE_GIVEN) return reinterpret_cast<const int32_t*>(thr_m)[i * d + j] != 0 ? 1.0f : 0.0f;  // caller's graph
  if (i == j) return 0.f;
  const uint32_t bits = rng_bits_at(key, nbits, (uint64_t)s * dd + (uint64_t)i * d + j, layout);
  if (mode == LIN_MODE_Z_REPARAM) {
    const float eps = rng_logistic(bits, tiny);
    return 1.0f / (1.0f + expf(-tau * (eps + alpha * sc_m[i * d + j])));
  }
  return (bits >> 9) < thr_m[i * d + j] ? 1.0f : 0.0f;
}

__device__ __forceinline__ Key2 lin_mode_key(int mode, Key2 carry, int M_global, int m_global, int layout) {
  const Key2 kp = rng_split_row_uniform(carry, (uint32_t)M_global + 1u, (uint32_t)m_global + 1u, layout);
  if (mode == LIN_MODE_THETA) return kp;            // dibs.py:510: particle key itself
  return rng_split_row_uniform(kp, 2u, 1u, layout); // dibs.py:350-351 / 430-431: subk_ of split(particle key)
}

template <int NT>
__device__ __forceinline__ void lin_load_common(float* X, const float* __restrict__ x, const LinGeom g, int tid) {
  for (int e = tid; e < g.np * g.ldx; e += 256) {
    const int n = e / g.ldx, c = e - n * g.ldx;
    X[e] = (n < g.N && c < g.d) ? x[(size_t)n * g.d + c] : 0.f;
  }
}

// WG = g o theta for sample s (zero padded); returns this thread's share of sum_ij g_ij logN(theta_ij)
template <int NT>
__device__ __forceinline__ float lin_build_wg(float* WG, const float* __restrict__ TH, int mode, Key2 key, uint64_t nbits, int s,
                                              const uint32_t* thr_m, const float* sc_m, float alpha, float tau, int layout,
                                              int tiny, float mu, float sig, const LinGeom g, int tid) {
  float prior = 0.f;
  const uint64_t dd = (uint64_t)g.d * g.d;
  for (int e = tid; e < g.kp * g.ldw; e += 256) {
    const int i = e / g.ldw, j = e - i * g.ldw;
    float v = 0.f;
    if (i < g.d && j < g.d) {
      const float gv = lin_sample_g(mode, key, nbits, dd, s, i, j, g.d, thr_m, sc_m, alpha, tau, layout, tiny);
      const float th = TH[i * g.d + j];
      v = gv * th;
      prior += gv * lin_logn(th, mu, sig);
    }
    WG[e] = v;
  }
  return prior;
}

// pred = X * WG for the row tiles of this wave; calls f(n, j, pred_nj) on every valid element
template <int NT, typename F>
__device__ __forceinline__ void lin_pred_tiles(const float* X, const float* WG, const LinGeom g, int lane, int wave, F&& f) {
  const int nrt = g.np >> 4;
  for (int ti = wave; ti < nrt; ti += 4) {
    f32x4 acc[NT];
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[tj] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ap = (ti * 16 + (lane & 15)) * g.ldx + (lane >> 4);
    const int bq = (lane >> 4) * g.ldw + (lane & 15);
    for (int k0 = 0; k0 < g.kp; k0 += 4) {
      const float a = X[ap + k0];
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, WG[bq + k0 * g.ldw + tj * 16], acc[tj], 0, 0, 0);
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = ti * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15);
        float v = acc[tj][r];
        asm volatile("" : "+v"(v));
        if (n < g.N && j < g.d) f(n, j, v);
      }
  }
}

// ---- the samples of one (particle, estimator) over several blocks ------------------------------------------------------------------
// Early in a run the softmax over the S samples is one-hot in float32 (the log-probabilities differ by hundreds) and one gradient per
// particle is evaluated; once the particles have sharpened, many samples keep a non-zero weight (config 3 at step 1 500: 13 on average,
// 53 for the worst particle; config 5 at step 300: 15 / 123) and ONE block per particle walked them one after the other -- the worst
// particle set the time of the launch (k_lin_grad 62 -> 1 070 us, k_nn_grad 3.2 -> 53 ms).  Now GRAD_NS blocks share a particle: the
// samples with non-zero weight are dealt round-robin in sample order (ordinal q -> block q mod GRAD_NS), every block accumulates its
// share, and the block that finishes LAST adds the partial sums in block order (a counter per (particle, estimator); partial sums stored
// at agent scope, as the kernel-matrix tiles do) and runs the epilogue.  The grouping is a function of the weights only -- not of the shard
// -- so the result does not depend on the rank count; with one non-zero weight block 0 does everything as before and nothing is exchanged.
// softmax statistics of a particle's S log-probabilities in double (as the oracle: dibs.py:376-382 through logsumexp): maximum, sum of
// exponentials, sum of the log-probabilities, and the number of samples whose weight is at least GRAD_W_MIN.  `red`: 3 NW doubles of LDS.
template <int NW = 4>
__device__ __forceinline__ void grad_softmax_stats(const float* __restrict__ lp, int S, double* red, double& mx, double& den, double& sm, int& nnz) {
  constexpr int NTHR = 64 * NW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  mx = -INFINITY;
  for (int s = tid; s < S; s += NTHR) mx = (double)lp[s] > mx ? (double)lp[s] : mx;
  mx = wave_max_d(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = red[0];
  for (int w = 1; w < NW; ++w) mx = red[w] > mx ? red[w] : mx;
  den = 0.0;
  sm = 0.0;
  for (int s = tid; s < S; s += NTHR) {
    den += exp((double)lp[s] - mx);
    sm += (double)lp[s];
  }
  den = wave_sum_d(den);
  sm = wave_sum_d(sm);
  __syncthreads();
  if (lane == 0) {
    red[wave] = den;
    red[NW + wave] = sm;
  }
  __syncthreads();
  den = 0.0;
  sm = 0.0;
  for (int w = 0; w < NW; ++w) {
    den += red[w];
    sm += red[NW + w];
  }
  double cnt = 0.0;
  for (int s = tid; s < S; s += NTHR) cnt += !((float)(exp((double)lp[s] - mx) / den) < GRAD_W_MIN) ? 1.0 : 0.0;  // (the ONE predicate: a NaN weight takes part)
  cnt = wave_sum_d(cnt);
  if (lane == 0) red[2 * NW + wave] = cnt;
  __syncthreads();
  cnt = 0.0;
  for (int w = 0; w < NW; ++w) cnt += red[2 * NW + w];
  nnz = (int)cnt;
}

// the partial sums of this block are complete (stored with grad_part_store): count this block; true for the LAST of `nact` blocks, which
// then reads all of them with grad_part_load.  `flag`: one int of LDS.
__device__ __forceinline__ void grad_part_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float grad_part_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// element `idx` of the partial rows 0 .. nact-1 (row stride `stride`), added in row order; all loads are issued before the first addition
// (a rolled loop over the rows has ONE load in flight per thread: 4 480 dependent trips past the L2 for a k_nn_grad row -- the last block
// of a particle took milliseconds)
template <int NSMAX, bool ATOMIC>
__device__ __forceinline__ float grad_part_sum(const float* base, size_t stride, size_t idx, int nact) {
  if (nact == 1) return ATOMIC ? grad_part_load(base + idx) : base[idx];  // (block-uniform; 0.f + v == v)
  float v[NSMAX];
#pragma unroll
  for (int b = 0; b < NSMAX; ++b) {
    const float* p = base + (size_t)(b < nact ? b : 0) * stride + idx;
    v[b] = ATOMIC ? grad_part_load(p) : *p;
  }
  float t = 0.f;
#pragma unroll
  for (int b = 0; b < NSMAX; ++b) t += b < nact ? v[b] : 0.f;
  return t;
}
__device__ __forceinline__ bool grad_last_block(unsigned int* ctr, int nact, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (every wave: its own partial stores are complete before the block counts itself)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int done = atomicAdd(ctr, 1u) + 1u;
    if (done == (unsigned int)nact) atomicExch(ctr, 0u);
    *flag = done == (unsigned int)nact;
  }
  __syncthreads();
  return *flag != 0;
}
