// JointDiBS + LinearGaussian likelihood kernels (gfx950).
//   log p(theta, D | G) = sum_ij g_ij logN(theta_ij; mu_e, sig_e) + sum_{n,j: not intervened} logN(x_nj; (x (g o theta))_nj, sqrt(obs_noise))
//   r = (1 - mask) o (x - x (g o theta)) / obs_noise
//   d/dg = logN(theta) + theta o (x^T r)            d/dtheta = g o (-(theta - mu_e)/sig_e^2 + x^T r)
// reference: dibs/models/linearGaussian.py:278-338; estimators dibs/inference/dibs.py:395-459 (Z, reparam),
//            :325-391 (Z, score), :488-551 (theta).  Both contractions run on v_mfma_f32_16x16x4_f32 with x, theta and
//            the per-sample operand resident in LDS.
#pragma once
#if !defined(DIBS_TU_LIN) && !defined(DIBS_TU_LIN_CHAINS)
#error "kernels_lin.h: the LinearGaussian kernels are compiled in tu_lin.hip, their per-chain forms in tu_lin_chains.hip, and nowhere else"
#endif
#include "kernels_joint.h"
#include "kernels_acyc_bf16.h"
#include "kernels_acyc_f16.h"

// The data a kernel of this file reads -- x, mask and the flag any_mask -- comes in one of two forms, chosen by the translation unit:
//   tu_lin.hip          launch arguments: one data set for every block (standalone engines, chains engines on shared data).  The macros
//                       below then spell out the parameters the kernels always had, and LIN_CHAIN_DATA is empty.
//   tu_lin_chains.hip   a LinChainData (joint_launch.h): the kernels are named k_..._chains and LIN_CHAIN_DATA(m) derives x, mask and
//                       any_mask of the chain of particle row m (m / M: block-uniform, scalar loads and a scalar offset).
// One source text, so that the two forms cannot drift apart (and one launch text for it, lin_launch.h), and no wrapper around the kernels:
// as __forceinline__ blocks under two __global__s the register allocation of k_lin_logprobs_pair and k_lin_grad changed.
// The annealed alpha of a step and the baseline rate of the score-function estimator follow the data: launch arguments in tu_lin.hip
// (LIN_ALPHA_PARAM / LIN_SFB_PARAM spell out `float alpha` / `double sf_baseline`), and in tu_lin_chains.hip locals of those names that
// LIN_CHAIN_DATA / LIN_CHAIN_SFB take from the chain's row of the per-chain table (LinChainData::hp, dibs_engine_set_chain_hparams;
// block-uniform: scalar loads beside the one of any_mask) -- always: the keys launch of a step writes every chain's alpha there, and the
// rows of an engine on which nothing was set hold the configuration's values, so the float is the one the chain's standalone engine
// passes.  The launch arguments of those names are not read (a select between the two cost the gradient kernels scalar registers).
#ifdef DIBS_TU_LIN_CHAINS
#define LIN_K(name_) name_##_chains
#define LIN_DATA_PARAMS LinChainData cd
#define LIN_ANY_PARAM
#define LIN_ALPHA_PARAM [[maybe_unused]] float alpha_launch
#define LIN_SFB_PARAM [[maybe_unused]] double sf_baseline_launch
#define LIN_CHAIN_DATA(m_)                                                           \
  const int chain_ = (m_) / cd.M;                                                    \
  const float* __restrict__ x = cd.x + (size_t)chain_ * N * d;                       \
  const int32_t* __restrict__ mask = cd.mask + (size_t)chain_ * N * d;               \
  const int any_mask = cd.any_mask[chain_];                                          \
  const float alpha = cd.hp[chain_].alpha;
#define LIN_CHAIN_SFB const double sf_baseline = cd.hp[chain_].sf_baseline;
#else
#define LIN_K(name_) name_
#define LIN_DATA_PARAMS const float* __restrict__ x, const int32_t* __restrict__ mask
#define LIN_ANY_PARAM , int any_mask
#define LIN_ALPHA_PARAM float alpha
#define LIN_SFB_PARAM double sf_baseline
#define LIN_CHAIN_DATA(m_)
#define LIN_CHAIN_SFB
#endif

// ------------------------------------------------------------------------------------------------
// log p(theta, D | G_s) for all samples.  grid = (ceil(S / spb), Mloc), block = 256
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void LIN_K(k_lin_logprobs)(LIN_DATA_PARAMS,
                                                      const float* __restrict__ theta, const float* __restrict__ scores,
                                                      const uint32_t* __restrict__ thr, float* __restrict__ logprobs, Key2 carry,
                                                      int mode, int m0, int M_global, int d, int N, int S, int spb, LIN_ALPHA_PARAM,
                                                      float tau, int layout, int tiny, float obs_noise, float mu, float sig
                                                      LIN_ANY_PARAM) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const LinGeom g = lin_geom(d, N, NT);
  float* X = smem;
  float* WG = X + (size_t)g.np * g.ldx;
  double* red = reinterpret_cast<double*>(smem + ((((size_t)g.np * g.ldx + (size_t)g.kp * g.ldw) + 3) & ~(size_t)3));
  const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LIN_CHAIN_DATA(m)
  const size_t dd = (size_t)d * d;
  const float* __restrict__ TH = theta + (size_t)m * dd;
  lin_load_common<NT>(X, x, g, tid);
  const Key2 key = lin_mode_key(mode, carry, M_global, m0 + m, layout);
  const uint64_t nbits = (uint64_t)S * dd;
  const float inv2 = 0.5f / obs_noise;
  const float lognorm_x = -0.5f * logf(obs_noise) - 0.918938533204672742f;
  for (int c = 0; c < spb; ++c) {
    const int s = blockIdx.x * spb + c;
    if (s >= S) break;
    __syncthreads();
    float part = lin_build_wg<NT>(WG, TH, mode, key, nbits, s, thr + (size_t)m * dd, scores + (size_t)m * dd, alpha, tau, layout,
                                  tiny, mu, sig, g, tid);
    __syncthreads();
    lin_pred_tiles<NT>(X, WG, g, lane, wave, [&](int n, int j, float pred) {
      if (any_mask && mask[(size_t)n * d + j]) return;
      const float e = X[n * g.ldx + j] - pred;
      part += lognorm_x - inv2 * e * e;
    });
    const double tot = wave_sum_d((double)part);
    if (lane == 0) red[wave] = tot;
    __syncthreads();
    if (tid == 0) logprobs[(size_t)m * S + s] = (float)(red[0] + red[1] + red[2] + red[3]);
  }
}

// Same, for the legacy PRNG layout with an even number of samples and N <= 128: sample s and s + S/2 share their Threefry
// calls (element e of the [S, d, d] draw is paired with e + S d d / 2), so a block takes both and builds both operands from
// one call per element.  x does not depend on the sample: every wave keeps its MFMA A fragments (and the x values of its
// output elements) in registers, so LDS holds the two per-sample operands only (row stride == 16 mod 32: conflict-free
// B-fragment reads) and four blocks fit on a CU.
// grid = (ceil(S / 2 / ppb), Mloc), block = 256
__host__ __device__ inline size_t lin_lds_bytes_pair(int d, int NT) {
  const int kp = (d + 3) & ~3, ldw2 = (NT & 1) ? 16 * NT : 16 * NT + 16;
  return (((size_t)2 * kp * ldw2 * 4 + 15) & ~(size_t)15) + 64 * 8;
}
// EPQ > 0: every thread owns the elements e = tid + 256 q (q < EPQ, covers d*d <= 256 EPQ) of the d x d operand and keeps
// their sample-independent factors (theta, logN(theta), exp(-alpha s) or the Bernoulli threshold, LDS offset) in registers
// for all pairs of the block; EPQ == 0 recomputes them per pair (large d: the registers go to the x fragments instead).
template <int NT, int EPQ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NT <= 4 ? 3 : 1, NT <= 4 ? 3 : 2))) void LIN_K(k_lin_logprobs_pair)(LIN_DATA_PARAMS,
                                                           const float* __restrict__ theta, const float* __restrict__ scores,
                                                           const uint32_t* __restrict__ thr, float* __restrict__ logprobs, Key2 carry,
                                                           int mode, int m0, int M_global, int d, int N, int S, int ppb, LIN_ALPHA_PARAM,
                                                           float tau, int layout, int tiny, float obs_noise, float mu, float sig
                                                           LIN_ANY_PARAM) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDW = lin_ldw2<NT>(), NU = 2, KSMAX = 4 * NT;
  const int kp = (d + 3) & ~3, ksteps = kp >> 2, nrt = (N + 15) >> 4;
  float* WG0 = smem;
  float* WG1 = WG0 + (size_t)kp * LDW;
  double* red = reinterpret_cast<double*>(smem + (((size_t)2 * kp * LDW + 3) & ~(size_t)3));
  const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LIN_CHAIN_DATA(m)
  const int dd = d * d;
  const float* __restrict__ TH = theta + (size_t)m * dd;
  const uint32_t* __restrict__ thr_m = thr + (size_t)m * dd;
  const float* __restrict__ sc_m = scores + (size_t)m * dd;
  // A fragments: row n = (wave + 4u) * 16 + (lane & 15), k = 4 ks + (lane >> 4); output elements (C layout):
  // n = (wave + 4u) * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15); wgt = 1 where the element counts in the likelihood
  float xa[NU][KSMAX], xe[NU][NT][4];
  uint32_t ok[NU];
  float nvalid = 0.f;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int na = (wave + 4 * u) * 16 + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks) {
      const int kk = 4 * ks + (lane >> 4);
      xa[u][ks] = (na < N && kk < d) ? x[(size_t)na * d + kk] : 0.f;
    }
    ok[u] = 0u;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = (wave + 4 * u) * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15);
        const bool v = n < N && j < d && !(any_mask && mask[(size_t)n * d + j]);
        xe[u][tj][r] = v ? x[(size_t)n * d + j] : 0.f;
        ok[u] |= (uint32_t)v << (tj * 4 + r);
        nvalid += v ? 1.0f : 0.0f;
      }
  }
  const TfKeys tk = tf_keys(lin_mode_key(mode, carry, M_global, m0 + m, layout));
  const uint32_t half = (uint32_t)(((uint64_t)S * dd) >> 1);
  const int hS = S >> 1;
  const float inv2 = 0.5f / obs_noise;
  const float lognorm_x = -0.5f * logf(obs_noise) - 0.918938533204672742f;
  const bool soft = mode == LIN_MODE_Z_REPARAM, fast = tau == 1.0f;
  const float ulo = tiny ? 1.17549435e-38f : 1.1920929e-07f;
  const int bq = (lane >> 4) * LDW + (lane & 15);
  const float inv_d = 1.0f / (float)d;
  for (int e = tid; e < 2 * kp * LDW; e += 256) smem[e] = 0.f;  // padding and diagonal: written once
  // sample-independent factors of element e: offset in the operand, theta, logN(theta), aux = exp(-alpha s) | alpha s | thr
  // (aux carries the Bernoulli threshold's bits in the hard-graph modes)
  auto factors = [&](int e, int& off, float& th, float& ln, float& aux) {
    const int i = (int)(((float)e + 0.5f) * inv_d), j = e - i * d;  // exact for e < 2^20
    off = (i == j) ? -1 : i * LDW + j;
    th = TH[e];
    ln = lin_logn(th, mu, sig);
    if (soft) {
      const float as = alpha * sc_m[e];
      aux = fast ? expf(-as) : as;
    } else {
      aux = __uint_as_float(thr_m[e]);
    }
  };
  int offs[EPQ > 0 ? EPQ : 1];
  float ths[EPQ > 0 ? EPQ : 1], lns[EPQ > 0 ? EPQ : 1], auxs[EPQ > 0 ? EPQ : 1];
  if constexpr (EPQ > 0) {
#pragma unroll
    for (int q = 0; q < EPQ; ++q) {
      const int e = tid + 256 * q;
      offs[q] = -1;
      ths[q] = lns[q] = auxs[q] = 0.f;
      if (e < dd) factors(e, offs[q], ths[q], lns[q], auxs[q]);
    }
  }
  float part[2];
  // one element of the pair (s0, s0 + S/2): one Threefry call, both operands
  auto element = [&](int e, uint32_t cbase, int off, float th, float ln, float aux) {
    if (off < 0) return;
    uint32_t y0, y1;
    threefry2x32_uh(tk, (uint32_t)e, cbase, half, y0, y1);  // counter cbase + e: cbase and half are the wave's
    float g0, g1;
    if (soft) {
      if (fast) {  // sigmoid(eps + a), eps = log(u / (1 - u))  ==  u / (u + (1 - u) exp(-a))
        const float u0 = rng_uniform(y0, ulo, 1.0f), u1 = rng_uniform(y1, ulo, 1.0f);
        g0 = u0 * __builtin_amdgcn_rcpf(fmaf(1.0f - u0, aux, u0));  // (v_rcp_f32: 1 ulp; an IEEE division is ten instructions)
        g1 = u1 * __builtin_amdgcn_rcpf(fmaf(1.0f - u1, aux, u1));
      } else {
        g0 = 1.0f / (1.0f + expf(-tau * (rng_logistic(y0, tiny) + aux)));
        g1 = 1.0f / (1.0f + expf(-tau * (rng_logistic(y1, tiny) + aux)));
      }
    } else {
      const uint32_t ta = __float_as_uint(aux);
      g0 = (y0 >> 9) < ta ? 1.0f : 0.0f;
      g1 = (y1 >> 9) < ta ? 1.0f : 0.0f;
    }
    WG0[off] = g0 * th;
    WG1[off] = g1 * th;
    part[0] = fmaf(g0, ln, part[0]);
    part[1] = fmaf(g1, ln, part[1]);
  };
  for (int c = 0; c < ppb; ++c) {
    const int s0 = blockIdx.x * ppb + c;
    if (s0 >= hS) break;
    __syncthreads();
    part[0] = part[1] = nvalid * lognorm_x;
    const uint32_t cbase = (uint32_t)((uint64_t)s0 * (uint64_t)dd);
    if constexpr (EPQ > 0) {
#pragma unroll
      for (int q = 0; q < EPQ; ++q) element(tid + 256 * q, cbase, offs[q], ths[q], lns[q], auxs[q]);
    } else {
      for (int e = tid; e < dd; e += 256) {
        int off;
        float th, ln, aux;
        factors(e, off, th, ln, aux);
        element(e, cbase, off, th, ln, aux);
      }
    }
    __syncthreads();
#pragma unroll
    for (int hsel = 0; hsel < 2; ++hsel) {
      const float* WG = hsel ? WG1 : WG0;
      float sq = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if (wave + 4 * u >= nrt) continue;
        f32x4 acc[NT];
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) acc[tj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
          if (ks >= ksteps) continue;
#pragma unroll
          for (int tj = 0; tj < NT; ++tj)
            acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u][ks], tj * 16 < LDW ? WG[bq + ks * 4 * LDW + tj * 16] : 0.f, acc[tj], 0, 0, 0);
        }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pv = acc[tj][r];
            asm volatile("" : "+v"(pv));
            const float er = ((ok[u] >> (tj * 4 + r)) & 1u) ? xe[u][tj][r] - pv : 0.f;
            sq = fmaf(er, er, sq);
          }
      }
      part[hsel] = fmaf(-inv2, sq, part[hsel]);
    }
    const double t0 = wave_sum_d((double)part[0]), t1 = wave_sum_d((double)part[1]);
    if (lane == 0) {
      red[wave] = t0;
      red[4 + wave] = t1;
    }
    __syncthreads();
    if (tid == 0) logprobs[(size_t)m * S + s0] = (float)(red[0] + red[1] + red[2] + red[3]);
    if (tid == 1) logprobs[(size_t)m * S + s0 + hS] = (float)(red[4] + red[5] + red[6] + red[7]);
  }
}

// Same pairing, 33 <= d <= 64, on the f16 matrix pipe with TWO block-scaled pieces per operand (the arithmetic of k_acyc_hf,
// kernels_acyc_f16.h: x 2^e = h + m, a product three v_mfma_f32_16x16x32_f16 -- 48 MFMA cycles for a 16 x 16 x 64 block where the f32 MFMA
// needs 512).  x's row fragments (left operand, split once per block) stay in registers; the per-sample operand g o theta is split as it is
// built -- both samples of the pair in ONE packed split, low halves to the first image, high halves to the second -- and written with
// 2-byte stores into the transposing-read image layout ([piece][column tile][row k][16 columns], chunk swizzle (c + (k >> 2)) % 4).  The
// MFMA is issued with swapped operands, so lane (g, r) holds pred[n = 16 ti + r][j = 16 tj + 4 g + i].  Scales: x by the exponent of max |x| (block reduction, once),
// theta by the exponent of max |theta_m| (block reduction, once; |g| <= 1) -- the pieces stay below 2^14, the product is unscaled once
// per output element.  (Round 3's three-piece bf16 variant of this kernel was retired in round 6: profiles/HISTORY.md.)
// grid = (ceil(S / 2 / ppb), Mloc), block = 64 NW, dynamic LDS = 2 * AHF_IMG_BYTES + 256
template <int EPQ, bool FOUR, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 8 ? 4 : 3, NW == 8 ? 4 : 3))) void LIN_K(k_lin_logprobs_hf)(
    LIN_DATA_PARAMS, const float* __restrict__ theta, const float* __restrict__ scores,
    const uint32_t* __restrict__ thr, float* __restrict__ logprobs, Key2 carry, int mode, int m0, int M_global, int d, int N, int S, int ppb,
    LIN_ALPHA_PARAM, float tau, int layout, int tiny, float obs_noise, float mu, float sig LIN_ANY_PARAM) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned char* const sb = reinterpret_cast<unsigned char*>(smem);
  double* red = reinterpret_cast<double*>(sb + 2 * AHF_IMG_BYTES);
  constexpr int NU = 8 / NW, NTHR = 64 * NW;
  const int nrt = (N + 15) >> 4;
  const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, r = lane & 15;
  LIN_CHAIN_DATA(m)
  const int dd = d * d;
  const float* __restrict__ TH = theta + (size_t)m * dd;
  const uint32_t* __restrict__ thr_m = thr + (size_t)m * dd;
  const float* __restrict__ sc_m = scores + (size_t)m * dd;
  // row n = (wave + 4 u) * 16 + r of x: the same 16 values (columns 16 tj + 4 g + i) are the lane's left-operand fragment and the x of its
  // output elements
  AhfFrag XA[NU];
  f32x4 xv[NU][ABF_NT];
  float xe[NU][ABF_NT][4];
  uint32_t ok[NU];
  float nvalid = 0.f, amax = 0.f;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int n = (wave + NW * u) * 16 + r;
    f32x4 (&v)[ABF_NT] = xv[u];
    ok[u] = 0u;
#pragma unroll
    for (int tj = 0; tj < ABF_NT; ++tj)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * tj + 4 * g4 + i;
        const bool inb = n < N && j < d;
        const float xv_ = inb ? x[(size_t)n * d + j] : 0.f;
        const bool valid = inb && !(any_mask && mask[(size_t)n * d + j]);
        v[tj][i] = xv_;
        xe[u][tj][i] = valid ? xv_ : 0.f;
        ok[u] |= (uint32_t)valid << (tj * 4 + i);
        nvalid += valid ? 1.0f : 0.0f;
        amax = fmaxf(amax, fabsf(xv_));
      }
  }
  // block-wide max |x| and max |theta_m| -> exponents of the two scales (pieces below 2^14)
  float tmax = 0.f;
  for (int e = tid; e < dd; e += NTHR) tmax = fmaxf(tmax, fabsf(TH[e]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, o, 64));
  }
  float* const redf = reinterpret_cast<float*>(red);
  if (lane == 0) {
    redf[wave] = amax;
    redf[NW + wave] = tmax;
  }
  __syncthreads();
  amax = tmax = 0.f;
#pragma unroll
  for (int w8 = 0; w8 < NW; ++w8) {
    amax = fmaxf(amax, redf[w8]);
    tmax = fmaxf(tmax, redf[NW + w8]);
  }
  auto scale_exp = [](float mx) {
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) e = 13 - ((int)((__float_as_uint(mx) >> 23) & 0xffu) - 127);
    return e > 60 ? 60 : (e < -60 ? -60 : e);
  };
  const int ex = __builtin_amdgcn_readfirstlane(scale_exp(amax)), et = __builtin_amdgcn_readfirstlane(scale_exp(tmax));
  const float th_scale = ahf_pow2(et), unscale = ahf_pow2(-(ex + et));
#pragma unroll
  for (int u = 0; u < NU; ++u) ahf_make_frag(xv[u], ahf_pow2(ex), XA[u]);
  __syncthreads();  // (red is reused by the sample loop)
  const TfKeys tk = tf_keys(lin_mode_key(mode, carry, M_global, m0 + m, layout));
  const uint32_t half = (uint32_t)(((uint64_t)S * dd) >> 1);
  const int hS = S >> 1;
  const float inv2 = 0.5f / obs_noise;
  const float lognorm_x = -0.5f * logf(obs_noise) - 0.918938533204672742f;
  const bool soft = mode == LIN_MODE_Z_REPARAM, fast = tau == 1.0f;
  const float ulo = tiny ? 1.17549435e-38f : 1.1920929e-07f;
  const int rd_off = (4 * g4 + (r >> 2)) * 32 + (((r & 3) + g4) & 3) * 8;
  const float inv_d = 1.0f / (float)d;
  for (int e = tid; e < 2 * AHF_IMG_BYTES / 16; e += NTHR) reinterpret_cast<float4*>(sb)[e] = make_float4(0.f, 0.f, 0.f, 0.f);  // padding, diagonal
  // sample-independent factors of element e = (i, j): byte offset of W[i][j] inside a piece, theta, logN(theta), aux (as k_lin_logprobs_pair)
  auto factors = [&](int e, int& off, float& th, float& ln, float& aux) {
    const int i = (int)(((float)e + 0.5f) * inv_d), j = e - i * d;  // exact for e < 2^20
    off = (i == j) ? -1 : (j >> 4) * ABF_TILE_BYTES + i * 32 + ((((j & 15) >> 2) + (i >> 2)) & 3) * 8 + (j & 3) * 2;
    th = TH[e];
    ln = lin_logn(th, mu, sig);
    th *= th_scale;  // (the operand carries theta 2^et)
    if (soft) {
      const float as = alpha * sc_m[e];
      aux = fast ? expf(-as) : as;
    } else {
      aux = __uint_as_float(thr_m[e]);
    }
  };
  int offs[EPQ > 0 ? EPQ : 1];
  float ths[EPQ > 0 ? EPQ : 1], lns[EPQ > 0 ? EPQ : 1], auxs[EPQ > 0 ? EPQ : 1];
  if constexpr (EPQ > 0) {
#pragma unroll
    for (int q = 0; q < EPQ; ++q) {
      const int e = tid + NTHR * q;
      offs[q] = -1;
      ths[q] = lns[q] = auxs[q] = 0.f;
      if (e < dd) factors(e, offs[q], ths[q], lns[q], auxs[q]);
    }
  }
  float part[2];
  auto element = [&](int e, uint32_t cbase, int off, float th, float ln, float aux) {
    if (off < 0) return;
    uint32_t y0, y1;
    threefry2x32_uh(tk, (uint32_t)e, cbase, half, y0, y1);  // counter cbase + e: cbase and half are the wave's
    float g0, g1;
    if (soft) {
      if (fast) {
        const float u0 = rng_uniform(y0, ulo, 1.0f), u1 = rng_uniform(y1, ulo, 1.0f);
        g0 = u0 * __builtin_amdgcn_rcpf(fmaf(1.0f - u0, aux, u0));  // (v_rcp_f32: 1 ulp; an IEEE division is ten instructions)
        g1 = u1 * __builtin_amdgcn_rcpf(fmaf(1.0f - u1, aux, u1));
      } else {
        g0 = 1.0f / (1.0f + expf(-tau * (rng_logistic(y0, tiny) + aux)));
        g1 = 1.0f / (1.0f + expf(-tau * (rng_logistic(y1, tiny) + aux)));
      }
    } else {
      const uint32_t ta = __float_as_uint(aux);
      g0 = (y0 >> 9) < ta ? 1.0f : 0.0f;
      g1 = (y1 >> 9) < ta ? 1.0f : 0.0f;
    }
    uint32_t ph, pm;
    ahf_split(g0 * th, g1 * th, 1.0f, ph, pm);
    unsigned char* const w0 = sb + off;
    *reinterpret_cast<uint16_t*>(w0) = (uint16_t)ph;
    *reinterpret_cast<uint16_t*>(w0 + AHF_PIECE_BYTES) = (uint16_t)pm;
    *reinterpret_cast<uint16_t*>(w0 + AHF_IMG_BYTES) = (uint16_t)(ph >> 16);
    *reinterpret_cast<uint16_t*>(w0 + AHF_IMG_BYTES + AHF_PIECE_BYTES) = (uint16_t)(pm >> 16);
    part[0] = fmaf(g0, ln, part[0]);
    part[1] = fmaf(g1, ln, part[1]);
  };
  for (int c = 0; c < ppb; ++c) {
    const int s0 = blockIdx.x * ppb + c;
    if (s0 >= hS) break;
    __syncthreads();
    part[0] = part[1] = nvalid * lognorm_x;
    const uint32_t cbase = (uint32_t)((uint64_t)s0 * (uint64_t)dd);
    if constexpr (EPQ > 0) {
#pragma unroll
      for (int q = 0; q < EPQ; ++q) element(tid + NTHR * q, cbase, offs[q], ths[q], lns[q], auxs[q]);
    } else {
      for (int e = tid; e < dd; e += NTHR) {
        int off;
        float th, ln, aux;
        factors(e, off, th, ln, aux);
        element(e, cbase, off, th, ln, aux);
      }
    }
    __syncthreads();
#pragma unroll
    for (int hsel = 0; hsel < 2; ++hsel) {
      const unsigned char* img = sb + hsel * AHF_IMG_BYTES;
      float sq = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if (wave + NW * u >= nrt) continue;
        f32x4 acc[ABF_NT];
        ahf_matmul<FOUR>(acc, XA[u], img, rd_off);
        // (without interventions every element that does not count is padding: x = 0 there and the prediction is an exact 0 -- zero rows of
        //  the left operand, zero columns of the right one --, so the residual needs no mask: one instruction less per element)
        if (any_mask) {
#pragma unroll
          for (int tj = 0; tj < ABF_NT; ++tj)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float pv = acc[tj][i];
              asm volatile("" : "+v"(pv));
              const float er = ((ok[u] >> (tj * 4 + i)) & 1u) ? fmaf(-pv, unscale, xe[u][tj][i]) : 0.f;
              sq = fmaf(er, er, sq);
            }
        } else {
#pragma unroll
          for (int tj = 0; tj < ABF_NT; ++tj)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float pv = acc[tj][i];
              asm volatile("" : "+v"(pv));
              const float er = fmaf(-pv, unscale, xe[u][tj][i]);
              sq = fmaf(er, er, sq);
            }
        }
      }
      part[hsel] = fmaf(-inv2, sq, part[hsel]);
    }
    const double t0 = wave_sum_d((double)part[0]), t1 = wave_sum_d((double)part[1]);
    if (lane == 0) {
      red[wave] = t0;
      red[NW + wave] = t1;
    }
    __syncthreads();
    if (tid < 2) {
      double tot = 0.0;
      for (int w8 = 0; w8 < NW; ++w8) tot += red[tid * NW + w8];
      logprobs[(size_t)m * S + s0 + tid * hS] = (float)tot;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// softmax-weighted gradient: w = softmax(l); only samples with w_s != 0 are re-evaluated (in float the weights of
// all but a few samples underflow to exactly 0 -- the oracle skips them the same way).
//   mode THETA     : grad_theta = sum_s w_s g_s o (-(theta - mu)/sig^2 + x^T r_s)   -> pack row (+ copy of theta)
//   mode Z_REPARAM : W = sum_s w_s (logN(theta) + theta o x^T r_s) o tau alpha g~(1 - g~), off-diagonal   -> w_lik
//   mode Z_SCORE   : W = scale * alpha (sum_s w_s G_s - P), off-diagonal                                 -> w_lik
// grid = Mloc, block = 256
// ------------------------------------------------------------------------------------------------
// one estimator's inputs / outputs; the theta and the Z estimator of a step run as blockIdx.y = 0 / 1 of ONE launch (each has
// only Mloc blocks -- half the CUs -- and they are independent once both sets of log-probs exist)
struct LinGradJob {
  const float* logprobs;
  float* out;
  size_t out_stride;
  float* theta_copy;
  float* baseline_out;
  Key2 carry;
  int mode;
};
template <int NT>
__global__ __launch_bounds__(256) void LIN_K(k_lin_grad)(LIN_DATA_PARAMS,
                                                  const float* __restrict__ theta, const float* __restrict__ scores,
                                                  const uint32_t* __restrict__ thr, LinGradJob job0, LinGradJob job1,
                                                  const float* __restrict__ baseline, int m0, int M_global, int d, int N, int S,
                                                  LIN_ALPHA_PARAM, float tau, int layout, int tiny, float obs_noise, float mu, float sig,
                                                  LIN_SFB_PARAM LIN_ANY_PARAM, GradSplit gs) {
  const LinGradJob job = blockIdx.y ? job1 : job0;  // (grid = (Mloc, 2 estimators, shares); particle = (x + z) mod Mloc: see k_nn_grad)
  const float* __restrict__ logprobs = job.logprobs;
  float* __restrict__ out = job.out;
  const size_t out_stride = job.out_stride;
  float* __restrict__ theta_copy = job.theta_copy;
  float* __restrict__ baseline_out = job.baseline_out;
  const Key2 carry = job.carry;
  const int mode = job.mode;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const LinGeom g = lin_geom(d, N, NT);
  float* X = smem;
  float* WG = X + (size_t)g.np * g.ldx;
  float* RS = WG + (size_t)g.kp * g.ldw;  // residuals [np][ldw]
  double* red = reinterpret_cast<double*>(smem + ((((size_t)g.np * g.ldx + (size_t)g.kp * g.ldw + (size_t)g.np * g.ldw) + 3) & ~(size_t)3));
  const int m = (int)((blockIdx.x + blockIdx.z) % gridDim.x), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LIN_CHAIN_DATA(m)
  LIN_CHAIN_SFB
  const size_t dd = (size_t)d * d;
  const float* __restrict__ TH = theta + (size_t)m * dd;
  const Key2 key = lin_mode_key(mode, carry, M_global, m0 + m, layout);
  const uint64_t nbits = (uint64_t)S * dd;
  const float* lp = logprobs + (size_t)m * S;
  // softmax statistics (double), number of samples with a non-zero weight; this block's share of them: ordinals q = bz, bz + NS, ...
  __shared__ float wch[GRAD_WCH];
  __shared__ int last_flag;
  double mx, den, sm;
  int nnz;
  grad_softmax_stats(lp, S, red, mx, den, sm, nnz);
  const int NS = gridDim.z, bz = blockIdx.z, nact = nnz < NS ? (nnz > 0 ? nnz : 1) : NS;
  if (bz >= nact) return;  // (block-uniform: no share -- before anything is staged)
  lin_load_common<NT>(X, x, g, tid);
  for (int e = tid; e < g.np * g.ldw; e += 256) RS[e] = 0.f;

  // accumulators in the MFMA C layout: element (i = ti*16 + (lane>>4)*4 + r, j = tj*16 + (lane&15)), ti = wave + 4*u
  constexpr int NU = (NT + 3) / 4;
  f32x4 acc[NU][NT];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[u][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float inv_on = 1.0f / obs_noise;
  const float* sc_m = scores + (size_t)m * dd;
  const uint32_t* thr_m = thr + (size_t)m * dd;

  int q = 0;  // ordinal of the next sample with a non-zero weight
  for (int s0 = 0; s0 < S; s0 += GRAD_WCH) {
    __syncthreads();
    if (s0 + tid < S) wch[tid] = (float)(exp((double)lp[s0 + tid] - mx) / den);
    __syncthreads();
  for (int s = s0; s < S && s < s0 + GRAD_WCH; ++s) {
    const float w = wch[s - s0];
    if (w < GRAD_W_MIN) continue;  // block-uniform
    if ((q++ % NS) != bz) continue;  // (another block's sample)
    if (mode == LIN_MODE_Z_SCORE) {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = (wave + 4 * u) * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15);
            if (i < d && j < d) acc[u][tj][r] += w * lin_sample_g(mode, key, nbits, dd, s, i, j, d, thr_m, sc_m, alpha, tau, layout, tiny);
          }
      continue;
    }
    __syncthreads();
    lin_build_wg<NT>(WG, TH, mode, key, nbits, s, thr_m, sc_m, alpha, tau, layout, tiny, mu, sig, g, tid);
    __syncthreads();
    lin_pred_tiles<NT>(X, WG, g, lane, wave, [&](int n, int j, float pred) {
      const bool mk = any_mask && mask[(size_t)n * d + j];
      RS[n * g.ldw + j] = mk ? 0.f : (X[n * g.ldx + j] - pred) * inv_on;
    });
    __syncthreads();
    // xtr = X^T * RS (K = np), then fold into the accumulators
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ti = wave + 4 * u;
      if (ti >= NT) continue;  // (not `break`: keeps the trip count constant so the loop unrolls)
      f32x4 t[NT];
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) t[tj] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int ap = (lane >> 4) * g.ldx + ti * 16 + (lane & 15);
      const int bq = (lane >> 4) * g.ldw + (lane & 15);
      for (int k0 = 0; k0 < g.np; k0 += 4) {
        const float a = X[ap + k0 * g.ldx];
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) t[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, RS[bq + k0 * g.ldw + tj * 16], t[tj], 0, 0, 0);
      }
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = ti * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15);
          if (i < d && j < d) {
            float xtr = t[tj][r];
            asm volatile("" : "+v"(xtr));
            const float th = TH[i * d + j];
            if (mode == LIN_MODE_THETA) {
              const float gv = lin_sample_g(mode, key, nbits, dd, s, i, j, d, thr_m, sc_m, alpha, tau, layout, tiny);
              acc[u][tj][r] += w * gv * (-(th - mu) / (sig * sig) + xtr);
            } else if (i != j) {
              const float gv = lin_sample_g(mode, key, nbits, dd, s, i, j, d, thr_m, sc_m, alpha, tau, layout, tiny);
              acc[u][tj][r] += w * (lin_logn(th, mu, sig) + th * xtr) * tau * alpha * gv * (1.0f - gv);
            }
          }
        }
    }
  }
  }
  if (nact > 1) {
    // partial sums in thread layout ([value][thread]: coalesced, no index arithmetic); the last block adds them in block order
    float* const base = gs.part + ((size_t)(m * 2 + (int)blockIdx.y) * NS) * gs.stride;
    float* const mine = base + (size_t)bz * gs.stride + tid;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) grad_part_store(mine + (size_t)((u * NT + tj) * 4 + r) * 256, acc[u][tj][r]);
    if (!grad_last_block(gs.ctr + (m * 2 + (int)blockIdx.y), nact, &last_flag)) return;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][tj][r] = grad_part_sum<GRAD_NS, true>(base, gs.stride, (size_t)((u * NT + tj) * 4 + r) * 256 + tid, nact);
  }
  // epilogue
  const float bold = baseline ? baseline[m] : 0.f;
  const float scale = (mode == LIN_MODE_Z_SCORE && sf_baseline > 0.0) ? (float)exp(-(double)bold) : 1.0f;
  float* om = out + (size_t)m * out_stride;
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (wave + 4 * u) * 16 + (lane >> 4) * 4 + r, j = tj * 16 + (lane & 15);
        if (i < d && j < d) {
          float v = acc[u][tj][r];
          if (mode == LIN_MODE_Z_SCORE) {
            const float p = (float)sigmoid_d((double)__fmul_rn(alpha, sc_m[i * d + j]));
            v = i == j ? 0.f : scale * alpha * (v - p);
          }
          om[i * d + j] = v;
          if (theta_copy) theta_copy[(size_t)m * out_stride + i * d + j] = TH[i * d + j];
        }
      }
  if (mode != LIN_MODE_THETA && baseline_out && tid == 0)
    baseline_out[m] = (mode == LIN_MODE_Z_SCORE) ? (float)(sf_baseline * (sm / S) + (1.0 - sf_baseline) * (double)bold) : bold;
}
