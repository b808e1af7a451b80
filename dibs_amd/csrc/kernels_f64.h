// Float64 engine (include/dibs_hip.h, dibs_config.reserved_i[1] = 64): MarginalDiBS + BGe + score-function estimator, one rank, one problem.
// Every quantity after a random draw is a double and every operation is the one the f64 build of oracle/dibs_oracle.c performs, in the same
// order, without contraction (the pragma below; tu_f64.hip is also compiled with -ffp-contract=off).  The draws themselves are the f32
// streams of rng.h: a Bernoulli edge compares the f32 uniform with the edge probability rounded to float (the `thr` test of the f32 engine),
// the acyclicity noise is the f32 logistic value of the oracle's C-library logf (a table over the 2^23 f32 uniforms, engine_f64.hip:
// f64_logistic_table) widened to double.  Only the matrix products of the acyclicity term differ in rounding from the oracle
// (v_mfma_f64_16x16x4_f64 accumulates with fused multiply-adds in its own order).
//   reference: dibs/inference/dibs.py:102-184, 325-391, 557-658; dibs/models/linearGaussian.py:63-118; dibs/graph_utils.py:8-28;
//              dibs/kernel.py:20-30; dibs/inference/svgd.py:165-267
// Launches of one step (engine_f64.hip, step_f64): k64_edge | k64_bge -> k64_weights (main stream) beside k64_acyc -> k64_acyc_reduce ->
// k64_kmat (second stream), then k64_grad -> k64_phi -> k64_update.
#pragma once
#include "common.h"
#include "launch.h"
#include "../../include/dibs_hip.h"

#pragma clang fp contract(off)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// scores = U V^T (k-ordered sum, one rounding per product and per add), edge probabilities p = sigmoid(alpha s) and the Bernoulli
// thresholds of the f32 engine formed from (float) p.  grid = Mloc, block = 256
__global__ __launch_bounds__(256) void k64_edge(F64Args a) {
  const int m = blockIdx.x, d = a.d, k = a.k, dd = d * d;
  const double* zm = a.z + (size_t)m * a.D;
  for (int o = threadIdx.x; o < dd; o += 256) {
    const int i = o / d, j = o - i * d;
    double acc = 0.0;
    for (int q = 0; q < k; ++q) acc = acc + zm[(i * k + q) * 2] * zm[(j * k + q) * 2 + 1];
    const size_t go = (size_t)m * dd + o;
    const double pv = sigmoid_d(a.alpha * acc);
    a.scores[go] = acc;
    a.probs[go] = pv;
    a.thr[go] = i == j ? 0u : (uint32_t)ceilf((float)pv * 8388608.0f);
  }
}

// BGe: one wave per (particle m, node j) walks the S samples: the parent set of j (lane i draws edge i -> j), then the node score from a
// Cholesky factorisation of R[pa + j, pa + j] with j last (the oracle's bge_mode 1, the same left-looking order), in double.  Lane r owns
// row r; the factor lives in LDS column-major (column q at A + 64 q).  grid = (ceil(d / 4), Mloc), block = 256, LDS = 4 * f64_bge_wave_bytes
__global__ __launch_bounds__(256) void k64_bge(F64Args a) {
  extern __shared__ double lds64[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = a.d, dd = d * d, j = blockIdx.x * 4 + wave, m = blockIdx.y;
  if (j >= d) return;  // (no block barrier below)
  double* A = lds64 + (size_t)wave * (f64_bge_wave_bytes(d) / 8);
  int* idx = (int*)(A + (size_t)d * 64);
  const Key2 pk = rng_split_row(a.carry_lik, (uint32_t)a.M + 1u, (uint32_t)m + 1u, a.L);  // subk of particle m   svgd.py:245
  const Key2 kg = rng_split_row(pk, 2u, 1u, a.L);                                           // subk, subk_ = split  dibs.py:350
  const uint64_t nbits = (uint64_t)a.S * dd;
  const uint32_t th = lane < d ? a.thr[(size_t)m * dd + (size_t)lane * d + j] : 0u;
  const double Nn = a.Nj[j], al = a.alpha_lambd;
  const double* R = a.R + (a.n_mats > 1 ? (size_t)j * dd : 0);
  for (int s = 0; s < a.S; ++s) {
    bool par = false;
    if (lane < d) par = (rng_bits_at(kg, nbits, (uint64_t)s * dd + (uint64_t)lane * d + j, a.L) >> 9) < th;  // u < (float) p
    const uint64_t mask = __ballot(par);
    const size_t code = ((size_t)m * d + j) * a.S + s;
    double score = 0.0;
    if (Nn != 0.0) {
      const int l = __popcll(mask), n = l + 1;
      if (par) idx[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
      if (lane == 0) idx[l] = j;
      wave_lds_fence();
      const int r = lane;
      if (r < n) {
        const double* Rr = R + (size_t)idx[r] * d;
        for (int q = 0; q <= r; ++q) A[q * 64 + r] = Rr[idx[q]];
      }
      wave_lds_fence();
      double ld = 0.0, ld_pa = 0.0;
      for (int kk = 0; kk < n; ++kk) {
        double t = 0.0;
        if (r >= kk && r < n) {
          t = A[kk * 64 + r];
          for (int p = 0; p < kk; ++p) t = t - A[p * 64 + r] * A[p * 64 + kk];
        }
        const double lkk = sqrt(__shfl(t, kk, 64));
        if (r > kk && r < n) A[kk * 64 + r] = t / lkk;
        if (kk == n - 1) ld_pa = ld;
        ld = ld + 2.0 * log(lkk);
        wave_lds_fence();
      }
      score = a.gam[(size_t)j * (d + 1) + l] + 0.5 * (Nn + al - d + l) * ld_pa - 0.5 * (Nn + al - d + l + 1) * ld;
    }
    if (lane == 0) {
      a.masks[code] = mask;  // (one word: n_vars <= 64)
      a.node_scores[code] = score;
    }
  }
}

// log-probabilities l_s = sum_j node scores, softmax weights w_s (with the score-function baseline), W_lik = scale alpha (sum_s w_s G_s - P)
// and the baseline update (dibs.py:363-382).  grid = Mloc, block = 256, LDS = 2 S doubles
__global__ __launch_bounds__(256) void k64_weights(F64Args a) {
  extern __shared__ double lds64[];
  __shared__ double s_mx, s_den, s_scale;
  double *lps = lds64, *w = lds64 + a.S;
  const int m = blockIdx.x, d = a.d, dd = d * d, S = a.S, tid = threadIdx.x;
  for (int s = tid; s < S; s += 256) {
    double tot = 0.0;
    for (int j = 0; j < d; ++j) tot = tot + a.node_scores[((size_t)m * d + j) * S + s];
    lps[s] = tot;
    a.logprobs[(size_t)m * S + s] = tot;
  }
  __syncthreads();
  if (tid == 0) {
    double mx = -INFINITY, den = 0.0;
    for (int s = 0; s < S; ++s) mx = lps[s] > mx ? lps[s] : mx;
    for (int s = 0; s < S; ++s) den = den + exp(lps[s] - mx);
    s_mx = mx;
    s_den = den;
    s_scale = a.sfb > 0 ? exp(-a.baseline[m]) : 1.0;
  }
  __syncthreads();
  for (int s = tid; s < S; s += 256) w[s] = exp(lps[s] - s_mx) / s_den;
  __syncthreads();
  for (int o = tid; o < dd; o += 256) {
    const int i = o / d, j = o - i * d;
    const uint64_t* mk = a.masks + ((size_t)m * d + j) * S;
    double acc = 0.0;
    for (int s = 0; s < S; ++s)
      if ((mk[s] >> i) & 1ull) acc = acc + w[s];
    const size_t go = (size_t)m * dd + o;
    a.w_lik[go] = i == j ? 0.0 : s_scale * a.alpha * (acc - a.probs[go]);
  }
  if (tid == 0) {
    double bsum = 0.0;
    for (int s = 0; s < S; ++s) bsum = bsum + lps[s];
    a.baseline[m] = a.sfb * (bsum / S) + (1 - a.sfb) * a.baseline[m];
  }
}

// C = A B of two dp x dp matrices in LDS (row stride ld) on the f64 matrix pipe: the 4 waves take the 16 x 16 output tiles in turn.
// v_mfma_f64_16x16x4_f64: A / B operands as the f32 16x16x4 form (lane l: A[l & 15][l >> 4], B[l >> 4][l & 15]); C / D entry r of lane l
// is C[(l >> 4) + 4 r][l & 15] (MI355X_MICROARCH.md: the f64 layout differs from every other MFMA).
__device__ __forceinline__ void k64_matmul(const double* A, const double* B, double* C, int dp, int ld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nt = dp / 16;
  for (int t = wave; t < nt * nt; t += 4) {
    const int ti = t / nt, tj = t - ti * nt;
    const double* ap = A + (size_t)(ti * 16 + (lane & 15)) * ld + (lane >> 4);
    const double* bp = B + (size_t)(lane >> 4) * ld + tj * 16 + (lane & 15);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < dp; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k0], bp[(size_t)k0 * ld], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(size_t)(ti * 16 + (lane >> 4) + 4 * r) * ld + tj * 16 + (lane & 15)] = acc[r];
  }
  __syncthreads();
}

// acyclicity: one block per chain (s, m): G~ = sigmoid(tau (eps + alpha s)), (I + G~ / d)^(d-1) by binary powering in the order of
// jnp.linalg.matrix_power (graph_utils.py:26), then the chain's term (M^(d-1))^T o tau alpha G~ (1 - G~) -> part[m][s].  Three dp x dp
// matrices in LDS (dp = n_vars rounded up to 16); G~ waits in `part` (each thread reads back only what it wrote).
// grid = (Sa, Mloc), block = 256, LDS = f64_acyc_lds_bytes
__global__ __launch_bounds__(256) void k64_acyc(F64Args a) {
  extern __shared__ double lds64[];
  const int s = blockIdx.x, m = blockIdx.y, d = a.d, dd = d * d, dp = a.dpad, ld = dp + 1, tid = threadIdx.x;
  double* buf[3] = {lds64, lds64 + (size_t)dp * ld, lds64 + (size_t)2 * dp * ld};
  const Key2 km = rng_split_row(a.carry_prior, (uint32_t)a.M + 1u, (uint32_t)m + 1u, a.L);  // the particle key itself  dibs.py:595
  const uint64_t nbits = (uint64_t)a.Sa * dd;
  double* part = a.part + ((size_t)m * a.Sa + s) * dd;
  const double* sc = a.scores + (size_t)m * dd;
  for (int o = tid; o < dp * dp; o += 256) {
    const int i = o / dp, j = o - i * dp;
    double v = 0.0;
    if (i < d && j < d) {
      double gv = 0.0;
      if (i != j) {
        const float e = a.ltab[rng_bits_at(km, nbits, (uint64_t)s * dd + (uint64_t)i * d + j, a.L) >> 9];  // logistic(bits), oracle's logf
        gv = sigmoid_d(a.tau * ((double)e + a.alpha * sc[i * d + j]));
      }
      part[i * d + j] = gv;
      v = (i == j ? 1.0 : 0.0) + gv / (double)d;
    }
    buf[0][(size_t)i * ld + j] = v;
  }
  __syncthreads();
  // result = m^(d-1): squarings of zb into a scratch buffer, result = result zb when the bit is set (the first time a copy of zb)
  int zi = 0, ri = -1, n = d - 1;
  bool first = true;
  while (n > 0) {
    if (!first) {
      int tmp = 0;
      while (tmp == zi || tmp == ri) ++tmp;
      k64_matmul(buf[zi], buf[zi], buf[tmp], dp, ld);
      zi = tmp;
    }
    first = false;
    const int bit = n & 1;
    n >>= 1;
    if (bit) {
      int tmp = 0;
      while (tmp == zi || tmp == ri) ++tmp;
      if (ri < 0) {
        for (int o = tid; o < dp * ld; o += 256) buf[tmp][o] = buf[zi][o];
        __syncthreads();
      } else {
        k64_matmul(buf[ri], buf[zi], buf[tmp], dp, ld);
      }
      ri = tmp;
    }
  }
  const double* pw = buf[ri];
  for (int o = tid; o < dp * dp; o += 256) {
    const int i = o / dp, j = o - i * dp;
    if (i < d && j < d) {
      const double gs = part[i * d + j];
      part[i * d + j] = i != j ? pw[(size_t)j * ld + i] * a.tau * a.alpha * gs * (1.0 - gs) : 0.0;
    }
  }
}

// W_acyc = (sum over the chains in order) / Sa.  grid = Mloc, block = 256
__global__ __launch_bounds__(256) void k64_acyc_reduce(F64Args a) {
  const int m = blockIdx.x, dd = a.d * a.d;
  for (int o = threadIdx.x; o < dd; o += 256) {
    double acc = 0.0;
    for (int s = 0; s < a.Sa; ++s) acc = acc + a.part[((size_t)m * a.Sa + s) * dd + o];
    a.w_acyc[(size_t)m * dd + o] = acc / (double)a.Sa;
  }
}

// grad_z = [W V, W^T U] - z / sigma^2 with W = W_lik - beta W_acyc + grad of the ER / SF graph prior (dibs.py:604-658).
// grid = Mloc, block = 256, LDS = (d d + d) doubles
__global__ __launch_bounds__(256) void k64_grad(F64Args a) {
  extern __shared__ double lds64[];
  const int m = blockIdx.x, d = a.d, k = a.k, dd = d * d, tid = threadIdx.x;
  double *W = lds64, *colsum = lds64 + dd;
  const double* P = a.probs + (size_t)m * dd;
  for (int j = tid; j < d; j += 256) {
    double cs = 0.0;
    for (int i = 0; i < d; ++i) cs = cs + (i == j ? 0.0 : P[i * d + j]);
    colsum[j] = cs;
  }
  __syncthreads();
  for (int o = tid; o < dd; o += 256) {
    const int i = o / d, j = o - i * d;
    double pr = 0.0;
    if (i != j) {
      const double dp = a.alpha * P[o] * (1.0 - P[o]);
      if (a.prior == DIBS_PRIOR_ER) pr = a.er_c * dp;
      else if (a.prior == DIBS_PRIOR_SF) pr = -3.0 / (1.0 + colsum[j]) * dp;
      else if (a.prior == DIBS_PRIOR_EDGEWISE) pr = a.prior_tab[o] * dp;
    }
    W[o] = a.w_lik[(size_t)m * dd + o] - a.beta * a.w_acyc[(size_t)m * dd + o] + pr;
  }
  __syncthreads();
  const double* zm = a.z + (size_t)m * a.D;
  double* gm = a.gradz + (size_t)m * a.D;
  for (int e = tid; e < d * k; e += 256) {
    const int i = e / k, q = e - i * k;
    double su = 0.0, sv = 0.0;
    for (int j = 0; j < d; ++j) {
      su = su + W[i * d + j] * zm[(j * k + q) * 2 + 1];
      sv = sv + W[j * d + i] * zm[(j * k + q) * 2];
    }
    gm[(i * k + q) * 2] = su - zm[(i * k + q) * 2] * a.inv_sig2;
    gm[(i * k + q) * 2 + 1] = sv - zm[(i * k + q) * 2 + 1] * a.inv_sig2;
  }
}

// kernel matrix kxx[a][b] = scale exp(-||z_a - z_b||^2 / h) (kernel.py:20-30).  grid = Mloc, block = 256
__global__ __launch_bounds__(256) void k64_kmat(F64Args a) {
  const int ia = blockIdx.x;
  const double* za = a.z + (size_t)ia * a.D;
  for (int b = threadIdx.x; b < a.M; b += 256) {
    const double* zb = a.z + (size_t)b * a.D;
    double s = 0.0;
    for (int64_t i = 0; i < a.D; ++i) {
      const double df = za[i] - zb[i];
      s = s + df * df;
    }
    a.kxx[(size_t)ia * a.M + b] = a.scale * exp(-s / a.h);
  }
}

// phi_a = -(1/M) sum_b [k[a,b] grad_b - (2/h) k[a,b] (z_b - z_a)] (svgd.py:194-224).  grid = (ceil(D / 256), Mloc), block = 256
__global__ __launch_bounds__(256) void k64_phi(F64Args a) {
  const int ia = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.D) return;
  const double za = a.z[(size_t)ia * a.D + i], c2 = 2.0 / a.h;
  const double* kr = a.kxx + (size_t)ia * a.M;
  double s = 0.0;
  for (int b = 0; b < a.M; ++b) {
    const double kk = kr[b];
    s = s + (kk * a.gradz[(size_t)b * a.D + i] - c2 * kk * (a.z[(size_t)b * a.D + i] - za));
  }
  a.phi[(size_t)ia * a.D + i] = -s / a.M;
}

// optimizer step (jax.example_libraries.optimizers: rmsprop gamma 0.9, eps 1e-8 inside the sqrt; gd), the oracle's f64 operation order
// (moment constant 1 - 0.9 in double).  grid = ceil(Mloc D / 256), block = 256
__global__ __launch_bounds__(256) void k64_update(F64Args a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.M * a.D) return;
  const double g = a.phi[i];
  if (a.opt == DIBS_OPT_RMSPROP) {
    const double v = a.vz[i] * 0.9 + g * g * (1.0 - 0.9);
    a.vz[i] = v;
    a.z[i] = a.z[i] - a.step * g / sqrt(v + 1e-8);
  } else {
    a.z[i] = a.z[i] - a.step * g;
  }
}
