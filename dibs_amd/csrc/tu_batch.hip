// translation unit: the table-reading kernels of the batched engine (include/dibs_hip.h, dibs_engine_set_problem_hparams; ProblemHP in
// common.h) and their launchers.  Each is the block of a standalone kernel under a __global__ that takes the scalar(s) of the block's problem
// from the per-problem table.  A unit of their own, so that the units of the standalone kernels compile what they compiled without them.
// Further down: the chain-aware kernels of the chains engine (n_chains; keys, block-diagonal kernel matrices) and their launchers, each
// also in a form that reads the per-chain table (dibs_engine_set_chain_hparams); the edge, acyclicity and tail launches above serve a
// chains engine's table tier as they are, with pM = one chain's particles.
#define DIBS_TU_BATCH
#include "engine_impl.h"
#include "kernels_edge_p.h"
#include "kernels_acyc.h"
#include "kernels_acyc_bf16.h"
#include "kernels_acyc_f16.h"
#include "bandwidth_select.h"

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
  const dim3 grid(a.units, a.Mloc);
  if (a.paired) {
    dibs_allow_lds((const void*)k_acyc_batch<NT, true>, lds);
    hipLaunchKernelGGL((k_acyc_batch<NT, true>), grid, dim3(256), lds, a.stream, a.scores, a.part, a.carry, a.m0, a.M, a.d, a.Sa, hp, pM, a.tau,
                       a.layout, a.tiny);
  } else {
    dibs_allow_lds((const void*)k_acyc_batch<NT, false>, lds);
    hipLaunchKernelGGL((k_acyc_batch<NT, false>), grid, dim3(256), lds, a.stream, a.scores, a.part, a.carry, a.m0, a.M, a.d, a.Sa, hp, pM, a.tau,
                       a.layout, a.tiny);
  }
}
template <bool FOUR>
static void launch_hf_batch(const AcycLaunch& a, const ProblemHP* hp, int pM) {
  const size_t lds = (size_t)AHF_LDS_BYTES;
  dibs_allow_lds((const void*)k_acyc_hf_batch<FOUR, 3>, lds);
  hipLaunchKernelGGL((k_acyc_hf_batch<FOUR, 3>), dim3(a.units, (a.Mloc + 7) & ~7), dim3(256), lds, a.stream, a.scores, a.eas, a.part, a.carry, a.m0,
                     a.M, a.Mloc, a.d, a.Sa, hp, pM, a.tau, a.layout, a.tiny);
}
void batch_launch_acyc_power(const AcycLaunch& a, const ProblemHP* hp, int pM) {
  if (a.pipe != DIBS_PIPE_F32 && a.paired && a.d >= 33) {  // (acyc_use_bf16 of tu_acyc.hip; the bf16 pipe never comes here)
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

// ---- chains engine (include/dibs_hip.h: n_chains = C > 1; rows [C * M], chain-major, ONE joint model on ONE data set) -------------------
// per-chain keys of one step from the C device-resident loop-carry keys, in the order of step_local for a joint model (svgd.py:695-703 per
// chain): carry_theta = carry, carry_lik = row 0 of split(carry_theta, M + 1), carry_prior = row 0 of split(carry_lik, M + 1), and the carry
// advances to row 0 of split(carry_prior, M + 1); particle m's key of an estimator is row 1 + m of that estimator's split.  grid = C
// (returns carry_prior: thread 0 of the caller advances the carry to row 0 of its split)
__device__ __forceinline__ Key2 chain_keys_block(Key2* __restrict__ carry, Key2* __restrict__ keys_theta, Key2* __restrict__ keys_lik,
                                                 Key2* __restrict__ keys_prior, int M, int layout) {
  const int p = blockIdx.x;
  const uint32_t n = (uint32_t)M + 1u;
  const Key2 c_theta = carry[p];
  const Key2 c_lik = rng_split_row(c_theta, n, 0u, layout);
  const Key2 c_prior = rng_split_row(c_lik, n, 0u, layout);
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    const size_t o = (size_t)p * M + m;
    keys_theta[o] = rng_split_row(c_theta, n, (uint32_t)m + 1u, layout);
    keys_lik[o] = rng_split_row(c_lik, n, (uint32_t)m + 1u, layout);
    keys_prior[o] = rng_split_row(c_prior, n, (uint32_t)m + 1u, layout);
  }
  __syncthreads();  // (every thread has read carry[p])
  return c_prior;
}
__global__ __launch_bounds__(256) void k_chain_keys(Key2* __restrict__ carry, Key2* __restrict__ keys_theta, Key2* __restrict__ keys_lik,
                                                    Key2* __restrict__ keys_prior, int M, int layout) {
  const Key2 c_prior = chain_keys_block(carry, keys_theta, keys_lik, keys_prior, M, layout);
  if (threadIdx.x == 0) carry[blockIdx.x] = rng_split_row(c_prior, (uint32_t)M + 1u, 0u, layout);
}
// per-chain hyper-parameters (dibs_engine_set_chain_hparams): the same block, and this step's annealed alpha and beta of chain p to its row
// of the table -- (float)(alpha_linear * t) with the product in double, as step_local forms it on the host and k_batch_keys for a problem
__global__ __launch_bounds__(256) void k_chain_keys_hp(Key2* __restrict__ carry, Key2* __restrict__ keys_theta, Key2* __restrict__ keys_lik,
                                                       Key2* __restrict__ keys_prior, int M, int layout, ProblemHP* __restrict__ hp, int t) {
  const Key2 c_prior = chain_keys_block(carry, keys_theta, keys_lik, keys_prior, M, layout);
  if (threadIdx.x == 0) {
    const int p = blockIdx.x;
    carry[p] = rng_split_row(c_prior, (uint32_t)M + 1u, 0u, layout);
    hp[p].alpha = (float)(hp[p].alpha_linear * (double)t);
    hp[p].beta = (float)(hp[p].beta_linear * (double)t);
  }
}
void chains_launch_keys(hipStream_t st, Key2* carry, Key2* keys_theta, Key2* keys_lik, Key2* keys_prior, int C, int M, int layout) {
  hipLaunchKernelGGL(k_chain_keys, dim3(C), dim3(256), 0, st, carry, keys_theta, keys_lik, keys_prior, M, layout);
}
void chains_launch_keys_hp(hipStream_t st, Key2* carry, Key2* keys_theta, Key2* keys_lik, Key2* keys_prior, int C, int M, int layout, ProblemHP* hp,
                           int t) {
  hipLaunchKernelGGL(k_chain_keys_hp, dim3(C), dim3(256), 0, st, carry, keys_theta, keys_lik, keys_prior, M, layout, hp, t);
}

// block-diagonal kernel matrix of one segment (z or theta), kout [C * M][M]: row a of chain p = a / M against the M particles of p only, by
// the code of the standalone launch (kmat_block, symmetric) -- bit-identical entries; ksum != null: kadd + k as well (the weight matrix
// kz + kt of the SVGD transform).  grid = (C * M, ceil(M / KMAT_BT))
__device__ __forceinline__ void kmat_chains_block(float* smem, const float* __restrict__ x, size_t stride, int len, float* __restrict__ kout, int M,
                                                  float scale, float h, const float* __restrict__ kadd, float* __restrict__ ksum) {
  const int a = blockIdx.x, p = a / M;
  const size_t ko = (size_t)p * M * M;
  kmat_block(smem, x + (size_t)p * M * stride, stride, 0, len, kout + ko, 0, M, scale, h, 1, a - p * M, blockIdx.y, kadd ? kadd + ko : nullptr,
             ksum ? ksum + ko : nullptr);
}
__global__ __launch_bounds__(256) void k_kmat_chains(const float* __restrict__ x, size_t stride, int len, float* __restrict__ kout, int M,
                                                     float scale, float h, const float* __restrict__ kadd, float* __restrict__ ksum) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  kmat_chains_block(smem, x, stride, len, kout, M, scale, h, kadd, ksum);
}
// per-chain hyper-parameters: the bandwidth of the block's chain from the table (theta_seg: the parameter kernel's h_theta)
__global__ __launch_bounds__(256) void k_kmat_chains_hp(const float* __restrict__ x, size_t stride, int len, float* __restrict__ kout, int M,
                                                        float scale, const ProblemHP* __restrict__ hp, int theta_seg,
                                                        const float* __restrict__ kadd, float* __restrict__ ksum) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const ProblemHP& r = hp[blockIdx.x / (unsigned)M];
  kmat_chains_block(smem, x, stride, len, kout, M, scale, theta_seg ? r.h_theta : r.h, kadd, ksum);
}
// ... the tiled form (standalone engines from DibsTuning::kmat_tiled_min particles): blockIdx.y = chain, one piece per tile (nsplit = 1: the
// entries do not depend on the cut, see KmatTile).  kt describes chain 0
__device__ __forceinline__ void kmat_tile_chains_block(float* smem, const KmatTile& kt, float h) {
  const size_t p = blockIdx.y, ko = p * (size_t)kt.M * kt.M;
  KmatTile k = kt;
  k.h = h;
  k.x = kt.x + p * (size_t)kt.M * kt.stride;
  k.kout = kt.kout + ko;
  if (kt.ksum) {
    k.kadd = kt.kadd + ko;
    k.ksum = kt.ksum + ko;
  }
  kmat_tile_block(smem, k, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x);
}
__global__ __launch_bounds__(KT_NT) void k_kmat_tile_chains(KmatTile kt) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  kmat_tile_chains_block(smem, kt, kt.h);
}
__global__ __launch_bounds__(KT_NT) void k_kmat_tile_chains_hp(KmatTile kt, const ProblemHP* __restrict__ hp, int theta_seg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const ProblemHP& r = hp[blockIdx.y];
  kmat_tile_chains_block(smem, kt, theta_seg ? r.h_theta : r.h);
}
// one segment's matrix of every chain on `st`; `tiled`: the choice of a standalone engine of M particles (made by the caller from M alone)
void chains_launch_kmat(hipStream_t st, bool tiled, const float* x, size_t len, float* kout, int C, int M, float scale, float h, const float* kadd,
                        float* ksum, size_t lds_direct) {
  if (tiled) {
    const int nta = (M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, nta, 1), nchunk = kmat_nchunk((int)len);
    const KmatTile kt{x, len, 0, (int)len, nullptr, 0, M, M, nchunk, nta, nta, 1, 1, nchunk, scale, h, kout, kadd, ksum, nullptr};
    dibs_allow_lds((const void*)k_kmat_tile_chains, kmat_tile_lds_bytes());
    hipLaunchKernelGGL(k_kmat_tile_chains, dim3((unsigned)tiles, (unsigned)C), dim3(KT_NT), kmat_tile_lds_bytes(), st, kt);
    return;
  }
  dibs_allow_lds((const void*)k_kmat_chains, lds_direct);
  hipLaunchKernelGGL(k_kmat_chains, dim3((unsigned)(C * M), (unsigned)((M + KMAT_BT - 1) / KMAT_BT)), dim3(256), lds_direct, st, x, len, (int)len, kout, M,
                     scale, h, kadd, ksum);
}
// ... with chain p's bandwidth from the table (per-chain hyper-parameters): the same grids, LDS sizes and tile descriptions
void chains_launch_kmat_hp(hipStream_t st, bool tiled, const float* x, size_t len, float* kout, int C, int M, float scale, const ProblemHP* hp,
                           int theta_seg, const float* kadd, float* ksum, size_t lds_direct) {
  if (tiled) {
    const int nta = (M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, nta, 1), nchunk = kmat_nchunk((int)len);
    const KmatTile kt{x, len, 0, (int)len, nullptr, 0, M, M, nchunk, nta, nta, 1, 1, nchunk, scale, 0.f, kout, kadd, ksum, nullptr};
    dibs_allow_lds((const void*)k_kmat_tile_chains_hp, kmat_tile_lds_bytes());
    hipLaunchKernelGGL(k_kmat_tile_chains_hp, dim3((unsigned)tiles, (unsigned)C), dim3(KT_NT), kmat_tile_lds_bytes(), st, kt, hp, theta_seg);
    return;
  }
  dibs_allow_lds((const void*)k_kmat_chains_hp, lds_direct);
  hipLaunchKernelGGL(k_kmat_chains_hp, dim3((unsigned)(C * M), (unsigned)((M + KMAT_BT - 1) / KMAT_BT)), dim3(256), lds_direct, st, x, len, (int)len, kout, M,
                     scale, hp, theta_seg, kadd, ksum);
}

// ---- median-heuristic kernel bandwidth (dibs_config.reserved_i[3]) -----------------------------------------------
// Per run (a standalone engine's particles, a problem, a chain) and segment (z, theta): h = median ||x_a - x_b||^2 / log(M + 1), selected on
// the device in front of the kernel matrices of every step.  Three launches on one stream: the distance pass below, the selection, then the
// table-reading kernel matrices above (the batched engine's: kernels_marginal.h), which find the bandwidth in the run's row of ProblemHP.
//
// 1. distance pass: the block functions of the kernel matrices with the DIST epilogue -- out [C * M][M] holds (float)tot of every pair, the
//    very sums the matrices form again behind the selection (same code, same grids: symmetric, zero diagonal).  Grids and LDS as
//    k_kmat_chains / k_kmat_tile_chains.
__global__ __launch_bounds__(256) void k_sqdist_chains(const float* __restrict__ x, size_t stride, int len, float* __restrict__ out, int M) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int a = blockIdx.x, p = a / M;
  kmat_block<true>(smem, x + (size_t)p * M * stride, stride, 0, len, out + (size_t)p * M * M, 0, M, 0.f, 0.f, 1, a - p * M, blockIdx.y);
}
__global__ __launch_bounds__(KT_NT) void k_sqdist_tile_chains(KmatTile kt) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const size_t p = blockIdx.y;
  KmatTile k = kt;
  k.x = kt.x + p * (size_t)kt.M * kt.stride;
  k.kout = kt.kout + p * (size_t)kt.M * kt.M;
  kmat_tile_block<true>(smem, k, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x);
}
void bandwidth_launch_sqdist(hipStream_t st, bool tiled, const float* x, size_t len, float* out, int C, int M, size_t lds_direct) {
  if (tiled) {
    const int nta = (M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, nta, 1), nchunk = kmat_nchunk((int)len);
    const KmatTile kt{x, len, 0, (int)len, nullptr, 0, M, M, nchunk, nta, nta, 1, 1, nchunk, 0.f, 0.f, out, nullptr, nullptr, nullptr};
    dibs_allow_lds((const void*)k_sqdist_tile_chains, kmat_tile_lds_bytes());
    hipLaunchKernelGGL(k_sqdist_tile_chains, dim3((unsigned)tiles, (unsigned)C), dim3(KT_NT), kmat_tile_lds_bytes(), st, kt);
    return;
  }
  dibs_allow_lds((const void*)k_sqdist_chains, lds_direct);
  hipLaunchKernelGGL(k_sqdist_chains, dim3((unsigned)(C * M), (unsigned)((M + KMAT_BT - 1) / KMAT_BT)), dim3(256), lds_direct, st, x, len, (int)len, out, M);
}

// 2. selection: one block per (run, segment on the median rule).  An exact radix select (bandwidth_select.h) on the bit patterns of the
//    P = M (M - 1) / 2 entries above the diagonal of the run's [M][M] block: four passes of one 8-bit digit each, most significant first,
//    for the two order statistics of the median at once (one histogram each; an odd P asks for the same one twice).  A pass counts with
//    integer LDS atomics only, so the result is the same whatever order the threads arrive in.  The values are RE-READ from the distance
//    buffer in every pass instead of being held in LDS: at most 255^2 floats = 254 KiB that the distance pass has just left in the L2,
//    read four times by 1 024 threads with coalesced loads, against 127 KiB of dynamic LDS that would keep the block off every CU on which
//    an acyclicity or estimator block of the other stream is resident -- this way the block needs 2 KiB.  Squared distances share their
//    leading digits (one or two exponents), so a thread merges runs of equal digits before it touches the histogram: the first passes
//    would otherwise be 32 000 atomics on one LDS word.  Wave w sweeps the rows w, w + 16, ... of the upper triangle, a lane the columns
//    a + 1 + lane, + 64, ...: contiguous loads, no division, and every loop bound a function of M (and the row) alone.  The walk from the
//    histogram to the digit is two levels of 16 (bw_walk): 16 threads per order statistic sum a group of bins each, one thread walks.
//    Thread 0 writes the bandwidth to the run's row of the table (h or h_theta) and to bw [C][2] (DIBS_BUF_BANDWIDTH).
__global__ __launch_bounds__(1024) void k_bandwidth_median(const float* __restrict__ sqd_z, const float* __restrict__ sqd_t, int seg_a, int seg_b,
                                                           int M, double inv_log, ProblemHP* __restrict__ hp, float* __restrict__ bw) {
  __shared__ uint32_t hist[2][BW_BINS];
  __shared__ uint32_t grp[2][BW_NGROUPS];
  __shared__ uint32_t sel[2][2];  // per order statistic: the digits chosen so far, the rank still wanted
  const int run = blockIdx.x, seg = blockIdx.y ? seg_b : seg_a, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* __restrict__ v = reinterpret_cast<const uint32_t*>((seg ? sqd_t : sqd_z) + (size_t)run * M * M);
  const uint32_t P = (uint32_t)M * (uint32_t)(M - 1) / 2u;
  const BwRanks want = bw_median_ranks(P);
  uint32_t pre[2] = {0u, 0u}, rank[2] = {want.lo, want.hi};
  for (int pass = 0; pass < BW_PASSES; ++pass) {
    for (int i = tid; i < 2 * BW_BINS; i += 1024) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t mask = bw_prefix_mask(pass);
    uint32_t last[2] = {0u, 0u}, cnt[2] = {0u, 0u};  // a thread's current run of equal digits
    for (int a = wave; a < M - 1; a += 16) {
      const uint32_t* __restrict__ row = v + (size_t)a * M;
      for (int b = a + 1 + lane; b < M; b += 64) {
        const uint32_t bits = row[b], dg = bw_digit(bits, pass);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if ((bits & mask) == pre[j]) {
            if (dg != last[j] && cnt[j]) {
              atomicAdd(&hist[j][last[j]], cnt[j]);
              cnt[j] = 0u;
            }
            last[j] = dg;
            ++cnt[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (cnt[j]) atomicAdd(&hist[j][last[j]], cnt[j]);
    __syncthreads();
    if (tid < 2 * BW_NGROUPS) grp[tid / BW_NGROUPS][tid % BW_NGROUPS] = bw_group_sum(hist[tid / BW_NGROUPS], tid % BW_NGROUPS);
    __syncthreads();
    if (tid == 0 || tid == 64) {  // (one wave per order statistic)
      const int j = tid >> 6;
      const BwStep s = bw_walk(hist[j], grp[j], rank[j]);
      sel[j][0] = pre[j] | (s.bin << (24 - 8 * pass));
      sel[j][1] = s.rank;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) pre[j] = sel[j][0], rank[j] = sel[j][1];
  }
  if (tid == 0) {
    const float h = bw_from_median(bw_median(bw_bits_to_float(pre[0]), bw_bits_to_float(pre[1]), P), inv_log);
    if (seg) hp[run].h_theta = h;
    else hp[run].h = h;
    bw[2 * run + seg] = h;
  }
}
// rule: bit 0 the latent segment, bit 1 theta (dibs_config.reserved_i[3]); M >= 2
void bandwidth_launch_select(hipStream_t st, const float* sqd_z, const float* sqd_t, int rule, int C, int M, ProblemHP* hp, float* bw) {
  const int nseg = (rule & 1) + ((rule >> 1) & 1), seg_a = (rule & 1) ? 0 : 1;
  if (!nseg) return;
  hipLaunchKernelGGL(k_bandwidth_median, dim3((unsigned)C, (unsigned)nseg), dim3(1024), 0, st, sqd_z, sqd_t, seg_a, 1, M, 1.0 / log((double)(M + 1)), hp, bw);
}
