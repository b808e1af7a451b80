// BDeu marginal likelihood of sampled graphs on discrete data (gfx950): the second producer of NODE_SCORES beside k_bge_chol.
//   definition: include/dibs_hip.h (BDEU), dibs_amd/models/discrete.py::bdeu_log_marginal_numpy; arithmetic: bdeu_score.h
//
// k_bdeu_nodes   one wave per problem (particle m, node j, sample s), grid-strided over the Mloc d S problems in the entry order of
//                node_scores, p = (m d + j) S + s; every entry is written.
// Per problem:
//   1. key mask = OR of the parents' field masks (LDS atomic OR, the lanes take the variables), log q = sum of the parents' log r_i
//      (lane-strided partial sums, wave_sum_d's fixed tree)
//   2. two passes of one grouping routine over the used rows of node j -- parent configurations c under `log a`, then (c, child value)
//      under `log a'` with the child's own field added to the key mask:
//        a. the table of rise: prefix sums of its terms, E[n - 1] = rise(log alpha, n), n <= the node's used rows -- each lane a contiguous
//           chunk, the chunk totals scanned by shuffles: N / 64 double logs per lane instead of one lane's N
//        b. an open-addressing table in LDS whose slots hold a ROW INDEX (claimed by compare-and-swap): a probe compares the full masked
//           keys of its row and the slot's, so a group is exactly a set of rows with equal masked keys, whatever the hash does; which
//           row claimed a slot depends on the arrival order, the groups do not
//        c. integer atomics per slot: the count and the smallest row index of the group
//        d. the group's term rise(log alpha, count) is attributed to its first row; lane l adds the terms of rows l, l + 64, ... in row
//           order, wave_sum_d adds the lanes
//   3. score = (pass 2) - (pass 1) in double.
// The value does not depend on the order in which lanes arrive: only integers go through atomics.
#pragma once
#include "common.h"
#include "bdeu_score.h"

struct BdeuArgs {
  const uint64_t* rows;      // [KW][N] packed observations, word-major (bdeu_pack_row)
  const uint64_t* used;      // [d][NW] bit n of node j: row n is used (interv_mask[n, j] == 0)
  const int32_t* nused;      // [d] used rows of node j
  const BdeuField* fields;   // [d]
  const double* log_arity;   // [d] log r_i
  const uint64_t* masks;     // [nprob][W] parent sets (bit i of word i / 64 = g[i, j])
  double* node_scores;       // [nprob]
  double log_ess;
  long long nprob;
  int N, KW, NW, d, S, W;
  uint32_t T;
  int waves;
  uint32_t wave_bytes, rows_bytes;
};

// one grouping pass (2a .. 2d above); returns sum over the groups of rise(log_alpha, count), the same value in every lane
template <bool ROWS_LDS>
__device__ __forceinline__ double bdeu_pass(const uint64_t* __restrict__ rows, const uint64_t* __restrict__ used_j, int N, int KW, int NW, int nu,
                                            double log_alpha, const uint64_t* km, double* E, uint32_t* rep, uint32_t* minrow, uint32_t* cnt,
                                            uint32_t* rowslot, uint32_t T, int lane) {
  wave_lds_fence();  // (the previous pass has read its table)
  const double alpha = exp(log_alpha);
  {
    const int ch = (nu + 63) >> 6, t0 = lane * ch, t1 = t0 + ch < nu ? t0 + ch : nu;
    double run = 0.0;
    for (int t = t0; t < t1; ++t) {
      run += bdeu_rise_term(log_alpha, alpha, t);
      E[t] = run;
    }
    double tot = run;  // inclusive scan of the chunk totals, lane order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double v = __shfl_up(tot, o, 64);
      if (lane >= o) tot += v;
    }
    double before = __shfl_up(tot, 1, 64);
    if (lane == 0) before = 0.0;
    for (int t = t0; t < t1; ++t) E[t] += before;
  }
  for (uint32_t t = lane; t < T; t += 64) {
    rep[t] = BDEU_EMPTY;
    minrow[t] = BDEU_EMPTY;
    cnt[t] = 0u;
  }
  wave_lds_fence();
  for (int it = 0; it < NW; ++it) {
    const int n = it * 64 + lane;
    const bool on = n < N && ((used_j[it] >> lane) & 1ull);
    if (on) {
      uint64_t h = 0;
      for (int w = 0; w < KW; ++w) {
        const uint64_t kw = km[w];
        if (kw) h = bdeu_mix(h, rows[(size_t)w * N + n] & kw);
      }
      uint32_t slot = bdeu_slot(h, T);
      bool found = false;
      for (uint32_t probe = 0; probe < T; ++probe) {  // (load factor <= 1/2: an empty slot ends every probe sequence)
        uint32_t r = atomicCAS(&rep[slot], BDEU_EMPTY, (uint32_t)n);
        if (r == BDEU_EMPTY) r = (uint32_t)n;  // claimed
        bool eq = true;
        if (r != (uint32_t)n)
          for (int w = 0; w < KW; ++w) {
            const uint64_t kw = km[w];
            if (kw) eq = eq && ((rows[(size_t)w * N + n] ^ rows[(size_t)w * N + r]) & kw) == 0ull;
          }
        if (eq) {
          found = true;
          break;
        }
        slot = (slot + 1u) & (T - 1u);
      }
      if (found) {
        atomicAdd(&cnt[slot], 1u);
        atomicMin(&minrow[slot], (uint32_t)n);
      }
      rowslot[n] = found ? slot : BDEU_EMPTY;
    }
  }
  wave_lds_fence();
  double part = 0.0;
  for (int it = 0; it < NW; ++it) {
    const int n = it * 64 + lane;
    const bool on = n < N && ((used_j[it] >> lane) & 1ull);
    if (on) {
      const uint32_t slot = rowslot[n];
      if (slot != BDEU_EMPTY && minrow[slot] == (uint32_t)n) {
        const uint32_t c = cnt[slot];
        if (c >= 1u && c <= (uint32_t)nu) part += E[c - 1u];
      }
    }
  }
  return wave_sum_d(part);
}

// grid: min(ceil(nprob / waves), resident blocks); block: 64 * a.waves threads; dynamic LDS: a.rows_bytes (ROWS_LDS) + waves * wave_bytes
template <bool ROWS_LDS>
__global__ __launch_bounds__(256) void k_bdeu_nodes(BdeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, KW = a.KW;
  const uint64_t* rows = a.rows;
  if (ROWS_LDS) {
    uint64_t* sr = reinterpret_cast<uint64_t*>(smem_raw);
    for (int e = tid; e < KW * N; e += (int)blockDim.x) sr[e] = a.rows[e];
    __syncthreads();
    rows = sr;
  }
  unsigned char* wb = smem_raw + (ROWS_LDS ? a.rows_bytes : 0u) + (size_t)wave * a.wave_bytes;
  uint64_t* km = reinterpret_cast<uint64_t*>(wb);  // [8]
  double* E = reinterpret_cast<double*>(wb + 64);  // [N]
  uint32_t* rep = reinterpret_cast<uint32_t*>(E + N);
  uint32_t* minrow = rep + a.T;
  uint32_t* cnt = minrow + a.T;
  uint32_t* rowslot = cnt + a.T;  // [N]
  const long long stride = (long long)gridDim.x * a.waves;
  for (long long p = (long long)blockIdx.x * a.waves + wave; p < a.nprob; p += stride) {
    const int j = (int)((p / a.S) % a.d);
    const uint64_t* pw = a.masks + (size_t)p * a.W;
    if (lane < BDEU_MAX_KW) km[lane] = 0ull;
    wave_lds_fence();
    for (int i = lane; i < a.d; i += 64)
      if (i != j && bdeu_is_parent(pw, i)) atomicOr(reinterpret_cast<unsigned long long*>(&km[a.fields[i].word]), (unsigned long long)a.fields[i].mask);
    const double lq = wave_sum_d(bdeu_log_q(pw, j, a.d, a.log_arity, lane, 64));
    wave_lds_fence();
    const int nu = a.nused[j];
    double score = 0.0;
    if (nu > 0) {  // (wave-uniform)
      const uint64_t* used_j = a.used + (size_t)j * a.NW;
      const double la = a.log_ess - lq;
      const double s_c = bdeu_pass<ROWS_LDS>(rows, used_j, N, KW, a.NW, nu, la, km, E, rep, minrow, cnt, rowslot, a.T, lane);
      wave_lds_fence();
      if (lane == 0) km[a.fields[j].word] |= a.fields[j].mask;  // (configuration, child value): the child's field joins the key
      wave_lds_fence();
      const double s_ck = bdeu_pass<ROWS_LDS>(rows, used_j, N, KW, a.NW, nu, la - a.log_arity[j], km, E, rep, minrow, cnt, rowslot, a.T, lane);
      score = s_ck - s_c;
    }
    if (lane == 0) a.node_scores[p] = score;
    wave_lds_fence();
  }
}
