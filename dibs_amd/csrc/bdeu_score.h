// BDeu marginal likelihood of discrete data: the arithmetic around the counting -- the bit-field layout of a packed
// observation row, log q of a parent set, the terms of `rise`, and the LDS plan of k_bdeu_nodes.  Plain C++17, nothing of HIP, no
// allocation, no globals: compiled by the kernel (kernels_bdeu.h), by the host packing (engine_data.hip) and by
// tests/tools/bdeu_score_check.cpp, which checks every function here against straightforward loops on a CPU.
//
//   score_j = sum over the parent configurations c that occur in the used rows:  - rise(log a, N_c) + sum_k rise(log a', N_ck)
//   log a = log eta - log q,  log a' = log a - log r_j,  log q = sum_{i in pa} log r_i
//   rise(log alpha, n) = 0 (n = 0),  log alpha + sum_{i=1}^{n-1} log(exp(log alpha) + i) (n >= 1)     (= lgamma(alpha + n) - lgamma(alpha))
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BDEU_HD __host__ __device__
#else
#define BDEU_HD
#endif

#define BDEU_MIN_ARITY 2
#define BDEU_MAX_ARITY 16
#define BDEU_MAX_KW 8       // 64-bit words of a packed row: at most 512 field bits
#define BDEU_MAX_N 4096     // observations: the largest table of one wave that fits a block's LDS (bdeu_plan)
#define BDEU_LDS_BYTES ((size_t)158 * 1024)
#define BDEU_EMPTY 0xFFFFFFFFu

// variable i of a packed row: `mask` (already shifted) inside 64-bit word `word`; the code is (row[word] & mask) >> shift
struct BdeuField {
  uint32_t word, shift;
  uint64_t mask;
};

// ceil(log2 r): bits of a code 0 .. r - 1
BDEU_HD inline int bdeu_field_bits(int r) {
  int b = 1;
  while ((1 << b) < r) ++b;
  return b;
}

// fields in variable order, a new word whenever the next field would straddle one; returns the number of words (the caller checks it
// against BDEU_MAX_KW)
inline int bdeu_layout(const int32_t* arities, int d, BdeuField* f) {
  uint32_t word = 0, used = 0;
  for (int i = 0; i < d; ++i) {
    const uint32_t b = (uint32_t)bdeu_field_bits(arities[i]);
    if (used + b > 64u) {
      ++word;
      used = 0;
    }
    f[i] = BdeuField{word, used, ((1ull << b) - 1ull) << used};
    used += b;
  }
  return (int)word + 1;
}

// the packed row of one observation; word w of row n lives at rows[w * stride + n] (word-major: the lanes of a wave read one word of 64
// consecutive rows as 512 contiguous bytes -- no LDS bank is hit twice by a half-wave)
inline void bdeu_pack_row(const int32_t* codes, int d, const BdeuField* f, uint64_t* rows, size_t stride, size_t n) {
  for (int i = 0; i < d; ++i) rows[f[i].word * stride + n] |= (uint64_t)(uint32_t)codes[i] << f[i].shift;
}

BDEU_HD inline bool bdeu_is_parent(const uint64_t* pw, int i) { return (pw[i >> 6] >> (i & 63)) & 1ull; }

// OR of the parents' field masks (host form; the kernel's lanes OR their variables into LDS words): rows n, n' have the same parent
// configuration  <=>  ((row_n[w] ^ row_n'[w]) & km[w]) == 0 for every word -- exact, no hash involved
inline void bdeu_keymask(const uint64_t* pw, int j, int d, const BdeuField* f, int KW, uint64_t* km) {
  for (int w = 0; w < KW; ++w) km[w] = 0;
  for (int i = 0; i < d; ++i)
    if (i != j && bdeu_is_parent(pw, i)) km[f[i].word] |= f[i].mask;
}

// partial sum of log r_i over the parents i = i0, i0 + stride, ... of node j (the whole sum: i0 = 0, stride = 1; lane l of a wave:
// i0 = l, stride = 64, the 64 partial sums then added by a fixed tree)
BDEU_HD inline double bdeu_log_q(const uint64_t* pw, int j, int d, const double* log_arity, int i0, int stride) {
  double s = 0.0;
  for (int i = i0; i < d; i += stride)
    if (i != j && bdeu_is_parent(pw, i)) s += log_arity[i];
  return s;
}

// term t of rise(log alpha, n) = sum_{t < n} term(t): log alpha itself for t = 0, log(alpha + t) behind it.  alpha = exp(log alpha) may
// have underflowed to 0 (hundreds of parents): the terms t >= 1 absorb that, and term 0 never needs alpha.
BDEU_HD inline double bdeu_rise_term(double log_alpha, double alpha, int t) { return t == 0 ? log_alpha : log(alpha + (double)t); }
BDEU_HD inline double bdeu_rise(double log_alpha, int n) {
  const double alpha = exp(log_alpha);
  double s = 0.0;
  for (int t = 0; t < n; ++t) s += bdeu_rise_term(log_alpha, alpha, t);
  return s;
}

// mixing step of the table hash over the masked key words (any function would do: slots hold row indices and a probe compares the full
// masked keys)
BDEU_HD inline uint64_t bdeu_mix(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
// first slot of a probe sequence in a table of T slots (a power of two, 64 .. 8192): the TOP log2 T bits of one more odd multiple of the
// mixed hash.  A product carries every bit upwards only, so its top bits depend on all 64 bits of every key word; a window lower down
// (bits 32 .. 44 of h were used once) never sees a field above it, and parents that sit late in a word all landed in a few slots.  The
// second multiplier is there because the low half of bdeu_mix's is close to 2^31: the top bits of h alone alternate between two runs for
// consecutive codes of a field at bit 32 (tests/tools/bdeu_score_check.cpp, check_hash).
BDEU_HD inline uint32_t bdeu_slot(uint64_t h, uint32_t T) { return (uint32_t)((h * 0xD6E8FEB86659FD93ull) >> (64 - __builtin_ctz(T))); }

// LDS plan of k_bdeu_nodes for N observations of KW words.  Per wave: key mask [8] u64 | rise prefix table [N] f64 | slots rep, minrow,
// cnt [T] u32 each | slot of every row [N] u32, T = the power of two >= 2 N (load factor <= 1/2).  Per block: the packed rows, when they
// fit.  The choice: the most resident waves per CU; on a tie the rows in LDS, then the larger block.
struct BdeuPlan {
  int waves, rows_lds;  // waves per block (4, 2, 1); packed rows staged in LDS
  uint32_t T;
  size_t wave_bytes, rows_bytes, lds_bytes;
};
BDEU_HD inline uint32_t bdeu_table_slots(int N) {
  uint32_t T = 64;
  while (T < 2u * (uint32_t)N) T <<= 1;
  return T;
}
BDEU_HD inline size_t bdeu_wave_bytes(int N) {
  return ((size_t)64 + (size_t)8 * N + (size_t)12 * bdeu_table_slots(N) + (size_t)4 * N + 15) & ~(size_t)15;
}
// false: no plan fits (N > BDEU_MAX_N)
inline bool bdeu_plan(int N, int KW, BdeuPlan* out) {
  if (N < 1 || N > BDEU_MAX_N || KW < 1 || KW > BDEU_MAX_KW) return false;
  const size_t wb = bdeu_wave_bytes(N), rb = ((size_t)KW * N * 8 + 15) & ~(size_t)15;
  int best = -1;
  for (int rows_lds = 1; rows_lds >= 0; --rows_lds)
    for (int waves = 4; waves >= 1; waves >>= 1) {
      const size_t lds = (rows_lds ? rb : 0) + waves * wb;
      if (lds > BDEU_LDS_BYTES) continue;
      int resident = waves * (int)(((size_t)160 * 1024) / lds);
      if (resident > 32) resident = 32;
      if (resident > best) {
        best = resident;
        *out = BdeuPlan{waves, rows_lds, bdeu_table_slots(N), wb, rows_lds ? rb : 0, lds};
      }
    }
  return best > 0;
}
