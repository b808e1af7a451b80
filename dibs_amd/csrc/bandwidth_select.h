// The arithmetic around the median-heuristic kernel bandwidth: plain C++17, nothing of HIP, no allocation, no
// globals -- the selection kernel (k_bandwidth_median, tu_batch.hip) and the host check (tests/tools/bandwidth_select_check.cpp) compile
// the same functions.
//   rule:  h = max((float)((double)med * inv_log), FLT_MIN),  inv_log = 1 / log(M + 1) formed on the host in double,
//          med = the median of the P = M (M - 1) / 2 off-diagonal squared distances v_ab (floats, >= 0)
//   selection: an exact radix select on the uint32 bit patterns of the v_ab (non-negative floats order as unsigned integers): four 8-bit
//          digits, most significant first; a pass counts, among the values that agree with the digits chosen so far, how many have each
//          value of the next digit (a 256-bin histogram), and bw_walk turns the histogram and the rank still wanted into the digit and the
//          rank inside that bin.  Integer counting only: the result does not depend on the order in which the values were counted.
#pragma once
#include <float.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BW_HD __host__ __device__
#else
#define BW_HD
#endif

#define BW_BINS 256
#define BW_PASSES 4

// the one or two order statistics of P >= 1 values that form the median: P odd: lo = hi = (P - 1) / 2; P even: P / 2 - 1 and P / 2
struct BwRanks {
  uint32_t lo, hi;
};
BW_HD inline BwRanks bw_median_ranks(uint32_t P) { return BwRanks{(P - 1u) / 2u, P / 2u}; }

// digit `pass` (0 = most significant) of a bit pattern, and the mask of the digits in front of it
BW_HD inline uint32_t bw_digit(uint32_t bits, int pass) { return (bits >> (24 - 8 * pass)) & 0xFFu; }
BW_HD inline uint32_t bw_prefix_mask(int pass) { return pass == 0 ? 0u : 0xFFFFFFFFu << (32 - 8 * pass); }

// The walk: the bin that holds the value of rank `rank` (0-based, among the values counted in hist) and the rank inside that bin.  Two
// levels of BW_GROUP bins, so that the serial part is 2 x 16 steps instead of 256 (on the device one thread walks; the group sums are
// formed by 16 threads, one group each): grp[g] = bw_group_sum(hist, g), then bw_walk over the groups and inside the group found.
// Every bin of a level is visited whatever the counts are: no data-dependent loop bound.  rank >= the sum of the counts (never asked
// for): bin 255, rank unchanged
#define BW_GROUP 16
#define BW_NGROUPS (BW_BINS / BW_GROUP)
struct BwStep {
  uint32_t bin, rank;
};
BW_HD inline uint32_t bw_group_sum(const uint32_t* hist, uint32_t g) {
  uint32_t s = 0;
  for (uint32_t b = 0; b < BW_GROUP; ++b) s += hist[g * BW_GROUP + b];
  return s;
}
BW_HD inline BwStep bw_walk_level(const uint32_t* counts, uint32_t n, uint32_t rank) {
  BwStep s{n - 1u, rank};
  uint32_t cum = 0;
  bool found = false;
  for (uint32_t b = 0; b < n; ++b) {
    const uint32_t c = counts[b];
    const bool here = !found && rank - cum < c;  // (cum <= rank while !found)
    s.bin = here ? b : s.bin;
    s.rank = here ? rank - cum : s.rank;
    found = found || here;
    cum += found ? 0u : c;
  }
  return s;
}
BW_HD inline BwStep bw_walk(const uint32_t* hist, const uint32_t* grp, uint32_t rank) {
  const BwStep g = bw_walk_level(grp, BW_NGROUPS, rank);
  const BwStep b = bw_walk_level(hist + g.bin * BW_GROUP, BW_GROUP, g.rank);
  return BwStep{g.bin * BW_GROUP + b.bin, b.rank};
}

BW_HD inline float bw_bits_to_float(uint32_t bits) {
  float v;
  memcpy(&v, &bits, 4);
  return v;
}
BW_HD inline uint32_t bw_float_to_bits(float v) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  return bits;
}

// the median from the order statistics at bw_median_ranks(P) -- equal for an odd P -- computed in float
BW_HD inline float bw_median(float v_lo, float v_hi, uint32_t P) { return (P & 1u) ? v_lo : 0.5f * (v_lo + v_hi); }
// the bandwidth; the floor keeps a run with more than half of its pairs identical (med = 0) finite
BW_HD inline float bw_from_median(float med, double inv_log) {
  const float h = (float)((double)med * inv_log);
  return h > FLT_MIN ? h : FLT_MIN;  // (NaN: FLT_MIN)
}
