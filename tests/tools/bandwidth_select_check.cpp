// Host check of the median-rule bandwidth's arithmetic (dibs_amd/csrc/bandwidth_select.h) and of its schedule (step_plan.h, StepFacts::median_h):
// stand-alone, no GPU, nothing of HIP.
//   g++ -std=c++17 -Wall -Werror tests/tools/bandwidth_select_check.cpp -o bandwidth_select_check && ./bandwidth_select_check
// (a) the four-pass radix select, driven by a host loop that does what k_bandwidth_median does (tu_batch.hip: per pass one 256-bin histogram
//     per wanted order statistic over the values that agree with the digits chosen so far, the group sums, then bw_walk), against std::sort for 1 .. 2 000
//     values of several kinds; (b) the median and the bandwidth formula on hand-computed cases; (c) the invariants of plan_step with
//     median_h over the grid of engine facts that step_plan_check.cpp walks.  tests/test_bandwidth_host.py builds and runs it.
#include "../../dibs_amd/csrc/bandwidth_select.h"
#include "../../dibs_amd/csrc/step_plan.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <limits>
#include <random>
#include <vector>

static int g_failures = 0;
static void check(bool ok, const char* what, long a = 0, long b = 0) {
  if (ok) return;
  if (++g_failures <= 20) fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

// ---- (a) the selection ---------------------------------------------------------------------------------------------------------------
// the two order statistics of the median of v (bit patterns), as the kernel finds them
static void select_host(const std::vector<float>& v, uint32_t out_bits[2]) {
  const uint32_t P = (uint32_t)v.size();
  const BwRanks want = bw_median_ranks(P);
  uint32_t pre[2] = {0u, 0u}, rank[2] = {want.lo, want.hi};
  for (int pass = 0; pass < BW_PASSES; ++pass) {
    uint32_t hist[2][BW_BINS] = {};
    const uint32_t mask = bw_prefix_mask(pass);
    for (float x : v) {
      const uint32_t bits = bw_float_to_bits(x);
      for (int j = 0; j < 2; ++j)
        if ((bits & mask) == pre[j]) ++hist[j][bw_digit(bits, pass)];
    }
    for (int j = 0; j < 2; ++j) {
      uint32_t grp[BW_NGROUPS];
      for (uint32_t g = 0; g < BW_NGROUPS; ++g) grp[g] = bw_group_sum(hist[j], g);
      const BwStep s = bw_walk(hist[j], grp, rank[j]);
      pre[j] |= s.bin << (24 - 8 * pass);
      rank[j] = s.rank;
    }
  }
  out_bits[0] = pre[0];
  out_bits[1] = pre[1];
}
static void check_values(std::vector<float> v, const char* kind, int n) {
  const uint32_t P = (uint32_t)v.size();
  check((int)P == n, "size", P, n);
  uint32_t got[2];
  select_host(v, got);
  std::sort(v.begin(), v.end());
  const BwRanks want = bw_median_ranks(P);
  check(want.lo <= want.hi && want.hi < P && want.hi - want.lo == (P & 1u ? 0u : 1u), "median ranks", P);
  check(got[0] == bw_float_to_bits(v[want.lo]) && got[1] == bw_float_to_bits(v[want.hi]), kind, P);
  const float med = bw_median(bw_bits_to_float(got[0]), bw_bits_to_float(got[1]), P);
  const float ref = (P & 1u) ? v[(P - 1) / 2] : 0.5f * (v[P / 2 - 1] + v[P / 2]);
  check(bw_float_to_bits(med) == bw_float_to_bits(ref), "median value", P);
}
static void check_select() {
  std::mt19937 rng(20161116u);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const float inf = std::numeric_limits<float>::infinity(), dmin = std::numeric_limits<float>::denorm_min();
  for (int n = 1; n <= 2000; ++n) {
    std::vector<float> v((size_t)n);
    for (float& x : v) x = uni(rng) * 300.f;  // (squared distances of a few hundred: one or two exponents)
    check_values(v, "random", n);
    for (float& x : v) x = ldexpf(uni(rng), (int)(rng() % 200u) - 100);  // (every exponent)
    check_values(v, "random exponents", n);
    if (n % 7 && n > 64) continue;  // (the structured kinds: every small size, then every seventh)
    check_values(std::vector<float>((size_t)n, 42.5f), "all equal", n);
    check_values(std::vector<float>((size_t)n, 0.f), "zeros", n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (rng() & 1u) ? 3.f : 7.f;
    check_values(v, "two values", n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = i < n / 2 ? 3.f : 7.f;  // (the median straddles the two for an even n)
    check_values(v, "two values, halves", n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = dmin * (float)(rng() % 1000u);
    check_values(v, "denormals", n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (rng() % 3u) ? uni(rng) : inf;
    check_values(v, "inf among finite", n);
    check_values(std::vector<float>((size_t)n, inf), "all inf", n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (float)(rng() % 5u);  // (small integers: many ties, zeros)
    check_values(v, "ties", n);
  }
}

// ---- (b) the formula -----------------------------------------------------------------------------------------------------------------
static void check_formula() {
  const BwRanks r1 = bw_median_ranks(1), r3 = bw_median_ranks(3), r6 = bw_median_ranks(6), r10 = bw_median_ranks(10);
  check(r1.lo == 0 && r1.hi == 0 && r3.lo == 1 && r3.hi == 1 && r6.lo == 2 && r6.hi == 3 && r10.lo == 4 && r10.hi == 5, "ranks of P = 1, 3, 6, 10");
  check(bw_median(2.f, 4.f, 6) == 3.f && bw_median(2.f, 2.f, 3) == 2.f, "median of two / of one");
  const double inv_log = 1.0 / log(8.0);  // M = 7
  check(bw_from_median(10.f, inv_log) == (float)(10.0 * inv_log), "h = (float)(med * inv_log)");
  check(bw_from_median(0.f, inv_log) == FLT_MIN, "med = 0 -> FLT_MIN");
  check(bw_from_median(1e-44f, inv_log) == FLT_MIN, "denormal med -> FLT_MIN");
  check(isinf(bw_from_median(std::numeric_limits<float>::infinity(), inv_log)), "inf stays inf");
  uint32_t hist[BW_BINS] = {};
  hist[3] = 2, hist[200] = 5, hist[255] = 1;
  uint32_t grp[BW_NGROUPS];
  for (uint32_t g = 0; g < BW_NGROUPS; ++g) grp[g] = bw_group_sum(hist, g);
  check(grp[0] == 2 && grp[12] == 5 && grp[15] == 1, "group sums");
  const BwStep a = bw_walk(hist, grp, 0), b = bw_walk(hist, grp, 1), c = bw_walk(hist, grp, 2), d = bw_walk(hist, grp, 6), e = bw_walk(hist, grp, 7);
  check(a.bin == 3 && a.rank == 0 && b.bin == 3 && b.rank == 1 && c.bin == 200 && c.rank == 0 && d.bin == 200 && d.rank == 4 && e.bin == 255 && e.rank == 0,
        "bw_walk on a hand-made histogram");
  check(bw_prefix_mask(0) == 0u && bw_prefix_mask(1) == 0xFF000000u && bw_prefix_mask(3) == 0xFFFFFF00u, "prefix masks");
  check(bw_digit(0x12345678u, 0) == 0x12u && bw_digit(0x12345678u, 3) == 0x78u, "digits");
}

// ---- (c) the schedule ----------------------------------------------------------------------------------------------------------------
// the facts of an engine as engine_alloc derives them: the grid of tests/tools/step_plan_check.cpp (engine_facts / check_grid there)
enum Family { BGE_SCORE, BGE_REPARAM, LINGAUSS, DENSENN, N_FAMILIES };
static StepFacts engine_facts(Family fam, int d, int k, int M, int Mloc, int S, bool stream2, bool w_tot) {
  StepFacts f{};
  f.joint = fam == LINGAUSS || fam == DENSENN;
  f.likelihood = fam == LINGAUSS ? DIBS_LIK_LINGAUSS : (fam == DENSENN ? DIBS_LIK_DENSENN : DIBS_LIK_BGE);
  f.estimator = fam == BGE_SCORE ? DIBS_EST_SCORE : DIBS_EST_REPARAM;
  f.d = d, f.k = k, f.M = M, f.Mloc = Mloc, f.D = 2LL * d * k, f.S = S;
  {
    const int dpad = (d + 15) & ~15;
    f.edge_kc = k;
    for (;;) {
      const int kp = (f.edge_kc + 3) & ~3;
      f.ldk = kp + ((2 - kp) % 32 + 32) % 32;
      if ((long long)2 * dpad * f.ldk * 4 <= 160 * 1024 - 8192 || f.edge_kc <= 16) break;
      f.edge_kc = f.edge_kc > 64 ? 64 : f.edge_kc / 2;
    }
  }
  f.stream2 = stream2;
  f.fork_flag = stream2;
  f.kmat_tiled_min = 128;
  if (M >= f.kmat_tiled_min) {
    const long long P = fam == LINGAUSS ? (long long)d * d : (fam == DENSENN ? (long long)d * (5 * d + 5 + 5 + 1) : 0);
    const long long E = (2 * f.D + 2 * P + 3) & ~3LL;
    long long ns = (512LL << 20) / ((long long)Mloc * M * 8);
    ns = ns > 32 ? 32 : (ns < 1 ? 1 : ns);
    if (2LL * M * E * 4 >= (1LL << 32)) ns = 0;
    f.kmat_ns_max = (int)ns;
    f.kmat_ctr = ns > 1 && Mloc == M;
  }
  f.w_tot = w_tot;
  f.terms = TERMS_ALL;
  return f;
}
static long check_plan() {
  static const int dk[] = {20, 50, 64, 65, 100, 200}, Ms[] = {32, 127, 128, 255, 256, 1024}, terms[] = {TERMS_LIK, TERMS_PRIOR, TERMS_ALL};
  long n = 0, n_s2 = 0, n_b = 0;
  check(!StepFacts{}.median_h, "median_h is false in a value-initialised StepFacts");
  for (int fam = 0; fam < N_FAMILIES; ++fam)
    for (int d : dk)
      for (int M : Ms)
        for (int shard = 0; shard < 2; ++shard)
          for (int stream2 = 0; stream2 < 2; ++stream2)
            for (int w_tot = 0; w_tot < 2; ++w_tot)
              for (int prof = 0; prof < 3; ++prof)
                for (int bits = 0; bits < 32; ++bits)
                  for (int t : terms) {
                    StepFacts f = engine_facts((Family)fam, d, d, M, shard ? M / 4 : M, 128, stream2 != 0, w_tot != 0);
                    f.profiling = prof > 0;
                    f.profiling_concurrent = prof == 2;
                    f.flags_now = (bits & 1) != 0;
                    f.kmat_ext = (bits & 2) != 0;
                    f.xk = (bits & 4) != 0;
                    f.no_kmat_fuse = (bits & 8) != 0;
                    f.no_kmat_grad = (bits & 16) != 0;
                    f.terms = t;
                    const StepPlan fixed = plan_step(f);
                    f.median_h = true;
                    const StepPlan p = plan_step(f);
                    ++n;
                    // never a fused placement or an external slab; the second stream where the step forks, phase B otherwise (explicit
                    // keys and a rank's slab, where nothing of phase A holds a kernel matrix, stay in phase B as without the flag)
                    check(p.place == KmatPlace::Stream2 || p.place == KmatPlace::PhaseB, "median_h: Stream2 or PhaseB only", fam, M);
                    const bool forks = p.fork != ForkKind::None;
                    check((p.place == KmatPlace::Stream2) == (forks && !f.xk && f.Mloc == f.M), "median_h: Stream2 <=> fork (loop step, one rank)", fam, M);
                    check(p.ns == 0 && p.cps == 0 && p.nrider == 0, "median_h: no rider split", fam, M);
                    // fork, join and the terms are what they are without the flag
                    check(p.fork == fixed.fork && p.join == fixed.join, "median_h: fork and join unchanged", fam, M);
                    check(p.do_lik == fixed.do_lik && p.do_prior == fixed.do_prior && p.score_lik == fixed.score_lik, "median_h: terms unchanged", fam, M);
                    n_s2 += p.place == KmatPlace::Stream2;
                    n_b += p.place == KmatPlace::PhaseB;
                  }
  check(n_s2 > 0 && n_b > 0, "the grid reaches both places", n_s2, n_b);
  return n;
}

int main() {
  check_select();
  check_formula();
  const long n = check_plan();
  if (g_failures) {
    fprintf(stderr, "bandwidth_select_check: %d checks failed\n", g_failures);
    return 1;
  }
  printf("bandwidth_select_check: ok, sizes 1 .. 2000, %ld plan grid points\n", n);
  return 0;
}
