// CPU check of dibs_amd/csrc/bdeu_score.h (the arithmetic k_bdeu_nodes and the host packing share) against straightforward loops:
//   rise and its terms against lgamma and against the sequential definition; log q against a plain sum; the field layout (no field
//   straddles a word, fields disjoint, codes round-trip) and the key-mask compare against a tuple compare of the parents' codes, for
//   arities 2, 3, 5, 16 and a layout of more than one word; the LDS plan's invariants for every N up to the limit; the table hash
//   (bdeu_mix, bdeu_slot) by the probes a sequential open-addressing table needs for distinct keys wherever their field sits in a word.
// Built and run by tests/test_bdeu_host.py:  g++ -std=c++17 -Wall -Werror bdeu_score_check.cpp
//   bdeu_score_check            every check; prints "bdeu_score_check: ok"
//   bdeu_score_check --plan N KW    prints `waves rows_lds T lds_bytes` of bdeu_plan(N, KW) and checks nothing (exit 2: no plan)
#include "../../dibs_amd/csrc/bdeu_score.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);      \
      fprintf(stderr, "\n");             \
      ++g_fail;                          \
    }                                    \
  } while (0)

static uint64_t rnd_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
  rnd_state ^= rnd_state << 13;
  rnd_state ^= rnd_state >> 7;
  rnd_state ^= rnd_state << 17;
  return (uint32_t)(rnd_state >> 32);
}

static void check_rise() {
  CHECK(bdeu_rise(-3.0, 0) == 0.0, "rise(., 0) must be 0");
  CHECK(bdeu_rise(-3.0, 1) == -3.0, "rise(log a, 1) must be log a");
  const double las[] = {log(1.0), log(10.0), log(1.0 / 3.0), log(1.0 / 1024.0), log(0.5 / 7.0)};
  for (double la : las)
    for (int n = 0; n <= 300; n += (n < 20 ? 1 : 37)) {
      const double a = exp(la), want = lgamma(a + n) - lgamma(a), got = bdeu_rise(la, n);
      CHECK(fabs(got - want) <= 1e-12 * (1.0 + fabs(want)), "rise(%g, %d) = %.17g, lgamma form %.17g", la, n, got, want);
      double s = 0.0;  // the definition, written out
      if (n >= 1) {
        s = la;
        for (int i = 1; i < n; ++i) s += log(exp(la) + i);
      }
      CHECK(got == s, "rise(%g, %d) differs from the written-out definition", la, n);
    }
  // alpha underflows to 0 (log a = -300 log 16, below the smallest denormal): finite, and equal to log a + lgamma(n)
  const double la = -300.0 * log(16.0);
  CHECK(exp(la) == 0.0, "expected underflow");
  const double got = bdeu_rise(la, 40);
  CHECK(isfinite(got) && fabs(got - (la + lgamma(40.0))) <= 1e-12 * fabs(got), "underflowed alpha: %.17g", got);
}

static void check_layout(const std::vector<int32_t>& ar, int expect_min_words) {
  const int d = (int)ar.size();
  std::vector<BdeuField> f(d);
  const int KW = bdeu_layout(ar.data(), d, f.data());
  CHECK(KW >= expect_min_words, "KW = %d, expected at least %d", KW, expect_min_words);
  std::vector<uint64_t> seen(KW, 0ull);
  for (int i = 0; i < d; ++i) {
    const int b = bdeu_field_bits(ar[i]);
    CHECK((1 << b) >= ar[i] && (b == 1 || (1 << (b - 1)) < ar[i]), "field bits of arity %d: %d", ar[i], b);
    CHECK((int)f[i].word < KW && f[i].shift + (uint32_t)b <= 64u, "field %d straddles a word", i);
    CHECK(f[i].mask == (((1ull << b) - 1ull) << f[i].shift), "field %d mask", i);
    CHECK((seen[f[i].word] & f[i].mask) == 0ull, "field %d overlaps another", i);
    seen[f[i].word] |= f[i].mask;
  }
  // random rows: pack, read the codes back, and compare pairs of rows under random parent sets both ways
  const int N = 48, W = (d + 63) / 64;
  std::vector<int32_t> codes((size_t)N * d);
  std::vector<uint64_t> rows((size_t)KW * N, 0ull);
  for (int n = 0; n < N; ++n) {
    for (int i = 0; i < d; ++i) codes[(size_t)n * d + i] = (n % 3 == 0 && n > 0) ? codes[(size_t)(n - 1) * d + i] * (i % 2) : (int32_t)(rnd() % (uint32_t)ar[i]);
    bdeu_pack_row(&codes[(size_t)n * d], d, f.data(), rows.data(), (size_t)N, (size_t)n);
  }
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < d; ++i)
      CHECK((int32_t)((rows[(size_t)f[i].word * N + n] & f[i].mask) >> f[i].shift) == codes[(size_t)n * d + i], "round trip of row %d, variable %d", n, i);
  std::vector<double> logr(d);
  for (int i = 0; i < d; ++i) logr[i] = log((double)ar[i]);
  for (int trial = 0; trial < 40; ++trial) {
    const int j = (int)(rnd() % (uint32_t)d);
    std::vector<uint64_t> pw(W, 0ull), km(KW);
    const uint32_t dens = trial % 4;  // 0: empty, 3: all others
    for (int i = 0; i < d; ++i)
      if (i != j && (dens == 3 || (dens && rnd() % 4u < dens))) pw[i >> 6] |= 1ull << (i & 63);
    if (trial % 5 == 0) pw[j >> 6] |= 1ull << (j & 63);  // (a set diagonal bit is ignored)
    bdeu_keymask(pw.data(), j, d, f.data(), KW, km.data());
    double lq = 0.0, lq_lanes = 0.0;
    for (int i = 0; i < d; ++i)
      if (i != j && ((pw[i >> 6] >> (i & 63)) & 1ull)) lq += logr[i];
    CHECK(bdeu_log_q(pw.data(), j, d, logr.data(), 0, 1) == lq, "log q");
    for (int l = 0; l < 64; ++l) lq_lanes += bdeu_log_q(pw.data(), j, d, logr.data(), l, 64);
    CHECK(fabs(lq_lanes - lq) <= 1e-12 * (1.0 + lq), "log q, lane-strided");
    for (int a = 0; a < N; ++a)
      for (int b = a; b < N; ++b) {
        bool tuple_eq = true, key_eq = true;
        for (int i = 0; i < d; ++i)
          if (i != j && ((pw[i >> 6] >> (i & 63)) & 1ull)) tuple_eq = tuple_eq && codes[(size_t)a * d + i] == codes[(size_t)b * d + i];
        for (int w = 0; w < KW; ++w) key_eq = key_eq && ((rows[(size_t)w * N + a] ^ rows[(size_t)w * N + b]) & km[w]) == 0ull;
        CHECK(tuple_eq == key_eq, "masked compare of rows %d, %d under trial %d", a, b, trial);
      }
  }
}

static void check_plan() {
  BdeuPlan pl;
  CHECK(!bdeu_plan(BDEU_MAX_N + 1, 1, &pl) && !bdeu_plan(0, 1, &pl) && !bdeu_plan(10, BDEU_MAX_KW + 1, &pl), "plans beyond the limits");
  CHECK(BDEU_MAX_N >= 1024, "the limit must admit 1024 observations");
  for (int KW = 1; KW <= BDEU_MAX_KW; ++KW)
    for (int N = 1; N <= BDEU_MAX_N; N += (N < 200 ? 1 : 61)) {
      CHECK(bdeu_plan(N, KW, &pl), "no plan for N = %d, KW = %d", N, KW);
      CHECK(pl.T >= 2u * (uint32_t)N && (pl.T & (pl.T - 1u)) == 0u, "table size");
      CHECK(pl.wave_bytes % 16 == 0 && pl.rows_bytes % 16 == 0, "alignment");
      CHECK(pl.wave_bytes >= 64u + 12u * (size_t)N + 12u * pl.T, "per-wave area");
      CHECK(!pl.rows_lds || pl.rows_bytes >= (size_t)KW * N * 8, "row area");
      CHECK(pl.lds_bytes == pl.rows_bytes + pl.waves * pl.wave_bytes && pl.lds_bytes <= BDEU_LDS_BYTES, "total");
      CHECK(pl.waves == 1 || pl.waves == 2 || pl.waves == 4, "waves");
    }
  CHECK(bdeu_plan(BDEU_MAX_N, BDEU_MAX_KW, &pl), "the largest size");
}

// N distinct keys of a 12-bit field at `shift`, inserted one after the other into an open-addressing table of T = bdeu_table_slots(N)
// slots with the header's own mix and slot and the kernel's step (slot + 1) & (T - 1); `lead` != 0: a first key word, the same in every
// row, mixed before.  Returns the slots visited in total.  Uniform hashing at load <= 1/2 visits at most 2.5 per insertion in expectation;
// a slot function that does not see the field's bits visits about N / 2.
static uint64_t hash_probes(int N, int shift, uint64_t lead, bool scattered) {
  const uint32_t T = bdeu_table_slots(N);
  std::vector<uint64_t> key(T, ~0ull);  // (no 12-bit field fills a word: ~0 is no key)
  uint64_t probes = 0;
  // distinct field values: 0 .. N - 1 themselves, or scattered -- an odd multiplier permutes 0 .. 4095
  for (int n = 0; n < N; ++n) {
    const uint64_t v = (uint64_t)(scattered ? ((uint32_t)n * 2741u + 977u) & 4095u : (uint32_t)n) << shift;
    uint64_t h = 0;
    if (lead) h = bdeu_mix(h, lead);
    h = bdeu_mix(h, v);
    uint32_t slot = bdeu_slot(h, T);
    CHECK(slot < T, "slot %u outside a table of %u", slot, T);
    for (;;) {
      ++probes;
      if (key[slot] == ~0ull) {
        key[slot] = v;
        break;
      }
      CHECK(key[slot] != v, "keys must be distinct");
      slot = (slot + 1u) & (T - 1u);
    }
  }
  return probes;
}

static void check_hash() {
  const int Ns[] = {64, 1024, 4096};
  const uint64_t leads[] = {0ull, 0x0000A5C3000F1E2Dull};
  uint64_t worst_num = 0, worst_den = 1;
  for (int N : Ns)
    for (int shift = 0; shift <= 52; shift += 4)
      for (uint64_t lead : leads)
        for (int scattered = 0; scattered < 2; ++scattered) {
          const uint64_t probes = hash_probes(N, shift, lead, scattered != 0);
          CHECK(probes <= 4ull * (uint64_t)N, "hash: N = %d, %s 12-bit keys at shift %d%s: %llu probes for %d insertions (more than 4 N)", N,
                scattered ? "scattered" : "consecutive", shift, lead ? " behind another word" : "", (unsigned long long)probes, N);
          if (probes * worst_den > worst_num * (uint64_t)N) worst_num = probes, worst_den = (uint64_t)N;
        }
  printf("check_hash: at most %.2f probes per insertion\n", (double)worst_num / (double)worst_den);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--plan")) {
    BdeuPlan pl;
    if (!bdeu_plan(atoi(argv[2]), atoi(argv[3]), &pl)) return 2;
    printf("%d %d %u %zu\n", pl.waves, pl.rows_lds, pl.T, pl.lds_bytes);
    return 0;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: bdeu_score_check [--plan N KW]\n");
    return 2;
  }
  check_rise();
  check_layout({2, 3, 5, 16}, 1);
  check_layout({2, 3, 4, 2, 5, 7, 8, 16, 3}, 1);
  check_layout(std::vector<int32_t>(130, 2), 3);   // 130 bits: three words
  check_layout(std::vector<int32_t>(40, 16), 3);   // 160 bits
  {
    std::vector<int32_t> ar;  // 3-bit fields: 21 per word, the 22nd would straddle
    for (int i = 0; i < 50; ++i) ar.push_back(5 + (i % 4));
    check_layout(ar, 3);
  }
  check_plan();
  check_hash();
  if (g_fail) {
    fprintf(stderr, "bdeu_score_check: %d failures\n", g_fail);
    return 1;
  }
  printf("bdeu_score_check: ok\n");
  return 0;
}
