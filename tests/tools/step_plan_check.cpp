// Host check of the SVGD step's schedule (dibs_amd/csrc/step_plan.h): stand-alone, no GPU, nothing of HIP.
//   g++ -std=c++17 -Wall -Werror tests/tools/step_plan_check.cpp -o step_plan_check && ./step_plan_check
// (a) the invariants of StepPlan over a grid of engine facts, (b) equality with the expressions step_local / launch_tail / step_update
// used before the plan existed (commit 6b2416b), (c) the pinned rows of the five bench.py configurations.  tests/test_step_plan_host.py
// builds and runs it.
#include "../../dibs_amd/csrc/step_plan.h"

#include <stdio.h>

static int g_failures = 0;
static long g_place[5], g_fork[5], g_join[4];  // grid points per choice (printed: the grid reaches every one)
static void check(bool ok, const char* what, const StepFacts& f) {
  if (ok) return;
  if (++g_failures <= 20)
    fprintf(stderr,
            "FAILED: %s\n  joint %d lik %d est %d d %d k %d M %d Mloc %d stream2 %d profiling %d/%d flags_now %d kmat_ns_max %d kmat_ctr %d w_tot %d "
            "kmat_ext %d xk %d terms %d no_fuse %d no_grad %d\n",
            what, f.joint, f.likelihood, f.estimator, f.d, f.k, f.M, f.Mloc, f.stream2, f.profiling, f.profiling_concurrent, f.flags_now,
            f.kmat_ns_max, f.kmat_ctr, f.w_tot, f.kmat_ext, f.xk, f.terms, f.no_kmat_fuse, f.no_kmat_grad);
}

// ---- the facts of an engine, as engine_alloc derives them (engine.hip) -----------------------------------------------------------------
enum Family { BGE_SCORE, BGE_REPARAM, LINGAUSS, DENSENN, N_FAMILIES };
static StepFacts engine_facts(Family fam, int d, int k, int M, int Mloc, int S, bool stream2, bool w_tot) {
  StepFacts f{};
  f.joint = fam == LINGAUSS || fam == DENSENN;
  f.likelihood = fam == LINGAUSS ? DIBS_LIK_LINGAUSS : (fam == DENSENN ? DIBS_LIK_DENSENN : DIBS_LIK_BGE);
  f.estimator = fam == BGE_SCORE ? DIBS_EST_SCORE : DIBS_EST_REPARAM;
  f.d = d;
  f.k = k;
  f.M = M;
  f.Mloc = Mloc;
  f.D = 2LL * d * k;
  f.S = S;
  {  // the chunking of k_edge_scores: one chunk when U and V fit in LDS
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
  f.fork_flag = stream2;  // (allocated with the second stream)
  f.kmat_tiled_min = 128;
  f.kmat_ns_max = 0;
  f.kmat_ctr = false;
  if (M >= f.kmat_tiled_min) {  // the tiled kernel matrix: room for up to 32 pieces per pair in 512 MiB; 32-bit row offsets
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

// ---- FROZEN: the schedule of the parent commit (6b2416b) -------------------------------------------------------------------------------
// A verbatim transcription of the boolean expressions of step_local, launch_tail, the BGe score branch and step_update at that commit,
// with the engine's fields replaced by the facts (e->x -> f.x, c.joint -> f.joint, pointers -> "is allocated").  This is the PARENT, not
// the code under test: it is never edited together with step_plan.h.  If the schedule is to change on purpose, this block and check (b)
// go; they are not to be adapted.
struct ParentSchedule {
  bool fork, join_now, flag_join, kmat_early, flag_fork, fork_pub_in_sample, ext_fork;
  bool fused_in_sample, fused_in_tail, update_launches;
  int ns, cps, nrider;
};
static bool parent_kmat_tiled_on(const StepFacts& f) { return f.kmat_ns_max > 0 && f.M >= f.kmat_tiled_min; }
static bool parent_edge_one_block(const StepFacts& f) { return f.d <= 64 && f.k <= 64 && f.edge_kc >= f.k && f.ldk <= 128; }
static ParentSchedule parent_schedule(const StepFacts& f) {
  ParentSchedule r{};
  const bool xk = f.xk;
  // step_local
  const bool do_lik = (f.terms & 1) != 0, do_prior = (f.terms & 2) != 0;
  bool kmat_early = false;
  bool kmat_fused = false;
  const bool fork = do_prior && do_lik && f.stream2, join_now = f.profiling && !f.profiling_concurrent;
  const bool flag_join = fork && !join_now && f.flags_now && f.Mloc <= 128;
  const bool kmat_on_s2 = f.joint || (long)f.M * f.D > 4L * f.S * f.d * f.d;
  const bool kmat_early_now = fork && !xk && kmat_on_s2 && f.Mloc == f.M && !f.kmat_ext;
  const bool tile_in_grad = !f.joint && !xk && !kmat_early_now && !f.kmat_ext && f.Mloc == f.M && f.kmat_ns_max > 1 && f.kmat_ctr &&
                            f.M >= f.kmat_tiled_min && f.Mloc < 256 && !f.w_tot && !f.no_kmat_fuse && !f.no_kmat_grad;
  const bool edge_p = parent_edge_one_block(f);
  const bool flag_fork = flag_join && !f.joint && !f.profiling && f.fork_flag && edge_p;
  const bool fork_pub_in_sample = flag_fork && do_lik && f.likelihood == DIBS_LIK_BGE && f.estimator == DIBS_EST_SCORE;
  const bool ext_fork = fork && !f.profiling;
  if (kmat_early_now) kmat_early = true;
  // the estimator branches: `else if (c.likelihood == DIBS_LIK_BGE)` behind the reparam branch
  if (!do_lik) {
  } else if (f.likelihood == DIBS_LIK_BGE && f.estimator == DIBS_EST_REPARAM) {
  } else if (f.likelihood == DIBS_LIK_BGE) {
    kmat_fused = false;
    if (!tile_in_grad && !parent_kmat_tiled_on(f) && !xk && !kmat_early && !f.kmat_ext && f.Mloc == f.M && f.D <= 32768 &&
        (size_t)f.D * 4 + 64 <= 80 * 1024 && !f.no_kmat_fuse) {
      kmat_fused = true;
      r.fused_in_sample = true;
    }
  }
  // launch_tail
  if (tile_in_grad) {
    const int nta = (f.M + 32 - 1) / 32, tiles = nta * (nta + 1) / 2, nchunk = ((int)f.D + 256 - 1) / 256;
    int ns = (256 - f.Mloc + tiles - 1) / tiles;
    ns = ns > nchunk ? nchunk : ns;
    ns = ns > f.kmat_ns_max ? f.kmat_ns_max : ns;
    const int cps = (nchunk + ns - 1) / ns;
    ns = (nchunk + cps - 1) / cps;
    if (ns > 1) {
      r.ns = ns;
      r.cps = cps;
      r.nrider = tiles * ns < 256 - f.Mloc ? tiles * ns : 256 - f.Mloc;
      kmat_fused = true;
      r.fused_in_tail = true;
    }
  }
  // step_update
  r.update_launches = !f.kmat_ext && !kmat_early && (!kmat_fused || f.joint);
  r.fork = fork;
  r.join_now = join_now;
  r.flag_join = flag_join;
  r.kmat_early = kmat_early;
  r.flag_fork = flag_fork;
  r.fork_pub_in_sample = fork_pub_in_sample;
  r.ext_fork = ext_fork;
  return r;
}
// ---- end of the frozen block -----------------------------------------------------------------------------------------------------------

// what the parent's launches amount to, in the plan's words
static KmatPlace parent_place(const ParentSchedule& r, const StepFacts& f) {
  if (r.kmat_early) return KmatPlace::Stream2;
  if (r.fused_in_tail) return KmatPlace::InTail;
  if (r.fused_in_sample) return KmatPlace::InSample;
  return f.kmat_ext ? KmatPlace::External : KmatPlace::PhaseB;
}
static ForkKind parent_fork(const ParentSchedule& r) {
  if (!r.fork) return ForkKind::None;
  if (r.fork_pub_in_sample) return ForkKind::FlagFromSample;
  if (r.flag_fork) return ForkKind::FlagFromEdge;
  return r.ext_fork ? ForkKind::StopEvent : ForkKind::Event;
}
static JoinKind parent_join(const ParentSchedule& r) {
  if (!r.fork) return JoinKind::None;
  if (r.flag_join) return JoinKind::Flag;
  return r.join_now ? JoinKind::EventAtOnce : JoinKind::Event;
}

static void check_point(const StepFacts& f) {
  const StepPlan p = plan_step(f);
  ++g_place[(int)p.place], ++g_fork[(int)p.fork], ++g_join[(int)p.join];
  const bool marginal = !f.joint, single = f.Mloc == f.M, timing_alone = f.profiling && !f.profiling_concurrent;
  const bool bge_score = f.likelihood == DIBS_LIK_BGE && f.estimator == DIBS_EST_SCORE;
  const bool one_block = edge_one_block(f.d, f.k, f.edge_kc, f.ldk);
  const bool flag_fork = p.fork == ForkKind::FlagFromEdge || p.fork == ForkKind::FlagFromSample;
  // (a) invariants
  check(p.do_lik == ((f.terms & TERMS_LIK) != 0) && p.do_prior == ((f.terms & TERMS_PRIOR) != 0), "do_lik / do_prior follow terms", f);
  check(p.score_lik == (bge_score && p.do_lik), "score_lik <=> BGe score estimator with do_lik", f);
  // (exactly one KmatPlace: the plan holds one enum value; that the PARENT's flags amount to exactly one place is checked under (b))
  check(!f.kmat_ext || p.place == KmatPlace::External, "kmat_ext => External", f);
  check(f.kmat_ext || p.place != KmatPlace::External, "External => kmat_ext", f);
  // explicit keys (dibs_engine_eval_gradients): nothing of phase A holds a kernel matrix, and -- the likelihood and the prior part being
  // evaluated in a call each -- there is no second stream to flag.  (With both parts in one call, which no caller asks for, the step
  // would fork like the loop's: the parent's expressions say so, and (b) holds the plan to them.)
  check(!f.xk || f.kmat_ext || p.place == KmatPlace::PhaseB, "xk => PhaseB (or an External slab that is there)", f);
  check(!f.xk || (!flag_fork && p.join != JoinKind::Flag) || f.terms == TERMS_ALL, "xk with one part of the terms => no flag of either kind", f);
  check(single || p.place == KmatPlace::External || p.place == KmatPlace::PhaseB, "Mloc != M => External or PhaseB", f);
  if (p.place == KmatPlace::InTail) {
    check(marginal && single && f.M < 256 && f.M >= f.kmat_tiled_min && !f.w_tot && p.ns > 1, "InTail => marginal, Mloc = M < 256, tiled, no w_tot, ns > 1", f);
    check(p.cps >= 1 && p.ns * p.cps >= (int)((f.D + KT_CH - 1) / KT_CH) && p.ns <= f.kmat_ns_max, "InTail: the pieces cover the chunk range and fit kpart", f);
    check(p.nrider >= 1 && f.Mloc + p.nrider <= 256, "InTail: riders fill at most the 256 CUs", f);
    check(!f.no_kmat_fuse && !f.no_kmat_grad && f.kmat_ctr, "InTail => not switched off, counters allocated", f);
  } else {
    check(p.ns == 0 && p.cps == 0 && p.nrider == 0, "no rider split outside InTail", f);
  }
  if (p.place == KmatPlace::InSample) {
    check(bge_score && p.do_lik && marginal && single, "InSample => BGe score with do_lik, single rank", f);
    check(f.M < f.kmat_tiled_min || f.kmat_ns_max <= 0, "InSample => the direct kernel matrix", f);
    check(f.D <= KMAT_CH && !f.no_kmat_fuse, "InSample => D <= KMAT_CH, not switched off", f);
  }
  check(p.place != KmatPlace::Stream2 || p.fork != ForkKind::None, "Stream2 => fork", f);
  check((p.fork == ForkKind::None) == (p.join == JoinKind::None), "fork and join together", f);
  if (p.join == JoinKind::Flag) check(p.fork != ForkKind::None && f.Mloc <= 128 && f.flags_now && !timing_alone, "Flag join => fork, Mloc <= 128, flags_now, no per-kernel timing", f);
  check((p.join == JoinKind::EventAtOnce) == (p.fork != ForkKind::None && timing_alone), "EventAtOnce <=> fork with per-kernel timing", f);
  if (flag_fork) check(p.join == JoinKind::Flag && marginal && !f.profiling && one_block && f.fork_flag, "flag fork => flag join, marginal, not profiling, edge_one_block", f);
  check((p.fork == ForkKind::FlagFromSample) == (flag_fork && bge_score), "FlagFromSample <=> flag fork and BGe score", f);
  check(p.fork != ForkKind::StopEvent || !f.profiling, "StopEvent => not profiling", f);
  check(p.fork != ForkKind::Event || f.profiling, "Event fork => profiling", f);
  check(f.stream2 || (p.fork == ForkKind::None && p.join == JoinKind::None), "no second stream => no fork, no join", f);
  // (b) the parent
  const ParentSchedule r = parent_schedule(f);
  check((int)r.kmat_early + (int)r.fused_in_sample + (int)r.fused_in_tail + (int)r.update_launches + (int)f.kmat_ext == 1, "parent: exactly one place", f);
  check(r.update_launches == (parent_place(r, f) == KmatPlace::PhaseB), "parent: step_update launches <=> PhaseB", f);
  check(p.place == parent_place(r, f), "place equals the parent's", f);
  check(p.fork == parent_fork(r), "fork equals the parent's", f);
  check(p.join == parent_join(r), "join equals the parent's", f);
  check(p.ns == r.ns && p.cps == r.cps && p.nrider == r.nrider, "rider split equals the parent's", f);
}

static long check_grid() {
  static const int dk[] = {20, 50, 64, 65, 100, 200}, Ms[] = {32, 127, 128, 255, 256, 1024}, terms[] = {TERMS_LIK, TERMS_PRIOR, TERMS_ALL};
  long n = 0;
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
                    check_point(f);
                    ++n;
                  }
  return n;
}

// (c) bench.py's configurations: default tuning, second stream, flags on, one rank, no profiling, S = 128, n_dim = n_vars
static void check_pinned() {
  struct Row {
    const char* name;
    Family fam;
    int d, M;
    KmatPlace place;
    ForkKind fork;
    JoinKind join;
  };
  static const Row rows[] = {
      {"headline", BGE_SCORE, 50, 128, KmatPlace::InTail, ForkKind::FlagFromSample, JoinKind::Flag},
      {"config 2", BGE_SCORE, 20, 32, KmatPlace::InSample, ForkKind::FlagFromSample, JoinKind::Flag},
      {"config 3", LINGAUSS, 50, 128, KmatPlace::Stream2, ForkKind::StopEvent, JoinKind::Flag},
      {"config 4", BGE_SCORE, 50, 1024, KmatPlace::Stream2, ForkKind::StopEvent, JoinKind::Event},
      {"config 5", DENSENN, 100, 256, KmatPlace::Stream2, ForkKind::StopEvent, JoinKind::Event},
  };
  for (const Row& r : rows) {
    StepFacts f = engine_facts(r.fam, r.d, r.d, r.M, r.M, 128, true, false);
    f.flags_now = true;
    const StepPlan p = plan_step(f);
    check(p.place == r.place && p.fork == r.fork && p.join == r.join, r.name, f);
    if (p.place != r.place || p.fork != r.fork || p.join != r.join)
      fprintf(stderr, "  %s: place %d fork %d join %d\n", r.name, (int)p.place, (int)p.fork, (int)p.join);
  }
  // the headline's riders: 10 tiles, 20 chunks -> 10 pieces of 2 chunks, 100 units on the 128 CUs the particles leave free
  StepFacts f = engine_facts(BGE_SCORE, 50, 50, 128, 128, 128, true, false);
  f.flags_now = true;
  const StepPlan p = plan_step(f);
  check(p.ns == 10 && p.cps == 2 && p.nrider == 100, "headline rider split 10 x 2 chunks, 100 riders", f);
  // the switches move the headline as documented (tuning.h): no riders -> nothing fused above kmat_tiled_min; nothing fused at all
  f.no_kmat_grad = true;
  check(plan_step(f).place == KmatPlace::PhaseB, "headline, DIBS_NO_KMAT_GRAD: PhaseB (tiled matrix: no KmatFuse)", f);
  f = engine_facts(BGE_SCORE, 20, 20, 32, 32, 128, true, false);
  f.flags_now = false;
  const StepPlan q = plan_step(f);
  check(q.place == KmatPlace::InSample && q.fork == ForkKind::StopEvent && q.join == JoinKind::Event, "config 2, DIBS_NO_FLAGS: InSample, StopEvent, Event", f);
}

int main() {
  const long n = check_grid();
  check_pinned();
  for (long c : g_place) g_failures += c == 0;
  for (long c : g_fork) g_failures += c == 0;
  for (long c : g_join) g_failures += c == 0;
  if (g_failures) {
    fprintf(stderr, "step_plan_check: %d checks failed\n", g_failures);
    return 1;
  }
  printf("step_plan_check: ok, %ld grid points\n", n);
  printf("  place: External %ld Stream2 %ld InSample %ld InTail %ld PhaseB %ld\n", g_place[0], g_place[1], g_place[2], g_place[3], g_place[4]);
  printf("  fork: None %ld Event %ld StopEvent %ld FlagFromEdge %ld FlagFromSample %ld\n", g_fork[0], g_fork[1], g_fork[2], g_fork[3], g_fork[4]);
  printf("  join: None %ld EventAtOnce %ld Event %ld Flag %ld\n", g_join[0], g_join[1], g_join[2], g_join[3]);
  return 0;
}
