// How one SVGD step of the float32 engine (step_local / step_update, engine_step.hip) is scheduled, decided ONCE per step and written down
// as a value: where this step's kernel matrices are computed, how the second stream is forked behind the edge kernel and how it is joined
// in front of k_particle_grad.  plan_step is a pure function of StepFacts -- plain C++17, nothing of HIP, no allocation, no globals -- so
// that the whole truth table can be checked on a CPU (tests/tools/step_plan_check.cpp).  step_multi (batched and chains engines) keeps
// its own schedule (EventFork, engine_impl.h) and is not planned here.
#pragma once
#include "../../include/dibs_hip.h"  // DIBS_LIK_*, DIBS_EST_*
#include "kmat_consts.h"             // KT_T, KMAT_CH, kmat_tile_count, kmat_nchunk

enum { TERMS_LIK = 1, TERMS_PRIOR = 2, TERMS_ALL = 3 };

// what step_local reads from the engine to decide (filled by step_facts, engine_step.hip)
struct StepFacts {
  bool joint;
  int likelihood, estimator;  // DIBS_LIK_*, DIBS_EST_*
  int d, k, M, Mloc;
  long long D;                // latent floats per particle (2 d k)
  int S;
  int edge_kc, ldk;           // what edge_one_block reads beside d and k
  bool stream2;               // the second stream exists
  bool profiling, profiling_concurrent;
  bool flags_now;             // the engine's in-kernel flags are on for this chunk (latch_flags)
  bool fork_flag;             // the fork's flag word is allocated
  int kmat_ns_max;            // 0: no tiled kernel matrix; otherwise the most pieces per pair its buffer has room for
  bool kmat_ctr;              // the per-tile counters of the riding tile units are allocated
  bool w_tot;                 // a particle's W, U, V do not fit one block's LDS (k_backproject_big follows k_particle_grad)
  bool kmat_ext;              // dibs_engine_kmat_values has computed the slab of this step's phase B
  bool xk;                    // explicit per-particle keys (dibs_engine_eval_gradients)
  int terms;                  // TERMS_*
  int kmat_tiled_min;         // DibsTuning
  bool no_kmat_fuse, no_kmat_grad;
  bool median_h = false;      // a kernel bandwidth comes from the median rule (dibs_config.reserved_i[3]): selected on the device in front
                              // of the kernel matrices, which are then launches of their own (no fused placement, no external slab)
};

// Exactly one place computes a step's kernel matrices:
enum class KmatPlace {
  External,  // dibs_engine_kmat_values, on a stream of the caller (overlapped exchange)
  Stream2,   // phase A: launch_kmat on the second stream, behind the acyclicity chain
  InSample,  // phase A: the latent matrix as extra blocks of the k_bge_sample launch (KmatFuse)
  InTail,    // phase A: the latent matrix as tile units riding in the k_particle_grad launch (TailArgs::kt)
  PhaseB,    // step_update launches it
};
// How the second stream learns that the edge scores are there:
enum class ForkKind {
  None,            // no second stream in this step: everything in stream order
  Event,           // an event recorded behind the edge kernel (while profiling)
  StopEvent,       // the edge launch's own completion signal (hipExtLaunchKernelGGL stop event)
  FlagFromEdge,    // a sequence number that k_edge_scores_p's last block publishes, polled by k_wait_flag at the head of the second stream
  FlagFromSample,  // ... that the first block of k_bge_sample publishes
};
// How the main stream learns that the second stream's chain is done:
enum class JoinKind {
  None,
  EventAtOnce,  // per-kernel timing (set_profiling(1)): the main stream waits right behind the chain, so that every kernel runs alone
  Event,        // an event wait in front of k_particle_grad
  Flag,         // k_particle_grad polls the word k_join_flag stores (tail_join_wait)
};

struct StepPlan {
  bool do_lik, do_prior;
  bool score_lik;  // the likelihood part is BGe's or BDeu's score estimator (k_bge_sample, k_bge_chol / k_bdeu_nodes; W_lik is formed inside k_particle_grad)
  KmatPlace place;
  ForkKind fork;
  JoinKind join;
  int ns, cps, nrider;  // InTail: the chunk range of a tile in ns pieces of cps chunks, nrider extra blocks; otherwise zeros
};

// one 16-wave block per particle (k_edge_scores_p)
inline bool edge_one_block(int d, int k, int edge_kc, int ldk) { return d <= 64 && k <= 64 && edge_kc >= k && ldk <= 128; }
// One kernel-matrix algorithm per global particle count, on every rank and at every launch site: from kmat_tiled_min particles the tiled
// kernel (whose entries do not depend on how the work was cut, kernels_kmat.h), below it the direct one.
inline bool kmat_tiled_on(int kmat_ns_max, int M, int kmat_tiled_min) { return kmat_ns_max > 0 && M >= kmat_tiled_min; }

// (static: a copy per translation unit that uses it, no symbol of the shared library)
static inline StepPlan plan_step(const StepFacts& f) {
  StepPlan p{(f.terms & TERMS_LIK) != 0, (f.terms & TERMS_PRIOR) != 0, false, KmatPlace::PhaseB, ForkKind::None, JoinKind::None, 0, 0, 0};
  const bool single_rank = f.Mloc == f.M;
  // (BDeu: the same schedule with k_bdeu_nodes in the place of k_bge_chol; it admits the score estimator only.  The estimator is SCORE or
  //  REPARAM: dibs_engine_create)
  p.score_lik = p.do_lik && (f.likelihood == DIBS_LIK_BGE || f.likelihood == DIBS_LIK_BDEU) && f.estimator == DIBS_EST_SCORE;

  // ---- the second stream ----
  // The acyclicity chain runs on the second stream beside the likelihood chain whenever a step has both.
  // While per-kernel timing is on (set_profiling(1)) the main stream joins right away, so that every duration is a kernel alone on the
  // GPU -- but the launch still goes to the second stream: with that (high-priority) queue in existence the same kernel takes 104 us
  // on the main stream and 96 us on its own.
  // (Until round 4 a small acyclicity launch -- <= 512 blocks: config 2, or a rank of a sharded headline run -- stayed on the main stream: the
  //  fork / join events cost 6 + 6 us of the critical path, more than such a launch could hide.  With the fork as the edge kernel's completion
  //  signal and the join polled inside k_particle_grad the second stream pays at every size: config 2 18 460 -> 20 440 steps/s, a rank of
  //  a 4- / 8-way headline run 101.0 -> 91.4 / 85.8 -> 78.0 us per step.)
  const bool fork = p.do_prior && p.do_lik && f.stream2;
  const bool timing_alone = f.profiling && !f.profiling_concurrent;
  // the join inside k_particle_grad (tail_join_wait, agent-scope loads of a flag word the second stream's last kernel stores) instead of an
  // event wait in front of it: -7 us per step.  The polling blocks hold their CUs while the second stream still has kernels to place, so
  // the flag is used only while they cannot fill the machine (<= 128 particles: one block each on half of the CUs) and the engine's flags
  // are on for this chunk (flags_now: latch_flags).  The wait is bounded (join_err; a chunk that saw a time-out is run again on events:
  // dibs_engine_run, dibs_engine_run_sharded).  Per-kernel timing always uses the event.
  const bool flag_join = fork && !timing_alone && f.flags_now && f.Mloc <= 128;
  if (fork) p.join = flag_join ? JoinKind::Flag : (timing_alone ? JoinKind::EventAtOnce : JoinKind::Event);
  // fork without an event (marginal models): k_edge_scores_p stores what
  // the second stream reads (scores, exp(-alpha s)) at agent scope, every block counts itself and the last one publishes a sequence number;
  // one polling wave (k_wait_flag) heads the second stream's chain.  The completion signal cost the NEXT kernel of the main stream 4.7 us
  // (edge -> sample gap; 1.0 us between plain launches).  With the two chains starting together the acyclicity stream must not have
  // priority over the sampling kernel (it took the machine: sampling 130 us, the factorisation then alone for 33): the stream is created
  // with the LOWEST priority.  bench.py, same box: event fork 5 193-5 217 steps/s; flag fork with greatest / normal / lowest priority
  // 5 218-5 226 / 5 296 / 5 341; config 2 20 560 -> 22 200.  Joint models keep the event (config 3: 2 345 vs 2 311 with the flag).
  const bool flag_fork = flag_join && !f.joint && !f.profiling && f.fork_flag && edge_one_block(f.d, f.k, f.edge_kc, f.ldk);
  if (flag_fork) {
    // BGe with the score estimator: the flag is published by the FIRST BLOCK OF k_bge_sample instead (it starts when the edge kernel has
    // ended and released its plain stores): no agent-scope stores and no counting in the edge kernel
    p.fork = p.score_lik ? ForkKind::FlagFromSample : ForkKind::FlagFromEdge;
  } else if (fork) {
    // fork without a record packet on the main stream: the event is the edge kernel's own completion signal (never while profiling: the
    // launch is then bracketed by timing events)
    p.fork = f.profiling ? ForkKind::Event : ForkKind::StopEvent;
  }

  // ---- the kernel matrices ----
  // A sharded rank (Mloc != M) has only its own particles in phase A: phase B computes its slab from the gathered rows, or the caller's
  // side stream has done so from the gathered values (External).  The same holds with explicit keys (nothing moves: no phase B follows).
  // Median-rule bandwidth (median_h): distance pass -> selection -> kernel matrices, in that order on one stream.  The fused placements
  // (InSample, InTail) carry a bandwidth as a launch argument of a kernel that starts before the selection could have run, and an External
  // slab was computed without one, so neither is chosen: the second stream where the step forks, phase B otherwise.  Fork and join are
  // what they are without the flag.  (dibs_engine_create admits the rule on one rank only and refuses dibs_engine_kmat_values.)
  if (f.median_h) {
    if (fork && !f.xk && single_rank) p.place = KmatPlace::Stream2;
    return p;
  }
  if (f.kmat_ext) {
    p.place = KmatPlace::External;
    return p;
  }
  if (f.xk || !single_rank) return p;
  // Single rank: the kernel matrices need only z (and theta), which are final when the step starts.  For the joint models, and for the
  // marginal model once the matrix is large against the sampling work (M D > 4 S d^2), they follow the acyclicity kernel on the second
  // stream, which otherwise idles until the likelihood chain on the main stream is done; the join before k_particle_grad covers them.
  // Measured: config 3 (joint, 128 particles) 1 400 -> 1 453 steps/s, config 4 (1 024 particles) 329 -> 395.  A marginal model with fewer
  // particles keeps the latent matrix on the main stream, inside a launch that has CUs to spare: at the headline size (128 particles) as
  // tile units in k_particle_grad, below kmat_tiled_min (config 2) as extra blocks of k_bge_sample (KmatFuse: 8 us of that kernel's 70 at
  // the headline size; on the second stream 3 999 -> 3 902 steps/s, and ahead of the acyclicity kernel it delays that kernel).
  if (fork && (f.joint || (long long)f.M * f.D > 4LL * f.S * f.d * f.d)) {
    p.place = KmatPlace::Stream2;
    return p;
  }
  if (f.joint || f.no_kmat_fuse) return p;  // (the fused forms carry the latent matrix only; joint <=> not BGe: dibs_engine_create)
  // marginal models, 128+ particles: the latent matrix as tile units riding in the k_particle_grad launch (TailArgs::kt)
  if (!f.no_kmat_grad && f.kmat_ns_max > 1 && f.kmat_ctr && f.M >= f.kmat_tiled_min && f.Mloc < 256 && !f.w_tot) {
    const int nta = (f.M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, nta, 1), nchunk = kmat_nchunk((int)f.D);  // (as launch_tail builds the KmatTile)
    // (pieces: enough units for the CUs the particles leave free, one round of them -- measured at the headline size, launch time on the
    //  event timer: no units 20.7 us; 100 units of 2 chunks 21.2; 70 of 3 chunks 25.2; 200 of 1 chunk on 128 blocks 25.8)
    int ns = (256 - f.Mloc + tiles - 1) / tiles;
    ns = ns > nchunk ? nchunk : ns;
    ns = ns > f.kmat_ns_max ? f.kmat_ns_max : ns;
    const int cps = (nchunk + ns - 1) / ns;
    ns = (nchunk + cps - 1) / cps;
    if (ns > 1) {
      p.place = KmatPlace::InTail;
      p.ns = ns;
      p.cps = cps;
      p.nrider = tiles * ns < 256 - f.Mloc ? tiles * ns : 256 - f.Mloc;
      return p;
    }
  }
  // BGe with the score estimator, direct kernel matrix, vector fits one LDS chunk: the latent matrix rides along in k_bge_sample (KmatFuse)
  if (p.score_lik && !kmat_tiled_on(f.kmat_ns_max, f.M, f.kmat_tiled_min) && f.D <= KMAT_CH && f.D * 4 + 64 <= 80 * 1024)
    p.place = KmatPlace::InSample;
  return p;
}
