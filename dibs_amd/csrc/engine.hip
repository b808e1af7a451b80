// libdibs_hip.so -- the C ABI (include/dibs_hip.h), gfx950 only.  This file: creation and destruction, state, dibs_engine_run, buffers,
// profiling.  The steps are in engine_step.hip and engine_f64.hip, data and scoring in engine_data.hip, the exchange in engine_comm.hip.
#include "engine_impl.h"
#include <atomic>

static thread_local std::string g_err;
int fail(const std::string& m) {
  g_err = m;
  return 1;
}

extern "C" const char* dibs_last_error(void) { return g_err.c_str(); }
extern "C" int dibs_abi_version(void) { return DIBS_ABI_VERSION; }

static int64_t theta_size(const dibs_config& c) {
  const int d = c.n_vars;
  if (!c.joint) return 0;
  if (c.likelihood == DIBS_LIK_LINGAUSS) return (int64_t)d * d;
  if (c.likelihood == DIBS_LIK_DENSENN) {
    int64_t p = 0;
    int in = d;
    for (int l = 0; l <= c.nn_n_hidden; ++l) {
      const int out = l < c.nn_n_hidden ? c.nn_hidden[l] : 1;
      p += (int64_t)d * in * out + (c.nn_bias ? (int64_t)d * out : 0);
      in = out;
    }
    return p;
  }
  return 0;
}

// Batched engines: do the kernels of a step take the per-problem values from the device table?  The sizes whose kernels have table-reading
// forms (k_edge_scores_p, k_acyc<NT> / k_acyc_hf, k_particle_grad with W, U, V in LDS); beyond them the launch arguments of the whole batch.
static bool batch_hp_tier(const dibs_engine* e) {
  return e->B > 1 && !e->chains && e->d <= 64 && e->k <= 64 && e->w_tot == nullptr && e->tune.acyc_pipe != DIBS_PIPE_BF16;
}
// ... and a chains engine: the same sizes, for the same reason (dibs_engine_set_chain_hparams); whether a step reads the table is decided
// when the table is made final (batch_hp_commit: some chain's values differ)
static bool chains_hp_sizes_ok(const dibs_engine* e) {
  return e->chains && e->d <= 64 && e->k <= 64 && e->w_tot == nullptr && e->tune.acyc_pipe != DIBS_PIPE_BF16;
}
// the configuration's own values: what a problem or chain has until it is given others
static dibs_chain_hparams config_hparams(const dibs_config& c) {
  return dibs_chain_hparams{c.alpha_linear, c.beta_linear, c.h_latent, c.h_theta, c.stepsize, c.score_function_baseline, c.latent_prior_std,
                            c.graph_prior_edges_per_node};
}

// Engines alive in this process.  The in-kernel flags (fork: k_wait_flag, join: tail_join_wait) are used by an engine that is ALONE in its
// process -- the production layout, one process per GPU: its two or three streams have a hardware queue each.  Several engines in one process
// (the single-GPU emulation of a sharded run, tests with rank engines) share hardware queues, and a polling kernel at the head of a shared
// queue holds up the kernels behind it, possibly the one it waits for, until its bound: those engines use events.  DIBS_FLAGS_MULTI=1 lifts
// the rule (scripts/gpu_shard_scaling.py: what a rank of a real run would do).
static std::atomic<int> g_live_engines{0};
static ProblemHP derive_problem_hp(const dibs_engine* e, const dibs_chain_hparams& h);  // (below, with the per-problem accessors)
// sizes, stream, events and every device buffer of a new engine; on failure the caller destroys the half-built engine
static int engine_alloc(dibs_engine* e, const dibs_config& c, void* stream) {
  e->cfg = c;
  e->tune = dibs_tuning_from_env();
  e->d = c.n_vars;
  e->k = c.n_dim;
  e->B = c.reserved_i[0] > 1 ? c.reserved_i[0] : 1;
  e->chains = c.reserved_i[2] > 1;  // chains engine: the row layout of a batched engine of n_chains "problems" (dibs_engine_create: n_problems <= 1)
  if (e->chains) e->B = c.reserved_i[2];
  e->M = c.n_particles;
  e->Mloc = e->B > 1 ? e->B * c.n_particles : c.n_particles / c.n_ranks;
  e->m0 = c.rank * (c.n_particles / c.n_ranks);
  e->N = c.n_observations;
  e->S = c.n_grad_mc_samples;
  e->Sa = c.n_acyclicity_mc_samples;
  e->W = (e->d + 63) / 64;
  e->D = (int64_t)e->d * e->k * 2;
  e->P = theta_size(c);
  e->E = ((2 * e->D + 2 * e->P) + 3) & ~(int64_t)3;
  e->Ev = ((e->D + e->P) + 3) & ~(int64_t)3;
  e->dpad = (e->d + 15) & ~15;
  {
    // k_edge_scores walks the latent dimension in chunks of edge_kc columns: one chunk when U and V fit in LDS (n_vars <= 112 with k = d)
    e->edge_kc = e->k;
    for (;;) {
      const int kp = (e->edge_kc + 3) & ~3;
      e->ldk = kp + ((2 - kp) % 32 + 32) % 32;  // ldk == 2 (mod 32): conflict-free MFMA operand reads
      if ((size_t)2 * e->dpad * e->ldk * 4 <= LDS_LIMIT - 8192 || e->edge_kc <= 16) break;
      e->edge_kc = e->edge_kc > 64 ? 64 : e->edge_kc / 2;
    }
  }
  e->acyc_nt = e->dpad / 16;
  // One acyclicity block per work unit: a PAIR of chains when the PRNG layout lets one Threefry call serve both (see k_acyc), else one
  // chain.  (The grouping of the Sa chains into partial sums depends on Sa, d and the layout alone -- not on the particle count or how
  //  the particles are sharded, so results do not differ between rank counts in the last float bit.)
  e->acyc_paired = c.rng_layout == DIBS_RNG_LEGACY && (e->Sa & 1) == 0 && (uint64_t)e->Sa * e->d * e->d < 0xFFFFFFFFull;
  e->acyc_units = e->acyc_paired ? e->Sa / 2 : e->Sa;
  e->sigz = latent_sigma(c.latent_prior_std, e->k);
  if (stream) {
    e->stream = (hipStream_t)stream;
    e->own_stream = false;
  } else {
    // the engine's own main stream at the greatest priority (its chain -- sampling, factorisation, tail -- is the later one of a step):
    // bench.py, same box, alternating: 5 336 / 5 349 steps/s against 5 328 / 5 321 at the normal priority
    int lo = 0, hi = 0;
    hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, hi) != hipSuccess) {
      (void)hipGetLastError();
      HIP_OK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    }
    e->own_stream = true;
  }
  HIP_OK(hipEventCreate(&e->ev0));
  HIP_OK(hipEventCreate(&e->ev1));
  if (!e->tune.no_stream2) {
    int lo = 0, hi = 0;
    hipDeviceGetStreamPriorityRange(&lo, &hi);  // (lo = least, hi = greatest priority)
    // round 3, headline size: serial 3 906 steps/s; second stream at least / normal / greatest priority 3 906 / 3 964 / 4 001.
    // round 5 (fork by flag, both chains start together -- see the flag fork in plan_step, step_plan.h): least priority; with the event fork the three
    // priorities measure the same now (5 193-5 217), configs 3 / 5 gain 1-2 % at the least priority, config 4 is unchanged.
    const int prio = lo;
    // (an optimisation only: without it every kernel goes to the engine stream)
    if (hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, prio) != hipSuccess &&
        hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking) != hipSuccess) {
      e->stream2 = nullptr;
      (void)hipGetLastError();
    }
  }
  if (e->stream2) {
    HIP_OK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&e->ev_k0, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&e->ev_k1, hipEventDisableTiming));
    HIP_OK(dalloc(&e->join_flag, (size_t)4));
    HIP_OK(dalloc(&e->fork_flag, (size_t)4));
    HIP_OK(hipHostMalloc((void**)&e->join_err, 4, hipHostMallocDefault));
    *e->join_err = 0u;
    // the in-kernel join needs the two streams to make progress side by side (see k_probe_wait): asked once per process and device
    static std::mutex mu;
    static std::map<int, bool> concurrent;
    std::lock_guard<std::mutex> lock(mu);
    auto it = concurrent.find(c.device_id);
    if (it == concurrent.end()) {
      unsigned int* pr = nullptr;
      HIP_OK(dalloc(&pr, (size_t)2));
      launch_stream_probe(e->stream, e->stream2, pr);
      HIP_OK(hipStreamSynchronize(e->stream));
      HIP_OK(hipStreamSynchronize(e->stream2));
      unsigned int seen = 0;
      HIP_OK(hipMemcpy(&seen, pr + 1, 4, hipMemcpyDeviceToHost));
      hipFree(pr);
      it = concurrent.emplace(c.device_id, seen != 0u).first;
    }
    e->streams_concurrent = it->second;
  }
  if (c.reserved_i[1] == 64) {
    // float64 engine: of the f32 engine's buffers only the parent sets and node scores (same layouts) and the counters; F64State (f64_alloc)
    // holds everything else
    const size_t Ml = e->Mloc;
    HIP_OK(dalloc(&e->masks, Ml * e->S * e->d * e->W));
    HIP_OK(dalloc(&e->node_scores, Ml * e->S * e->d));
    HIP_OK(dalloc(&e->counters, (size_t)DIBS_N_COUNTERS));
    hipDeviceSynchronize();
    return 0;
  }
  const size_t Ml = e->Mloc, dd = (size_t)e->d * e->d;
  HIP_OK(dalloc(&e->z, Ml * e->D));
  HIP_OK(dalloc(&e->vz, Ml * e->D));
  HIP_OK(dalloc(&e->theta, Ml * e->P));
  HIP_OK(dalloc(&e->vtheta, Ml * e->P));
  HIP_OK(dalloc(&e->baseline, Ml));
  HIP_OK(dalloc(&e->baseline2, Ml));
  HIP_OK(dalloc(&e->scores, Ml * dd));
  HIP_OK(dalloc(&e->probs, Ml * dd));
  if (e->d <= 112) HIP_OK(dalloc(&e->eas, Ml * dd));
  HIP_OK(dalloc(&e->thr, Ml * dd));
  HIP_OK(dalloc(&e->w_lik, Ml * dd));
  if (e->d > 112) {
    if (hipMalloc((void**)&e->acyc_big, acyc_big_elems(e->Mloc, e->d, e->Sa) * 4) != hipSuccess) {
      e->acyc_big = nullptr;
      (void)hipGetLastError();
      return fail("n_vars > 112: the matrix powers of the acyclicity term go through global memory: hipMalloc of " +
                  std::to_string(acyc_big_elems(e->Mloc, e->d, e->Sa) * 4 >> 20) + " MiB failed");
    }
  } else {
    HIP_OK(dalloc(&e->acyc_part, Ml * e->acyc_units * dd));
  }
  HIP_OK(dalloc(&e->w_acyc, Ml * dd));
  {
    const bool score_lik = lik_marginal(c.likelihood) && c.grad_estimator_z == DIBS_EST_SCORE;
    const int ldz = tail_ldz(e->d, e->k, e->S, score_lik, LDS_LIMIT - 2048);
    if (tail_lds_bytes(e->d, ldz, e->S, e->W, score_lik, 0) > LDS_LIMIT - 2048) HIP_OK(dalloc(&e->w_tot, Ml * dd));
  }
  HIP_OK(dalloc(&e->logprobs_z, Ml * e->S));
  HIP_OK(dalloc(&e->logprobs_th, Ml * e->S));
  HIP_OK(dalloc(&e->pack, (size_t)(e->B > 1 ? e->Mloc : e->M) * e->E));
  if (e->B > 1) {
    HIP_OK(dalloc(&e->bcarry, (size_t)e->B));
    HIP_OK(dalloc(&e->bkeys_lik, (size_t)e->Mloc));
    HIP_OK(dalloc(&e->bkeys_prior, (size_t)e->Mloc));
    if (e->chains) HIP_OK(dalloc(&e->bkeys_theta, (size_t)e->Mloc));
    HIP_OK(dalloc(&e->hp, (size_t)e->B));
    e->hp_host.assign((size_t)e->B, config_hparams(c));
  }
  e->median_rule = c.reserved_i[3];
  if (e->median_rule) {
    if (e->B == 1) {  // a standalone engine on the rule: a one-row table of the configuration's values, final from the start
      HIP_OK(dalloc(&e->hp, (size_t)1));
      e->hp_host.assign((size_t)1, config_hparams(c));
      const ProblemHP row = derive_problem_hp(e, e->hp_host[0]);
      HIP_OK(hipMemcpy(e->hp, &row, sizeof row, hipMemcpyHostToDevice));
      e->hp_final = true;
    }
    if (e->median_rule & 1) HIP_OK(dalloc(&e->sqd_z, Ml * e->M));
    if (e->median_rule & 2) HIP_OK(dalloc(&e->sqd_t, Ml * e->M));
    HIP_OK(dalloc(&e->bw, (size_t)2 * e->B));
  }
  // (k_phi_gemm reads whole 128-row x 32-column tiles without bounds checks: rows padded to a multiple of 128, one more tile row of slack)
  const size_t kpad = (((Ml + 127) / 128) * 128 - Ml) * e->M + 64;
  HIP_OK(dalloc(&e->kz, Ml * e->M + kpad));
  if (c.joint) HIP_OK(dalloc(&e->kt, Ml * e->M + kpad));
  if (c.joint) HIP_OK(dalloc(&e->ksum, Ml * e->M + kpad));
  if (e->M >= e->tune.kmat_tiled_min && e->B == 1) {  // (the same rule on every rank: it depends on the global particle count only)
    // room for up to 32 pieces per pair, less for many particles (<= 512 MiB); 1 = no buffer, every unit holds whole distances
    size_t ns = ((size_t)512 << 20) / (Ml * e->M * 8);
    ns = ns > 32 ? 32 : (ns < 1 ? 1 : ns);
    if (!kmat_tile_addressable((size_t)2 * e->M, e->E > e->Ev ? e->E : e->Ev, 0, 0)) ns = 0;  // (32-bit row offsets in the tile kernel)
    if (ns > 1 && hipMalloc((void**)&e->kpart, ns * Ml * e->M * 8) != hipSuccess) {
      e->kpart = nullptr;
      (void)hipGetLastError();
      ns = 1;
    }
    e->kmat_ns_max = (int)ns;
    if (ns > 1 && e->Mloc == e->M) {
      const size_t nta = (e->M + KT_T - 1) / KT_T;
      HIP_OK(dalloc(&e->kmat_ctr, nta * (nta + 1) / 2));
    }
  }
  HIP_OK(dalloc(&e->phi_z, Ml * e->D));
  HIP_OK(dalloc(&e->phi_th, Ml * e->P));
  HIP_OK(dalloc(&e->counters, (size_t)DIBS_N_COUNTERS));
  if (c.likelihood == DIBS_LIK_BDEU) {
    // the sampling launch is BGe's (k_bge_sample): it reads a node's statistics for the closed form of an empty parent set and queues the
    // rest.  Zero tables make that score 0 (N_j = 0); k_bdeu_nodes then writes every entry, and k_particle_grad resets the queue counters
    e->bdeu = new BdeuState();
    e->bdeu->log_ess = log(c.reserved_d[0] > 0 ? c.reserved_d[0] : 1.0);
    const size_t dp = (size_t)e->d + 1;
    HIP_OK(dalloc(&e->bge.Rp, 2 * dp * dp));
    e->bge.Qp = e->bge.Rp + dp * dp;
    HIP_OK(dalloc(&e->bge.gam, (size_t)e->d * dp));
    HIP_OK(dalloc(&e->bge.Nj, (size_t)e->d));
    HIP_OK(dalloc(&e->bge.ldR, (size_t)1));
    e->bge.n_mats = 1;
  }
  if (lik_marginal(c.likelihood)) {
    HIP_OK(dalloc(&e->masks, Ml * e->S * e->d * e->W));
    HIP_OK(dalloc(&e->node_scores, Ml * e->S * e->d));
    e->bq.cap = (uint32_t)(Ml * e->S * e->d);
    HIP_OK(dalloc(&e->bq.list, (size_t)BGE_NQ * e->bq.cap * bge_entry_u4(e->W)));  // (one list per size tier, each sized for every problem)
    HIP_OK(dalloc(&e->bq.counts, (size_t)16));
    if (c.grad_estimator_z == DIBS_EST_REPARAM) {
      HIP_OK(dalloc(&e->soft_ds, Ml * e->S * dd));
      if (e->d > 128) {
        const size_t prob = Ml * e->S;
        e->soft_blocks = (int)(prob < 1024 ? prob : 1024);
        HIP_OK(dalloc(&e->soft_tri, (size_t)e->soft_blocks * 4 * 2 * bge_soft_tri(e->d)));
      }
    }
  }
  if (c.joint) {
    if (joint_alloc(&e->jw, e->Mloc, e->d, e->N, e->S) != 0) return fail("joint work buffers: hipMalloc failed");
  }
  e->hp_tier = batch_hp_tier(e);
  e->chain_hp_ok = chains_hp_sizes_ok(e);
  hipDeviceSynchronize();  // the zero fills above ran on the null stream; the engine's own stream does not wait for it
  return 0;
}

extern "C" int dibs_engine_create(const dibs_config* cfg, void* stream, dibs_engine** out) {
  if (!cfg || !out) return fail("null argument");
  *out = nullptr;
  const dibs_config& c = *cfg;
  if (c.abi_version != DIBS_ABI_VERSION) return fail("dibs_config.abi_version mismatch");
  if (c.reserved_i[3] != 0) {
    // median-heuristic kernel bandwidth (reserved_i[3]: bit 0 the latent kernel, bit 1 the parameter kernel; include/dibs_hip.h)
    const std::string pre = "median bandwidth: ";
    const int rule = c.reserved_i[3];
    if (rule < 0 || rule > 3) return fail(pre + "dibs_config.reserved_i[3] (bandwidth rule) must be 0 .. 3 (bit 0: latent kernel, bit 1: parameter kernel), got " + std::to_string(rule));
    if ((rule & 2) && !c.joint) return fail(pre + "bit 1 (the parameter kernel) needs a joint model; a marginal model has no parameter kernel");
    if (c.reserved_i[1] == 64) return fail(pre + "the float64 engine is not supported (float32 only)");
    if (c.n_ranks > 1) return fail(pre + "n_ranks must be 1 (the selection needs the distances of all particles; a sharded run holds a slab)");
    if (c.n_particles >= 256)
      return fail(pre + "n_particles (per run) must be < 256: the GEMM form of the SVGD transform (k_phi_gemm) has no table-reading form and the "
                        "selection is one block per run -- both are the follow-up");
    if (c.n_particles < 2) return fail(pre + "n_particles must be >= 2 (one particle has no pair to take a median of)");
  }
  {
    // chains engine (reserved_i[2] = n_chains = C > 1, include/dibs_hip.h): C chains of one joint model on one data set, one rank, float32
    const int64_t C = c.reserved_i[2];
    const std::string pre = "chains engine (n_chains > 1): ";
    if (C < 0) return fail(pre + "n_chains (reserved_i[2]) must be >= 0");
    if (C > 1) {
      if (c.reserved_i[0] > 1) return fail(pre + "n_problems (reserved_i[0]) must be 0 or 1 (chains share one data set; a batch of problems has no chains)");
      if (!c.joint) return fail(pre + "marginal models are not supported (JointDiBS only; MarginalDiBS restarts are a batched engine, n_problems)");
      if (c.n_ranks != 1) return fail(pre + "n_ranks must be 1 (chains are not sharded over ranks)");
      if (c.reserved_i[1] == 64) return fail(pre + "float64 is not supported (the float64 engine runs MarginalDiBS + BGe only)");
      const DibsTuning tn = dibs_tuning_from_env();
      if (c.n_particles >= 256 || c.n_particles >= tn.kmat_t64_min)
        return fail(pre + "n_particles (per chain) must be < 256 (the GEMM form of the SVGD transform is not batched)");
      const int64_t rows = C * (int64_t)(c.n_particles > 0 ? c.n_particles : 1);
      if (rows > ((int64_t)1 << 24)) return fail(pre + "n_chains * n_particles must be <= 2^24");
      // Per-row arrays of C M rows that kernels of the standalone step address with 32-bit element offsets (or that are safe only while they
      // stay below 2^31 elements): the packed rows, the d x d arrays and the acyclicity partial sums (at most Sa blocks per particle), the
      // per-sample arrays, DenseNN's per-hidden-unit first-layer tables.  One rule for all of them.
      const int64_t d = c.n_vars, k = c.n_dim > 0 ? c.n_dim : 1, lim = (int64_t)1 << 31;
      const bool nn_ok = c.likelihood != DIBS_LIK_DENSENN || (c.nn_n_hidden >= 1 && c.nn_n_hidden <= DIBS_MAX_HIDDEN_LAYERS);  // (validated below)
      const int64_t row_elems = 4 * d * k + 2 * (nn_ok ? theta_size(c) : 0) + 4;
      const int64_t h0 = c.likelihood == DIBS_LIK_DENSENN && c.nn_n_hidden >= 1 && c.nn_hidden[0] > 0 ? c.nn_hidden[0] : 1;
      const int64_t Sa = c.n_acyclicity_mc_samples > 0 ? c.n_acyclicity_mc_samples : 1, S = c.n_grad_mc_samples > 0 ? c.n_grad_mc_samples : 1;
      if (rows * row_elems >= lim || rows * d * d * Sa >= lim || rows * d * d * h0 >= lim || rows * S >= lim)
        return fail(pre + "n_chains * n_particles rows are too many for this model size (a per-row array would pass 2^31 elements)");
    }
  }
  {
    // precision (reserved_i[1]): 0 / 32 = float32, 64 = the float64 engine (MarginalDiBS + BGe + score estimator, one rank, one problem)
    const int prec = c.reserved_i[1];
    if (prec != 0 && prec != 32 && prec != 64)
      return fail("float64 engine: dibs_config.reserved_i[1] (precision) must be 0 or 32 (float32) or 64 (float64), got " + std::to_string(prec));
    if (prec == 64) {
      if (c.joint) return fail("float64 engine: joint models are not supported (MarginalDiBS + BGe only)");
      if (c.likelihood != DIBS_LIK_BGE) return fail("float64 engine: only the BGe marginal likelihood is supported");
      if (c.grad_estimator_z != DIBS_EST_SCORE) return fail("float64 engine: the reparam estimator is not supported (score-function estimator only)");
      if (c.n_ranks != 1) return fail("float64 engine: n_ranks must be 1");
      if (c.reserved_i[0] > 1) return fail("float64 engine: n_problems must be 1 (no batched float64 engine)");
      if (c.n_vars < 2 || c.n_vars > 64) return fail("float64 engine: n_vars must be in [2, 64]");
      if (c.n_particles > 1024) return fail("float64 engine: n_particles must be <= 1024");
    }
  }
  if (c.n_vars < 2 || c.n_vars > 256) return fail("n_vars must be in [2, 256]");
  // 113 .. 256 variables: the LDS-resident kernels give way to the global-memory paths (kernels_acyc_big.h, k_backproject_big, chunked
  // k_edge_scores, k_bge_chol_wide).  The joint models run on their general paths there: LinearGaussian on the Gram-matrix kernels,
  // DenseNonlinearGaussian on kernels_nn_generic.h; beyond the LDS capacity (two n_vars x n_vars float operands: 141, one: 198) the blocks
  // keep them in global scratch (round 5: the limits of 141 / 198 variables are gone); soft-graph BGe has its own limit below
  if (c.n_dim < 1) return fail("n_dim must be >= 1");
  if (c.n_particles < 1 || c.n_grad_mc_samples < 1 || c.n_acyclicity_mc_samples < 1) return fail("sizes must be >= 1");
  if (c.n_ranks < 1 || c.rank < 0 || c.rank >= c.n_ranks) return fail("bad rank / n_ranks");
  if (c.n_particles % c.n_ranks) return fail("n_particles must be divisible by n_ranks");
  {
    // batched engine (n_problems > 1, include/dibs_hip.h): MarginalDiBS + BGe + score estimator on one rank
    const int64_t B = c.reserved_i[0];
    if (B < 0) return fail("n_problems (reserved_i[0]) must be >= 0");
    if (B > 1) {
      if (c.joint) return fail("batched engine (n_problems > 1): joint models are not supported (MarginalDiBS + BGe only)");
      if (c.likelihood != DIBS_LIK_BGE) return fail("batched engine (n_problems > 1): only the BGe marginal likelihood is supported");
      if (c.grad_estimator_z != DIBS_EST_SCORE)
        return fail("batched engine (n_problems > 1): the reparam estimator is not supported (score-function estimator only)");
      if (c.n_ranks != 1) return fail("batched engine (n_problems > 1): n_ranks must be 1 (a batch is not sharded over ranks)");
      const DibsTuning tn = dibs_tuning_from_env();
      if (c.n_particles >= 256 || c.n_particles >= tn.kmat_t64_min)
        return fail("batched engine (n_problems > 1): n_particles (per problem) must be < 256");
      const int64_t d = c.n_vars, rows = B * c.n_particles;
      // queue code (m d + j) S + s of k_bge_sample / k_bge_chol is 32-bit, and so is every queue's capacity (rows d S entries)
      if (rows * d * c.n_grad_mc_samples >= ((int64_t)1 << 32))
        return fail("batched engine (n_problems > 1): n_problems * n_particles * n_vars * n_grad_mc_samples must be < 2^32");
      // k_bge_chol addresses the stacked matrices [B d][2][d + 1][d + 1] with 32-bit float offsets
      if (d <= 128 && 2 * B * d * (d + 1) * (d + 1) >= ((int64_t)1 << 31))
        return fail("batched engine (n_problems > 1): n_problems * n_vars * (n_vars + 1)^2 too large for the factorisation kernel");
      if (rows > ((int64_t)1 << 24)) return fail("batched engine (n_problems > 1): n_problems * n_particles too large");
    }
  }
  if (c.grad_estimator_z != DIBS_EST_SCORE && c.grad_estimator_z != DIBS_EST_REPARAM)
    return fail("Unknown gradient estimator");  // dibs.py:318 (ValueError)
  if (c.optimizer != DIBS_OPT_GD && c.optimizer != DIBS_OPT_RMSPROP) return fail("unknown optimizer");  // svgd.py:122
  if (c.likelihood < 0 || c.likelihood > DIBS_LIK_BDEU) return fail("unknown likelihood model");
  if (c.graph_prior < 0 || c.graph_prior > DIBS_PRIOR_EDGEWISE) return fail("unknown graph prior");
  if (c.graph_prior == DIBS_PRIOR_EDGEWISE && c.reserved_i[0] > 1)
    return fail("batched engine (n_problems > 1): the edge-wise graph prior is not supported (the table-reading tail kernel has no edge-wise "
                "form, and per-problem tables are not built)");
  if (c.likelihood == DIBS_LIK_BDEU) {
    // BDeu on discrete data (include/dibs_hip.h, BDEU): MarginalDiBS, score-function estimator, float32 engine
    if (c.joint) return fail("BDeu: joint = 1 is not supported (a marginal likelihood: MarginalDiBS only)");
    if (c.grad_estimator_z == DIBS_EST_REPARAM)
      return fail("BDeu: the reparam estimator is not supported (a count-based score has no soft-graph form; score-function estimator only)");
    if (c.n_observations < 1 || c.n_observations > BDEU_MAX_N)
      return fail("BDeu: n_observations = " + std::to_string(c.n_observations) + " but must be in [1, " + std::to_string(BDEU_MAX_N) +
                  "] (the grouping table of one wave must fit a block's LDS)");
  }
  if (!c.joint && !lik_marginal(c.likelihood))
    return fail("MarginalDiBS needs a marginal likelihood (BGe, BDeu)");
  if (c.joint && c.likelihood == DIBS_LIK_BGE)
    return fail("JointDiBS + BGe is not constructible (BGe has no parameters; linearGaussian.py:53-54)");
  if (c.likelihood == DIBS_LIK_BGE && c.grad_estimator_z == DIBS_EST_REPARAM) {
    // soft-graph BGe (kernels_bge_soft.h): one or two matrix rows per lane, packed factor + inverse columns per wave in LDS; beyond 128
    // variables four rows per lane and the triangles in global scratch
    if (c.n_vars <= 128 && bge_soft_waves(c.n_vars, false) < 1)
      return fail("BGe + reparam estimator: n_vars too large for the device kernel");
  }
  if (lik_marginal(c.likelihood) && c.grad_estimator_z == DIBS_EST_SCORE &&
      bge_sample_lds_bytes(c.n_vars, c.n_grad_mc_samples, (c.n_vars + 63) / 64) > LDS_LIMIT - 2048)
    return fail("BGe: n_grad_mc_samples too large (the parent sets of one node's samples are staged in LDS)");
  if (c.likelihood == DIBS_LIK_DENSENN) {
    // one hidden layer of <= 64 units with <= 128 observations runs on the MFMA kernels of kernels_nn.h, every other stack on the
    // general path of kernels_nn_generic.h
    if (c.nn_n_hidden < 1 || c.nn_n_hidden > DIBS_MAX_HIDDEN_LAYERS) return fail("DenseNonlinearGaussian: 1 to " + std::to_string(DIBS_MAX_HIDDEN_LAYERS) + " hidden layers");
    for (int l = 0; l < c.nn_n_hidden; ++l)
      if (c.nn_hidden[l] < 1) return fail("DenseNonlinearGaussian: hidden widths must be >= 1");
    if (c.nn_activation < 0 || c.nn_activation > 3) return fail("Invalid activation function");  // nonlinearGaussian.py:61 (KeyError)
  }
  if (c.graph_prior == DIBS_PRIOR_ER) {
    const double p = er_edge_prob(c);
    if (!(p > 0.0 && p < 1.0)) return fail("Erdos-Renyi prior: edge probability must be in (0, 1)");
  }
  {
    if ((size_t)2 * 4 * c.n_particles * 4 + 4096 > LDS_LIMIT) return fail("n_particles too large (kernel rows must fit in LDS)");
    // k_particle_grad keeps a particle's score-space gradient, its Z and (score estimator) the per-sample weights in LDS; beyond that
    // size W goes through global memory (k_backproject_big) and only the per-sample weights have to fit
    const bool score_lik = lik_marginal(c.likelihood) && c.grad_estimator_z == DIBS_EST_SCORE;
    if (tail_lds_bytes(c.n_vars, 0, c.n_grad_mc_samples, (c.n_vars + 63) / 64, score_lik, 0) > LDS_LIMIT - 2048 ||
        backproject_big_lds(c.n_vars) > LDS_LIMIT - 2048)
      return fail("n_grad_mc_samples (or n_vars) too large: a particle's sample weights do not fit in LDS");
  }
  // (LinearGaussian: x beyond the LDS capacity takes the Gram-matrix path; DenseNonlinearGaussian the general path)
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail("no HIP device");
  HIP_OK(hipSetDevice(c.device_id));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, c.device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(std::string("libdibs_hip is built for gfx950 only; device is ") + prop.gcnArchName);

  dibs_engine* e = new dibs_engine();  // value-initialised: every POD member starts at zero
  g_live_engines.fetch_add(1);
  if (engine_alloc(e, c, stream) || (c.reserved_i[1] == 64 && f64_alloc(e))) {
    const std::string msg = g_err;
    dibs_engine_destroy(e);  // frees whatever had been allocated (stream, events, buffers)
    g_err = msg;
    return 1;
  }
  *out = e;
  return 0;
}

extern "C" int dibs_engine_destroy(dibs_engine* e) {
  if (!e) return 0;
  g_live_engines.fetch_sub(1);
  hipSetDevice(e->cfg.device_id);
  if (e->stream) hipStreamSynchronize(e->stream);
  if (e->stream2) hipStreamSynchronize(e->stream2);
  void* ptrs[] = {e->z, e->vz, e->theta, e->vtheta, e->baseline, e->baseline2, e->scores, e->probs, e->eas, e->thr, e->w_lik, e->acyc_part, e->w_acyc,
                  e->logprobs_z, e->logprobs_th, e->pack, e->kz, e->kt, e->phi_z, e->phi_th, e->counters, e->masks,
                  e->node_scores, e->x, e->mask, e->bq.list, e->bq.counts, e->soft_ds, e->acyc_big, e->w_tot, e->join_flag, e->fork_flag, e->carry_bak, e->soft_tri, e->ksum, e->kpart, e->kmat_ctr, e->bcarry, e->bkeys_lik, e->bkeys_prior, e->bkeys_theta, e->hp, e->edge_tab, e->edge_tab64, e->sqd_z, e->sqd_t, e->bw};
  for (void* p : ptrs)
    if (p) hipFree(p);
  joint_free(&e->jw);
  delete e->f64;
  delete e->bdeu;
  dibs_engine_comm_destroy(e);
  if (e->stream2) hipStreamDestroy(e->stream2);
  if (e->ev_fork) hipEventDestroy(e->ev_fork);
  if (e->ev_join) hipEventDestroy(e->ev_join);
  if (e->ev_k0) hipEventDestroy(e->ev_k0);
  if (e->ev_k1) hipEventDestroy(e->ev_k1);
  if (e->join_err) hipHostFree(e->join_err);
  if (e->ev0) hipEventDestroy(e->ev0);
  if (e->ev1) hipEventDestroy(e->ev1);
  for (auto& pe : e->pending) {
    hipEventDestroy(pe.second.first);
    hipEventDestroy(pe.second.second);
  }
  if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
  delete e;
  return 0;
}

extern "C" int dibs_engine_set_state(dibs_engine* e, const float* z, const float* v_z, const float* theta,
                                     const float* v_theta, const uint32_t* key, const float* baseline) {
  if (!e) return fail("null engine");
  if (e->f64) return fail("float64 engine: use dibs_engine_set_state_f64 (the f32 state accessors would round)");
  if (e->B > 1 && key) return fail("batched engine: the loop-carry keys go through dibs_engine_set_keys (key must be null)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->B > 1 && batch_hp_commit(e)) return 1;
  const size_t nz = (size_t)e->Mloc * e->D * 4, nt = (size_t)e->Mloc * e->P * 4;
  if (z || theta) e->vals_fresh = false;
  if (z || theta) e->kmat_ext = false;  // (an externally computed kernel slab belonged to the old values: phase B computes its own unless
                                        //  dibs_engine_kmat_values is called again for the new ones)
  if (z) HIP_OK(hipMemcpy(e->z, z, nz, hipMemcpyHostToDevice));
  if (v_z) HIP_OK(hipMemcpy(e->vz, v_z, nz, hipMemcpyHostToDevice));
  if (theta && nt) HIP_OK(hipMemcpy(e->theta, theta, nt, hipMemcpyHostToDevice));
  if (v_theta && nt) HIP_OK(hipMemcpy(e->vtheta, v_theta, nt, hipMemcpyHostToDevice));
  if (key) e->key = Key2{key[0], key[1]};
  if (baseline) HIP_OK(hipMemcpy(e->baseline, baseline, (size_t)e->Mloc * 4, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int dibs_engine_get_state(dibs_engine* e, float* z, float* v_z, float* theta, float* v_theta, uint32_t* key,
                                     float* baseline) {
  if (!e) return fail("null engine");
  if (e->f64) return fail("float64 engine: use dibs_engine_get_state_f64 (the f32 state accessors would round)");
  if (e->B > 1 && key) return fail("batched engine: the loop-carry keys go through dibs_engine_get_keys (key must be null)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const size_t nz = (size_t)e->Mloc * e->D * 4, nt = (size_t)e->Mloc * e->P * 4;
  if (z) HIP_OK(hipMemcpy(z, e->z, nz, hipMemcpyDeviceToHost));
  if (v_z) HIP_OK(hipMemcpy(v_z, e->vz, nz, hipMemcpyDeviceToHost));
  if (theta && nt) HIP_OK(hipMemcpy(theta, e->theta, nt, hipMemcpyDeviceToHost));
  if (v_theta && nt) HIP_OK(hipMemcpy(v_theta, e->vtheta, nt, hipMemcpyDeviceToHost));
  if (key) {
    key[0] = e->key.a;
    key[1] = e->key.b;
  }
  if (baseline) HIP_OK(hipMemcpy(baseline, e->baseline, (size_t)e->Mloc * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- batched engine: the loop-carry keys per problem (include/dibs_hip.h, n_problems) ----------------------------------------------------
extern "C" int dibs_engine_get_keys(dibs_engine* e, uint32_t* keys) {
  if (need_batch(e)) return 1;
  if (!keys) return fail("null argument");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  HIP_OK(hipMemcpy(keys, e->bcarry, (size_t)e->B * sizeof(Key2), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int dibs_engine_set_keys(dibs_engine* e, const uint32_t* keys) {
  if (need_batch(e)) return 1;
  if (!keys) return fail("null argument");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  HIP_OK(hipMemcpy(e->bcarry, keys, (size_t)e->B * sizeof(Key2), hipMemcpyHostToDevice));
  return 0;
}

// ---- batched engine: per-problem hyper-parameters (include/dibs_hip.h, dibs_engine_set_problem_hparams) ---------------------------------
static dibs_config problem_config(const dibs_engine* e, const dibs_chain_hparams& h) {
  dibs_config c = e->cfg;
  c.alpha_linear = h.alpha_linear;
  c.beta_linear = h.beta_linear;
  c.h_latent = h.h_latent;
  c.h_theta = h.h_theta;
  c.stepsize = h.stepsize;
  c.score_function_baseline = h.score_function_baseline;
  c.latent_prior_std = h.latent_prior_std;
  c.graph_prior_edges_per_node = h.graph_prior_edges_per_node;
  return c;
}
// the scalars the standalone engine derives on the host from a configuration (launch_tail, launch_phi_update, launch_kmat), per problem
static ProblemHP derive_problem_hp(const dibs_engine* e, const dibs_chain_hparams& h) {
  const dibs_config c = problem_config(e, h);
  const float sigz = latent_sigma(c.latent_prior_std, e->k);
  return ProblemHP{c.alpha_linear, c.beta_linear, c.score_function_baseline, 0.f, 0.f, (float)er_log_odds(c), 1.0f / (sigz * sigz),
                   (float)c.h_latent, (float)c.stepsize, (float)c.h_theta};
}
static bool same_derived(const ProblemHP& a, const ProblemHP& b) {
  return a.alpha_linear == b.alpha_linear && a.beta_linear == b.beta_linear && a.sf_baseline == b.sf_baseline && a.prior_c == b.prior_c &&
         a.inv_sig2 == b.inv_sig2 && a.h == b.h && a.stepsize == b.stepsize && a.h_theta == b.h_theta;
}

// what the per-problem and the per-chain accessors check alike, each with its own wording: the run index (`range`); for a setter
// (set != null) also that the table is not final yet (`frozen`) and the edge probability of an Erdos-Renyi prior (`er`)
static int hp_check(const dibs_engine* e, int i, const std::string& range, const dibs_chain_hparams* set = nullptr, const std::string& frozen = "",
                    const std::string& er = "") {
  if (i < 0 || i >= e->B) return fail(range);
  if (!set) return 0;
  if (e->hp_final) return fail(frozen);
  const dibs_config c = problem_config(e, *set);
  if (c.graph_prior == DIBS_PRIOR_ER) {  // (what dibs_engine_create asks of the shared value)
    const double pr = er_edge_prob(c);
    if (!(pr > 0.0 && pr < 1.0)) return fail(er + ": Erdos-Renyi prior: edge probability must be in (0, 1)");
  }
  return 0;
}

extern "C" int dibs_engine_set_problem_hparams(dibs_engine* e, int32_t p, const dibs_problem_hparams* hp) {
  if (!e || !hp) return fail("batched engine: dibs_engine_set_problem_hparams: null engine or argument");
  if (refuse_chains(e, "dibs_engine_set_problem_hparams (the chains of a JointDiBS + LinearGaussian engine take their own values through "
                       "dibs_engine_set_chain_hparams)"))
    return 1;
  if (e->B <= 1) return fail("batched engine: dibs_engine_set_problem_hparams needs one (dibs_config.reserved_i[0] = n_problems must be > 1)");
  // (h_theta: a marginal model has no parameter kernel; the configuration's value rides along)
  const dibs_chain_hparams h{hp->alpha_linear, hp->beta_linear, hp->h_latent, e->cfg.h_theta, hp->stepsize, hp->score_function_baseline,
                             hp->latent_prior_std, hp->graph_prior_edges_per_node};
  if (hp_check(e, p, "batched engine: dibs_engine_set_problem_hparams: problem index out of range", &h,
               "batched engine: dibs_engine_set_problem_hparams after the particles were initialised (init_particles_batch / set_state / run): "
               "latent_prior_std enters the initial draw and the device table is written once",
               "batched engine: problem " + std::to_string(p)))
    return 1;
  if (!e->hp_tier && !same_derived(derive_problem_hp(e, h), derive_problem_hp(e, config_hparams(e->cfg))))
    return fail("batched engine: problem " + std::to_string(p) + ": hyper-parameters that differ from the configuration's need n_vars <= 64 and "
                "n_dim <= 64 (and the default acyclicity pipe); this engine's kernels take them as launch arguments of the whole batch");
  e->hp_host[(size_t)p] = h;
  return 0;
}

extern "C" int dibs_engine_get_problem_hparams(dibs_engine* e, int32_t p, dibs_problem_hparams* hp) {
  if (!e || !hp) return fail("batched engine: dibs_engine_get_problem_hparams: null engine or argument");
  if (e->B <= 1) return fail("batched engine: dibs_engine_get_problem_hparams needs one (dibs_config.reserved_i[0] = n_problems must be > 1)");
  if (hp_check(e, p, "batched engine: dibs_engine_get_problem_hparams: problem index out of range")) return 1;
  const dibs_chain_hparams& h = e->hp_host[(size_t)p];
  *hp = dibs_problem_hparams{h.alpha_linear, h.beta_linear, h.h_latent, h.stepsize, h.score_function_baseline, h.latent_prior_std,
                             h.graph_prior_edges_per_node};
  return 0;
}

// ---- chains engine: per-chain hyper-parameters (include/dibs_hip.h, PER-CHAIN HYPER-PARAMETERS) ------------------------------------------
static bool differs_from_config(const dibs_engine* e, const dibs_chain_hparams& h) {
  return !same_derived(derive_problem_hp(e, h), derive_problem_hp(e, config_hparams(e->cfg)));
}
bool chains_hp_differ(const dibs_engine* e) {
  if (!e->chains) return false;
  for (const dibs_chain_hparams& h : e->hp_host)
    if (differs_from_config(e, h)) return true;
  return false;
}

extern "C" int dibs_engine_set_chain_hparams(dibs_engine* e, int32_t c, const dibs_chain_hparams* hp) {
  const std::string pre = "chains engine (n_chains > 1): dibs_engine_set_chain_hparams: ";
  if (!e || !hp) return fail(pre + "null engine or argument");
  if (!e->chains) return fail(pre + "needs a chains engine (dibs_config.reserved_i[2] = n_chains must be > 1)");
  if (hp_check(e, c, pre + "chain index " + std::to_string(c) + " out of range (n_chains = " + std::to_string(e->B) + ")", hp,
               pre + "called after the particles were initialised (init_particles_batch / set_state / run): latent_prior_std enters the "
                     "initial draw and the device table is written once",
               pre + "chain " + std::to_string(c)))
    return 1;
  if (differs_from_config(e, *hp)) {
    if (e->cfg.likelihood != DIBS_LIK_LINGAUSS)
      return fail(pre + "chain " + std::to_string(c) + ": hyper-parameters that differ from the configuration's are LinearGaussian only (the "
                        "DenseNonlinearGaussian kernels have no per-chain form: its chains share every hyper-parameter)");
    if (!e->chain_hp_ok)
      return fail(pre + "chain " + std::to_string(c) + ": hyper-parameters that differ from the configuration's need n_vars <= 64 and n_dim <= 64 "
                        "(got " + std::to_string(e->d) + ", " + std::to_string(e->k) + ") and an acyclicity pipe other than bf16; this engine's "
                        "kernels take them as launch arguments of all chains");
    if (e->cdata.shared)
      return fail(pre + "chain " + std::to_string(c) + ": hyper-parameters that differ from the configuration's need per-chain data "
                        "(dibs_engine_set_data_problem for every chain), but this engine's chains share the data set given by dibs_engine_set_data");
  }
  e->hp_host[(size_t)c] = *hp;
  return 0;
}

extern "C" int dibs_engine_get_chain_hparams(dibs_engine* e, int32_t c, dibs_chain_hparams* hp) {
  const std::string pre = "chains engine (n_chains > 1): dibs_engine_get_chain_hparams: ";
  if (!e || !hp) return fail(pre + "null engine or argument");
  if (!e->chains) return fail(pre + "needs a chains engine (dibs_config.reserved_i[2] = n_chains must be > 1)");
  if (hp_check(e, c, pre + "chain index " + std::to_string(c) + " out of range (n_chains = " + std::to_string(e->B) + ")")) return 1;
  *hp = e->hp_host[(size_t)c];
  return 0;
}

// ---- edge-wise graph prior (include/dibs_hip.h, EDGE-WISE GRAPH PRIOR) --------------------------------------------------------------------
extern "C" int dibs_engine_set_edge_prior(dibs_engine* e, const double* edge_probs) {
  const std::string pre = "dibs_engine_set_edge_prior: ";
  if (!e || !edge_probs) return fail(pre + "null engine or argument");
  if (e->cfg.graph_prior != DIBS_PRIOR_EDGEWISE)
    return fail(pre + "this engine's graph prior is not edge-wise (dibs_config.graph_prior must be DIBS_PRIOR_EDGEWISE)");
  const int d = e->d;
  const size_t dd = (size_t)d * d;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      const double p = edge_probs[(size_t)i * d + j];
      if (i != j && !(p > 0.0 && p < 1.0)) {  // (NaN fails both comparisons)
        char buf[160];
        snprintf(buf, sizeof buf, "entry (%d, %d) = %g: every off-diagonal edge probability must be finite and strictly inside (0, 1)", i, j, p);
        return fail(pre + buf);
      }
    }
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));  // (the staging buffer of an earlier call is free; kernels of a step driven from outside are done)
  if (e->f64) e->edge_host64.resize(dd);
  else e->edge_host32.resize(dd);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      const double p = edge_probs[(size_t)i * d + j];
      const double l = i == j ? 0.0 : log(p) - log(1 - p);  // (er_log_odds)
      if (e->f64) e->edge_host64[(size_t)i * d + j] = l;
      else e->edge_host32[(size_t)i * d + j] = (float)l;
    }
  if (e->f64) {
    if (!e->edge_tab64) HIP_OK(hipMalloc((void**)&e->edge_tab64, dd * 8));  // (the copy below fills all of it)
    HIP_OK(hipMemcpyAsync(e->edge_tab64, e->edge_host64.data(), dd * 8, hipMemcpyHostToDevice, e->stream));
  } else {
    if (!e->edge_tab) HIP_OK(hipMalloc((void**)&e->edge_tab, dd * 4));
    HIP_OK(hipMemcpyAsync(e->edge_tab, e->edge_host32.data(), dd * 4, hipMemcpyHostToDevice, e->stream));
  }
  e->edge_tab_set = true;
  return 0;
}

int batch_hp_commit(dibs_engine* e) {
  if (e->hp_final) return 0;
  if (e->chains && e->cfg.graph_prior == DIBS_PRIOR_EDGEWISE && chains_hp_differ(e))
    return fail("chains engine (n_chains > 1): the edge-wise graph prior is not supported together with per-chain hyper-parameters that differ "
                "from the configuration's (dibs_engine_set_chain_hparams): the table-reading tail kernel has no edge-wise form, and per-problem "
                "tables are not built");
  std::vector<ProblemHP> tab((size_t)e->B);
  for (int p = 0; p < e->B; ++p) tab[(size_t)p] = derive_problem_hp(e, e->hp_host[(size_t)p]);
  HIP_OK(hipMemcpy(e->hp, tab.data(), tab.size() * sizeof(ProblemHP), hipMemcpyHostToDevice));
  e->hp_final = true;
  if (e->chains) {
    // the chains' tier: some chain's scalars differ from the configuration's -- step_multi takes the table-reading launches.  The
    // per-chain forms of the LinearGaussian kernels (per-chain data) read alpha and the baseline rate from the table either way
    e->hp_tier = chains_hp_differ(e);
    e->jw.chain_hp = e->hp;
  }
  std::vector<LinGramHost>().swap(e->cdata.gram);  // (chains engine, per-chain data: the data is final too -- the host copies of the Gram matrices go)
  return 0;
}

// kernels that may need more than the default 64 KiB of dynamic LDS (see launch.h).  One attribute call per (device, kernel) and size
// increase, not one per launch; the table is shared by every engine of the process, so it is keyed by device and guarded by a mutex
// (ctypes releases the GIL: two engines may be stepped from two host threads).
int dibs_cu_count() {
  static std::mutex mu;
  static std::map<int, int> cus;
  int dev = 0;
  hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  int& n = cus[dev];
  if (n == 0) {
    hipDeviceProp_t prop;
    n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return n;
}
void dibs_allow_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> granted;
  if (bytes <= 48 * 1024) return;
  int dev = 0;
  hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  size_t& g = granted[{dev, kernel}];
  if (bytes > g) {
    hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    g = bytes;
  }
}

void drain_timers(dibs_engine* e) {
  for (auto& pe : e->pending) {
    hipEventSynchronize(pe.second.second);
    float ms = 0.f;
    hipEventElapsedTime(&ms, pe.second.first, pe.second.second);
    e->t_ms[pe.first] += ms;
    e->t_n[pe.first] += 1;
    hipEventDestroy(pe.second.first);
    hipEventDestroy(pe.second.second);
  }
  e->pending.clear();
}

// does this chunk / call use the in-kernel flags?  Decided here, once per chunk (not per step): the tuning switch, an earlier time-out,
// the creation-time probe, and the engine being alone in its process (several engines share hardware queues: a polling kernel at the head
// of a shared queue holds up the kernels behind it, possibly the one it waits for)
void latch_flags(dibs_engine* e) {
  e->flags_now = !e->tune.no_flags && !e->flags_off && e->join_flag != nullptr && e->streams_concurrent &&
                 (e->tune.flags_multi || g_live_engines.load() == 1);
}

// after a chunk has been synchronised: did a kernel give up waiting for a flag (tail_join_wait / k_wait_flag)?  Clears the word.
unsigned int take_join_err(dibs_engine* e) {
  if (!e->join_err || !*e->join_err) return 0u;
  const unsigned int code = *e->join_err;
  *e->join_err = 0u;
  return code;
}
int join_failure(unsigned int code, const char* what) {
  return fail(std::string(code == 2u ? "internal: the edge kernel's completion flag did not arrive (k_wait_flag on the second stream timed out)"
                                     : "internal: the acyclicity stream's completion flag did not arrive (k_particle_grad timed out waiting)") + what);
}

// the steps of one chunk enqueued (step(t): 0 or 1 as every internal call), then both streams synchronised and the timers drained
template <typename Step>
static int run_chunk(dibs_engine* e, int t_start, int n_steps, Step step) {
  for (int t = t_start; t < t_start + n_steps; ++t) {
    if (step(t)) return 1;
    if (e->profiling && e->pending.size() > 4096) drain_timers(e);
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
  if (e->profiling) drain_timers(e);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int dibs_engine_run(dibs_engine* e, int32_t t_start, int32_t n_steps) {
  if (!e) return fail("null engine");
  if (e->B > 1 && !e->chains && !e->has_data) return fail("dibs_engine_set_data_problem has not been called for every problem");
  if (e->chains && !e->has_data && !e->cdata.set.empty()) {
    size_t c = 0;
    while (c < e->cdata.set.size() && e->cdata.set[c]) ++c;
    return fail("chains engine (n_chains > 1): dibs_engine_run: dibs_engine_set_data_problem has not been called for chain " + std::to_string(c) +
                " (per-chain data: every chain needs its own)");
  }
  if (e->chains && e->cdata.set.empty() && chains_hp_differ(e))  // (no data yet, or -- kept out by both setters -- one shared data set)
    return fail("chains engine (n_chains > 1): dibs_engine_run: some chain's hyper-parameters differ from the configuration's "
                "(dibs_engine_set_chain_hparams), which needs per-chain data: dibs_engine_set_data_problem has not been called for every chain");
  if (!e->has_data) return fail("dibs_engine_set_data has not been called");
  if (need_edge_prior(e)) return 1;
  if (e->B > 1) {  // (batched or chains engine)
    HIP_OK(hipSetDevice(e->cfg.device_id));
    if (batch_hp_commit(e)) return 1;
    return run_chunk(e, t_start, n_steps, [e](int t) { return step_multi(e, t); });
  }
  if (e->f64) {
    HIP_OK(hipSetDevice(e->cfg.device_id));
    return run_chunk(e, t_start, n_steps, [e](int t) { return step_f64(e, t); });
  }
  if (e->cfg.n_ranks != 1) return fail("dibs_engine_run is single-rank; use step_local / step_update");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  latch_flags(e);
  const bool guarded = e->flags_now && n_steps > 0;
  const auto step = [e](int t) { return step_local(e, t, packed_rows(e, e->pack)) || step_update(e, t, packed_source(e, e->pack)); };
  if (guarded && carry_copy(e, false)) return 1;  // (one launch per chunk: 10 MB at the headline size, ~4 us)
  if (run_chunk(e, t_start, n_steps, step)) return 1;
  unsigned int code = take_join_err(e);
  if (code && guarded) {
    // a polling kernel ran into its bound: its step, and every step behind it, used operands that were not complete.  Back to the
    // chunk's start, flags off for good, the same steps again on events.
    e->flags_off = true;
    ++e->flag_fallbacks;
    latch_flags(e);
    if (carry_copy(e, true)) return 1;
    if (run_chunk(e, t_start, n_steps, step)) return 1;
    code = take_join_err(e);
  }
  if (code) return join_failure(code, "; the results of this chunk are invalid");
  return 0;
}

extern "C" int dibs_engine_flag_fallbacks(const dibs_engine* e) { return e ? e->flag_fallbacks : -1; }
extern "C" int dibs_engine_debug_drop_next_flag(dibs_engine* e) {
  if (!e) return fail("null engine");
  e->debug_drop_flag = true;
  return 0;
}

// the device Threefry routines of rng.h on caller-given arguments (dibs_debug_threefry): thread i takes counter c0[i]
__global__ __launch_bounds__(256) void k_debug_threefry(Key2 key, uint32_t half, uint32_t off_b, const uint32_t* __restrict__ c0, int n,
                                                        uint32_t* __restrict__ out) {
  const TfKeys tk = tf_keys(key);
  half = tf_uniform(half);
  off_b = tf_uniform(off_b);
  for (int i = threadIdx.x; i < n; i += 256) {
    uint32_t s0, s1, a0, a1, b0, b1;
    threefry2x32_uh(tk, c0[i], 0u, half, s0, s1);
    threefry2x32_uh2(tk, c0[i], 0u, off_b, half, a0, a1, b0, b1);
    uint32_t* o = out + 6 * (size_t)i;
    o[0] = s0; o[1] = s1; o[2] = a0; o[3] = a1; o[4] = b0; o[5] = b1;
  }
}
extern "C" int dibs_debug_threefry(uint32_t k0, uint32_t k1, uint32_t half, uint32_t off_b, const uint32_t* c0, int32_t n, uint32_t* out) {
  if (!c0 || !out || n < 0) return fail("dibs_debug_threefry: null argument or negative n");
  if (n == 0) return 0;
  uint32_t *dc = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc(&dc, (size_t)n * 4));
  if (hipMalloc(&dout, (size_t)n * 24) != hipSuccess) {
    hipFree(dc);
    return fail("dibs_debug_threefry: hipMalloc failed");
  }
  hipError_t rc = hipMemcpy(dc, c0, (size_t)n * 4, hipMemcpyHostToDevice);
  if (rc == hipSuccess) {
    hipLaunchKernelGGL(k_debug_threefry, dim3(1), dim3(256), 0, 0, Key2{k0, k1}, half, off_b, dc, n, dout);
    rc = hipGetLastError();
  }
  if (rc == hipSuccess) rc = hipMemcpy(out, dout, (size_t)n * 24, hipMemcpyDeviceToHost);
  hipFree(dc);
  hipFree(dout);
  if (rc != hipSuccess) return fail(std::string("dibs_debug_threefry: ") + hipGetErrorString(rc));
  return 0;
}

extern "C" int64_t dibs_engine_gather_elems_per_rank(const dibs_engine* e) { return e ? (int64_t)e->Mloc * e->E : 0; }

extern "C" int dibs_engine_sync(dibs_engine* e) {
  if (!e) return fail("null engine");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->profiling) drain_timers(e);
  if (const unsigned int code = take_join_err(e)) {
    e->flags_off = true;  // (a loop driven step by step from outside cannot be repeated here: the caller's steps since the last sync are lost)
    return join_failure(code, "; the steps since the last dibs_engine_sync are invalid (the engine uses events from now on)");
  }
  return 0;
}

extern "C" int64_t dibs_engine_theta_size(const dibs_engine* e) { return e ? e->P : 0; }

struct BufInfo {
  const void* p;
  int64_t bytes;
};
static BufInfo buf_info(const dibs_engine* e, int which) {
  const int64_t Ml = e->Mloc, dd = (int64_t)e->d * e->d;
  if (const F64State* f = e->f64) {  // float64 engine: the float buffers in double (NODE_SCORES / PARENT_MASKS as below)
    switch (which) {
      case DIBS_BUF_Z: return {f->z, Ml * e->D * 8};
      case DIBS_BUF_V_Z: return {f->vz, Ml * e->D * 8};
      case DIBS_BUF_SCORES: return {f->scores, Ml * dd * 8};
      case DIBS_BUF_LOGPROBS_Z: return {f->logprobs, Ml * e->S * 8};
      case DIBS_BUF_W_LIK: return {f->w_lik, Ml * dd * 8};
      case DIBS_BUF_W_ACYC: return {f->w_acyc, Ml * dd * 8};
      case DIBS_BUF_GRAD_Z: return {f->gradz, Ml * e->D * 8};
      case DIBS_BUF_KXX: return {f->kxx, Ml * e->M * 8};
      case DIBS_BUF_PHI_Z: return {f->phi, Ml * e->D * 8};
      case DIBS_BUF_BASELINE: return {f->baseline, Ml * 8};
      case DIBS_BUF_NODE_SCORES: case DIBS_BUF_PARENT_MASKS: break;
      default: return {nullptr, -1};  // (theta, packed and gathered rows: the f32 engine's, which a float64 engine does not have)
    }
  }
  switch (which) {
    case DIBS_BUF_Z: return {e->z, Ml * e->D * 4};
    case DIBS_BUF_V_Z: return {e->vz, Ml * e->D * 4};
    case DIBS_BUF_THETA: return {e->theta, Ml * e->P * 4};
    case DIBS_BUF_V_THETA: return {e->vtheta, Ml * e->P * 4};
    case DIBS_BUF_SCORES: return {e->scores, Ml * dd * 4};
    case DIBS_BUF_LOGPROBS_Z: return {e->logprobs_z, Ml * e->S * 4};
    case DIBS_BUF_LOGPROBS_THETA: return {e->logprobs_th, Ml * e->S * 4};
    case DIBS_BUF_W_LIK: return {e->w_lik, Ml * dd * 4};
    case DIBS_BUF_W_ACYC: return {e->w_acyc, Ml * dd * 4};
    case DIBS_BUF_KXX: return {e->kz, Ml * e->M * 4};
    case DIBS_BUF_PHI_Z: return {e->phi_z, Ml * e->D * 4};
    case DIBS_BUF_PHI_THETA: return {e->phi_th, Ml * e->P * 4};
    case DIBS_BUF_BASELINE: return {e->baseline, Ml * 4};
    case DIBS_BUF_NODE_SCORES: return {e->node_scores, e->node_scores ? Ml * e->S * e->d * 8 : 0};
    case DIBS_BUF_PARENT_MASKS: return {e->masks, e->masks ? Ml * e->S * e->d * e->W * 8 : 0};
    case DIBS_BUF_GATHER: return {e->pack, (int64_t)(e->B > 1 ? e->Mloc : e->M) * e->E * 4};
    case DIBS_BUF_GRAD_Z: return {nullptr, Ml * e->D * 4};
    case DIBS_BUF_GRAD_THETA: return {nullptr, Ml * e->P * 4};
    case DIBS_BUF_PROBLEM_STEP: return {nullptr, e->B > 1 ? (int64_t)e->B * 8 : -1};  // (alpha, beta) out of the table's rows
    case DIBS_BUF_BANDWIDTH: return {nullptr, (int64_t)e->B * 8};  // (h_latent, h_theta) per run: configuration / table values, median segments from e->bw
    case DIBS_BUF_SQDIST_Z: return {e->sqd_z, e->sqd_z ? Ml * e->M * 4 : -2};  // (-2: the segment is not on the median rule)
    case DIBS_BUF_SQDIST_THETA: return {e->sqd_t, e->sqd_t ? Ml * e->M * 4 : -2};
    default: return {nullptr, -1};
  }
}

extern "C" int64_t dibs_engine_buffer_bytes(const dibs_engine* e, int32_t which) { return e ? buf_info(e, which).bytes : -1; }

extern "C" int dibs_engine_read_buffer(dibs_engine* e, int32_t which, void* host, int64_t nbytes) {
  if (!e || !host) return fail("null argument");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const BufInfo bi = buf_info(e, which);
  if (bi.bytes == -2) return fail("no such buffer (the squared distances exist only for a segment on the median bandwidth rule, dibs_config.reserved_i[3])");
  if (bi.bytes < 0) return fail(e->f64 ? "float64 engine: no such buffer (theta / packed / gathered rows belong to the float32 engine)" : "unknown buffer id");
  if (bi.bytes != nbytes) return fail("buffer size mismatch: expected " + std::to_string(bi.bytes) + " bytes");
  if (nbytes == 0) return 0;
  if (!e->f64 && (which == DIBS_BUF_GRAD_Z || which == DIBS_BUF_GRAD_THETA)) {  // strided rows of the packed buffer (single-rank engine buffer)
    const size_t off = which == DIBS_BUF_GRAD_Z ? (size_t)e->D : (size_t)(2 * e->D + e->P);
    const size_t w = which == DIBS_BUF_GRAD_Z ? (size_t)e->D * 4 : (size_t)e->P * 4;
    HIP_OK(hipMemcpy2D(host, w, e->pack + (size_t)e->m0 * e->E + off, (size_t)e->E * 4, w, e->Mloc, hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == DIBS_BUF_PROBLEM_STEP) {
    HIP_OK(hipMemcpy2D(host, 8, (const char*)e->hp + offsetof(ProblemHP, alpha), sizeof(ProblemHP), 8, (size_t)e->B, hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == DIBS_BUF_BANDWIDTH) {
    // fixed rule: the values the launches take (the configuration's, or a run's own: per-problem / per-chain hyper-parameters); a segment
    // on the median rule: what the selection of the last step wrote (zeros before the first step)
    float* out = (float*)host;
    for (int p = 0; p < e->B; ++p) {
      const bool own = !e->hp_host.empty();
      out[2 * p] = (float)(own ? e->hp_host[(size_t)p].h_latent : e->cfg.h_latent);
      out[2 * p + 1] = (float)(own ? e->hp_host[(size_t)p].h_theta : e->cfg.h_theta);
    }
    if (e->median_rule) {
      std::vector<float> dev((size_t)2 * e->B);
      HIP_OK(hipMemcpy(dev.data(), e->bw, dev.size() * 4, hipMemcpyDeviceToHost));
      for (int p = 0; p < e->B; ++p)
        for (int s = 0; s < 2; ++s)
          if (e->median_rule >> s & 1) out[2 * p + s] = dev[(size_t)2 * p + s];
    }
    return 0;
  }
  if (which == DIBS_BUF_KXX && e->kt) {  // kxx = k_z + k_theta
    std::vector<float> a((size_t)e->Mloc * e->M), b(a.size());
    HIP_OK(hipMemcpy(a.data(), e->kz, a.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data(), e->kt, a.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < a.size(); ++i) ((float*)host)[i] = a[i] + b[i];
    return 0;
  }
  HIP_OK(hipMemcpy(host, bi.p, nbytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int dibs_engine_set_profiling(dibs_engine* e, int32_t enable) {
  if (!e) return fail("null engine");
  hipStreamSynchronize(e->stream);
  drain_timers(e);
  e->profiling = enable != 0;
  e->profiling_concurrent = enable == 2;
  return 0;
}

extern "C" int dibs_engine_reset_timers(dibs_engine* e) {
  if (!e) return fail("null engine");
  hipStreamSynchronize(e->stream);
  drain_timers(e);
  for (int i = 0; i < DIBS_K_COUNT; ++i) {
    e->t_ms[i] = 0;
    e->t_n[i] = 0;
  }
  hipMemset(e->counters, 0, DIBS_N_COUNTERS * sizeof(unsigned long long));
  return 0;
}

extern "C" int dibs_engine_get_timers(dibs_engine* e, double* total_ms, int64_t* launches, int32_t n) {
  if (!e) return fail("null engine");
  hipStreamSynchronize(e->stream);
  drain_timers(e);
  for (int i = 0; i < n && i < DIBS_K_COUNT; ++i) {
    if (total_ms) total_ms[i] = e->t_ms[i];
    if (launches) launches[i] = e->t_n[i];
  }
  return 0;
}

extern "C" int dibs_engine_get_counters(dibs_engine* e, double* out, int32_t n) {
  if (!e || !out) return fail("null argument");
  HIP_OK(hipStreamSynchronize(e->stream));
  unsigned long long h[DIBS_N_COUNTERS];
  HIP_OK(hipMemcpy(h, e->counters, sizeof h, hipMemcpyDeviceToHost));
  for (int i = 0; i < n && i < DIBS_N_COUNTERS; ++i) out[i] = (double)h[i];
  return 0;
}
