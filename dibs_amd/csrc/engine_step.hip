// One SVGD step of the float32 engines (include/dibs_hip.h): the launch blocks, step_local / step_update (phases A and B, split at the
// exchange point), step_multi, and the entry points that drive them.  The kernels of kernels_marginal.h and kernels_tail.h are compiled here,
// and only here.
#define DIBS_TU_STEP
#include "kernels_marginal.h"
#include "engine_impl.h"

void launch_stream_probe(hipStream_t main_stream, hipStream_t second_stream, unsigned int* words) {
  hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, main_stream, words, words + 1);
  hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, second_stream, words);
}

extern "C" int dibs_engine_init_particles(dibs_engine* e, const uint32_t key[2]) {
  if (!e || !key) return fail("null argument");
  if (e->chains) return fail("chains engine (n_chains > 1): use dibs_engine_init_particles_batch (one key per chain)");
  if (e->B > 1) return fail("batched engine: use dibs_engine_init_particles_batch");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  const int L = e->cfg.rng_layout;
  const Key2 k0{key[0], key[1]};
  e->key = rng_split_row(k0, 2, 0, L);                     // key, subk = split(key)            svgd.py:294
  const Key2 subk = rng_split_row(k0, 2, 1, L);
  const Key2 ikey = rng_split_row(subk, 2, 0, L);          // key, subk = split(key)            svgd.py:145 / :509
  const Key2 isub = rng_split_row(subk, 2, 1, L);
  const uint64_t ntot = (uint64_t)e->M * e->D, nloc = (uint64_t)e->Mloc * e->D;
  if (e->f64) return f64_init_particles(e, isub);
  hipLaunchKernelGGL(k_init_z, dim3((unsigned)((nloc + 255) / 256)), dim3(256), 0, e->stream, e->z, isub, ntot,
                     (uint64_t)e->m0 * e->D, nloc, e->sigz, L);
  if (e->cfg.joint) {
    const Key2 tsub = rng_split_row(ikey, 2, 1, L);        // key, subk = split(key); sample_parameters(key=subk)  svgd.py:512-513
    if (e->cfg.likelihood == DIBS_LIK_LINGAUSS) {
      const uint64_t tt = (uint64_t)e->M * e->P, tl = (uint64_t)e->Mloc * e->P;
      hipLaunchKernelGGL(k_init_theta_lin, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, e->stream, e->theta, tsub, tt,
                         (uint64_t)e->m0 * e->P, tl, (float)e->cfg.lin_mean_edge, (float)e->cfg.lin_sig_edge,
                         (float)e->cfg.lin_min_edge, L);
    } else if (e->cfg.likelihood == DIBS_LIK_DENSENN) {
      const NNParams np_ = nn_params(e->cfg);
      joint_nn_init_theta(e->theta, (size_t)e->P, tsub, e->m0, e->Mloc, e->M, e->d, np_, L, e->stream);
    } else {
      return fail("sample_parameters not implemented for this likelihood");
    }
  }
  e->kmat_ext = false;  // (a kernel slab computed by dibs_engine_kmat_values belonged to the particles that were just replaced)
  e->vals_fresh = false;
  HIP_OK(hipMemsetAsync(e->vz, 0, (size_t)e->Mloc * e->D * 4, e->stream));
  if (e->P) HIP_OK(hipMemsetAsync(e->vtheta, 0, (size_t)e->Mloc * e->P * 4, e->stream));
  HIP_OK(hipMemsetAsync(e->baseline, 0, (size_t)e->Mloc * 4, e->stream));
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int dibs_engine_init_particles_batch(dibs_engine* e, const uint32_t* keys) {
  if (need_batch(e)) return 1;
  if (!keys) return fail("null argument");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (batch_hp_commit(e)) return 1;  // (the per-problem values are final from here on: latent_prior_std enters the draw below)
  const int L = e->cfg.rng_layout;
  std::vector<Key2> carry((size_t)e->B);
  const uint64_t n = (uint64_t)e->M * e->D;
  for (int p = 0; p < e->B; ++p) {  // per problem exactly dibs_engine_init_particles(keys[p]) of a standalone engine
    const Key2 k0{keys[2 * p], keys[2 * p + 1]};
    carry[p] = rng_split_row(k0, 2, 0, L);
    const Key2 subk = rng_split_row(k0, 2, 1, L);
    const Key2 isub = rng_split_row(subk, 2, 1, L);
    hipLaunchKernelGGL(k_init_z, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->z + (size_t)p * n, isub, n, (uint64_t)0, n,
                       latent_sigma(e->hp_host[(size_t)p].latent_prior_std, e->k), L);
    if (e->chains) {  // (chain p's parameters: the launch of dibs_engine_init_particles for a joint model, rows p M .. p M + M - 1)
      const Key2 ikey = rng_split_row(subk, 2, 0, L);
      const Key2 tsub = rng_split_row(ikey, 2, 1, L);
      float* const th = e->theta + (size_t)p * e->M * e->P;
      if (e->cfg.likelihood == DIBS_LIK_LINGAUSS) {
        const uint64_t tt = (uint64_t)e->M * e->P;
        hipLaunchKernelGGL(k_init_theta_lin, dim3((unsigned)((tt + 255) / 256)), dim3(256), 0, e->stream, th, tsub, tt, (uint64_t)0, tt,
                           (float)e->cfg.lin_mean_edge, (float)e->cfg.lin_sig_edge, (float)e->cfg.lin_min_edge, L);
      } else {
        joint_nn_init_theta(th, (size_t)e->P, tsub, 0, e->M, e->M, e->d, nn_params(e->cfg), L, e->stream);
      }
    }
  }
  HIP_OK(hipMemcpyAsync(e->bcarry, carry.data(), carry.size() * sizeof(Key2), hipMemcpyHostToDevice, e->stream));
  HIP_OK(hipMemsetAsync(e->vz, 0, (size_t)e->Mloc * e->D * 4, e->stream));
  if (e->chains) HIP_OK(hipMemsetAsync(e->vtheta, 0, (size_t)e->Mloc * e->P * 4, e->stream));
  HIP_OK(hipMemsetAsync(e->baseline, 0, (size_t)e->Mloc * 4, e->stream));
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

// the matrix-power launch of the acyclicity term; while profiling, a single-kernel launch is stamped by the launch itself (kernel start /
// end, what rocprofv3 reports) instead of an event pair around it, which on the second stream also times ~7 us of dispatch latency
static void acyc_power_timed(dibs_engine* e, AcycLaunch al, hipStream_t st) {
  if (e->profiling && acyc_power_takes_events(al)) {
    hipEventCreate(&al.ev_start);
    hipEventCreate(&al.ev_stop);
    acyc_launch_power(al);
    e->pending.push_back({DIBS_K_ACYC, {al.ev_start, al.ev_stop}});
    return;
  }
  KTimer tm(e, DIBS_K_ACYC, st);
  acyc_launch_power(al);
}

static bool kmat_tiled_on(const dibs_engine* e) { return kmat_tiled_on(e->kmat_ns_max, e->M, e->tune.kmat_tiled_min); }  // (step_plan.h)
// rows of all M particles at x + m * stride + off (len floats); this engine's slab [Mloc][M] (symmetric when it holds every particle)
static void kmat_launch_tiled(dibs_engine* e, hipStream_t st, const float* x, size_t stride, size_t off, size_t len, float* kout, float scale, float h,
                              const float* kadd, float* ksum) {
  const int sym = e->Mloc == e->M;
  // many particles: 64 x 64 tiles (half the bytes per pair; entries bit-identical to the 32 x 32 kernel's) -- from 512 particles, where
  // there are enough of them for every CU (DibsTuning::kmat_t64_min)
  if (e->M >= e->tune.kmat_t64_min && kmat_tile64_ok(x, stride, off, len)) {
    const int nta = (e->Mloc + KT2_T - 1) / KT2_T, ntb = (e->M + KT2_T - 1) / KT2_T, tiles = kmat_tile_count(nta, ntb, sym);
    const int nchunk = kmat_nchunk64((int)len), ns = kmat_pick_nsplit(tiles, nchunk, e->kmat_ns_max), cps = (nchunk + ns - 1) / ns;
    const KmatTile kt{x, stride, off, (int)len, e->kpart, e->m0, e->Mloc, e->M, nchunk, nta, ntb, sym, ns, cps, scale, h, kout, kadd, ksum, nullptr};
    dibs_allow_lds((const void*)k_kmat_tile64, kmat_tile64_lds_bytes());
    const int units = tiles * ns;
    hipLaunchKernelGGL(k_kmat_tile64, dim3((unsigned)(units < 256 ? units : 256)), dim3(KT2_NT), kmat_tile64_lds_bytes(), st, kt);
    if (ns > 1)
      hipLaunchKernelGGL(k_kmat_finish, dim3(e->Mloc), dim3(256), 0, st, (const double*)e->kpart, ns, e->Mloc, e->M, sym, scale, h, kout, kadd, ksum, KT2_T);
    return;
  }
  const int nta = (e->Mloc + KT_T - 1) / KT_T, ntb = (e->M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, ntb, sym);
  const int nchunk = kmat_nchunk((int)len), ns = kmat_pick_nsplit(tiles, nchunk, e->kmat_ns_max), cps = (nchunk + ns - 1) / ns;
  const KmatTile kt{x, stride, off, (int)len, e->kpart, e->m0, e->Mloc, e->M, nchunk, nta, ntb, sym, ns, cps, scale, h, kout, kadd, ksum, nullptr};
  dibs_allow_lds((const void*)k_kmat_tile, kmat_tile_lds_bytes());
  // (persistent blocks, one per CU by their registers, looping over the units with the next step's rows prefetched)
  const int units = tiles * ns;
  hipLaunchKernelGGL(k_kmat_tile, dim3((unsigned)(units < 256 ? units : 256)), dim3(KT_NT), kmat_tile_lds_bytes(), st, kt);
  if (ns > 1) hipLaunchKernelGGL(k_kmat_finish, dim3(e->Mloc), dim3(256), 0, st, (const double*)e->kpart, ns, e->Mloc, e->M, sym, scale, h, kout, kadd, ksum, KT_T);
}

// ---- one SVGD step, split at the exchange point ----------------------------------------------
// ---- the launch blocks that the steps share ---------------------------------------------------------------------------------------------
// the matrix powers of the acyclicity term and their reduction on `st`, keys from `carry` (Mg: see step_local)
static void launch_acyc(dibs_engine* e, hipStream_t st, Key2 carry, int Mg, float alpha) {
  const dibs_config& c = e->cfg;
  const AcycLaunch al{st, e->scores, e->acyc_part, e->w_acyc, e->acyc_big, carry, e->m0, Mg, e->Mloc, e->d, e->Sa, e->acyc_units,
                      e->acyc_paired, alpha, (float)c.tau, c.rng_layout, c.logistic_minval_tiny, nullptr, nullptr, e->eas, e->tune.acyc_pipe,
                      e->tune.acyc_hfw_max};
  acyc_power_timed(e, al, st);
  KTimer tm(e, DIBS_K_ACYC_REDUCE, st);
  acyc_launch_reduce(al);
}

// How the edge-score launch tells the second stream that the scores are there: not at all (stream order, or an event recorded behind it), by
// the launch's own completion signal (hipExtLaunchKernelGGL stop event), or by a sequence number that k_edge_scores_p's last block publishes
// (++e->fork_seq -> e->fork_flag; needs edge_one_block).  At most one of the two (ForkKind::StopEvent / FlagFromEdge, step_plan.h).
struct EdgeFork {
  hipEvent_t stop_ev = nullptr;
  bool publish = false;
};
static bool edge_one_block(const dibs_engine* e) { return edge_one_block(e->d, e->k, e->edge_kc, e->ldk); }  // (step_plan.h)
// counters: phase time stamps of the tiled kernel while profiling, else null (a stop event is never given while profiling)
static void launch_edge_scores(dibs_engine* e, hipStream_t st, float alpha, const EdgeFork& fk, unsigned long long* counters) {
  KTimer tm(e, DIBS_K_EDGE, st);
  const size_t lds = (size_t)2 * e->dpad * e->ldk * 4;
  if (edge_one_block(e)) {
    allow_lds(k_edge_scores_p, lds);
    unsigned int* const none = nullptr;
    unsigned int *const ctr = fk.publish ? e->fork_flag + 1 : none, *const flag = fk.publish ? e->fork_flag : none;
    const unsigned int seq = fk.publish ? ++e->fork_seq : 0u;
    if (fk.stop_ev)
      hipExtLaunchKernelGGL(k_edge_scores_p, dim3(e->Mloc), dim3(1024), lds, st, nullptr, fk.stop_ev, 0, e->z, e->scores, e->thr, e->probs,
                            e->eas, alpha, e->d, e->k, e->dpad, e->ldk, ctr, flag, seq);
    else
      hipLaunchKernelGGL(k_edge_scores_p, dim3(e->Mloc), dim3(1024), lds, st, e->z, e->scores, e->thr, e->probs, e->eas, alpha, e->d,
                         e->k, e->dpad, e->ldk, ctr, flag, seq);
    return;
  }
  const int ntile = (e->dpad / 16) * (e->dpad / 16);
  int nby = ntile >= 16 ? 4 : (ntile >= 8 ? 2 : 1);
  while (4 * nby * EDGE_MAXT < ntile) nby *= 2;  // (a wave keeps the accumulators of at most EDGE_MAXT tiles)
  const int per_wave = (ntile + 4 * nby - 1) / (4 * nby);
#define EDGE_LAUNCH(MAXT_)                                                                                                             \
  {                                                                                                                                    \
    allow_lds(k_edge_scores<MAXT_>, lds);                                                                                              \
    if (fk.stop_ev)                                                                                                                    \
      hipExtLaunchKernelGGL(k_edge_scores<MAXT_>, dim3(e->Mloc, nby), dim3(256), lds, st, nullptr, fk.stop_ev, 0, e->z, e->scores,     \
                            e->thr, e->probs, e->eas, alpha, e->d, e->k, e->dpad, e->ldk, e->edge_kc, counters);                       \
    else                                                                                                                               \
      hipLaunchKernelGGL(k_edge_scores<MAXT_>, dim3(e->Mloc, nby), dim3(256), lds, st, e->z, e->scores, e->thr, e->probs, e->eas,      \
                         alpha, e->d, e->k, e->dpad, e->ldk, e->edge_kc, counters);                                                    \
  }
  if (per_wave <= 1) EDGE_LAUNCH(1) else if (per_wave <= 4) EDGE_LAUNCH(4) else EDGE_LAUNCH(EDGE_MAXT)
#undef EDGE_LAUNCH
}

// rows of all M particles: particle m's vector at base + m * stride + off
struct KmatRows {
  const float* base;
  size_t stride, off;
};
static size_t kmat_lds_bytes(size_t len) { return (size_t)(((len < KMAT_CH ? len : (size_t)KMAT_CH) + 3) & ~(size_t)3) * 4; }
static bool multi_kmat_tiled(const dibs_engine* e);  // (below, with the multi-run steps)
// Median-rule bandwidth (dibs_config.reserved_i[3]; kernels and launchers in tu_batch.hip): on `st`, in front of the kernel matrices, the
// squared distances of every segment on the rule and the selection that writes h / h_theta of every run's table row and e->bw.  Reads
// e->z / e->theta, which are final when a step starts and are what the packed rows of phase B hold (one rank).  e->B runs: 1 = a
// standalone engine with its one-row table
static void launch_bandwidth(dibs_engine* e, hipStream_t st) {
  KTimer tm(e, DIBS_K_BANDWIDTH, st);
  const bool tiled = multi_kmat_tiled(e);
  if (e->median_rule & 1) bandwidth_launch_sqdist(st, tiled, e->z, (size_t)e->D, e->sqd_z, e->B, e->M, kmat_lds_bytes((size_t)e->D));
  if (e->median_rule & 2) bandwidth_launch_sqdist(st, tiled, e->theta, (size_t)e->P, e->sqd_t, e->B, e->M, kmat_lds_bytes((size_t)e->P));
  bandwidth_launch_select(st, e->sqd_z, e->sqd_t, e->median_rule, e->B, e->M, e->hp, e->bw);
}
// This engine's kernel-matrix slab(s) on `st`: the latent one, then for the joint models theta's with kz / ksum.
// tiled (kernels_kmat.h: partial sums per 32 x 32 tile and chunk, then one finishing block per row) from 128 particles: config 4 597 ->
// 645 steps/s, config 5 108.5 -> 115, config 3 2290 -> 2328 on the same box (each row is read once per tile instead of once per pair)
static void launch_kmat(dibs_engine* e, hipStream_t st, const KmatRows& z, const KmatRows& th) {
  const dibs_config& c = e->cfg;
  if (e->median_rule) {
    // median rule (launch_bandwidth has run on `st`): the table-reading forms of the chains engine with ONE run -- the same block
    // functions, the bandwidth from the engine's one-row table; rows from e->z / e->theta (see launch_bandwidth)
    const bool tiled = multi_kmat_tiled(e);
    chains_launch_kmat_hp(st, tiled, e->z, (size_t)e->D, e->kz, 1, e->M, (float)c.scale_latent, e->hp, 0, nullptr, nullptr, kmat_lds_bytes((size_t)e->D));
    if (c.joint)
      chains_launch_kmat_hp(st, tiled, e->theta, (size_t)e->P, e->kt, 1, e->M, (float)c.scale_theta, e->hp, 1, e->kz, e->ksum,
                            kmat_lds_bytes((size_t)e->P));
    return;
  }
  if (kmat_tiled_on(e)) {
    kmat_launch_tiled(e, st, z.base, z.stride, z.off, (size_t)e->D, e->kz, (float)c.scale_latent, (float)c.h_latent, nullptr, nullptr);
    if (c.joint) kmat_launch_tiled(e, st, th.base, th.stride, th.off, (size_t)e->P, e->kt, (float)c.scale_theta, (float)c.h_theta, e->kz, e->ksum);
    return;
  }
  const int ksym = e->Mloc == e->M;  // single rank: the slab is the whole (symmetric) matrix
  allow_lds(k_kmat, kmat_lds_bytes(e->D > e->P ? e->D : e->P));
  const dim3 kg(e->Mloc, (e->M + KMAT_BT - 1) / KMAT_BT);
  hipLaunchKernelGGL(k_kmat, kg, dim3(256), kmat_lds_bytes(e->D), st, z.base, z.stride, z.off, (int)e->D, e->kz, e->m0, e->M,
                     (float)c.scale_latent, (float)c.h_latent, ksym, (const float*)nullptr, (float*)nullptr);
  if (c.joint)
    hipLaunchKernelGGL(k_kmat, kg, dim3(256), kmat_lds_bytes(e->P), st, th.base, th.stride, th.off, (int)e->P, e->kt, e->m0, e->M,
                       (float)c.scale_theta, (float)c.h_theta, ksym, (const float*)e->kz, e->ksum);
}

// the launch arguments of the joint models' estimators (joint_launch.h); LinearGaussian sets its three prior floats afterwards
static JointLaunch joint_launch_args(dibs_engine* e, const RowTarget& rt, int Mg, float alpha) {
  const dibs_config& c = e->cfg;
  return JointLaunch{e->stream, e->z, e->theta, e->scores, e->thr, e->w_lik, e->logprobs_z, e->logprobs_th, e->baseline,
                     e->baseline2, rt.base, rt.stride, rt.th_off, rt.gth_off, rt.copy_vals, e->m0, Mg, e->Mloc, e->d,
                     e->N, e->S, alpha, (float)c.tau, c.rng_layout, c.logistic_minval_tiny, c.grad_estimator_z, c.score_function_baseline,
                     0.f, 0.f, 0.f, e->tune.lin_f32, e->tune.nn_f32};
}

// The estimators of a joint model (LinearGaussian / DenseNonlinearGaussian) on the main stream: two timed launches per family.  M_choice:
// JointLaunch::M_choice (0: a standalone engine); msg_pre / msg_post: what surrounds the model's name in the message of a failed scratch
// allocation; swap_baselines: the updated score-function baselines become the loop's.
static int launch_joint_estimators(dibs_engine* e, const RowTarget& rt, int Mg, float alpha, Key2 carry_theta, Key2 carry_lik, int M_choice,
                                   const char* msg_pre, const char* msg_post, bool swap_baselines) {
  const dibs_config& c = e->cfg;
  JointLaunch jl = joint_launch_args(e, rt, Mg, alpha);
  jl.M_choice = M_choice;
  if (c.likelihood == DIBS_LIK_LINGAUSS) {
    jl.obs_noise = (float)c.lin_obs_noise;
    jl.mean_edge = (float)c.lin_mean_edge;
    jl.sig_edge = (float)c.lin_sig_edge;
    {
      KTimer tm(e, DIBS_K_LIN_THETA);  // ("lin_logprobs": both log-prob launches)
      if (joint_lin_all_logprobs(&e->jw, jl, carry_theta, carry_lik)) return fail(std::string(msg_pre) + "LinearGaussian" + msg_post);
    }
    {
      KTimer tm(e, DIBS_K_LIN_Z);      // ("lin_grad": the theta and the Z estimator in one launch)
      if (joint_lin_all_grads(&e->jw, jl, carry_theta, carry_lik)) return fail(std::string(msg_pre) + "LinearGaussian" + msg_post);
    }
  } else {  // DIBS_LIK_DENSENN: the callers are joint models, and dibs_engine_create admits these two likelihoods only
    const NNParams np_ = nn_params(c);
    {
      KTimer tm(e, DIBS_K_NN_THETA);
      if (joint_nn_dispatch(&e->jw, jl, carry_theta, LIN_MODE_THETA, np_, (size_t)e->P))
        return fail(std::string(msg_pre) + "DenseNonlinearGaussian" + msg_post);
    }
    {
      KTimer tm(e, DIBS_K_NN_Z);
      if (joint_nn_dispatch(&e->jw, jl, carry_lik, c.grad_estimator_z == 0 ? LIN_MODE_Z_SCORE : LIN_MODE_Z_REPARAM, np_, (size_t)e->P))
        return fail(std::string(msg_pre) + "DenseNonlinearGaussian" + msg_post);
    }
  }
  if (swap_baselines) std::swap(e->baseline, e->baseline2);
  return 0;
}

// what differs between the tail launches of the steps
struct TailOpts {
  float alpha, beta;
  bool score_lik;   // BGe with the score estimator: softmax weights, W_lik and the baseline are part of the kernel
  bool do_prior;    // false: beta = 0, no graph prior, no Gaussian term
  float* w_lik;     // W_lik: output (score_lik) or input -- the estimator's, or zeros when only the prior part is wanted
  bool flag_join;   // the kernel polls e->join_flag for e->join_seq itself (tail_join_wait)
  unsigned long long* counters;  // profiling: phase time stamps; null in production
  int ns = 0, cps = 0, nrider = 0;  // ns > 1: the latent kernel matrix as nrider blocks of tile units riding in the launch (TailArgs::kt;
                                    // the split of KmatPlace::InTail, step_plan.h)
};
// one block per particle: (score estimator: softmax weights -> W_lik,) total score-space gradient, back-projection, packed row
static void launch_tail(dibs_engine* e, const RowTarget& rt, const TailOpts& o) {
  const dibs_config& c = e->cfg;
  KTimer tm(e, DIBS_K_TAIL);
  const float er_c = (float)er_log_odds(c);
  // (w_tot != null: W, U, V of a particle do not fit in one block's LDS -- phases A, B here, the back-projection in k_backproject_big)
  // (terms: without the prior part beta = 0, no graph prior, no Gaussian term; without the likelihood part a zero W_lik is the input)
  const float inv_sig2 = o.do_prior ? 1.0f / (e->sigz * e->sigz) : 0.f;
  const int ldz = e->w_tot ? 0 : tail_ldz(e->d, e->k, e->S, o.score_lik, LDS_LIMIT - 2048);
  const int cap = o.score_lik ? tail_stage_cap(e->d, ldz, e->S, e->W, LDS_LIMIT - 2048) : 0;
  const size_t lds = tail_lds_bytes(e->d, ldz, e->S, e->W, o.score_lik, cap);
  TailArgs ta{o.score_lik ? e->node_scores : nullptr, e->masks, e->logprobs_z, e->baseline, e->baseline2, c.score_function_baseline,
              o.score_lik ? e->bq.counts : nullptr, e->S, e->W, cap, e->probs, o.w_lik, e->w_acyc, o.alpha,
              o.do_prior ? o.beta : 0.f, o.do_prior ? c.graph_prior : (int)DIBS_PRIOR_UNIFORM, er_c,
              e->z, rt.base, rt.stride, rt.copy_vals, e->m0, e->d, e->k, ldz, inv_sig2, o.counters,
              e->w_tot, o.flag_join ? e->join_flag : nullptr, e->join_seq, e->join_err, e->Mloc,
              KmatTile{nullptr, 0, 0, 0, nullptr, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr}};
  size_t lds_g = lds;
  if (o.ns > 1) {
    const int nta = (e->M + KT_T - 1) / KT_T, nchunk = kmat_nchunk((int)e->D);
    ta.kt = KmatTile{e->z, (size_t)e->D, 0, (int)e->D, e->kpart, 0, e->Mloc, e->M, nchunk, nta, nta, 1, o.ns, o.cps, (float)c.scale_latent,
                     (float)c.h_latent, e->kz, nullptr, nullptr, e->kmat_ctr};
    lds_g = lds > kmat_tile_lds_bytes() ? lds : kmat_tile_lds_bytes();
  }
  if (ta.prior_kind == DIBS_PRIOR_EDGEWISE) {  // (the table exists: need_edge_prior at every entry point)
    edge_launch_tail(e->stream, ta, e->edge_tab, e->Mloc + o.nrider, lds_g);
  } else {
    allow_lds(k_particle_grad, lds_g);
    hipLaunchKernelGGL(k_particle_grad, dim3(e->Mloc + o.nrider), dim3(TAIL_NT), lds_g, e->stream, ta);
  }
  if (e->w_tot) {
    const size_t lb = backproject_big_lds(e->d);
    allow_lds(k_backproject_big, lb);
    hipLaunchKernelGGL(k_backproject_big, dim3(e->Mloc, (e->d + 15) / 16, (e->k + 31) / 32), dim3(256), lb, e->stream, e->w_tot, e->z, rt.base, rt.stride,
                       rt.copy_vals, e->m0, e->d, e->k, inv_sig2);
  }
}

// one segment (z or theta) of the SVGD transform + optimizer step
struct PhiSeg {
  size_t val_off, grad_off, len;
  int is_theta;
  float *x, *v, *phi_out;
  float h;
};
// bandwidth and step-size arguments of a k_phi_update launch: the scalars, or for a batched engine its per-problem table and nothing
template <bool BATCH>
static PhiBandwidthArg<BATCH> phi_h_arg(const dibs_engine* e, float h) {
  if constexpr (BATCH) return e->hp;
  else return h;
}
template <bool BATCH>
static PhiStepArg<BATCH> phi_step_arg(const dibs_engine* e) {
  if constexpr (BATCH) return 0;
  else return (float)e->cfg.stepsize;
}
// k_phi_update over `rows` particles per problem (a batched engine: grid.y = problem, the BATCH instantiation, each problem exactly a
// standalone launch); rows of all particles at pack + m * stride; vals_send / vals_stride: the overlapped exchange's copy of the new values
static void launch_phi_update(dibs_engine* e, const float* pack, size_t stride, const PhiSeg& s, int rows, float* vals_send, size_t vals_stride) {
  const dibs_config& c = e->cfg;
  // particles per block: as many as keep >= 1024 blocks in flight and the tables within the LDS budget
  // (headline size: TA = 16 / 8 / 4 measured 20.5 / 18.9 / 26.0 us)
  const long cols = (long)((s.len + 63) / 64);
  int ta = 16;
  while (ta > 4 && (cols * ((rows + ta - 1) / ta) < 1024 || phi_update_lds_bytes(ta, e->M) > 56 * 1024)) ta >>= 1;
  const size_t lds = phi_update_lds_bytes(ta, e->M);
  const int ngroups = (rows + ta - 1) / ta;
  const dim3 g((unsigned)(8 * ngroups * ((cols + 7) / 8)), (unsigned)e->B);
  // joint models: the weights are kz + kt (e->ksum, formed by the k_kmat launch of kt), the repulsion uses the segment's own matrix
  const float* const kw = e->kt ? e->ksum : e->kz;
  const float* const kseg = e->kt ? (s.is_theta ? e->kt : e->kz) : nullptr;
  // FULL: whole 8-pair batches per wave and whole particle groups (no clamps inside the kernel)
  // (the table forms: multi-run engines, and a standalone engine whose bandwidth the median rule writes into its one-row table -- grid.y = 1)
  const bool table = e->B > 1 || e->median_rule != 0;
  const bool full = e->M % 64 == 0 && rows % ta == 0 && (size_t)e->M * stride * 4 < ((size_t)1 << 32);  // (32-bit buffer offsets)
#define PHI_LAUNCH(TA_, F_, J_, B_)                                                                                                        \
  {                                                                                                                                        \
    allow_lds(k_phi_update<TA_, F_, J_, B_>, lds);                                                                                         \
    hipLaunchKernelGGL((k_phi_update<TA_, F_, J_, B_>), g, dim3(256), lds, e->stream, pack, stride, s.val_off, s.grad_off, (int)s.len, kw,  \
                       kseg, s.is_theta, s.x, s.v, s.phi_out, e->m0, rows, e->M, phi_h_arg<B_>(e, s.h), phi_step_arg<B_>(e),               \
                       c.optimizer == DIBS_OPT_RMSPROP,                                                                                    \
                       (int)cols, ngroups, vals_send, vals_stride, s.is_theta ? (size_t)e->D : (size_t)0);                                 \
  }
#define PHI_PICK(TA_)                                                                                                                      \
  if (table && e->kt) { if (full) PHI_LAUNCH(TA_, true, true, true) else PHI_LAUNCH(TA_, false, true, true) }                              \
  else if (table) { if (full) PHI_LAUNCH(TA_, true, false, true) else PHI_LAUNCH(TA_, false, false, true) }                                \
  else if (e->kt) { if (full) PHI_LAUNCH(TA_, true, true, false) else PHI_LAUNCH(TA_, false, true, false) }                                \
  else { if (full) PHI_LAUNCH(TA_, true, false, false) else PHI_LAUNCH(TA_, false, false, false) }
  if (ta == 16) { PHI_PICK(16) } else if (ta == 8) { PHI_PICK(8) } else { PHI_PICK(4) }
#undef PHI_PICK
#undef PHI_LAUNCH
}

// (rng.h: rng_explicit_row) the carry slot carries the address of the key of GLOBAL particle 0
static Key2 key_array_as_carry(const Key2* local, int m0) {
  const uint64_t p = (uint64_t)(uintptr_t)(local - m0);
  return Key2{(uint32_t)p, (uint32_t)(p >> 32)};
}

// what plan_step reads of the engine (step_plan.h)
static StepFacts step_facts(const dibs_engine* e, bool xk, int terms) {
  const dibs_config& c = e->cfg;
  StepFacts f;
  f.joint = c.joint != 0;
  f.likelihood = c.likelihood;
  f.estimator = c.grad_estimator_z;
  f.d = e->d;
  f.k = e->k;
  f.M = e->M;
  f.Mloc = e->Mloc;
  f.D = e->D;
  f.S = e->S;
  f.edge_kc = e->edge_kc;
  f.ldk = e->ldk;
  f.stream2 = e->stream2 != nullptr;
  f.profiling = e->profiling;
  f.profiling_concurrent = e->profiling_concurrent;
  f.flags_now = e->flags_now;
  f.fork_flag = e->fork_flag != nullptr;
  f.kmat_ns_max = e->kmat_ns_max;
  f.kmat_ctr = e->kmat_ctr != nullptr;
  f.w_tot = e->w_tot != nullptr;
  f.kmat_ext = e->kmat_ext;
  f.xk = xk;
  f.terms = terms;
  f.kmat_tiled_min = e->tune.kmat_tiled_min;
  f.no_kmat_fuse = e->tune.no_kmat_fuse;
  f.no_kmat_grad = e->tune.no_kmat_grad;
  f.median_h = e->median_rule != 0;
  return f;
}

// xk == null: the step of the SVGD loop (keys from the loop-carry key, which advances).  xk != null: the same kernels with the caller's
// per-particle keys, the loop-carry key untouched; `terms` selects the likelihood part (estimators + their share of grad_z), the prior
// part (acyclicity, Gaussian and graph prior), or both.
int step_local(dibs_engine* e, int t, const RowTarget& rt, const StepKeys* xk, int terms, const float* zero_w) {
  const dibs_config& c = e->cfg;
  const float alpha = (float)(c.alpha_linear * t), beta = (float)(c.beta_linear * t);
  const int L = c.rng_layout;
  Key2 carry_theta{0, 0}, carry_lik, carry_prior;
  int Mg = e->M;  // particle count of the key derivation (row 1 + m of split(carry, M + 1)); -1: explicit keys
  if (xk) {
    Mg = -1;
    carry_theta = key_array_as_carry(xk->theta, e->m0);
    carry_lik = key_array_as_carry(xk->lik, e->m0);
    carry_prior = key_array_as_carry(xk->prior, e->m0);
  } else {
    Key2 carry = e->key;
    if (c.joint) {
      carry_theta = carry;
      carry = next_carry(e, carry);
    }
    carry_lik = carry;
    carry = next_carry(e, carry);
    carry_prior = carry;
    carry = next_carry(e, carry);
    e->key = carry;
  }
  // every decision of the step's schedule, before the first launch (step_plan.h has the reasons and the measurements)
  const StepPlan plan = plan_step(step_facts(e, xk != nullptr, terms));
  const bool fork = plan.fork != ForkKind::None, flag_fork = plan.fork == ForkKind::FlagFromEdge || plan.fork == ForkKind::FlagFromSample;
  const bool score_lik = plan.score_lik;
  e->kmat_place = plan.place;

  EdgeFork ef;
  if (plan.fork == ForkKind::FlagFromSample) ++e->fork_seq;        // (the edge kernel publishes nothing: k_bge_sample's first block does, below)
  else if (plan.fork == ForkKind::FlagFromEdge) ef.publish = true;  // (the last block publishes fork_seq: k_wait_flag on the second stream)
  else if (plan.fork == ForkKind::StopEvent) ef.stop_ev = e->ev_fork;
  launch_edge_scores(e, e->stream, alpha, ef, e->profiling ? e->counters + 8 : nullptr);
  if (fork) {
    if (flag_fork) {
      hipLaunchKernelGGL(k_wait_flag, dim3(1), dim3(64), 0, e->stream2, (const unsigned int*)e->fork_flag, e->fork_seq, 0u, e->join_err);
    } else {
      if (plan.fork == ForkKind::Event) hipEventRecord(e->ev_fork, e->stream);
      hipStreamWaitEvent(e->stream2, e->ev_fork, 0);
    }
    launch_acyc(e, e->stream2, carry_prior, Mg, alpha);
  }
  if (plan.place == KmatPlace::Stream2) {
    if (plan.join == JoinKind::EventAtOnce) {  // per-kernel timing: one kernel at a time
      hipEventRecord(e->ev_k1, e->stream2);
      hipStreamWaitEvent(e->stream, e->ev_k1, 0);
      hipEventRecord(e->ev_k0, e->stream);
      hipStreamWaitEvent(e->stream2, e->ev_k0, 0);
    }
    if (e->median_rule) launch_bandwidth(e, e->stream2);  // (distance pass -> selection -> kernel matrices, one stream)
    KTimer tm(e, DIBS_K_KMAT, e->stream2);
    // (Mloc == M here, so m0 == 0 and the slab is the whole symmetric matrix: the arguments launch_kmat derives are the literal 0 and 1)
    launch_kmat(e, e->stream2, KmatRows{e->z, (size_t)e->D, 0}, KmatRows{e->theta, (size_t)e->P, 0});
  }
  switch (plan.join) {
    case JoinKind::None: break;
    case JoinKind::Flag:
      ++e->join_seq;
      if (e->debug_drop_flag) e->debug_drop_flag = false;  // (dibs_engine_debug_drop_next_flag: this step's flag is never stored)
      else hipLaunchKernelGGL(k_join_flag, dim3(1), dim3(1), 0, e->stream2, e->join_flag, e->join_seq);
      break;
    case JoinKind::EventAtOnce:
      hipEventRecord(e->ev_join, e->stream2);
      hipStreamWaitEvent(e->stream, e->ev_join, 0);
      break;
    case JoinKind::Event: hipEventRecord(e->ev_join, e->stream2); break;
  }
  if (!plan.do_lik) {
    // (prior terms only: no estimator runs, the tail takes a zero likelihood gradient)
  } else if (score_lik) {
    const BgeParams bp = e->bge.params();
    {  // (queue counters: zero at creation, reset by k_particle_grad at the end of every step)
      KTimer tm(e, DIBS_K_BGE_NODES);
      KmatFuse kf{nullptr, nullptr, 0, 0, 0, 0.f, 0.f, nullptr, 0u};
      if (plan.place == KmatPlace::InSample)  // the latent kernel matrix rides along (see KmatFuse)
        kf = KmatFuse{e->z, e->kz, (int)e->D, e->M, (e->d + 3) / 4, (float)c.scale_latent, (float)c.h_latent, nullptr, 0u};
      if (plan.fork == ForkKind::FlagFromSample) {  // (the edge kernel stored plainly and published nothing: this launch's first block does, see KmatFuse)
        kf.pub_flag = e->fork_flag;
        kf.pub_seq = e->fork_seq;
      }
      bge_launch_sample(true, e->stream, e->thr, e->masks, e->node_scores, bp, carry_lik, e->m0, Mg, e->Mloc, e->d, e->S, e->W, L,
                        e->bq, kf);
    }
    if (c.likelihood == DIBS_LIK_BDEU) {  // the second producer of the node scores: counts of the sampled parent sets' configurations
      KTimer tm(e, DIBS_K_BGE_BIG);
      if (bdeu_launch(e, e->stream, e->bdeu->train, e->masks, e->node_scores, (long long)e->Mloc * e->d * e->S, e->S)) return 1;
    } else {
      KTimer tm(e, DIBS_K_BGE_BIG);
      bge_launch_chol(e->stream, e->node_scores, bp, e->bq, e->d, e->S, e->profiling ? e->counters : nullptr);
    }
    // (softmax weights, W_lik and the baseline are part of k_particle_grad below)
  } else if (c.likelihood == DIBS_LIK_BGE) {  // the reparam estimator
    const BgeSoftParams sp{e->bge.R, e->bge.Nj, e->bge.alpha_lambd, e->bge.alpha_mu, e->bge.log_t, e->bge.n_mats};
    KTimer tm(e, DIBS_K_BGE_NODES);
    bge_soft_launch(sp, e->scores, carry_lik, e->m0, Mg, e->Mloc, e->d, e->S, alpha, (float)c.tau, L, c.logistic_minval_tiny,
                    e->soft_ds, e->logprobs_z, e->w_lik, e->stream, e->soft_tri, e->soft_blocks);
  } else {  // a joint model: LinearGaussian or DenseNonlinearGaussian (dibs_engine_create admits no other likelihood)
    // (explicit-key evaluation: the loop's baselines stay, the updated ones are read from baseline2)
    if (launch_joint_estimators(e, rt, Mg, alpha, carry_theta, carry_lik, 0, "", ": scratch area: hipMalloc failed", !xk)) return 1;
  }
  if (plan.join == JoinKind::Event || plan.join == JoinKind::EventAtOnce) {
    // (covers the kernel matrices: they precede the end of the second stream's chain.  Flag: k_particle_grad polls the flag itself)
    hipStreamWaitEvent(e->stream, e->ev_join, 0);
  } else if (!fork && plan.do_prior) {
    // (folding this reduction into k_particle_grad for small grids -- one dependent launch less -- was measured and dropped: the tail
    //  kernel grows by more than the launch it saves: config 2 54.3 -> 55.3 us/step, a rank of an 8-way headline run 91.4 -> 99.2)
    launch_acyc(e, e->stream, carry_prior, Mg, alpha);
  }
  launch_tail(e, rt, TailOpts{alpha, beta, score_lik, plan.do_prior, plan.do_lik ? e->w_lik : const_cast<float*>(zero_w),
                              plan.join == JoinKind::Flag, e->profiling ? e->counters : nullptr, plan.ns, plan.cps, plan.nrider});
  if (score_lik && !xk) std::swap(e->baseline, e->baseline2);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
  return 0;
}

int step_update(dibs_engine* e, int t, const RowSource& rs, float* vals_send) {
  (void)t;
  const float* const pack = rs.base;
  const dibs_config& c = e->cfg;
  const bool kmat_ext = e->kmat_ext;  // computed from the gathered values on the caller's side stream (dibs_engine_kmat_values)
  e->kmat_ext = false;
  // the particles move: plane 0 of the in-engine overlapped exchange no longer holds them (run_sharded's overlapped branch gathers the new
  // values right behind this call and sets the flag again; every other caller -- packed protocol, dibs_engine_run, step_update -- leaves
  // it cleared, so that the next overlapped chunk / gather_particles re-gathers instead of using the stale plane)
  e->vals_fresh = false;
  // (whether a slab of the caller's is there is known only now: dibs_engine_kmat_values may run beside phase A, after its plan was made,
  //  and set_state / init_particles discard the slab)
  KmatPlace place = e->kmat_place;
  if (place == KmatPlace::External || place == KmatPlace::PhaseB) place = kmat_ext ? KmatPlace::External : KmatPlace::PhaseB;
  if (place == KmatPlace::PhaseB) {
    if (e->median_rule) launch_bandwidth(e, e->stream);
    KTimer tm(e, DIBS_K_KMAT);
    launch_kmat(e, e->stream, KmatRows{pack, rs.stride, rs.z_off}, KmatRows{pack, rs.stride, rs.th_off});
  }
  {
    KTimer tm(e, DIBS_K_PHI_UPDATE);
    auto phi = [&](const PhiSeg& s) {
      if (e->M >= 256) {  // many particles: the transform as one GEMM on the matrix pipe (a function of the GLOBAL count only)
        const long cols = (long)((s.len + 63) / 64);
        const int nrb = (e->Mloc + PG_BM - 1) / PG_BM;
#define PHI_GEMM(J_)                                                                                                                        \
        hipLaunchKernelGGL(k_phi_gemm<J_>, dim3((unsigned)(8 * nrb * ((cols + 7) / 8))), dim3(256), 0, e->stream, pack, rs.stride, s.val_off, \
                           s.grad_off, (int)s.len, e->kz, e->kt, s.is_theta, s.x, s.v, s.phi_out, e->m0, e->Mloc, e->M, s.h, (float)c.stepsize, \
                           c.optimizer == DIBS_OPT_RMSPROP, (int)cols, nrb, vals_send, (size_t)e->Ev, s.is_theta ? (size_t)e->D : (size_t)0);
        if (e->kt) { PHI_GEMM(true) } else { PHI_GEMM(false) }
#undef PHI_GEMM
        return;
      }
      launch_phi_update(e, pack, rs.stride, s, e->Mloc, vals_send, (size_t)e->Ev);
    };
    phi(PhiSeg{rs.z_off, rs.gz_off, (size_t)e->D, 0, e->z, e->vz, e->phi_z, (float)c.h_latent});
    if (c.joint) phi(PhiSeg{rs.th_off, rs.gth_off, (size_t)e->P, 1, e->theta, e->vtheta, e->phi_th, (float)c.h_theta});
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
  return 0;
}

// the loop carry of this rank (svgd.py:315: optimizer states, key, baselines) copied aside / back in ONE launch
struct CopySegs {
  const float* src[5];
  float* dst[5];
  size_t n[5];
};
__global__ __launch_bounds__(256) void k_copy_segs(CopySegs c) {
  const int sg = (int)blockIdx.y;
  const float* __restrict__ a = c.src[sg];
  float* __restrict__ b = c.dst[sg];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < c.n[sg]; i += (size_t)gridDim.x * 256) b[i] = a[i];
}
int carry_copy(dibs_engine* e, bool restore) {
  const size_t nz = (size_t)e->Mloc * e->D, nt = (size_t)e->Mloc * e->P, nb = (size_t)e->Mloc;
  // (no zero fill: dalloc's memset runs on the null stream, which the engine's non-blocking stream does not wait for -- it could land after
  //  the copy below and wipe the backup of the first guarded chunk; every element is written by that copy before it is read)
  if (!e->carry_bak) HIP_OK(hipMalloc((void**)&e->carry_bak, (2 * nz + 2 * nt + nb) * sizeof(float)));
  float* const b = e->carry_bak;
  float* live[5] = {e->z, e->vz, e->theta, e->vtheta, e->baseline};
  float* bak[5] = {b, b + nz, b + 2 * nz, b + 2 * nz + nt, b + 2 * nz + 2 * nt};
  const size_t n[5] = {nz, nz, nt, nt, nb};
  CopySegs c;
  for (int i = 0; i < 5; ++i) {
    c.src[i] = restore ? bak[i] : live[i];
    c.dst[i] = restore ? live[i] : bak[i];
    c.n[i] = n[i];
  }
  hipLaunchKernelGGL(k_copy_segs, dim3(256, 5), dim3(256), 0, e->stream, c);
  if (restore) e->key = e->key_bak;
  else e->key_bak = e->key;
  return 0;
}

// ---- multi-run engines (include/dibs_hip.h): batched (n_problems = B > 1) and chains (n_chains = C > 1, e->chains, B = C) ----------------
// One step of B runs in the launches of one standalone step: rows [B * M] run-major, every per-particle kernel over all rows with explicit
// keys (Mg = -1, rng_explicit_row) that the keys kernel derives from the B device-resident carries; the kernel matrices are block-diagonal
// [B * M][M] and phi sums over a run's own block (k_phi_update's BATCH forms, grid.y = run).  Fork / join of the second stream by events
// only (no flags), the kernel matrices standalone on the second stream (no fusions).  Every choice a standalone engine makes from its
// particle count is made from M, one run's (the kernel-matrix algorithm, phi's TA / FULL, JointLaunch::M_choice), never from B * M.
// The two kinds differ where step_local branches between the BGe score estimator and a joint model:
//  * batched: B independent MarginalDiBS + BGe problems, each with its own data.  The BGe kernels look up problem m / M's statistics (BATCH
//    instantiations); one kernel matrix (latent).
//  * chains: C chains of one joint model.  The data is shared, so every kernel that reads it runs unchanged over all rows; chain-aware are
//    the keys, the two kernel matrices (latent -> kz, theta -> kt and kz + kt -> ksum) and phi (JOINT + BATCH forms).  With per-chain data
//    (LinearGaussian, dibs_engine_set_data_problem for every chain) the step is the same: joint_lin_all_logprobs / joint_lin_all_grads take
//    the launch text of lin_launch.h as compiled with the per-chain kernels (tu_lin_chains.hip) when JointWork::n_chain_data is set.
// Hyper-parameters: per run, from the device table e->hp (ProblemHP; dibs_engine_set_problem_hparams / dibs_engine_set_chain_hparams, by
// default the configuration's values in every row).  A batched engine's keys kernel forms this step's alpha and beta of every problem in
// double, as the host does for a standalone engine; its kernel matrix and phi always read the table.  The edge, acyclicity and tail kernels
// read it where they have a table-reading form (e->hp_tier; kernels and launchers in tu_batch.hip, pM = M) and otherwise take the
// configuration's values as launch arguments (set_problem_hparams accepts no others there).  e->hp_tier of a chains engine: some chain's
// values differ from the configuration's (LinearGaussian with per-chain data, n_vars, n_dim <= 64).  Then the keys launch also forms every
// chain's alpha and beta in its row of the table, the kernel matrices take chain p's h / h_theta, phi reads the table as it always did, and
// the per-chain estimator kernels take alpha and the baseline rate of the block's chain (LinChainData::hp; they always do).  Without
// differing values the launches are those of a chains engine on which nothing was set.
// The table-reading forms of the edge, acyclicity and tail launches are launch blocks of step_multi alone, so that the blocks the
// standalone step shares with it stay what they were.
static void batch_edge_scores(dibs_engine* e) {
  KTimer tm(e, DIBS_K_EDGE, e->stream);
  batch_launch_edge_scores(e->stream, e->z, e->scores, e->thr, e->probs, e->eas, e->hp, e->M, e->Mloc, e->d, e->k, e->dpad, e->ldk);
}
static void batch_acyc(dibs_engine* e, hipStream_t st, Key2 carry) {
  const dibs_config& c = e->cfg;
  const AcycLaunch al{st, e->scores, e->acyc_part, e->w_acyc, nullptr, carry, 0, -1, e->Mloc, e->d, e->Sa, e->acyc_units,
                      e->acyc_paired, 0.f, (float)c.tau, c.rng_layout, c.logistic_minval_tiny, nullptr, nullptr, e->eas, e->tune.acyc_pipe,
                      e->tune.acyc_hfw_max};
  {
    KTimer tm(e, DIBS_K_ACYC, st);
    batch_launch_acyc_power(al, e->hp, e->M);
  }
  KTimer tm(e, DIBS_K_ACYC_REDUCE, st);
  acyc_launch_reduce(al);
}
// (the tail as launch_tail builds it for a multi-run step -- score_lik: the BGe score estimator, otherwise a joint model; prior terms on,
//  W, U, V in LDS, no riders, no join flag; alpha, beta, the prior constant, 1 / sigma^2 and the baseline rate: k_particle_grad_batch fills
//  them in from the table)
static void multi_tail_hp(dibs_engine* e, const RowTarget& rt, bool score_lik) {
  const dibs_config& c = e->cfg;
  KTimer tm(e, DIBS_K_TAIL);
  const int ldz = tail_ldz(e->d, e->k, e->S, score_lik, LDS_LIMIT - 2048);
  const int cap = score_lik ? tail_stage_cap(e->d, ldz, e->S, e->W, LDS_LIMIT - 2048) : 0;
  const size_t lds = tail_lds_bytes(e->d, ldz, e->S, e->W, score_lik, cap);
  const TailArgs ta{score_lik ? e->node_scores : nullptr, e->masks, e->logprobs_z, e->baseline, e->baseline2, 0.0,
                    score_lik ? e->bq.counts : nullptr, e->S, e->W, cap, e->probs, e->w_lik, e->w_acyc, 0.f, 0.f, c.graph_prior, 0.f, e->z,
                    rt.base, rt.stride, rt.copy_vals, 0, e->d, e->k, ldz, 0.f, nullptr, nullptr, nullptr, 0u, nullptr, e->Mloc,
                    KmatTile{nullptr, 0, 0, 0, nullptr, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr}};
  batch_launch_tail(e->stream, ta, e->hp, e->M, e->Mloc, lds);
}

// the kernel-matrix algorithm of a standalone engine of M particles (its kmat_tiled_on): tiled from kmat_tiled_min particles, direct below
static bool multi_kmat_tiled(const dibs_engine* e) {
  return e->M >= e->tune.kmat_tiled_min && kmat_tile_addressable((size_t)2 * e->M, e->E > e->Ev ? e->E : e->Ev, 0, 0);
}
static void kmat_batch(dibs_engine* e, hipStream_t st) {
  const dibs_config& c = e->cfg;
  KTimer tm(e, DIBS_K_KMAT, st);
  if (multi_kmat_tiled(e)) {
    const int nta = (e->M + KT_T - 1) / KT_T, tiles = kmat_tile_count(nta, nta, 1), nchunk = kmat_nchunk((int)e->D);
    const KmatTile kt{e->z, (size_t)e->D, 0, (int)e->D, nullptr, 0, e->M, e->M, nchunk, nta, nta, 1, 1, nchunk, (float)c.scale_latent,
                      (float)c.h_latent, e->kz, nullptr, nullptr, nullptr};
    dibs_allow_lds((const void*)k_kmat_tile_batch, kmat_tile_lds_bytes());
    hipLaunchKernelGGL(k_kmat_tile_batch, dim3((unsigned)tiles, (unsigned)e->B), dim3(KT_NT), kmat_tile_lds_bytes(), st, kt, (const ProblemHP*)e->hp);
    return;
  }
  const size_t lds = kmat_lds_bytes((size_t)e->D);
  allow_lds(k_kmat_batch, lds);
  hipLaunchKernelGGL(k_kmat_batch, dim3(e->Mloc, (e->M + KMAT_BT - 1) / KMAT_BT), dim3(256), lds, st, (const float*)e->z, (size_t)e->D, (int)e->D,
                     e->kz, e->M, (float)c.scale_latent, (const ProblemHP*)e->hp);
}
static void kmat_chains(dibs_engine* e, hipStream_t st) {
  const dibs_config& c = e->cfg;
  KTimer tm(e, DIBS_K_KMAT, st);
  const bool tiled = multi_kmat_tiled(e);
  if (e->hp_tier || e->median_rule) {  // (median rule: the selection has written every chain's h / h_theta of this step)
    chains_launch_kmat_hp(st, tiled, e->z, (size_t)e->D, e->kz, e->B, e->M, (float)c.scale_latent, e->hp, 0, nullptr, nullptr,
                          kmat_lds_bytes((size_t)e->D));
    chains_launch_kmat_hp(st, tiled, e->theta, (size_t)e->P, e->kt, e->B, e->M, (float)c.scale_theta, e->hp, 1, e->kz, e->ksum,
                          kmat_lds_bytes((size_t)e->P));
  } else {
    chains_launch_kmat(st, tiled, e->z, (size_t)e->D, e->kz, e->B, e->M, (float)c.scale_latent, (float)c.h_latent, nullptr, nullptr,
                       kmat_lds_bytes((size_t)e->D));
    chains_launch_kmat(st, tiled, e->theta, (size_t)e->P, e->kt, e->B, e->M, (float)c.scale_theta, (float)c.h_theta, e->kz, e->ksum,
                       kmat_lds_bytes((size_t)e->P));
  }
}

int step_multi(dibs_engine* e, int t) {
  const dibs_config& c = e->cfg;
  const bool chains = e->chains, tier = e->hp_tier;
  const float alpha = (float)(c.alpha_linear * t), beta = (float)(c.beta_linear * t);
  const int L = c.rng_layout, R = e->Mloc;  // (one rank: m0 = 0)
  if (!chains) {
    hipLaunchKernelGGL(k_batch_keys, dim3(e->B), dim3(256), 0, e->stream, e->bcarry, e->bkeys_lik, e->bkeys_prior, e->M, L, e->hp, t);
  } else if (tier || e->jw.n_chain_data) {
    // (per-chain data: the per-chain estimator kernels read the step's alpha from the table, so the keys launch forms it there also when no
    //  chain's values differ -- the same launch with two more stores per chain)
    chains_launch_keys_hp(e->stream, e->bcarry, e->bkeys_theta, e->bkeys_lik, e->bkeys_prior, e->B, e->M, L, e->hp, t);
  } else {
    chains_launch_keys(e->stream, e->bcarry, e->bkeys_theta, e->bkeys_lik, e->bkeys_prior, e->B, e->M, L);
  }
  const Key2 carry_lik = key_array_as_carry(e->bkeys_lik, 0), carry_prior = key_array_as_carry(e->bkeys_prior, 0);
  if (tier) batch_edge_scores(e);
  else launch_edge_scores(e, e->stream, alpha, EdgeFork{}, nullptr);
  // acyclicity term and kernel matrices on the second stream (they need only this step's scores / z / theta), the estimators on the first
  const EventFork ef(e);
  if (ef.fork()) return 1;
  if (tier) batch_acyc(e, ef.s2, carry_prior);
  else launch_acyc(e, ef.s2, carry_prior, -1, alpha);
  if (e->median_rule) launch_bandwidth(e, ef.s2);
  if (chains) kmat_chains(e, ef.s2);
  else kmat_batch(e, ef.s2);
  if (ef.chain_done()) return 1;
  const RowTarget rt = packed_rows(e, e->pack);
  if (chains) {
    // (per-chain data: the estimator kernels read alpha and the baseline rate from the table; the two arguments here are not read)
    if (launch_joint_estimators(e, rt, -1, alpha, key_array_as_carry(e->bkeys_theta, 0), carry_lik, e->M, "chains engine (n_chains > 1): ",
                                ": scratch area: hipMalloc failed, or the partial sums of all chains pass the gradient kernel's addressing limit", true))
      return 1;
  } else {
    BgeParams bp = e->bge.params();
    bp.pM = e->M;
    {
      KTimer tm(e, DIBS_K_BGE_NODES);
      bge_launch_sample_batch(e->stream, e->thr, e->masks, e->node_scores, bp, carry_lik, R, e->d, e->S, e->W, L, e->bq);
    }
    KTimer tm(e, DIBS_K_BGE_BIG);
    bge_launch_chol_batch(e->stream, e->node_scores, bp, e->bq, e->d, e->S);
  }
  if (ef.join()) return 1;
  const bool score_lik = !chains;
  if (tier) multi_tail_hp(e, rt, score_lik);
  else launch_tail(e, rt, TailOpts{alpha, beta, score_lik, true, e->w_lik, false, nullptr});
  if (score_lik) std::swap(e->baseline, e->baseline2);
  {
    // SVGD transform + optimizer step: k_phi_update's BATCH instantiations, grid.y = run, each run exactly a standalone launch
    KTimer tm(e, DIBS_K_PHI_UPDATE);
    launch_phi_update(e, e->pack, (size_t)e->E, PhiSeg{0, (size_t)e->D, (size_t)e->D, 0, e->z, e->vz, e->phi_z, (float)c.h_latent}, e->M, nullptr, 0);
    if (chains)
      launch_phi_update(e, e->pack, (size_t)e->E, PhiSeg{(size_t)(2 * e->D), (size_t)(2 * e->D + e->P), (size_t)e->P, 1, e->theta, e->vtheta, e->phi_th,
                                                         (float)c.h_theta}, e->M, nullptr, 0);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
  return 0;
}

// ---- the entry points of a loop driven from outside (include/dibs_hip.h) ----------------------------------------------------------------
extern "C" int dibs_engine_step_local(dibs_engine* e, int32_t t, void* send_dev) {
  if (!e || !send_dev) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_step_local is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_step_local (only dibs_engine_run steps it)")) return 1;
  if (e->B > 1) return fail("batched engine: only dibs_engine_run steps it");
  if (!e->has_data) return fail("dibs_engine_set_data has not been called");
  if (need_edge_prior(e)) return 1;
  HIP_OK(hipSetDevice(e->cfg.device_id));
  latch_flags(e);
  // send_dev holds only this rank's rows: [Mloc, E]; kernels index rows by global particle id
  float* base = (float*)send_dev - (size_t)e->m0 * e->E;
  return step_local(e, t, packed_rows(e, base));
}

// ---- overlapped exchange (see include/dibs_hip.h): values travel right after the optimizer step, gradients between the phases ----
extern "C" int64_t dibs_engine_plane_elems_per_rank(const dibs_engine* e) { return e ? (int64_t)e->Mloc * e->Ev : 0; }

extern "C" int dibs_engine_export_values(dibs_engine* e, void* vals_send_dev) {
  if (!e || !vals_send_dev) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_export_values is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_export_values")) return 1;
  HIP_OK(hipSetDevice(e->cfg.device_id));
  float* dst = (float*)vals_send_dev;
  HIP_OK(hipMemcpy2DAsync(dst, (size_t)e->Ev * 4, e->z, (size_t)e->D * 4, (size_t)e->D * 4, (size_t)e->Mloc, hipMemcpyDeviceToDevice, e->stream));
  if (e->P)
    HIP_OK(hipMemcpy2DAsync(dst + e->D, (size_t)e->Ev * 4, e->theta, (size_t)e->P * 4, (size_t)e->P * 4, (size_t)e->Mloc, hipMemcpyDeviceToDevice,
                            e->stream));
  return 0;
}

extern "C" int dibs_engine_step_local_grads(dibs_engine* e, int32_t t, void* grads_send_dev) {
  if (!e || !grads_send_dev) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_step_local_grads is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_step_local_grads (only dibs_engine_run steps it)")) return 1;
  if (e->B > 1) return fail("batched engine: only dibs_engine_run steps it");
  if (!e->has_data) return fail("dibs_engine_set_data has not been called");
  if (need_edge_prior(e)) return 1;
  HIP_OK(hipSetDevice(e->cfg.device_id));
  latch_flags(e);
  // rows [grad_z | grad_theta] of this rank's particles, stride Ev; kernels index rows by global particle id
  float* base = (float*)grads_send_dev - (size_t)e->m0 * e->Ev;
  return step_local(e, t, RowTarget{base, (size_t)e->Ev, 0, 0, (size_t)e->D, 0});
}

// kernel-matrix slab(s) of the NEXT phase B from the values of all particles (plane 0), launched on `stream` -- the caller's side stream,
// behind its all-gather of the values, i.e. beside phase A and without any synchronisation of its own.  The caller orders phase B behind it
// (one event it needs anyway: phase B reads plane 0 as well).
extern "C" int dibs_engine_kmat_values(dibs_engine* e, const void* vals_all_dev, void* stream) {
  if (!e || !vals_all_dev || !stream) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_kmat_values is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_kmat_values (only dibs_engine_run steps it)")) return 1;
  if (e->B > 1) return fail("batched engine: only dibs_engine_run steps it");
  if (e->median_rule)
    return fail("median bandwidth: dibs_engine_kmat_values is not supported (a slab computed beside phase A has no selected bandwidth; the "
                "rule runs on one rank, where dibs_engine_run / step_local + step_update compute the matrices themselves)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  const float* vals = (const float*)vals_all_dev;
  launch_kmat(e, (hipStream_t)stream, KmatRows{vals, (size_t)e->Ev, 0}, KmatRows{vals, (size_t)e->Ev, (size_t)e->D});
  HIP_OK(hipGetLastError());
  e->kmat_ext = true;
  return 0;
}

extern "C" int dibs_engine_step_update_planes(dibs_engine* e, int32_t t, const void* planes_dev, void* vals_send_dev) {
  if (!e || !planes_dev) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_step_update_planes is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_step_update_planes (only dibs_engine_run steps it)")) return 1;
  if (e->B > 1) return fail("batched engine: only dibs_engine_run steps it");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  return step_update(e, t, plane_source(e, (const float*)planes_dev), (float*)vals_send_dev);
}

extern "C" int dibs_engine_step_update(dibs_engine* e, int32_t t, const void* recv_dev) {
  if (!e || !recv_dev) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_engine_step_update is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_step_update (only dibs_engine_run steps it)")) return 1;
  if (e->B > 1) return fail("batched engine: only dibs_engine_run steps it");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  return step_update(e, t, packed_source(e, (const float*)recv_dev));
}

// ---- gradient estimators for explicit per-particle keys (include/dibs_hip.h) ------------------------------------------------
// reference: DiBS.eltwise_grad_z_likelihood (dibs.py:295-321), eltwise_grad_theta_likelihood (:467-485), eltwise_grad_latent_prior (:626-658)
extern "C" int dibs_engine_eval_gradients(dibs_engine* e, int32_t t, const uint32_t* keys_theta, const uint32_t* keys_lik, const uint32_t* keys_prior,
                                          float* grad_z_lik, float* baseline_out, float* grad_theta, float* grad_z_prior) {
  if (!e) return fail("null engine");
  if (e->f64) return fail("float64 engine: dibs_engine_eval_gradients is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_engine_eval_gradients")) return 1;
  if (e->B > 1) return fail("batched engine: dibs_engine_eval_gradients is not supported");
  if (!e->has_data) return fail("dibs_engine_set_data has not been called");
  if (need_edge_prior(e)) return 1;
  const dibs_config& c = e->cfg;
  const bool want_lik = keys_lik != nullptr || keys_theta != nullptr, want_prior = keys_prior != nullptr;
  if (c.joint && want_lik && (!keys_lik || !keys_theta)) return fail("joint model: pass the keys of the theta AND the Z estimator (both run in one pass)");
  if (!c.joint && keys_theta) return fail("keys_theta given for a marginal model");
  if (want_lik && !c.joint && !keys_lik) return fail("keys_lik missing");
  HIP_OK(hipSetDevice(c.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const size_t nk = (size_t)e->Mloc * 2;
  DevBuf<uint32_t> dk;   // [3][Mloc][2]
  DevBuf<float> zero_w;  // [Mloc][d][d] zeros: the likelihood gradient of the prior-only pass
  HIP_OK(dk.alloc(3 * nk));
  const uint32_t* src[3] = {keys_theta, keys_lik, keys_prior};
  for (int i = 0; i < 3; ++i)
    if (src[i]) HIP_OK(hipMemcpy(dk.p + i * nk, src[i], nk * 4, hipMemcpyHostToDevice));
  const StepKeys xk{reinterpret_cast<const Key2*>(dk.p), reinterpret_cast<const Key2*>(dk.p + nk), reinterpret_cast<const Key2*>(dk.p + 2 * nk)};
  const size_t wz = (size_t)e->D * 4, wt = (size_t)e->P * 4;
  const float* rows = e->pack + (size_t)e->m0 * e->E;
  if (want_lik) {
    if (step_local(e, t, packed_rows(e, e->pack), &xk, TERMS_LIK)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    if (grad_z_lik) HIP_OK(hipMemcpy2D(grad_z_lik, wz, rows + e->D, (size_t)e->E * 4, wz, e->Mloc, hipMemcpyDeviceToHost));
    if (grad_theta && e->P) HIP_OK(hipMemcpy2D(grad_theta, wt, rows + 2 * e->D + e->P, (size_t)e->E * 4, wt, e->Mloc, hipMemcpyDeviceToHost));
    if (baseline_out) HIP_OK(hipMemcpy(baseline_out, e->baseline2, (size_t)e->Mloc * 4, hipMemcpyDeviceToHost));  // (not swapped in: see step_local)
  }
  if (want_prior) {
    HIP_OK(zero_w.alloc((size_t)e->Mloc * e->d * e->d));
    if (step_local(e, t, packed_rows(e, e->pack), &xk, TERMS_PRIOR, zero_w.p)) return 1;
    HIP_OK(hipStreamSynchronize(e->stream));
    if (grad_z_prior) HIP_OK(hipMemcpy2D(grad_z_prior, wz, rows + e->D, (size_t)e->E * 4, wz, e->Mloc, hipMemcpyDeviceToHost));
  }
  if (e->profiling) drain_timers(e);
  HIP_OK(hipGetLastError());
  return 0;
}
