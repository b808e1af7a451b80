/*
 * dibs_hip.h -- C ABI of the MI355X-native DiBS SVGD engine (libdibs_hip.so).
 *
 * The reference (larslorch/dibs) has no FFI: its boundary is the Python class API
 *   MarginalDiBS(...).sample(...)   dibs/inference/svgd.py:60-77, 274-331
 *   JointDiBS(...).sample(...)      dibs/inference/svgd.py:425-442, 730-795
 * Each entry point below names the reference interface it replaces.  The Python facade
 * (dibs_amd/inference/svgd.py) binds these with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, non-zero on error; dibs_last_error() gives
 * the thread-local message.  Host buffers are caller-owned, row-major, float32 / int32 / uint32.
 * The engine owns all device memory.  A handle is not thread-safe; distinct handles are independent.
 */
#ifndef DIBS_HIP_H
#define DIBS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIBS_ABI_VERSION 2
#define DIBS_MAX_HIDDEN_LAYERS 8

enum { DIBS_LIK_BGE = 0, DIBS_LIK_LINGAUSS = 1, DIBS_LIK_DENSENN = 2, DIBS_LIK_BDEU = 3 /* discrete data: see BDEU */ };
enum { DIBS_PRIOR_ER = 0, DIBS_PRIOR_SF = 1, DIBS_PRIOR_UNIFORM = 2, DIBS_PRIOR_EDGEWISE = 3 /* see dibs_engine_set_edge_prior */ };
enum { DIBS_EST_SCORE = 0, DIBS_EST_REPARAM = 1 };
enum { DIBS_OPT_GD = 0, DIBS_OPT_RMSPROP = 1 };
enum { DIBS_RNG_LEGACY = 0, DIBS_RNG_PARTITIONABLE = 1 };
enum { DIBS_ACT_RELU = 0, DIBS_ACT_TANH = 1, DIBS_ACT_SIGMOID = 2, DIBS_ACT_LEAKYRELU = 3 };

/* POD mirror of the constructor kwargs (svgd.py:60-77 / 425-442) + the sizes sample() fixes
 * (svgd.py:274) + the hyper-parameters of the recognised model classes. */
typedef struct dibs_config {
  int32_t abi_version;      /* DIBS_ABI_VERSION */
  int32_t n_vars;           /* d   = x.shape[-1]                                   dibs.py:67        */
  int32_t n_dim;            /* k   = n_dim_particles (default d)                   svgd.py:138-139   */
  int32_t n_particles;      /* M (global, all ranks)                               svgd.py:274       */
  int32_t n_observations;   /* N   = x.shape[0]                                                      */
  int32_t n_grad_mc_samples;        /* S                                            dibs.py:60        */
  int32_t n_acyclicity_mc_samples;  /* Sa                                           dibs.py:61        */
  int32_t joint;            /* 0 = MarginalDiBS, 1 = JointDiBS                                       */
  int32_t likelihood;       /* DIBS_LIK_*                                                            */
  int32_t graph_prior;      /* DIBS_PRIOR_*                                                          */
  int32_t grad_estimator_z; /* DIBS_EST_*                                           dibs.py:309-318   */
  int32_t optimizer;        /* DIBS_OPT_*                                           svgd.py:117-122   */
  int32_t rng_layout;       /* DIBS_RNG_*  (jax_threefry_partitionable)                              */
  int32_t logistic_minval_tiny; /* 0: uniform minval = finfo.eps (jax default), 1: finfo.tiny        */
  int32_t has_interventions;/* advisory: 0 = interv_mask all zero (the engine derives everything from the mask passed to
                               dibs_engine_set_data; the field only records the caller's view)          svgd.py:86-87     */
  int32_t nn_n_hidden;      /* DenseNonlinearGaussian: len(hidden_layers)           nonlinearGaussian.py:105 */
  int32_t nn_hidden[DIBS_MAX_HIDDEN_LAYERS];
  int32_t nn_activation;    /* DIBS_ACT_*                                                            */
  int32_t nn_bias;
  int32_t rank;             /* particle shard: this engine owns particles                            */
  int32_t n_ranks;          /*   [rank*M/n_ranks, (rank+1)*M/n_ranks)                                */
  int32_t device_id;
  int32_t reserved_i[5];    /* [0] n_problems: 0 / 1 = one problem; B > 1 = a batched engine (see dibs_engine_set_data_problem)
                               [1] precision: 0 / 32 = float32, 64 = the float64 engine (see dibs_engine_set_data_f64)
                               [2] n_chains: 0 / 1 = one chain (the standalone engine); C > 1 = a chains engine (see CHAINS ENGINE)
                               [3] bandwidth rule: 0 = h_latent / h_theta as given; bit 0: the latent kernel's bandwidth, bit 1: the
                                   parameter kernel's (joint models) by the median heuristic (see MEDIAN-HEURISTIC KERNEL BANDWIDTH) */

  double alpha_linear;      /* dibs.py:70 */
  double beta_linear;       /* dibs.py:71 */
  double tau;               /* dibs.py:72 */
  double h_latent;          /* kernel.py:16 / :46  (kernel_param "h" / "h_latent") */
  double h_theta;           /* kernel.py:46 */
  double scale_latent;      /* kernel.py:16 / :46 */
  double scale_theta;
  double stepsize;          /* optimizer_param["stepsize"]   svgd.py:83 */
  double score_function_baseline; /* dibs.py:76 */
  double latent_prior_std;  /* <= 0: default 1/sqrt(k)       svgd.py:142, 301-302 */
  double graph_prior_edges_per_node; /* graph.py:27-30 */
  double bge_alpha_mu;      /* linearGaussian.py:44 */
  double bge_alpha_lambd;   /* <= 0: default d + 2           linearGaussian.py:45 */
  double lin_obs_noise;     /* linearGaussian.py:190 */
  double lin_mean_edge;
  double lin_sig_edge;
  double lin_min_edge;
  double nn_obs_noise;      /* nonlinearGaussian.py:105 */
  double nn_sig_param;
  double reserved_d[6];     /* [0] DIBS_LIK_BDEU: the equivalent sample size; <= 0 means 1.0 (see BDEU) */
} dibs_config;

typedef struct dibs_engine dibs_engine;

/* names of device buffers readable through dibs_engine_read_buffer (parity tests / callbacks) */
enum {
  DIBS_BUF_Z = 0,          /* f32 [Mloc, d, k, 2]                                 */
  DIBS_BUF_V_Z = 1,        /* f32 [Mloc, d, k, 2]   rmsprop avg_sq_grad           */
  DIBS_BUF_THETA = 2,      /* f32 [Mloc, P]         theta leaves concatenated     */
  DIBS_BUF_V_THETA = 3,
  DIBS_BUF_SCORES = 4,     /* f32 [Mloc, d, d]      U V^T                          */
  DIBS_BUF_LOGPROBS_Z = 5, /* f32 [Mloc, S]         l_s of the Z estimator         */
  DIBS_BUF_W_LIK = 6,      /* f32 [Mloc, d, d]      dl/dscores of the likelihood   */
  DIBS_BUF_W_ACYC = 7,     /* f32 [Mloc, d, d]      E[dh/dscores]                  */
  DIBS_BUF_GRAD_Z = 8,     /* f32 [Mloc, d, k, 2]   d/dz log p(z, D)               */
  DIBS_BUF_GRAD_THETA = 9, /* f32 [Mloc, P]                                        */
  DIBS_BUF_KXX = 10,       /* f32 [Mloc, M]         kxx[a_local, b_global]         */
  DIBS_BUF_PHI_Z = 11,     /* f32 [Mloc, d, k, 2]                                  */
  DIBS_BUF_BASELINE = 12,  /* f32 [Mloc]                                           */
  DIBS_BUF_NODE_SCORES = 13,/* f64 [Mloc, d, S]     BGe per-node scores            */
  DIBS_BUF_PARENT_MASKS = 14,/* u64 [Mloc, d, S, W] sampled parent sets of node j (bit i of word i/64 = g[i, j]) */
  DIBS_BUF_LOGPROBS_THETA = 15, /* f32 [Mloc, S]                                   */
  DIBS_BUF_PHI_THETA = 16,
  DIBS_BUF_GATHER = 17,    /* f32 packed all-gather payload        */
  DIBS_BUF_PROBLEM_STEP = 18, /* f32 [B, 2]  batched engines: (alpha, beta) of the last step as the device formed them per problem */
  DIBS_BUF_BANDWIDTH = 19,    /* f32 [B, 2]  (h_latent, h_theta) the last step's kernel matrices used, per run (B = 1: the standalone engine).
                                 Fixed rule: the configuration's (or the run's own) values; see MEDIAN-HEURISTIC KERNEL BANDWIDTH */
  DIBS_BUF_SQDIST_Z = 20,     /* f32 [B * M, M]  squared distances ||z_a - z_b||^2 the selection of the last step saw, per run: symmetric, zero
                                 diagonal.  Only while the latent kernel is on the median rule ("no such buffer" otherwise)               */
  DIBS_BUF_SQDIST_THETA = 21, /* f32 [B * M, M]  the same for theta (parameter kernel on the median rule)                                */
  DIBS_BUF_COUNT
};

/* kernel ids for dibs_engine_get_timers */
enum {
  DIBS_K_EDGE = 0, DIBS_K_BGE_NODES = 1, DIBS_K_LIK_WEIGHTS = 2, DIBS_K_ACYC = 3, DIBS_K_ZGRAD = 4,
  DIBS_K_KMAT = 5, DIBS_K_PHI_UPDATE = 6, DIBS_K_LIN_THETA = 7, DIBS_K_LIN_Z = 8, DIBS_K_NN_THETA = 9,
  DIBS_K_NN_Z = 10, DIBS_K_PACK = 11, DIBS_K_BGE_BIG = 12 /* the three queue launches */, DIBS_K_ACYC_REDUCE = 13 /* k_acyc_reduce */, DIBS_K_TAIL = 14 /* k_particle_grad */,
  DIBS_K_BANDWIDTH = 15 /* median-rule bandwidth: distance pass + k_bandwidth_median */,
  DIBS_K_COUNT = 16
};

const char* dibs_last_error(void);
int dibs_abi_version(void);

/* replaces MarginalDiBS.__init__ / JointDiBS.__init__ (svgd.py:60-122, 425-487): validates the config,
 * selects the device, allocates all device state.  `stream` is a hipStream_t to launch on (NULL: the
 * engine creates its own). */
int dibs_engine_create(const dibs_config* cfg, void* stream, dibs_engine** out);
int dibs_engine_destroy(dibs_engine* e);

/* x: f32 [N, d]; interv_mask: i32 [N, d] or NULL; bge_mean_obs: f32 [d] or NULL  (svgd.py:61-64, 86-87) */
int dibs_engine_set_data(dibs_engine* e, const float* x, const int32_t* interv_mask, const float* bge_mean_obs);

/* replaces the prologue of sample() (svgd.py:293-307 / 750-766): key,subk = split(key);
 * _sample_initial_random_particles(subk); zero optimizer state and baselines; keeps the carry key. */
int dibs_engine_init_particles(dibs_engine* e, const uint32_t key[2]);

/* checkpoint / resume of the loop carry (svgd.py:315: (opt_state_z[, opt_state_theta], key, sf_baseline));
 * any pointer may be NULL (left untouched / not returned).  z, v_z: f32 [Mloc, d, k, 2]; theta, v_theta:
 * f32 [Mloc, P]; key: u32 [2]; baseline: f32 [Mloc]. */
int dibs_engine_set_state(dibs_engine* e, const float* z, const float* v_z, const float* theta,
                          const float* v_theta, const uint32_t* key, const float* baseline);
int dibs_engine_get_state(dibs_engine* e, float* z, float* v_z, float* theta, float* v_theta,
                          uint32_t* key, float* baseline);

/* replaces _svgd_loop(start, n_steps, carry) (svgd.py:269-272 / 724-727): runs steps t_start ..
 * t_start+n_steps-1 entirely on the device, blocking until done.  Single-rank engines only. */
int dibs_engine_run(dibs_engine* e, int32_t t_start, int32_t n_steps);

/* Inside a chunk the engine synchronises its two streams through flag words polled by kernels (cheaper than events by ~10 us per step).  The
 * waits are bounded; should one run into its bound (a device masked down to a few CUs, another process filling the GPU, a serialising tool),
 * dibs_engine_run / dibs_engine_run_sharded restore the loop carry they copied at the start of the chunk, switch this engine to events for
 * good and run the same steps again -- callers see only the delay.  (In a sharded run the ranks agree on this with one tiny all-gather per
 * chunk and repeat together.)  Returns how many chunks were repeated so far (-1: null handle). */
int dibs_engine_flag_fallbacks(const dibs_engine* e);
/* fault injection for the tests of that path: the next step that would publish the second stream's completion flag does not, so the polling
 * kernel runs into its bound (0.2 s) exactly once.  No effect on an engine that is not using the flags. */
int dibs_engine_debug_drop_next_flag(dibs_engine* e);
/* for the tests of the device Threefry routines (csrc/rng.h: wave-uniform key, half and offsets): one block evaluates, for every i < n, the
 * single routine on counters (c0[i], c0[i] + half) and the paired routine on (c0[i], c0[i] + half) and (c0[i] + off_b, c0[i] + off_b + half),
 * all sums mod 2^32, with key (k0, k1).  c0: host u32 [n]; out: host u32 [n][6] = {single y0, y1, pair a y0, y1, pair b y0, y1}.
 * Uses the current device and its null stream; blocking. */
int dibs_debug_threefry(uint32_t k0, uint32_t k1, uint32_t half, uint32_t off_b, const uint32_t* c0, int32_t n, uint32_t* out);

/* multi-rank split of one _svgd_step (svgd.py:226-267): phase A = per-particle estimators for the local
 * shard + packing of [z | grad_z (| theta | grad_theta)] into the send buffer; the caller all-gathers
 * (RCCL, torch.distributed) send -> recv; phase B = kernel matrix slab, phi and optimizer step for the
 * local shard.  Buffers are device pointers owned by the caller (torch tensors). Asynchronous on the
 * engine stream. */
int dibs_engine_step_local(dibs_engine* e, int32_t t, void* send_dev);
int dibs_engine_step_update(dibs_engine* e, int32_t t, const void* recv_dev);
int64_t dibs_engine_gather_elems_per_rank(const dibs_engine* e);
int dibs_engine_sync(dibs_engine* e);

/* The same split with the exchange OVERLAPPED (no reference counterpart: the reference has no multi-device code; the arithmetic is
 * svgd.py:226-267 / 673-721 unchanged).  The kernel matrix and the repulsive term need the VALUES [z | theta] of all particles, which
 * are final as soon as the previous optimizer step is done; only the GRADIENTS depend on phase A.  So each rank
 *   dibs_engine_step_update_planes(e, t, planes, vals_send)      ... ends phase B of step t with its new values in `vals_send`, rows
 *       [Mloc, Ev] of [z | theta] (dibs_engine_export_values writes them for the initial state);
 *   the caller all-gathers them on a SIDE stream into plane 0 of `planes` ([2][M][Ev] floats) and, behind the gather on that stream,
 *   dibs_engine_kmat_values(e, plane0, side_stream)              launches the kernel-matrix slab of step t + 1 -- both beside phase A;
 *   dibs_engine_step_local_grads(e, t + 1, grads_send)           phase A, writing only [grad_z | grad_theta] rows [Mloc, Ev];
 *   the caller all-gathers the gradient rows into plane 1 (the only exchange between the phases: half the bytes of the packed rows),
 *   makes the engine stream wait for the side stream's work, and calls dibs_engine_step_update_planes for step t + 1: phi + optimizer.
 * Results are bit-identical to step_local / step_update and to the single-rank engine.  Ev = dibs_engine_plane_elems_per_rank / Mloc. */
int64_t dibs_engine_plane_elems_per_rank(const dibs_engine* e);
int dibs_engine_export_values(dibs_engine* e, void* vals_send_dev);
int dibs_engine_step_local_grads(dibs_engine* e, int32_t t, void* grads_send_dev);
int dibs_engine_kmat_values(dibs_engine* e, const void* vals_all_dev, void* stream);
int dibs_engine_step_update_planes(dibs_engine* e, int32_t t, const void* planes_dev, void* vals_send_dev);

/* The exchange INSIDE the engine (north_star: "a single RCCL all-gather over xGMI per step"; no reference counterpart -- the reference has
 * no multi-device code): the step loop of a particle-sharded run in C, the collective issued by the engine on its own
 * stream through RCCL (bound at run time: librccl.so.1, in a torch process torch's copy).  One process per GPU:
 *   rank 0:      dibs_comm_unique_id(id)            once per communicator (DIBS_COMM_ID_BYTES each); the bytes go to every rank by any
 *                                                   means (MPI, a file, torch.distributed.broadcast_object_list ...)
 *   every rank:  dibs_engine_comm_init(e, ids, n)   ncclCommInitRank with rank = cfg.rank of cfg.n_ranks on the engine's device;
 *                                                   n = 1: one communicator; n = 2: a second one for the side stream of the overlapped exchange
 *                dibs_engine_run_sharded(e, t_start, n_steps, overlapped)   replaces _svgd_loop (svgd.py:269-272 / 724-727), blocking:
 *                   overlapped = 0:  phase A -> ncclAllGather of the packed rows [z | grad_z | theta | grad_theta] -> phase B   (per step)
 *                   overlapped = 1:  values [z | theta] all-gathered on a side stream beside phase A (kernel-matrix slab behind the gather),
 *                                    only the gradient rows between the phases (see the step_update_planes protocol above)
 *                dibs_engine_gather_particles(e, z_all, theta_all)          all ranks' particles on every rank (sample()'s return value)
 * Results are bit-identical to dibs_engine_run of a single-rank engine, for any number of ranks. */
#define DIBS_COMM_ID_BYTES 128
int dibs_comm_unique_id(void* id_out);
int dibs_engine_comm_init(dibs_engine* e, const void* ids, int32_t n_ids);
int dibs_engine_comm_destroy(dibs_engine* e);
int dibs_engine_run_sharded(dibs_engine* e, int32_t t_start, int32_t n_steps, int32_t overlapped);
int dibs_engine_gather_particles(dibs_engine* e, float* z_all, float* theta_all);

/* The same loop with the exchange through MAPPED PEER MEMORY instead of RCCL (no reference counterpart; dibs_amd/csrc/exchange_ipc.h): ranks that
 * share one device -- where RCCL refuses a communicator ("duplicate GPU") -- or devices with peer access.  One PROCESS per rank:
 *   every rank:  dibs_engine_ipc_export(e, blob)          allocates the rank's exchange arena and writes DIBS_IPC_HANDLE_BYTES describing it
 *                                                         (hipIpcMemHandle + sizes); the bytes of ALL ranks go to every rank, in rank order,
 *                                                         by any means (a file, a pipe, torch.distributed.all_gather_object ...)
 *                dibs_engine_comm_init_ipc(e, blobs_all)  maps the peers' arenas (n_ranks * DIBS_IPC_HANDLE_BYTES bytes)
 *                dibs_engine_run_sharded / dibs_engine_gather_particles as above (both protocols); dibs_engine_comm_destroy unmaps.
 * The all-gather of a step is every rank storing its rows into every peer's arena plus one sequence word per peer and exchange; buffers
 * alternate between two copies, so no acknowledgement travels back.  A rank waits at most DIBS_IPC_TIMEOUT_MS (environment, read by
 * dibs_engine_comm_init_ipc; default 10 000) for its peers' rows, then the run returns an error.  Results are bit-identical to
 * dibs_engine_run of a single-rank engine and to the RCCL path. */
#define DIBS_IPC_HANDLE_BYTES 128
int dibs_engine_ipc_export(dibs_engine* e, void* blob_out);
int dibs_engine_comm_init_ipc(dibs_engine* e, const void* blobs_all);

/* BATCHED ENGINE (no reference counterpart; the JAX equivalent is vmap of the SVGD loop over keys and data): dibs_config.reserved_i[0] =
 * n_problems = B > 1 makes one engine hold B independent MarginalDiBS + BGe problems (score-function estimator, one rank).  They share
 * every size (d, k, n_particles = M PER PROBLEM, S, Sa), the graph prior and -- unless dibs_engine_set_problem_hparams says otherwise -- every
 * hyper-parameter; each has its own data, intervention mask, PRNG key and M particles.  Device arrays hold B * M rows, problem-major: dibs_engine_get_state / set_state / read_buffer see all of them
 * (their key argument must be NULL), and each launch of a step covers the whole batch.  Problem p ends bit-identical to a standalone engine
 * run with (x_p, mask_p, key_p) and the same chunking.  dibs_engine_create rejects joint models, the reparam estimator, n_ranks != 1 and
 * n_particles >= 256; dibs_engine_set_data / init_particles / eval_gradients / step_* / the sharded loop and dibs_score_graphs are refused.
 *   dibs_engine_set_data_problem(e, p, x, n_obs, mask, mean_obs)  the BGe statistics of problem p (x: f32 [n_obs, d]; n_obs may differ
 *                                                                 between problems; mask: i32 [n_obs, d] or NULL; mean_obs: f32 [d] or NULL)
 *   dibs_engine_init_particles_batch(e, keys)                      keys: u32 [B][2]; problem p as dibs_engine_init_particles(keys[p])
 *   dibs_engine_get_keys / dibs_engine_set_keys(e, keys)           the B loop-carry keys, u32 [B][2] */
int dibs_engine_set_data_problem(dibs_engine* e, int32_t p, const float* x, int32_t n_obs, const int32_t* interv_mask,
                                 const float* bge_mean_obs);
int dibs_engine_init_particles_batch(dibs_engine* e, const uint32_t* keys);
int dibs_engine_get_keys(dibs_engine* e, uint32_t* keys);
int dibs_engine_set_keys(dibs_engine* e, const uint32_t* keys);

/* PER-PROBLEM HYPER-PARAMETERS of a batched engine (a hyper-parameter sweep in one engine; the Python side is
 * dibs_amd.inference.sample_sweep).  The seven double fields of dibs_config that select no size, code path or buffer -- each is a scalar a
 * kernel of the standalone engine takes as a launch argument -- may differ between the problems of a batch.  A problem whose values were
 * never set has the configuration's.  Everything else stays shared: sizes, prior / optimizer / estimator kind, rng_layout, tau,
 * scale_latent, the BGe parameters.  Problem p still ends bit-identical to a standalone engine configured with p's values.
 *   dibs_engine_set_problem_hparams(e, p, hp)   validated as dibs_engine_create validates the shared value (Erdos-Renyi: edge probability
 *       in (0, 1); latent_prior_std <= 0: the default 1/sqrt(k)).  Only on a batched engine, and only before
 *       dibs_engine_init_particles_batch / dibs_engine_set_state / the first dibs_engine_run (latent_prior_std enters the initial draw; the
 *       device table is written once, then).  Values that differ from the configuration's need n_vars <= 64 and n_dim <= 64 (and the
 *       default acyclicity pipe: not DIBS_ACYC_BF16): the kernels of the larger sizes take them as launch arguments of the whole batch.
 *   dibs_engine_get_problem_hparams(e, p, hp)   the values in force (latent_prior_std as given, <= 0 meaning the default)
 * Every misuse fails with a message that starts "batched engine: ". */
typedef struct dibs_problem_hparams {
  double alpha_linear;
  double beta_linear;
  double h_latent;
  double stepsize;
  double score_function_baseline;
  double latent_prior_std;
  double graph_prior_edges_per_node;
} dibs_problem_hparams;
int dibs_engine_set_problem_hparams(dibs_engine* e, int32_t p, const dibs_problem_hparams* hp);
int dibs_engine_get_problem_hparams(dibs_engine* e, int32_t p, dibs_problem_hparams* hp);

/* CHAINS ENGINE (random restarts of a joint model; the JAX equivalent is vmap of the SVGD loop over keys): dibs_config.reserved_i[2] =
 * n_chains = C > 1 makes one engine run C independent chains of ONE JointDiBS model (LinearGaussian or DenseNonlinearGaussian, either Z
 * estimator, any graph prior, either optimizer) on ONE data set: the data, every size and every hyper-parameter are shared, each chain has
 * its own PRNG key and n_particles = M particles.  Device arrays hold C * M rows, chain-major; each launch of a step covers all chains, the
 * kernel matrices are block-diagonal [C * M][M] and the SVGD transform sums over a chain's own block.  Chain c ends bit-identical to a
 * standalone engine run with keys[c] and the same chunking.  It is driven by entry points that exist:
 *   dibs_engine_set_data(e, x, mask, NULL)              once: the data is shared;  OR, LinearGaussian only,
 *   dibs_engine_set_data_problem(e, c, x, n_obs, mask, NULL)   for EVERY chain c: chain c runs on a data set of its own (see below)
 *   dibs_engine_init_particles_batch(e, keys)           keys: u32 [C][2]; chain c as dibs_engine_init_particles(keys[c])
 *   dibs_engine_get_keys / dibs_engine_set_keys         the C loop-carry keys, u32 [C][2]
 *   dibs_engine_get_state / set_state / read_buffer     C * M rows, theta and v_theta included (their key argument must be NULL)
 *   dibs_engine_run                                     the steps
 * dibs_engine_create rejects n_chains < 0, n_problems > 1 together with chains, marginal models, n_ranks != 1, float64, n_particles >= 256
 * per chain (the GEMM form of the SVGD transform is not batched), more than 2^24 rows, and sizes at which a per-row array of C * M rows
 * (packed rows, scores, partial sums of the acyclicity term, log-probabilities, first-layer tables) would pass 2^31 elements.
 * dibs_engine_set_problem_hparams / init_particles, the sharded entry points, step_local* / step_update* / kmat_values,
 * dibs_engine_eval_gradients and dibs_score_graphs are refused.  Every such failure starts "chains engine (n_chains > 1): ".
 * PER-CHAIN DATA (the evaluation loop of a study: the same model on many data sets of one size; JointDiBS + LinearGaussian).  A chains
 * engine takes its data in exactly one of the two ways above.  With dibs_engine_set_data_problem the data, the masks and, where x does not
 * fit LDS, the Gram matrices are stacked per chain ([C][N][d], [C][n_gram][d][d]), and the six LinearGaussian kernel families run in a form
 * that takes the pointers and the intervention flag of the block's chain (row / M: block-uniform).  Chain c ends bit-identical to a
 * standalone engine given chain c's data and key -- also where some chains have interventions and others none (there a mask-free chain's
 * single Gram matrix is repeated n_vars times: the same doubles, summed in the same order).  Rules, each an error that starts
 * "chains engine (n_chains > 1): " and names the call: dibs_engine_set_data_problem after dibs_engine_set_data and dibs_engine_set_data
 * after dibs_engine_set_data_problem are refused (a new engine changes the way); a DenseNonlinearGaussian engine refuses it (its chains
 * share one data set); n_obs must equal dibs_config.n_observations (it selects LDS sizes and kernels), c must be in [0, C), bge_mean_obs
 * NULL; a chain's data may be given again until the particles are initialised (init_particles_batch / set_state / run), not after -- as
 * dibs_engine_set_problem_hparams; dibs_engine_run with some but not all chains given data fails and names the first missing chain (with
 * no data at all: "dibs_engine_set_data has not been called").
 * PER-CHAIN HYPER-PARAMETERS (a hyper-parameter grid of one joint model in one engine; the Python side is
 * dibs_amd.inference.sample_joint_sweep; JointDiBS + LinearGaussian).  The eight double fields of dibs_config below -- the seven of
 * dibs_problem_hparams and h_theta, the bandwidth of the parameter kernel -- may differ between the chains.  A chain whose values were never
 * set has the configuration's.  Everything else stays shared: sizes, N, S, Sa, prior / optimizer / estimator kind, tau, scale_*, rng_layout
 * and the likelihood's obs_noise, mean_edge, sig_edge.  Chain c ends bit-identical to a standalone engine configured with c's values.
 *   dibs_engine_set_chain_hparams(e, c, hp)   validated as dibs_engine_create validates the shared value (Erdos-Renyi: edge probability in
 *       (0, 1); latent_prior_std <= 0: the default 1/sqrt(k)); only before dibs_engine_init_particles_batch / dibs_engine_set_state / the
 *       first dibs_engine_run (latent_prior_std of chain c enters chain c's initial draw; the device table is written once, then).
 *   dibs_engine_get_chain_hparams(e, c, hp)   the values in force (latent_prior_std as given, <= 0 meaning the default)
 * Values equal to the configuration's are accepted on every chains engine and change nothing: the step is launch for launch the one of an
 * engine on which nothing was set.  Values that DIFFER from the configuration's
 *   - are accepted only on a LinearGaussian engine (the DenseNonlinearGaussian kernels have no per-chain form),
 *   - need n_vars <= 64, n_dim <= 64 and an acyclicity pipe other than bf16 (the sizes whose edge, acyclicity and tail kernels have
 *     table-reading forms, as for dibs_engine_set_problem_hparams),
 *   - need per-chain data: dibs_engine_set_data_problem for every chain (a sweep over one data set uploads it C times, C * N * d * 8 bytes
 *     with the mask).  dibs_engine_set_data on an engine that holds differing values is refused, and so are differing values on an engine
 *     whose data came through dibs_engine_set_data; dibs_engine_run with differing values and no per-chain data fails and says so.
 * With differing values a step forms every chain's annealed alpha and beta on the device (in double, as the host does for a standalone
 * engine), the edge, acyclicity, tail and kernel-matrix launches read the chain's row of the device table, and the per-chain forms of the
 * LinearGaussian kernels take alpha and score_function_baseline of the block's chain from it.  Every misuse fails with a message that
 * starts "chains engine (n_chains > 1): " and names the call. */
typedef struct dibs_chain_hparams {
  double alpha_linear;
  double beta_linear;
  double h_latent;
  double h_theta;
  double stepsize;
  double score_function_baseline;
  double latent_prior_std;
  double graph_prior_edges_per_node;
} dibs_chain_hparams;
int dibs_engine_set_chain_hparams(dibs_engine* e, int32_t c, const dibs_chain_hparams* hp);
int dibs_engine_get_chain_hparams(dibs_engine* e, int32_t c, dibs_chain_hparams* hp);

/* FLOAT64 ENGINE (no reference counterpart as such: the reference reaches double precision through JAX_ENABLE_X64,
 * dibs/models/nonlinearGaussian.py:183-185): dibs_config.reserved_i[1] = 64 makes the engine compute what the f64 build of the oracle
 * (oracle/dibs_oracle.c with real = double) computes.  The random draws stay the f32 streams of the f32 engine (Threefry bits, f32 uniform /
 * normal / logistic values); everything after a draw is double: the data and the BGe statistics, scores, edge probabilities, matrix powers,
 * node scores, softmax weights, gradients, kernel matrix, phi, z, v_z and the baselines.  A Bernoulli edge compares the f32 uniform with
 * the edge probability rounded to float, as the oracle does, so the sampled graphs equal the f64 oracle's bit for bit.  The two draws that
 * pass through a C-library function -- the initial normals (log1p) and the acyclicity logistic values (logf) -- take their value from the
 * host's C library in the oracle's order (a table over the 2^23 f32 uniforms for the logistic), so they too equal the oracle's.  This is NOT JAX's
 * x64 stream (under x64, JAX draws float64 uniforms from 64 random bits).
 * Supported: MarginalDiBS + BGe, score-function estimator, one rank, one problem, 2 <= n_vars <= 64, n_particles <= 1024 (any prior,
 * interventions, bge_mean_obs, baseline, optimizer, rng layout).  dibs_engine_create rejects everything else with an error that starts
 * "float64 engine:", before any device call.  dibs_engine_run steps it; dibs_engine_read_buffer / dibs_engine_buffer_bytes give the float
 * buffers (Z, V_Z, SCORES, LOGPROBS_Z, W_LIK, W_ACYC, GRAD_Z, KXX, PHI_Z, BASELINE) as f64 arrays, NODE_SCORES / PARENT_MASKS unchanged;
 * the other ids (theta, packed / gathered rows) do not exist on a float64 engine (buffer_bytes -1, read_buffer fails).
 * dibs_engine_set_data accepts f32 data (widened exactly); dibs_engine_get_state / set_state / eval_gradients / step_* / the sharded loop /
 * gather_particles and dibs_score_graphs fail on a float64 engine (they would round).
 *   dibs_engine_set_data_f64(e, x, mask, mean_obs)   x: f64 [N, d]; mask: i32 [N, d] or NULL; mean_obs: f64 [d] or NULL
 *   dibs_engine_set_state_f64 / get_state_f64        as the f32 pair with double z, v_z [M, d, k, 2] and baseline [M]; theta, v_theta NULL
 *   dibs_engine_precision(e)                         32 or 64 (-1: null handle) */
int dibs_engine_set_data_f64(dibs_engine* e, const double* x, const int32_t* interv_mask, const double* bge_mean_obs);
int dibs_engine_set_state_f64(dibs_engine* e, const double* z, const double* v_z, const double* theta, const double* v_theta,
                              const uint32_t* key, const double* baseline);
int dibs_engine_get_state_f64(dibs_engine* e, double* z, double* v_z, double* theta, double* v_theta, uint32_t* key, double* baseline);
int dibs_engine_precision(const dibs_engine* e);

/* EDGE-WISE GRAPH PRIOR (no reference counterpart as a class; in the reference any traced graph_model object is accepted, this is the
 * commonest one: independent edges, each with a probability of its own).  dibs_config.graph_prior = DIBS_PRIOR_EDGEWISE and
 *   dibs_engine_set_edge_prior(e, edge_probs)   edge_probs: f64 [d][d] row-major, edge_probs[i][j] = prior probability of the edge i -> j;
 *       the diagonal is ignored, every other entry must be finite and strictly inside (0, 1) (the rule of the Erdos-Renyi prior: the
 *       log odds must be finite; "forbidden" and "required" are probabilities such as 1e-6 and 1 - 1e-6 -- p(G | Z) is not masked).
 * The soft log-prior is sum_{i != j} g_ij L_ij with L = log(p) - log(1 - p) formed in double (as the Erdos-Renyi constant is) and kept on
 * the device as float (float32 engine) or double (float64 engine), diagonal 0; its derivative takes the place of the Erdos-Renyi constant
 * in the per-particle gradient kernel, so a table with the Erdos-Renyi probability in every entry reproduces DIBS_PRIOR_ER bit for bit.
 * The call may be repeated between runs (the copy is ordered on the engine's stream).  It fails on an engine whose prior is not
 * DIBS_PRIOR_EDGEWISE, for a null argument and for an entry outside (0, 1), naming the entry.  Until it has been called, dibs_engine_run /
 * run_sharded / step_local / step_local_grads / eval_gradients fail with "dibs_engine_set_edge_prior has not been called".
 * One table per engine: the chains of a chains engine share it.  The batched marginal engine (n_problems > 1) refuses the prior at
 * creation and a chains engine with per-chain hyper-parameters that differ refuses it when the particles are initialised: the
 * table-reading kernels of those tiers have no edge-wise form, and per-problem tables are not built. */
int dibs_engine_set_edge_prior(dibs_engine* e, const double* edge_probs);

/* MEDIAN-HEURISTIC KERNEL BANDWIDTH (no reference counterpart: the reference's kernels take fixed h; the rule is Liu & Wang 2016).
 * dibs_config.reserved_i[3] != 0 makes the engine select a kernel's bandwidth on the device in every step, per RUN (the M particles of a
 * standalone engine, of one problem of a batched engine, of one chain) and per SEGMENT (bit 0: latent z, bit 1: parameters theta):
 *   v_ab = (float)tot_ab, tot_ab the double sum of squared differences the kernel-matrix code forms for the pair (a, b) before its exp;
 *   med  = median of the P = M (M - 1) / 2 values v_ab, a < b: P odd the order statistic (P - 1) / 2, P even 0.5f * (v[P/2 - 1] + v[P/2]);
 *   h    = max((float)((double)med * (1 / log((double)(M + 1)))), FLT_MIN)    (the floor: more than half of the pairs identical)
 * and the kernel matrix is what it always is, (float)(scale * exp(-tot_ab / (double)h)).  The selection is exact (a radix select on the bit
 * patterns, integer counting) and so bit-reproducible; non-finite distances give an unspecified but deterministic h.  h_latent / h_theta
 * of a segment on the rule are not read.  A step with the rule equals, bit for bit, the step of a fixed-rule engine configured with the
 * float values DIBS_BUF_BANDWIDTH reports for it.  The kernel matrices are then launches of their own behind the selection (distance
 * pass -> selection -> kernel matrices on one stream; none of the fused placements of the fixed rule), also in dibs_engine_step_local /
 * dibs_engine_step_update of a single rank.  Batched and chains engines take the rule as they take per-run bandwidths: run i stays
 * bit-identical to the standalone engine.  With reserved_i[3] == 0 the engine is launch for launch what it was.
 * Limits, each an error of dibs_engine_create that starts "median bandwidth: ": n_particles (per run) >= 256 (the GEMM form of the SVGD
 * transform has no table-reading form and the selection is one block per run: the follow-up), n_particles < 2, n_ranks > 1, the float64
 * engine, bit 1 on a marginal model, a rule outside 0 .. 3; dibs_engine_kmat_values on such an engine fails the same way. */

/* BDEU: MarginalDiBS on DISCRETE data (no reference counterpart as a class; the score is the Bayesian-Dirichlet equivalent uniform
 * marginal likelihood of Heckerman, Geiger & Chickering 1995).  dibs_config.likelihood = DIBS_LIK_BDEU, dibs_config.reserved_d[0] = the
 * equivalent sample size eta (<= 0: 1.0).  x holds category codes as floats: variable i has arity r_i and takes the values 0 .. r_i - 1.
 *   node j uses the rows n with interv_mask[n, j] == 0 (a parent's value is used in every such row);  pa = {i : g[i, j] = 1}
 *   log a = log eta - sum_{i in pa} log r_i,   log a' = log a - log r_j
 *   rise(log alpha, n) = 0 for n = 0,  log alpha + sum_{i=1}^{n-1} log(exp(log alpha) + i) for n >= 1   (= lgamma(alpha + n) - lgamma(alpha))
 *   score_j = sum over the parent configurations c that occur in the used rows:  - rise(log a, N_c) + sum_k rise(log a', N_ck)
 *   log p(D | G) = sum_j score_j;  a node without used rows scores 0.
 * All arithmetic is double, counts are integers, and the value does not depend on the order in which threads arrive.
 * The step is the BGe score estimator's with one kernel exchanged: the same sampling launch (the same Threefry streams, so the same
 * graphs for a key), k_bdeu_nodes in the place of the factorisation, then everything that consumes DIBS_BUF_NODE_SCORES.  Its time is
 * reported under DIBS_K_BGE_BIG.  DIBS_BUF_NODE_SCORES / DIBS_BUF_PARENT_MASKS read back as for BGe.
 *   dibs_engine_set_arities(e, arities)   arities: i32 [d].  Required before dibs_engine_set_data and before dibs_score_graphs on a BDeu
 *       engine (either call without it is an error, never a default); an error on an engine that is not BDeu.  Fails for an arity outside
 *       2 .. 16 and when the bit fields of a packed row (ceil(log2 r_i) bits per variable, no field straddling a 64-bit word) need more
 *       than 512 bits -- e.g. 256 variables of arity <= 4 or 128 of arity <= 16 fit.  Calling it again discards the engine's data.
 * dibs_engine_set_data / dibs_score_graphs keep their signatures; they check every entry of x / x_ho to be integral and in [0, r_i) and
 * fail with the row and column of the first that is not.  n_observations / n_ho may be at most 4096 (one wave's grouping table must fit a
 * block's LDS; the message states the limit).  On a BDeu engine dibs_score_graphs works in chunks of n_grad_mc_samples graphs and leaves
 * the last chunk's parent sets and per-node scores (double) in DIBS_BUF_PARENT_MASKS / DIBS_BUF_NODE_SCORES, laid out [d][S'][W] / [d][S']
 * with S' the chunk's graph count, at the start of the buffers: `out` is float, the sum over the nodes of those doubles is not rounded.
 * dibs_engine_create refuses, each with a message that starts "BDeu: ": joint = 1, the reparam estimator (a count-based score has no
 * soft-graph form), n_observations > 4096.  The float64, batched and chains engines refuse the likelihood as they refuse any but their own. */
int dibs_engine_set_arities(dibs_engine* e, const int32_t* arities);

/* debugging / parity: copy a device buffer to the host (nbytes must match); theta size query */
int dibs_engine_read_buffer(dibs_engine* e, int32_t which, void* host, int64_t nbytes);
int64_t dibs_engine_buffer_bytes(const dibs_engine* e, int32_t which);
int64_t dibs_engine_theta_size(const dibs_engine* e);

/* per-kernel HIP-event timers.  enable=1 brackets every launch with events on the stream it is launched on and serialises the step
 * (the main stream waits for the acyclicity kernel before it continues: each duration is the kernel alone on the GPU); enable=2 keeps the production schedule -- the acyclicity kernel on the engine's second
 * stream beside the likelihood kernels -- and times it with events on that stream (durations of overlapping kernels include the sharing). */
int dibs_engine_set_profiling(dibs_engine* e, int32_t enable);
/* Gradient estimators of ONE step for the engine's current particles (dibs_engine_set_state) with EXPLICIT per-particle PRNG keys --
 * what the reference exposes as DiBS.eltwise_grad_z_likelihood(zs, thetas, baselines, t, subkeys) -> (grads, baselines)
 * (dibs/inference/dibs.py:295-321), DiBS.eltwise_grad_theta_likelihood(zs, thetas, t, subkeys) (:467-485) and
 * DiBS.eltwise_grad_latent_prior(zs, subkeys, t) (:626-658).  Same kernels as a step of dibs_engine_run, only the key of particle m
 * is keys_*[m] instead of row 1 + m of split(loop-carry key, M + 1); the loop-carry key does not advance.
 *   keys_theta / keys_lik / keys_prior : uint32 [Mloc][2] host arrays or NULL (NULL, NULL -> no likelihood pass; keys_prior NULL -> no
 *                                        prior pass).  Joint models run the theta and the Z estimator in one pass: pass both or neither.
 *   grad_z_lik  [Mloc][d][k][2] : estimator of grad_Z log p(theta, D | Z);  baseline_out [Mloc]: the updated score-function baselines
 *                                 (input baselines = the engine's state);  grad_theta [Mloc][P]: estimator of grad_theta (joint only)
 *   grad_z_prior [Mloc][d][k][2]: -beta(t) E[grad h] - Z / sigma_z^2 + grad log p(G_alpha(Z))
 * Any output may be NULL.  Blocking.  The loop state -- particles, optimizer moments, loop-carry key, score-function baselines -- is left
 * untouched (the updated baselines are only returned); the per-step scratch of the engine (packed rows, W_lik, log-probabilities, queues)
 * is overwritten, as by any step. */
int dibs_engine_eval_gradients(dibs_engine* e, int32_t t, const uint32_t* keys_theta, const uint32_t* keys_lik, const uint32_t* keys_prior,
                               float* grad_z_lik, float* baseline_out, float* grad_theta, float* grad_z_prior);
int dibs_engine_get_timers(dibs_engine* e, double* total_ms, int64_t* launches, int32_t n); /* arrays of DIBS_K_COUNT */
int dibs_engine_reset_timers(dibs_engine* e);
/* effective (executed) flop / problem-size counters of the BGe node kernel for the roofline */
int dibs_engine_get_counters(dibs_engine* e, double* out, int32_t n);

/* replaces likelihood_model.interventional_log_marginal_prob / interventional_log_joint_prob evaluated on a
 * batch of hard graphs (svgd.py:110-113, 370-372, 475-478, 838-841): g: i32 [n, d, d]; theta: f32 [n, P] or
 * NULL; x_ho: f32 [n_ho, d]; mask_ho: i32 [n_ho, d] or NULL; out: f32 [n]. */
int dibs_score_graphs(dibs_engine* e, const int32_t* g, const float* theta, int32_t n, const float* x_ho,
                      const int32_t* mask_ho, int32_t n_ho, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIBS_HIP_H */
