// The float64 engine's host side (dibs_config.reserved_i[1] = 64, include/dibs_hip.h; kernels in kernels_f64.h / tu_f64.hip): host draws,
// buffers, the step, state accessors.  Its data entry point (dibs_engine_set_data_f64) is with the BGe statistics in engine_data.hip.
#include "engine_impl.h"

// The float64 engine's draws whose value passes through a C-library function rounded to float: jax.random.normal's -log1p (erfinv) and
// jax.random.logistic's logf.  The f64 oracle (oracle/dibs_oracle.c: normal_from_bits, logistic_from_bits) calls the C library; no device
// math library rounds exactly as it does (glibc's logf differs from the correctly rounded value for ~0.5 % of these arguments, and its
// variant depends on the CPU).  So these values come from the host's C library, in the oracle's operation order: the initial normal draws
// directly (dibs_engine_init_particles, once per run), the logistic draws through a table over all 2^23 f32 uniforms (an f32 uniform is
// (bits >> 9) * 2^-23 mapped onto [lo, 1): 23 bits decide it), built once per process and flag and read by k64_acyc.
static float f64_host_normal(uint32_t bits) {
  static const float A[9] = {2.81022636e-08f, 3.43273939e-07f, -3.5233877e-06f, -4.39150654e-06f, 0.00021858087f,
                             -0.00125372503f, -0.00417768164f, 0.246640727f, 1.50140941f};
  static const float B[9] = {-0.000200214257f, 0.000100950558f, 0.00134934322f, -0.00367342844f, 0.00573950773f,
                             -0.0076224613f, 0.00943887047f, 1.00167406f, 2.83297682f};
  const float x = rng_uniform(bits, -0.99999994f, 1.0f);  // (host: every operation rounded on its own, rng.h)
  volatile float xx = -x * x;
  float w = (float)(-log1p((double)xx));
  const float* cf = w < 5.0f ? A : B;
  w = w < 5.0f ? w - 2.5f : sqrtf(w) - 3.0f;
  float p = cf[0];
  for (int i = 1; i < 9; ++i) {
    volatile float pw = p * w;
    p = cf[i] + pw;
  }
  volatile float px = p * x;
  return 1.41421354f * px;
}
static const float* f64_logistic_table(int tiny) {
  static std::mutex mu;
  static std::vector<float> tab[2];
  std::lock_guard<std::mutex> lock(mu);
  std::vector<float>& t = tab[tiny ? 1 : 0];
  if (t.empty()) {
    t.resize((size_t)1 << 23);
    const float lo = tiny ? 1.17549435e-38f : 1.1920929e-07f;
    for (uint32_t i = 0; i < (1u << 23); ++i) {
      const float x = rng_uniform(i << 9, lo, 1.0f);
      volatile float q = x / (1.0f - x);
      t[i] = logf(q);
    }
  }
  return t.data();
}

// the float64 engine's buffers (after engine_alloc, which allocated the parent-set and node-score buffers of the same layouts as the f32
// engine's)
int f64_alloc(dibs_engine* e) {
  e->f64 = new F64State();
  F64State& f = *e->f64;
  const size_t Ml = e->Mloc, dd = (size_t)e->d * e->d;
  HIP_OK(dalloc(&f.ltab, (size_t)1 << 23));
  HIP_OK(hipMemcpy(f.ltab, f64_logistic_table(e->cfg.logistic_minval_tiny), ((size_t)1 << 23) * 4, hipMemcpyHostToDevice));
  HIP_OK(dalloc(&f.z, Ml * e->D));
  HIP_OK(dalloc(&f.vz, Ml * e->D));
  HIP_OK(dalloc(&f.baseline, Ml));
  HIP_OK(dalloc(&f.scores, Ml * dd));
  HIP_OK(dalloc(&f.probs, Ml * dd));
  HIP_OK(dalloc(&f.thr, Ml * dd));
  HIP_OK(dalloc(&f.w_lik, Ml * dd));
  HIP_OK(dalloc(&f.w_acyc, Ml * dd));
  HIP_OK(dalloc(&f.part, Ml * e->Sa * dd));
  HIP_OK(dalloc(&f.logprobs, Ml * e->S));
  HIP_OK(dalloc(&f.gradz, Ml * e->D));
  HIP_OK(dalloc(&f.kxx, Ml * e->M));
  HIP_OK(dalloc(&f.phi, Ml * e->D));
  hipDeviceSynchronize();  // (the zero fills ran on the null stream)
  return 0;
}

// z = (double)(normal_f32 * std_f32), the oracle's orc_init_particles (see f64_host_normal); isub: the key of dibs_engine_init_particles
int f64_init_particles(dibs_engine* e, Key2 isub) {
  const int L = e->cfg.rng_layout;
  const uint64_t ntot = (uint64_t)e->M * e->D, nloc = (uint64_t)e->Mloc * e->D;
  std::vector<double> z(nloc);
  for (uint64_t i = 0; i < nloc; ++i) {
    volatile float v = f64_host_normal(rng_bits_at(isub, ntot, (uint64_t)e->m0 * e->D + i, L)) * e->sigz;
    z[i] = (double)v;
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  HIP_OK(hipMemcpy(e->f64->z, z.data(), nloc * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(e->f64->vz, 0, nloc * 8));
  HIP_OK(hipMemset(e->f64->baseline, 0, (size_t)e->Mloc * 8));
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

// ---- float64 engine (dibs_config.reserved_i[1] = 64, include/dibs_hip.h; kernels_f64.h) ----------------------------------------------
// One step: the loop-carry key advances as in step_local (split for the likelihood, then for the prior); edge scores on the main stream,
// the acyclicity chains, their reduction and the kernel matrix on the second stream (fork / join by events: EventFork, as step_multi), BGe sampling and
// node scores -> weights -> per-particle gradient -> phi -> optimizer on the main stream.
int step_f64(dibs_engine* e, int t) {
  const dibs_config& c = e->cfg;
  const F64State& f = *e->f64;
  F64Args a{};
  a.d = e->d; a.k = e->k; a.M = e->M; a.S = e->S; a.Sa = e->Sa; a.dpad = e->dpad; a.L = c.rng_layout; a.tiny = c.logistic_minval_tiny;
  a.prior = c.graph_prior; a.opt = c.optimizer; a.n_mats = f.n_mats; a.D = e->D;
  a.alpha = c.alpha_linear * t;
  a.beta = c.beta_linear * t;
  a.tau = c.tau;
  a.er_c = er_log_odds(c);
  a.prior_tab = e->edge_tab64;  // (DIBS_PRIOR_EDGEWISE: present, dibs_engine_run asks need_edge_prior)
  const double sigz = c.latent_prior_std > 0 ? c.latent_prior_std : (double)(1.0f / sqrtf((float)e->k));  // (the oracle's latent_std)
  a.inv_sig2 = 1.0 / (sigz * sigz);
  a.sfb = c.score_function_baseline;
  a.h = c.h_latent;
  a.scale = c.scale_latent;
  a.step = c.stepsize;
  a.alpha_lambd = f.alpha_lambd;
  a.carry_lik = e->key;
  a.carry_prior = next_carry(e, a.carry_lik);
  e->key = next_carry(e, a.carry_prior);
  a.z = f.z; a.vz = f.vz; a.baseline = f.baseline; a.scores = f.scores; a.probs = f.probs; a.w_lik = f.w_lik; a.w_acyc = f.w_acyc;
  a.part = f.part; a.logprobs = f.logprobs; a.gradz = f.gradz; a.kxx = f.kxx; a.phi = f.phi; a.thr = f.thr; a.masks = e->masks;
  a.node_scores = e->node_scores; a.R = f.R; a.Nj = f.Nj; a.gam = f.gam; a.ltab = f.ltab;
  {
    KTimer tm(e, DIBS_K_EDGE);
    f64_launch_edge(e->stream, a);
  }
  const EventFork ef(e);
  hipStream_t s2 = ef.s2;
  if (ef.fork()) return 1;
  {
    KTimer tm(e, DIBS_K_ACYC, s2);
    f64_launch_acyc(s2, a);
  }
  {
    KTimer tm(e, DIBS_K_ACYC_REDUCE, s2);
    f64_launch_acyc_reduce(s2, a);
  }
  {
    KTimer tm(e, DIBS_K_KMAT, s2);
    f64_launch_kmat(s2, a);
  }
  if (ef.chain_done()) return 1;
  {
    KTimer tm(e, DIBS_K_BGE_NODES);
    f64_launch_bge(e->stream, a);
  }
  {
    KTimer tm(e, DIBS_K_LIK_WEIGHTS);
    f64_launch_weights(e->stream, a);
  }
  if (ef.join()) return 1;
  {
    KTimer tm(e, DIBS_K_ZGRAD);
    f64_launch_grad(e->stream, a);
  }
  {
    KTimer tm(e, DIBS_K_PHI_UPDATE);
    f64_launch_phi(e->stream, a);
    f64_launch_update(e->stream, a);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
  return 0;
}

// ---- state, precision (include/dibs_hip.h) ----------------------------------------------------------------------
extern "C" int dibs_engine_precision(const dibs_engine* e) { return !e ? -1 : (e->f64 ? 64 : 32); }

extern "C" int dibs_engine_set_state_f64(dibs_engine* e, const double* z, const double* v_z, const double* theta, const double* v_theta,
                                         const uint32_t* key, const double* baseline) {
  if (!e) return fail("null engine");
  if (!e->f64) return fail("dibs_engine_set_state_f64: not a float64 engine (dibs_config.reserved_i[1] = 64)");
  if (theta || v_theta) return fail("float64 engine: theta / v_theta must be null (MarginalDiBS has no parameters)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const size_t nz = (size_t)e->Mloc * e->D * 8;
  if (z) HIP_OK(hipMemcpy(e->f64->z, z, nz, hipMemcpyHostToDevice));
  if (v_z) HIP_OK(hipMemcpy(e->f64->vz, v_z, nz, hipMemcpyHostToDevice));
  if (key) e->key = Key2{key[0], key[1]};
  if (baseline) HIP_OK(hipMemcpy(e->f64->baseline, baseline, (size_t)e->Mloc * 8, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int dibs_engine_get_state_f64(dibs_engine* e, double* z, double* v_z, double* theta, double* v_theta, uint32_t* key, double* baseline) {
  if (!e) return fail("null engine");
  if (!e->f64) return fail("dibs_engine_get_state_f64: not a float64 engine (dibs_config.reserved_i[1] = 64)");
  if (theta || v_theta) return fail("float64 engine: theta / v_theta must be null (MarginalDiBS has no parameters)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const size_t nz = (size_t)e->Mloc * e->D * 8;
  if (z) HIP_OK(hipMemcpy(z, e->f64->z, nz, hipMemcpyDeviceToHost));
  if (v_z) HIP_OK(hipMemcpy(v_z, e->f64->vz, nz, hipMemcpyDeviceToHost));
  if (key) {
    key[0] = e->key.a;
    key[1] = e->key.b;
  }
  if (baseline) HIP_OK(hipMemcpy(baseline, e->f64->baseline, (size_t)e->Mloc * 8, hipMemcpyDeviceToHost));
  return 0;
}
