// Data of an engine (include/dibs_hip.h): BGe sufficient statistics on the host, dibs_engine_set_data / _problem / _f64, and
// dibs_score_graphs.
#include "engine_impl.h"

// in-place inverse and log-determinant of an SPD matrix (Cholesky, double)
static bool spd_inverse_logdet(std::vector<double>& a, int n, double* logdet) {
  std::vector<double> L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0);
  double ld = 0;
  for (int j = 0; j < n; ++j) {
    double s = a[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) s -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(s > 0.0)) return false;
    const double dj = sqrt(s);
    ld += 2.0 * log(dj);
    L[(size_t)j * n + j] = dj;
    for (int i = j + 1; i < n; ++i) {
      double t = a[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = t / dj;
    }
  }
  for (int c = 0; c < n; ++c) {  // Li = L^-1 (lower), column by column
    Li[(size_t)c * n + c] = 1.0 / L[(size_t)c * n + c];
    for (int i = c + 1; i < n; ++i) {
      double t = 0;
      for (int k = c; k < i; ++k) t -= L[(size_t)i * n + k] * Li[(size_t)k * n + c];
      Li[(size_t)i * n + c] = t / L[(size_t)i * n + i];
    }
  }
  for (int i = 0; i < n; ++i)  // A^-1 = Li^T Li
    for (int j = 0; j <= i; ++j) {
      double t = 0;
      for (int k = i; k < n; ++k) t += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
      a[(size_t)i * n + j] = a[(size_t)j * n + i] = t;
    }
  *logdet = ld;
  return true;
}

// The host part of bge_prepare: the statistics of one data set (n_mats = 1 without interventions, d with) in double -- R_j, N_j, the table
// of log_gamma_term and the scalars -- from float or double observations.  The float64 engine uploads them as they are; the float32
// engine derives its float forms from them (bge_f32_forms).
struct BgeHost {
  int n_mats = 1;
  double alpha_lambd = 0, alpha_mu = 0, log_t = 0;
  std::vector<double> R, Nj, gam;
};
template <typename T>
static int bge_host_stats(BgeHost* st, const dibs_config& cfg, int d, int N, const T* x, const int32_t* mask, const T* mean_obs) {
  const double amu = cfg.bge_alpha_mu;
  st->alpha_lambd = cfg.bge_alpha_lambd > 0 ? cfg.bge_alpha_lambd : d + 2.0;
  if (!(st->alpha_lambd > d + 1)) return fail("BGe: alpha_lambd must be > n_vars + 1");  // linearGaussian.py:47
  const double small_t = amu * (st->alpha_lambd - d - 1) / (amu + 1);
  st->alpha_mu = amu;
  st->log_t = log(small_t);
  bool any = false;
  if (mask)
    for (int64_t i = 0; i < (int64_t)N * d; ++i) any |= mask[i] != 0;
  st->n_mats = any ? d : 1;
  const int n_mats = st->n_mats;
  std::vector<double>& R = st->R;
  std::vector<double>& Nj = st->Nj;
  std::vector<double>& gam = st->gam;
  R.assign((size_t)n_mats * d * d, 0.0);
  Nj.assign(d, 0.0);
  gam.assign((size_t)d * (d + 1), 0.0);
  // With interventions this is d matrices of d^2 sums over N rows (1.3e10 products at d = 256, N = 768: 18 s as a plain triple loop, found
  // by tests/test_gpu_max_size.py).  The sums s[a][b] = s[b][a] run over the centred rows xc of the node, b innermost: every s[a][b] adds
  // the same terms in the same order as the triple loop did (a row that is left out adds 0 * 0), so R is the same to the last bit.
  std::vector<double> xb(d), xc((size_t)N * d), s(d);
  for (int jm = 0; jm < n_mats; ++jm) {
    double Nn = 0;
    for (int n = 0; n < N; ++n) Nn += (any && mask[(int64_t)n * d + jm]) ? 0.0 : 1.0;
    for (int a = 0; a < d; ++a) {
      double sa = 0;
      for (int n = 0; n < N; ++n)
        if (!(any && mask[(int64_t)n * d + jm])) sa += (double)x[(int64_t)n * d + a];
      xb[a] = Nn > 0 ? sa / Nn : 0.0;
    }
    for (int n = 0; n < N; ++n) {
      const bool out = any && mask[(int64_t)n * d + jm];
      for (int a = 0; a < d; ++a) xc[(size_t)n * d + a] = out ? 0.0 : (double)x[(int64_t)n * d + a] - xb[a];
    }
    const double f = Nn * amu / (Nn + amu);
    for (int a = 0; a < d; ++a) {
      for (int b = a; b < d; ++b) s[b] = 0;
      for (int n = 0; n < N; ++n) {
        const double* __restrict__ row = xc.data() + (size_t)n * d;
        double* __restrict__ sp = s.data();
        const double xa = row[a];
        for (int b = a; b < d; ++b) sp[b] += xa * row[b];
      }
      const double ma = mean_obs ? (double)mean_obs[a] : 0.0;
      for (int b = a; b < d; ++b) {
        const double mb = mean_obs ? (double)mean_obs[b] : 0.0;
        R[(size_t)jm * d * d + (size_t)a * d + b] = (a == b ? small_t : 0.0) + s[b] + f * (xb[a] - ma) * (xb[b] - mb);
        if (b != a) R[(size_t)jm * d * d + (size_t)b * d + a] = 0.0 + s[b] + f * (xb[b] - mb) * (xb[a] - ma);
      }
    }
    if (any) Nj[jm] = Nn;
    else
      for (int j = 0; j < d; ++j) Nj[j] = Nn;
  }
  for (int j = 0; j < d; ++j)
    for (int l = 0; l <= d; ++l) {
      const double Nn = Nj[j], al = st->alpha_lambd;
      gam[(size_t)j * (d + 1) + l] = 0.5 * (log(amu) - log(Nn + amu)) + lgamma(0.5 * (Nn + al - d + l + 1)) -
                                     lgamma(0.5 * (al - d + l + 1)) - 0.5 * Nn * log(M_PI) +
                                     0.5 * (al - d + 2 * l + 1) * log(small_t);
    }
  return 0;
}

// R as float, R padded to (d + 1) x (d + 1), its inverse (padded) and log-determinant: what the f32 kernels read (kernels_bge.h)
struct BgeHostF32 {
  std::vector<float> R, Rp, Qp;
  std::vector<double> ldR;
};
static int bge_f32_forms(BgeHostF32* f, const BgeHost& h, int d) {
  const int n_mats = h.n_mats, dp = d + 1;
  f->R.assign(h.R.begin(), h.R.end());
  f->Rp.assign((size_t)n_mats * dp * dp, 0.f);
  f->Qp.assign((size_t)n_mats * dp * dp, 0.f);
  f->ldR.assign(n_mats, 0.0);
  for (int jm = 0; jm < n_mats; ++jm) {
    std::vector<double> Rd(h.R.begin() + (size_t)jm * d * d, h.R.begin() + (size_t)(jm + 1) * d * d);
    for (int a = 0; a < d; ++a)
      for (int b = 0; b < d; ++b) f->Rp[(size_t)jm * dp * dp + (size_t)a * dp + b] = (float)Rd[(size_t)a * d + b];
    if (!spd_inverse_logdet(Rd, d, &f->ldR[jm])) return fail("BGe: R is not positive definite");
    for (int a = 0; a < d; ++a)
      for (int b = 0; b < d; ++b) f->Qp[(size_t)jm * dp * dp + (size_t)a * dp + b] = (float)Rd[(size_t)a * d + b];
  }
  return 0;
}

static int bge_prepare(BgeStats* st, const dibs_config& cfg, int d, int N, const float* x, const int32_t* mask, const float* mean_obs) {
  st->release();
  BgeHost h;
  BgeHostF32 f;
  if (bge_host_stats(&h, cfg, d, N, x, mask, mean_obs) || bge_f32_forms(&f, h, d)) return 1;
  st->alpha_lambd = h.alpha_lambd;
  st->alpha_mu = h.alpha_mu;
  st->log_t = h.log_t;
  st->n_mats = h.n_mats;
  const std::vector<float> &R = f.R, &Rp = f.Rp, &Qp = f.Qp;
  const std::vector<double> &Nj = h.Nj, &gam = h.gam, &ldR = f.ldR;
  HIP_OK(dalloc(&st->R, R.size()));
  // R and Q = R^-1 in one allocation: the factorisation kernel addresses a problem's matrix as a 32-bit float offset from Rp, and two
  // separate hipMalloc blocks can lie more than 2^31 floats apart on a 288 GB device (intermittent memory faults with interventions or
  // d > 80, where the matrices are not LDS-resident; found by tests/tools/gpu_fuzz.py)
  HIP_OK(dalloc(&st->Rp, Rp.size() + Qp.size()));
  st->Qp = st->Rp + Rp.size();
  HIP_OK(dalloc(&st->gam, gam.size()));
  HIP_OK(dalloc(&st->Nj, Nj.size()));
  HIP_OK(dalloc(&st->ldR, ldR.size()));
  HIP_OK(hipMemcpy(st->R, R.data(), R.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st->Rp, Rp.data(), Rp.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st->Qp, Qp.data(), Qp.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st->gam, gam.data(), gam.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st->Nj, Nj.data(), Nj.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st->ldR, ldR.data(), ldR.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// ---- BDeu: arities, packed data, the launch (include/dibs_hip.h, BDEU; bdeu_score.h) --------------------------------------------------------
extern "C" int dibs_engine_set_arities(dibs_engine* e, const int32_t* arities) {
  if (!e || !arities) return fail("null argument");
  if (!e->bdeu) return fail("dibs_engine_set_arities: not a BDeu engine (dibs_config.likelihood = DIBS_LIK_BDEU)");
  const int d = e->d;
  for (int i = 0; i < d; ++i)
    if (arities[i] < BDEU_MIN_ARITY || arities[i] > BDEU_MAX_ARITY)
      return fail("BDeu: arity " + std::to_string(arities[i]) + " of variable " + std::to_string(i) + " is outside the supported range [" +
                  std::to_string(BDEU_MIN_ARITY) + ", " + std::to_string(BDEU_MAX_ARITY) + "]");
  std::vector<BdeuField> f((size_t)d);
  const int KW = bdeu_layout(arities, d, f.data());
  if (KW > BDEU_MAX_KW)
    return fail("BDeu: the bit fields of a packed row need " + std::to_string(KW) + " 64-bit words, more than " + std::to_string(BDEU_MAX_KW) +
                " (512 bits: e.g. 256 variables of arity <= 4 or 128 of arity <= 16)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  BdeuState& b = *e->bdeu;
  e->has_data = false;  // (data packed under another layout is gone)
  e->score_cache.valid = false;
  b.train.release();
  b.ho.release();
  b.arities.assign(arities, arities + d);
  b.fields = f;
  b.KW = KW;
  std::vector<double> lr((size_t)d);
  for (int i = 0; i < d; ++i) lr[i] = log((double)arities[i]);
  if (!b.d_fields) HIP_OK(dalloc(&b.d_fields, (size_t)d));
  if (!b.d_log_arity) HIP_OK(dalloc(&b.d_log_arity, (size_t)d));
  HIP_OK(hipMemcpy(b.d_fields, f.data(), (size_t)d * sizeof(BdeuField), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.d_log_arity, lr.data(), (size_t)d * 8, hipMemcpyHostToDevice));
  return 0;
}

// checks every code (integral, 0 <= x < r_i), packs the rows and the per-node used-row bits, uploads them
static int bdeu_prepare(dibs_engine* e, BdeuData* out, const char* what, const float* x, const int32_t* mask, int N) {
  const BdeuState& b = *e->bdeu;
  if (b.arities.empty()) return fail(std::string("BDeu: ") + what + ": dibs_engine_set_arities has not been called");
  BdeuPlan pl;
  if (N < 1 || !bdeu_plan(N, b.KW, &pl))
    return fail(std::string("BDeu: ") + what + ": " + std::to_string(N) + " observations, but the kernel supports 1 .. " + std::to_string(BDEU_MAX_N) +
                " (the grouping table of one wave must fit a block's LDS)");
  const int d = e->d, KW = b.KW, NW = (N + 63) / 64;
  std::vector<uint64_t> rows((size_t)KW * N, 0ull), used((size_t)d * NW, 0ull);
  std::vector<int32_t> nused((size_t)d, 0), codes((size_t)d);
  for (int n = 0; n < N; ++n) {
    for (int i = 0; i < d; ++i) {
      const float v = x[(size_t)n * d + i];
      if (!(v >= 0.0f && v < (float)b.arities[i] && v == floorf(v))) {
        char buf[64];
        snprintf(buf, sizeof buf, "%g", (double)v);
        return fail(std::string("BDeu: ") + what + ": x[" + std::to_string(n) + ", " + std::to_string(i) + "] = " + buf +
                    " is not a category code of variable " + std::to_string(i) + " (integers 0 .. " + std::to_string(b.arities[i] - 1) + ")");
      }
      codes[i] = (int32_t)v;
      if (!(mask && mask[(size_t)n * d + i] != 0)) {
        used[(size_t)i * NW + (n >> 6)] |= 1ull << (n & 63);
        ++nused[i];
      }
    }
    bdeu_pack_row(codes.data(), d, b.fields.data(), rows.data(), (size_t)N, (size_t)n);
  }
  out->release();
  HIP_OK(dalloc(&out->rows, rows.size()));
  HIP_OK(dalloc(&out->used, used.size()));
  HIP_OK(dalloc(&out->nused, nused.size()));
  HIP_OK(hipMemcpy(out->rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(out->used, used.data(), used.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(out->nused, nused.data(), nused.size() * 4, hipMemcpyHostToDevice));
  out->N = N;
  out->NW = NW;
  return 0;
}

int bdeu_launch(dibs_engine* e, hipStream_t st, const BdeuData& data, const uint64_t* masks, double* node_scores, long long nprob, int S) {
  const BdeuState& b = *e->bdeu;
  BdeuArgs a{};
  a.rows = data.rows;
  a.used = data.used;
  a.nused = data.nused;
  a.fields = b.d_fields;
  a.log_arity = b.d_log_arity;
  a.masks = masks;
  a.node_scores = node_scores;
  a.log_ess = b.log_ess;
  a.nprob = nprob;
  a.N = data.N;
  a.KW = b.KW;
  a.NW = data.NW;
  a.d = e->d;
  a.S = S;
  a.W = e->W;
  if (!data.rows || bdeu_launch_nodes(st, a)) return fail("BDeu: no data, or no LDS plan for its size");
  return 0;
}

extern "C" int dibs_engine_set_data(dibs_engine* e, const float* x, const int32_t* interv_mask, const float* bge_mean_obs) {
  if (!e || !x) return fail("null argument");
  if (e->bdeu && e->bdeu->arities.empty()) return fail("BDeu: dibs_engine_set_data: dibs_engine_set_arities has not been called");
  if (e->B > 1 && !e->chains) return fail("batched engine: use dibs_engine_set_data_problem");
  if (e->chains && !e->cdata.set.empty())
    return fail("chains engine (n_chains > 1): dibs_engine_set_data after dibs_engine_set_data_problem is not supported (the chains of this engine "
                "have data sets of their own; one shared data set needs a new engine)");
  if (e->chains && chains_hp_differ(e))
    return fail("chains engine (n_chains > 1): dibs_engine_set_data: some chain's hyper-parameters differ from the configuration's "
                "(dibs_engine_set_chain_hparams), which needs per-chain data: dibs_engine_set_data_problem for every chain");
  if (e->f64) {  // float64 engine: the data widened exactly
    const size_t n = (size_t)e->N * e->d;
    std::vector<double> x64(x, x + n), mo64;
    if (bge_mean_obs) mo64.assign(bge_mean_obs, bge_mean_obs + e->d);
    return dibs_engine_set_data_f64(e, x64.data(), interv_mask, bge_mean_obs ? mo64.data() : nullptr);
  }
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  e->score_cache.valid = false;  // (the BGe prior mean travels with the data)
  e->has_data = false;  // (a failure below leaves the engine without data: the next step reports it instead of reading freed statistics)
  const size_t n = (size_t)e->N * e->d;
  if (e->x) hipFree(e->x);
  if (e->mask) hipFree(e->mask);
  e->x = nullptr;
  e->mask = nullptr;
  HIP_OK(dalloc(&e->x, n));
  HIP_OK(dalloc(&e->mask, n));
  HIP_OK(hipMemcpy(e->x, x, n * 4, hipMemcpyHostToDevice));
  if (interv_mask) HIP_OK(hipMemcpy(e->mask, interv_mask, n * 4, hipMemcpyHostToDevice));
  if (e->cfg.likelihood == DIBS_LIK_BGE) {
    e->has_mean_obs = bge_mean_obs != nullptr;
    if (bge_mean_obs) e->mean_obs.assign(bge_mean_obs, bge_mean_obs + e->d);
    if (bge_prepare(&e->bge, e->cfg, e->d, e->N, x, interv_mask, bge_mean_obs)) return 1;
  } else if (e->cfg.likelihood == DIBS_LIK_BDEU) {
    if (bdeu_prepare(e, &e->bdeu->train, "dibs_engine_set_data", x, interv_mask, e->N)) return 1;
  } else {
    if (joint_set_data(&e->jw, x, interv_mask, e->N, e->d)) return fail("joint_set_data failed");
    if (e->cfg.likelihood == DIBS_LIK_LINGAUSS && !joint_lin_fast_path(e->d, e->N, e->tune.lin_gram) && joint_lin_set_gram(&e->jw, x, interv_mask, e->N, e->d))
      return fail("LinearGaussian: Gram matrices: hipMalloc failed");
  }
  e->has_data = true;
  if (e->chains) e->cdata.shared = true;  // (from the first call that succeeded: the chains share this data set)
  return 0;
}

// ---- chains engine: data per chain (include/dibs_hip.h, CHAINS ENGINE; JointDiBS + LinearGaussian) ------------------------
// Chain c's observations and mask go to slice c of the workspace's [C][N][d] arrays (tu_lin.hip, joint_chain_data_*); on the Gram path the
// chain's matrices are built by the host code of a standalone engine and kept until every chain has arrived, then stacked and uploaded.
// The engine has its data when every chain has.  Allowed until the particles are initialised (as dibs_engine_set_problem_hparams).
static int chains_set_data_problem(dibs_engine* e, int32_t c, const float* x, int32_t n_obs, const int32_t* interv_mask,
                                   const float* bge_mean_obs) {
  const std::string pre = "chains engine (n_chains > 1): dibs_engine_set_data_problem: ";
  if (e->cdata.shared)
    return fail("chains engine (n_chains > 1): dibs_engine_set_data_problem after dibs_engine_set_data is not supported (the chains share the data set "
                "given by dibs_engine_set_data; per-chain data needs a new engine)");
  if (e->cfg.likelihood != DIBS_LIK_LINGAUSS)
    return fail(pre + "per-chain data is LinearGaussian only (DenseNonlinearGaussian chains share one data set: dibs_engine_set_data)");
  if (!x) return fail(pre + "null argument");
  if (c < 0 || c >= e->B) return fail(pre + "chain index " + std::to_string(c) + " out of range (n_chains = " + std::to_string(e->B) + ")");
  if (n_obs != e->N)
    return fail(pre + "n_obs = " + std::to_string(n_obs) + " but dibs_config.n_observations = " + std::to_string(e->N) +
                " (the number of observations selects LDS sizes and kernels: every chain has the configuration's)");
  if (bge_mean_obs) return fail(pre + "bge_mean_obs must be NULL (joint models have no BGe prior mean)");
  if (e->hp_final)
    return fail(pre + "called after the particles were initialised (init_particles_batch / set_state / run): give every chain its data first");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
  const int C = e->B, d = e->d, N = e->N;
  const bool gram = !joint_lin_fast_path(d, N, e->tune.lin_gram);  // (d and N only: every chain's choice, and its standalone engine's)
  e->has_data = false;
  if (e->cdata.set.empty()) {
    if (joint_chain_data_alloc(&e->jw, C, e->M, N, d)) return fail(pre + "hipMalloc of the per-chain data [n_chains][n_observations][n_vars] failed");
    e->cdata.set.assign((size_t)C, 0);
    if (gram) e->cdata.gram.assign((size_t)C, LinGramHost{});
  }
  e->cdata.set[(size_t)c] = 0;
  if (joint_chain_data_set(&e->jw, c, x, interv_mask, N, d)) return fail(pre + "copying the chain's data to the device failed");
  if (gram) joint_lin_gram_host(&e->cdata.gram[(size_t)c], x, interv_mask, N, d);
  e->cdata.set[(size_t)c] = 1;
  bool all = true;
  for (char f : e->cdata.set) all = all && f;
  if (all && gram && joint_chain_gram_commit(&e->jw, d, e->cdata.gram)) {
    e->cdata.set[(size_t)c] = 0;  // (this chain's call can be repeated)
    return fail(pre + "LinearGaussian: Gram matrices of all chains: hipMalloc failed");
  }
  e->has_data = all;
  return 0;
}

// ---- batched engine: data per problem (include/dibs_hip.h, n_problems) ----------------------------------------------------
extern "C" int dibs_engine_set_data_problem(dibs_engine* e, int32_t p, const float* x, int32_t n_obs, const int32_t* interv_mask,
                                            const float* bge_mean_obs) {
  if (e && e->chains) return chains_set_data_problem(e, p, x, n_obs, interv_mask, bge_mean_obs);
  if (need_batch(e)) return 1;
  if (!x) return fail("null argument");
  if (p < 0 || p >= e->B) return fail("problem index out of range");
  if (n_obs < 1) return fail("n_obs must be >= 1");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->stream2) HIP_OK(hipStreamSynchronize(e->stream2));
  const int d = e->d, dp = d + 1;
  const size_t msz = (size_t)dp * dp;
  BgeHost h;
  BgeHostF32 f;
  if (bge_host_stats(&h, e->cfg, d, n_obs, x, interv_mask, bge_mean_obs) || bge_f32_forms(&f, h, d)) return 1;
  dibs_engine::BatchStats& b = e->bst;
  if (b.set.empty()) {
    b.Rp.assign((size_t)e->B * d * msz, 0.f);
    b.Qp.assign((size_t)e->B * d * msz, 0.f);
    b.gam.assign((size_t)e->B * d * dp, 0.0);
    b.Nj.assign((size_t)e->B * d, 0.0);
    b.ldR.assign((size_t)e->B * d, 0.0);
    b.set.assign((size_t)e->B, 0);
  }
  b.alpha_lambd = h.alpha_lambd;
  // problem p's rows p d .. p d + d - 1: without interventions the one matrix (and logdet) repeated for every node -- the values the
  // standalone engine reads for every node from its single copy
  for (int j = 0; j < d; ++j) {
    const int jm = h.n_mats > 1 ? j : 0;
    const size_t row = (size_t)p * d + j;
    memcpy(&b.Rp[row * msz], &f.Rp[(size_t)jm * msz], msz * 4);
    memcpy(&b.Qp[row * msz], &f.Qp[(size_t)jm * msz], msz * 4);
    b.ldR[row] = f.ldR[jm];
    b.Nj[row] = h.Nj[j];
    memcpy(&b.gam[row * dp], &h.gam[(size_t)j * dp], (size_t)dp * 8);
  }
  b.set[p] = 1;
  e->has_data = false;
  e->score_cache.valid = false;
  BgeStats& st = e->bge;
  if (!st.Rp) {  // the stacked arrays, allocated once ([B d] rows; Rp and Qp in one allocation, see bge_prepare)
    HIP_OK(dalloc(&st.Rp, 2 * b.Rp.size()));
    st.Qp = st.Rp + b.Rp.size();
    HIP_OK(dalloc(&st.gam, b.gam.size()));
    HIP_OK(dalloc(&st.Nj, b.Nj.size()));
    HIP_OK(dalloc(&st.ldR, b.ldR.size()));
    hipDeviceSynchronize();  // (dalloc's zero fills ran on the null stream)
  }
  st.alpha_lambd = h.alpha_lambd;
  st.alpha_mu = h.alpha_mu;
  st.log_t = h.log_t;
  st.n_mats = e->B * d;
  const size_t r0 = (size_t)p * d;
  HIP_OK(hipMemcpy(st.Rp + r0 * msz, &b.Rp[r0 * msz], (size_t)d * msz * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st.Qp + r0 * msz, &b.Qp[r0 * msz], (size_t)d * msz * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st.gam + r0 * dp, &b.gam[r0 * dp], (size_t)d * dp * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st.Nj + r0, &b.Nj[r0], (size_t)d * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(st.ldR + r0, &b.ldR[r0], (size_t)d * 8, hipMemcpyHostToDevice));
  bool all = true;
  for (char f : b.set) all = all && f;
  e->has_data = all;
  return 0;
}

extern "C" int dibs_score_graphs(dibs_engine* e, const int32_t* g, const float* theta, int32_t n, const float* x_ho,
                                 const int32_t* mask_ho, int32_t n_ho, float* out) {
  if (!e || !g || !x_ho || !out) return fail("null argument");
  if (e->f64) return fail("float64 engine: dibs_score_graphs is not supported (dibs_engine_run only)");
  if (refuse_chains(e, "dibs_score_graphs (score with a standalone engine)")) return 1;
  if (e->B > 1) return fail("batched engine: dibs_score_graphs is not supported (score with a standalone engine)");
  if (n <= 0) return 0;
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  const dibs_config& c = e->cfg;
  const int d = e->d;
  const size_t dd = (size_t)d * d;
  DevBuf<float> d_out;
  HIP_OK(d_out.alloc((size_t)n));
  dibs_engine::ScoreCache& sc = e->score_cache;
  const size_t n_x = (size_t)n_ho * d;
  const bool cached = sc.matches(x_ho, mask_ho, n_x);
  if (!cached) sc.valid = false;
  if (c.likelihood == DIBS_LIK_BGE) {
    BgeStats& st = sc.st;  // statistics of (x_ho, mask_ho)
    if (!cached) {
      if (bge_prepare(&st, c, d, n_ho, x_ho, mask_ho, e->has_mean_obs ? e->mean_obs.data() : nullptr)) return 1;
      sc.remember(x_ho, mask_ho, n_x);
    }
    const int W = e->W, CH = 512;
    DevBuf<uint64_t> d_masks;
    DevBuf<double> d_ns;
    DevBuf<uint4> q_list;
    DevBuf<unsigned int> q_counts;
    HIP_OK(d_masks.alloc((size_t)d * CH * W));
    HIP_OK(d_ns.alloc((size_t)d * CH));
    HIP_OK(q_list.alloc((size_t)BGE_NQ * d * CH * bge_entry_u4(W)));
    HIP_OK(q_counts.alloc((size_t)BGE_NQ));
    const BgeQueues sq{q_list.p, q_counts.p, (uint32_t)(d * CH)};  // scratch queues for this call
    const BgeParams bp = st.params();
    std::vector<uint64_t> hm((size_t)d * CH * W);
    for (int q0 = 0; q0 < n; q0 += CH) {
      const int S = n - q0 < CH ? n - q0 : CH;
      std::fill(hm.begin(), hm.end(), 0ull);
      for (int s = 0; s < S; ++s)
        for (int i = 0; i < d; ++i)
          for (int j = 0; j < d; ++j)
            if (i != j && g[(size_t)(q0 + s) * dd + (size_t)i * d + j] != 0) hm[((size_t)j * S + s) * W + (i >> 6)] |= 1ull << (i & 63);
      HIP_OK(hipMemcpy(d_masks.p, hm.data(), (size_t)d * S * W * 8, hipMemcpyHostToDevice));
      HIP_OK(hipMemsetAsync(sq.counts, 0, BGE_NQ * sizeof(unsigned int), e->stream));
      bge_launch_sample(false, e->stream, nullptr, d_masks.p, d_ns.p, bp, Key2{0, 0}, 0, 1, 1, d, S, W, 0, sq,
                        KmatFuse{nullptr, nullptr, 0, 0, 0, 0.f, 0.f, nullptr, 0u});
      bge_launch_chol(e->stream, d_ns.p, bp, sq, d, S, nullptr);
      bge_launch_sum_nodes(e->stream, d_ns.p, d_out.p + q0, d, S);
      HIP_OK(hipStreamSynchronize(e->stream));
    }
  } else if (c.likelihood == DIBS_LIK_BDEU) {
    if (e->bdeu->arities.empty()) return fail("BDeu: dibs_score_graphs: dibs_engine_set_arities has not been called");
    if (!cached) {
      if (bdeu_prepare(e, &e->bdeu->ho, "dibs_score_graphs", x_ho, mask_ho, n_ho)) return 1;
      sc.remember(x_ho, mask_ho, n_x);
    }
    // chunks of n_grad_mc_samples graphs through the engine's own parent-set and node-score buffers ([1 .. Mloc][d][S][W] / [..][d][S]: a
    // chunk of S' <= S graphs fills the first d S' entries as [d][S']): the last chunk's doubles stay readable (include/dibs_hip.h, BDEU)
    const int W = e->W, CH = e->S;
    std::vector<uint64_t> hm((size_t)d * CH * W);
    for (int q0 = 0; q0 < n; q0 += CH) {
      const int S = n - q0 < CH ? n - q0 : CH;
      std::fill(hm.begin(), hm.end(), 0ull);
      for (int s = 0; s < S; ++s)
        for (int i = 0; i < d; ++i)
          for (int j = 0; j < d; ++j)
            if (i != j && g[(size_t)(q0 + s) * dd + (size_t)i * d + j] != 0) hm[((size_t)j * S + s) * W + (i >> 6)] |= 1ull << (i & 63);
      HIP_OK(hipMemcpy(e->masks, hm.data(), (size_t)d * S * W * 8, hipMemcpyHostToDevice));
      if (bdeu_launch(e, e->stream, e->bdeu->ho, e->masks, e->node_scores, (long long)d * S, S)) return 1;
      bge_launch_sum_nodes(e->stream, e->node_scores, d_out.p + q0, d, S);
      HIP_OK(hipStreamSynchronize(e->stream));
    }
  } else if (c.likelihood == DIBS_LIK_LINGAUSS || c.likelihood == DIBS_LIK_DENSENN) {
    if (!theta) return fail("theta required");
    const bool nn = c.likelihood == DIBS_LIK_DENSENN;
    struct { JointWork& jw; } jg{sc.jw};
    if (!cached) {
      if (joint_set_data(&jg.jw, x_ho, mask_ho, n_ho, d)) return fail("joint_set_data failed");
      if (!nn && !joint_lin_fast_path(d, n_ho, e->tune.lin_gram) && joint_lin_set_gram(&jg.jw, x_ho, mask_ho, n_ho, d)) return fail("LinearGaussian: Gram matrices: hipMalloc failed");
      sc.remember(x_ho, mask_ho, n_x);
    }
    const size_t P = nn ? (size_t)e->P : dd;
    DevBuf<float> d_th;
    DevBuf<int32_t> d_g;
    HIP_OK(d_th.alloc((size_t)n * P));
    HIP_OK(d_g.alloc((size_t)n * dd));
    HIP_OK(hipMemcpy(d_th.p, theta, (size_t)n * P * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_g.p, g, (size_t)n * dd * 4, hipMemcpyHostToDevice));
    if (nn) {
      const NNParams np_ = nn_params(c);
      if (joint_nn_score_given(jg.jw, d_th.p, d_g.p, d_out.p, n, d, n_ho, np_, P, e->stream)) return fail("DenseNonlinearGaussian: scratch area: hipMalloc failed");
    } else if (joint_lin_score_given(jg.jw, d_th.p, d_g.p, d_out.p, n, d, n_ho, (float)c.lin_obs_noise, (float)c.lin_mean_edge,
                                     (float)c.lin_sig_edge, e->stream)) {
      return fail("LinearGaussian: scratch area: hipMalloc failed");
    }
    HIP_OK(hipStreamSynchronize(e->stream));
  } else {
    return fail("dibs_score_graphs: likelihood not supported yet");
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(out, d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- float64 engine: data (include/dibs_hip.h) ----------------------------------------------------------------------
// BGe statistics of the data in double, the oracle's bge_prepare (linearGaussian.py:78-94) to the letter; never rounded to float
extern "C" int dibs_engine_set_data_f64(dibs_engine* e, const double* x, const int32_t* interv_mask, const double* bge_mean_obs) {
  if (!e || !x) return fail("null argument");
  if (!e->f64) return fail("dibs_engine_set_data_f64: not a float64 engine (dibs_config.reserved_i[1] = 64)");
  HIP_OK(hipSetDevice(e->cfg.device_id));
  HIP_OK(hipStreamSynchronize(e->stream));
  e->has_data = false;
  F64State& f = *e->f64;
  BgeHost h;
  if (bge_host_stats(&h, e->cfg, e->d, e->N, x, interv_mask, bge_mean_obs)) return 1;
  const std::vector<double> &R = h.R, &Nj = h.Nj, &gam = h.gam;
  void* old[] = {f.R, f.Nj, f.gam};
  for (void* p_ : old)
    if (p_) hipFree(p_);
  f.R = f.Nj = f.gam = nullptr;
  HIP_OK(dalloc(&f.R, R.size()));
  HIP_OK(dalloc(&f.Nj, Nj.size()));
  HIP_OK(dalloc(&f.gam, gam.size()));
  HIP_OK(hipMemcpy(f.R, R.data(), R.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(f.Nj, Nj.data(), Nj.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(f.gam, gam.data(), gam.size() * 8, hipMemcpyHostToDevice));
  f.alpha_lambd = h.alpha_lambd;
  f.n_mats = h.n_mats;
  e->has_data = true;
  return 0;
}
