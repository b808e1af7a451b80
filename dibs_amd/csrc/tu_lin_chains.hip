// translation unit: the per-chain forms of the JointDiBS + LinearGaussian kernels (kernels_lin.h, kernels_lin_gram.h) for a chains engine
// whose chains have their own data sets (include/dibs_hip.h, CHAINS ENGINE; LinChainData in joint_launch.h).  DIBS_TU_LIN_CHAINS makes the
// two headers define every kernel under the name k_..._chains with a LinChainData in place of the data pointers and the intervention flag:
// a block serves one particle row m, so its chain c = m / M is block-uniform -- scalar loads and a scalar offset.  A unit of their own, so
// that tu_lin.hip compiles the kernels of standalone engines and shared-data chains engines from the source text it always compiled.  The
// launchers are called by tu_lin.hip's with the grid, the LDS size and the per-block counts chosen there.
#define DIBS_TU_LIN_CHAINS
#include "launch.h"
#include "kernels_lin.h"
#include "kernels_lin_gram.h"

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
#define LIN_LOGPROB_ARGS                                                                                                                   \
  cd, jl.theta, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M, jl.d, jl.N, jl.S, per, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, \
      jl.mean_edge, jl.sig_edge
#define NT_SWITCH(CALL_)      \
  switch (nt) {               \
    case 1: CALL_(1); break;  \
    case 2: CALL_(2); break;  \
    case 3: CALL_(3); break;  \
    case 4: CALL_(4); break;  \
    case 5: CALL_(5); break;  \
    case 6: CALL_(6); break;  \
    default: CALL_(7); break; \
  }

void lin_chains_launch_logprobs(int nt, dim3 grid, size_t lds, const LinChainData& cd, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                                int per) {
#define CALL(NT_)                                    \
  {                                                  \
    allow_lds(k_lin_logprobs_chains<NT_>, lds);      \
    hipLaunchKernelGGL(k_lin_logprobs_chains<NT_>, grid, dim3(256), lds, jl.stream, LIN_LOGPROB_ARGS); \
  }
  NT_SWITCH(CALL)
#undef CALL
}

// (epq: 4, 10, 16 for nt <= 4, 0 beyond -- the instantiations of joint_lin_logprobs, tu_lin.hip)
template <int NT>
static void launch_pair_nt(int epq, dim3 grid, size_t lds, const LinChainData& cd, const JointLaunch& jl, float* lp, Key2 carry, int mode, int per) {
#define PAIR(EPQ_)                                                                                               \
  {                                                                                                              \
    allow_lds(k_lin_logprobs_pair_chains<NT, EPQ_>, lds);                                                        \
    hipLaunchKernelGGL((k_lin_logprobs_pair_chains<NT, EPQ_>), grid, dim3(256), lds, jl.stream, LIN_LOGPROB_ARGS); \
  }
  if constexpr (NT <= 4) {
    if (epq == 4) PAIR(4)
    else if (epq == 10) PAIR(10)
    else PAIR(16)
  } else {
    PAIR(0)
  }
#undef PAIR
}
void lin_chains_launch_pair(int nt, int epq, dim3 grid, size_t lds, const LinChainData& cd, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                            int per) {
#define CALL(NT_) launch_pair_nt<NT_>(epq, grid, lds, cd, jl, lp, carry, mode, per)
  NT_SWITCH(CALL)
#undef CALL
}

// ((epq, four): (5, false), (5, true), (8, true), eight waves -- the instantiations of joint_lin_logprobs)
void lin_chains_launch_hf(int epq, bool four, dim3 grid, size_t lds, const LinChainData& cd, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                          int per) {
#define HF(EPQ_, FOUR_)                                                                                                      \
  {                                                                                                                          \
    allow_lds(k_lin_logprobs_hf_chains<EPQ_, FOUR_, 8>, lds);                                                                \
    hipLaunchKernelGGL((k_lin_logprobs_hf_chains<EPQ_, FOUR_, 8>), grid, dim3(64 * 8), lds, jl.stream, LIN_LOGPROB_ARGS);    \
  }
  if (!four) HF(5, false)
  else if (epq == 5) HF(5, true)
  else HF(8, true)
#undef HF
}

void lin_chains_launch_grad(int nt, dim3 grid, size_t lds, const LinChainData& cd, const JointLaunch& jl, const LinGradJob& jt, const LinGradJob& jz,
                            const GradSplit& gs) {
#define CALL(NT_)                                                                                                                            \
  {                                                                                                                                          \
    allow_lds(k_lin_grad_chains<NT_>, lds);                                                                                                  \
    hipLaunchKernelGGL(k_lin_grad_chains<NT_>, grid, dim3(256), lds, jl.stream, cd, jl.theta, jl.scores, jl.thr, jt, jz, jl.baseline, jl.m0, \
                       jl.M, jl.d, jl.N, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge, jl.sf_baseline, \
                       gs);                                                                                                                  \
  }
  NT_SWITCH(CALL)
#undef CALL
}

void ling_chains_launch_logprobs(dim3 grid, size_t lds, const LinChainData& cd, int ng, const JointLaunch& jl, float* lp, Key2 carry, int mode,
                                 float* ops_glob) {
  allow_lds(k_ling_logprobs_chains, lds);
  hipLaunchKernelGGL(k_ling_logprobs_chains, grid, dim3(256), lds, jl.stream, cd, ng, jl.theta, jl.scores, jl.thr, lp, carry, mode, jl.m0, jl.M,
                     jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge, ops_glob);
}

void ling_chains_launch_grad(dim3 grid, size_t lds, const LinChainData& cd, int ng, const JointLaunch& jl, const LinGradJob& jt, const LinGradJob& jz,
                             float* ops_glob, const GradSplit& gs) {
  allow_lds(k_ling_grad_chains, lds);
  hipLaunchKernelGGL(k_ling_grad_chains, grid, dim3(256), lds, jl.stream, cd, ng, jl.theta, jl.scores, jl.thr, jt, jz, jl.baseline, jl.m0, jl.M,
                     jl.d, jl.S, jl.alpha, jl.tau, jl.layout, jl.tiny, jl.obs_noise, jl.mean_edge, jl.sig_edge, jl.sf_baseline, ops_glob, gs);
}
