// translation unit: the per-chain forms of the JointDiBS + LinearGaussian kernels (kernels_lin.h, kernels_lin_gram.h) for a chains engine
// whose chains have their own data sets (include/dibs_hip.h, CHAINS ENGINE; LinChainData in joint_launch.h).  DIBS_TU_LIN_CHAINS makes the
// two headers define every kernel under the name k_..._chains with a LinChainData in place of the data pointers and the intervention flag:
// a block serves one particle row m, so its chain c = m / M is block-uniform -- scalar loads and a scalar offset.  A unit of their own, so
// that tu_lin.hip compiles the kernels of standalone engines and shared-data chains engines from the source text it always compiled.
// lin_launch.h, the launch text of both units, defines this unit's entry points lin_all_logprobs_chains / lin_all_grads_chains; they are
// called by joint_lin_all_logprobs / joint_lin_all_grads (tu_lin.hip).
#define DIBS_TU_LIN_CHAINS
#include "launch.h"
#include "kernels_lin.h"
#include "kernels_lin_gram.h"
#include "lin_launch.h"
