// pbd_eval.hip — whole evaluation episodes, the policy form: the closed-loop
// rollout kernels of pbd_policy.hip with EvalWrapper's sums kept on chip
// (env_step_body's EVL, pbd_kernels.hip) and only the last step's block
// stored, and their family for the env launcher (launch_env_family,
// pbd_launch.h, over pbd_dispatch.h's decision). Built with pbd_policy.hip's
// flags; the kernels of the other units are not touched. The open-loop form:
// pbd_eval_open.hip.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_dispatch.h"
#include "pbd_kernels.hip"
#include "pbd_launch.h"

namespace bx {

template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR
env_eval_policy_kernel(EnvArgs A, PolArgs Q, EvalArgs V) {
  env_step_body<L, MODE, F, M, EK, true, false, true, true>(A, Q, V);
}
// the Ant kernel held to 256 registers, as env_policy_rollout_wide_kernel (ZH
// off: with the frozen side in registers it spilled 6 VGPRs, 28 B of scratch)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_eval_policy_wide_kernel(EnvArgs A, PolArgs Q, EvalArgs V) {
  env_step_body<L, MODE, F, M, EK, true, false, true, true, false, false>(A, Q, V);
}

BX_ENV_FAMILY(EvalPolicyFamily, FAM_EVAL_POLICY, env_eval_policy_kernel, env_eval_policy_wide_kernel)
hipError_t launch_env_eval_policy(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                  hipStream_t s, const EnvArgs& a, const PolArgs& q,
                                  const EvalArgs& v, int fold) {
  return launch_env_family<EvalPolicyFamily>(L, feat, gw, tpb, n_envs, lds, s, fold, a, q, v);
}

}  // namespace bx
