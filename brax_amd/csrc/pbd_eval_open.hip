// pbd_eval_open.hip — whole evaluation episodes, the open-loop form: the
// K-step rollout kernels of pbd_single.hip (actions read at act + t *
// act_step) with EvalWrapper's sums kept on chip (env_step_body's EVL,
// pbd_kernels.hip) and only the last step's block stored, and their family for
// the env launcher (launch_env_family, pbd_launch.h, over pbd_dispatch.h's
// decision; this family has the Humanoid kernels). Built with pbd_single.hip's
// flags; the kernels of the other units are not touched. The policy form:
// pbd_eval.hip.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_dispatch.h"
#include "pbd_kernels.hip"
#include "pbd_launch.h"

namespace bx {

template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR
env_eval_kernel(EnvArgs A, EvalArgs V) {
  env_step_body<L, MODE, F, M, EK, true, false, false, true>(A, PolArgs{}, V);
}
// the Ant kernel held to 256 registers, as env_rollout_wide_kernel
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_eval_wide_kernel(EnvArgs A, EvalArgs V) {
  env_step_body<L, MODE, F, M, EK, true, false, false, true>(A, PolArgs{}, V);
}

BX_ENV_FAMILY(EvalOpenFamily, FAM_EVAL_OPEN, env_eval_kernel, env_eval_wide_kernel)
hipError_t launch_env_eval_open(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                hipStream_t s, const EnvArgs& a, const EvalArgs& v, int fold) {
  return launch_env_family<EvalOpenFamily>(L, feat, gw, tpb, n_envs, lds, s, fold, a, v);
}

}  // namespace bx
