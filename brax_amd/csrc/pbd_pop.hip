// pbd_pop.hip — one episode per perturbed policy: the evaluation kernels of
// pbd_eval.hip with each env reading its own parameter row, the identity
// head, the reward shift and the observation moments kept on chip
// (env_step_body's POP, pbd_kernels.hip), and their family for the env
// launcher (launch_env_family, pbd_launch.h, over pbd_dispatch.h's decision).
// Built with pbd_eval.hip's flags; the kernels of the other units are not
// touched.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_dispatch.h"
#include "pbd_kernels.hip"
#include "pbd_launch.h"

namespace bx {

template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR
env_eval_pop_kernel(EnvArgs A, PolArgs Q, EvalArgs V, PopArgs N) {
  env_step_body<L, MODE, F, M, EK, true, false, true, true, true>(A, Q, V, N);
}
// the Ant kernel held to 256 registers, as env_eval_policy_wide_kernel (ZH
// off: with the frozen side in registers its scratch grew from 52 to 88 B)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_eval_pop_wide_kernel(EnvArgs A, PolArgs Q, EvalArgs V, PopArgs N) {
  env_step_body<L, MODE, F, M, EK, true, false, true, true, true, false>(A, Q, V, N);
}

BX_ENV_FAMILY(PopulationFamily, FAM_POPULATION, env_eval_pop_kernel, env_eval_pop_wide_kernel)
hipError_t launch_env_eval_population(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                      hipStream_t s, const EnvArgs& a, const PolArgs& q,
                                      const EvalArgs& v, const PopArgs& n, int fold) {
  return launch_env_family<PopulationFamily>(L, feat, gw, tpb, n_envs, lds, s, fold, a, q, v, n);
}

}  // namespace bx
