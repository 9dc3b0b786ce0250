// pbd_pop.hip — one episode per perturbed policy: the evaluation kernels of
// pbd_eval.hip with each env reading its own parameter row, the identity
// head, the reward shift and the observation moments kept on chip
// (env_step_body's POP, pbd_kernels.hip), and their launcher. Built with
// pbd_eval.hip's flags; the kernels of the other units are not touched.
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
// the Ant kernel held to 256 registers, as env_eval_policy_wide_kernel
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_eval_pop_wide_kernel(EnvArgs A, PolArgs Q, EvalArgs V, PopArgs N) {
  env_step_body<L, MODE, F, M, EK, true, false, true, true, true>(A, Q, V, N);
}

static void launch_pop(void (*k)(EnvArgs, PolArgs, EvalArgs, PopArgs), dim3 grid, int tpb, size_t lds,
                       hipStream_t s, const EnvArgs& a, const PolArgs& q, const EvalArgs& v,
                       const PopArgs& n) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(tpb), lds, s, a, q, v, n);
}

static int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cached[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

#define BX_EVAL_POP_CASE(VL, VF, VM, UNUSED) \
  case single_key(VL, VF, VM): launch_pop(env_eval_pop_kernel<VL, 1, VF, VM>, grid, tpb, lds, s, a, q, v, n); break;

// launch_env_policy_single's selection (pbd_policy.hip), kernel for kernel
hipError_t launch_env_eval_population(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                      hipStream_t s, const EnvArgs& a, const PolArgs& q,
                                      const EvalArgs& v, const PopArgs& n, int fold) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  const int k = a.P.kind;
  const bool jb = (fold & 2) != 0;
  const bool ant_ok = jb && ((fold & 4) != 0 || !cb_feat(F_G1 | F_JH));
  if (fold && ant_ok && L == 16 && gw <= 4 && k == BX_ENV_ANT && feat == (F_G1 | F_JH)) {
    const bool wide = (int64_t)grid.x * (tpb / 64 > 0 ? tpb / 64 : 1) > 4 * (int64_t)cu_count();
    if (wide)
      launch_pop(env_eval_pop_wide_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, q, v, n);
    else
      launch_pop(env_eval_pop_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, q, v, n);
    return hipGetLastError();
  }
  constexpr int F_CHEETAH = F_CC | F_TW | F_JH | F_R2 | F_R2G;
  if (fold && jb && L == 16 && gw <= 4 && k == BX_ENV_HALFCHEETAH && (feat & ~F_G1) == F_CHEETAH) {
    launch_pop(env_eval_pop_kernel<16, 1, F_CHEETAH, 4, EK_CHEETAH>, grid, tpb, lds, s, a, q, v, n);
    return hipGetLastError();
  }
  constexpr int F_PUSHER = F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G;
  if (fold && L == 16 && k == BX_ENV_PUSHER && (feat & ~F_G1) == F_PUSHER) {
    if (gw <= 4) launch_pop(env_eval_pop_kernel<16, 1, F_PUSHER, 4, EK_PUSHER>, grid, tpb, lds, s, a, q, v, n);
    else launch_pop(env_eval_pop_kernel<16, 1, F_PUSHER, 8, EK_PUSHER>, grid, tpb, lds, s, a, q, v, n);
    return hipGetLastError();
  }
  const SingleVariant sv = single_variant(L, feat, gw);
  switch (single_key(sv.L, sv.F, sv.M)) {
    BX_SINGLE_VARIANTS(BX_EVAL_POP_CASE, 0)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bx
