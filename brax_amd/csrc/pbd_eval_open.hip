// pbd_eval_open.hip — whole evaluation episodes, the open-loop form: the
// K-step rollout kernels of pbd_single.hip (actions read at act + t *
// act_step) with EvalWrapper's sums kept on chip (env_step_body's EVL,
// pbd_kernels.hip) and only the last step's block stored, and their launcher.
// Built with pbd_single.hip's flags; the kernels of the other units are not
// touched. The policy form: pbd_eval.hip.
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

static void launch_evo(void (*k)(EnvArgs, EvalArgs), dim3 grid, int tpb, size_t lds, hipStream_t s,
                       const EnvArgs& a, const EvalArgs& v) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(tpb), lds, s, a, v);
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

#define BX_EVAL_OPEN_CASE(VL, VF, VM, UNUSED) \
  case single_key(VL, VF, VM): launch_evo(env_eval_kernel<VL, 1, VF, VM>, grid, tpb, lds, s, a, v); break;

// launch_env_step_single's selection (pbd_single.hip) for a K-step launch: the
// env kinds' own kernels where their conditions hold, else the variant list's
hipError_t launch_env_eval_open(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                hipStream_t s, const EnvArgs& a, const EvalArgs& v, int fold) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  const int k = a.P.kind;
  const bool jb = (fold & 2) != 0;
  const bool ant_ok = jb && ((fold & 4) != 0 || !cb_feat(F_G1 | F_JH));
  if (fold && ant_ok && L == 16 && gw <= 4 && k == BX_ENV_ANT && feat == (F_G1 | F_JH)) {
    const bool wide = (int64_t)grid.x * (tpb / 64 > 0 ? tpb / 64 : 1) > 4 * (int64_t)cu_count();
    if (wide)
      launch_evo(env_eval_wide_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, v);
    else
      launch_evo(env_eval_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, v);
    return hipGetLastError();
  }
  if (fold && L == 16 && gw <= 4 && (k == BX_ENV_HUMANOID || k == BX_ENV_HUMANOID_STANDUP) &&
      feat == (F_SPH | F_G1)) {
    launch_evo(env_eval_kernel<16, 1, F_SPH | F_G1, 4, EK_HUM>, grid, tpb, lds, s, a, v);
    return hipGetLastError();
  }
  constexpr int F_CHEETAH = F_CC | F_TW | F_JH | F_R2 | F_R2G;
  if (fold && jb && L == 16 && gw <= 4 && k == BX_ENV_HALFCHEETAH && (feat & ~F_G1) == F_CHEETAH) {
    launch_evo(env_eval_kernel<16, 1, F_CHEETAH, 4, EK_CHEETAH>, grid, tpb, lds, s, a, v);
    return hipGetLastError();
  }
  constexpr int F_PUSHER = F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G;
  if (fold && L == 16 && k == BX_ENV_PUSHER && (feat & ~F_G1) == F_PUSHER) {
    if (gw <= 4) launch_evo(env_eval_kernel<16, 1, F_PUSHER, 4, EK_PUSHER>, grid, tpb, lds, s, a, v);
    else launch_evo(env_eval_kernel<16, 1, F_PUSHER, 8, EK_PUSHER>, grid, tpb, lds, s, a, v);
    return hipGetLastError();
  }
  // HumanoidStandup: the Humanoid system lying down, 22 ground rows (F_R2)
  if (fold && L == 16 && (k == BX_ENV_HUMANOID || k == BX_ENV_HUMANOID_STANDUP) &&
      feat == (F_SPH | F_G1 | F_R2)) {
    launch_evo(env_eval_kernel<16, 1, F_SPH | F_G1 | F_R2, 8, EK_HUM>, grid, tpb, lds, s, a, v);
    return hipGetLastError();
  }
  const SingleVariant sv = single_variant(L, feat, gw);
  switch (single_key(sv.L, sv.F, sv.M)) {
    BX_SINGLE_VARIANTS(BX_EVAL_OPEN_CASE, 0)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bx
