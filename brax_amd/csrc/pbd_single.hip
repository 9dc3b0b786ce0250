// pbd_single.hip — the SINGLE-mode translation unit: the register-hoisted step
// kernels over the bodies of pbd_kernels.hip (built with the max-ILP
// scheduler), their packed / wide / rollout variants, and the unit's kernel
// family for the env launcher (launch_env_family, pbd_launch.h: the decision
// which system gets which kernel is pbd_dispatch.h's, shared by every env
// launch unit). The item-loop / MULTI / reset kernels: pbd_generic.hip.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_dispatch.h"
#include "pbd_kernels.hip"
#include "pbd_launch.h"
#include "pbd_stamps.h"

namespace bx {

// one step on the packed layout (bx_env_step_packed: Env.step's host path)
// through the PK body, under its own name (the benchmarked envs' kernels)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR env_step_packed_kernel(EnvArgs A) {
  env_step_body<L, MODE, F, M, EK, true, true>(A);
}
// the Ant step kernel held to 256 registers (2 waves per SIMD) for batches
// past one wave per SIMD: at 4,096 envs the unbounded kernel's single wave
// per SIMD is 7 % faster (29.8 vs 32.0 us), but at 32,768 envs (8 waves per
// SIMD) it runs 8 residency rounds against this one's 4 (152 vs 219 M
// env-steps/s, tools/ab_ant_waves.sh)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_step_wide_kernel(EnvArgs A) {
  env_step_body<L, MODE, F, M, EK>(A);
}
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_rollout_wide_kernel(EnvArgs A) {
  env_step_body<L, MODE, F, M, EK, true>(A);
}
// the same body under its own name for multi-step launches of the
// benchmarked envs' kernels (bx_env_rollout_packed), so a profile tells
// K-step launches from single steps; the Ant kind's with the per-step tail on
// running addresses (env_step_body's RT)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR env_rollout_kernel(EnvArgs A) {
  constexpr bool RT = EK == EK_ANT && L == 16 && MODE == MODE_SINGLE;
  env_step_body<L, MODE, F, M, EK, true, false, false, false, false, true, RT>(A);
}

// the system step: the variant's kernel (generated from the variant list,
// pbd_dispatch.h; single_variant yields listed variants only, so the default
// arm is not reached)
#define BX_SYSTEM_STEP_CASE(VL, VF, VM, UNUSED) \
  case single_key(VL, VF, VM): launch_one(system_step_kernel<VL, 1, VF, VM>, grid, tpb, lds, s, a); break;
hipError_t launch_system_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                     hipStream_t s, const StepArgs& a) {
  const dim3 grid = single_grid(L, tpb, n_envs);
  const SingleVariant v = single_variant(L, feat, gw);
  switch (single_key(v.L, v.F, v.M)) {
    BX_SINGLE_VARIANTS(BX_SYSTEM_STEP_CASE, 0)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the unit's family: step_kernel's choice (pbd_dispatch.h) among the five
// kernel templates above; the wide kernels exist for Ant only, the rollout
// kernel for the kind kernels that have one
struct StepFamily {
  static constexpr EnvFamily id = FAM_STEP;
  template <int L, int F, int M, int EK>
  static auto kernel(const EnvArgs& a, bool wide) -> void (*)(EnvArgs) {
    const StepKernel k = step_kernel(KindVariant{F, M, EK}, wide, a.n_steps, a.packed != 0);
    if constexpr (EK == EK_ANT) {
      if (k == K_ROLLOUT_WIDE) return env_rollout_wide_kernel<L, 1, F, M, EK>;
      if (k == K_STEP_WIDE) return env_step_wide_kernel<L, 1, F, M, EK>;
    }
    if constexpr (has_rollout_kernel(F, EK))
      if (k == K_ROLLOUT) return env_rollout_kernel<L, 1, F, M, EK>;
    if (k == K_STEP_PACKED) return env_step_packed_kernel<L, 1, F, M, EK>;
    return env_step_kernel<L, 1, F, M, EK>;
  }
};
hipError_t launch_env_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                  hipStream_t s, const EnvArgs& a, int fold) {
  return launch_env_family<StepFamily>(L, feat, gw, tpb, n_envs, lds, s, fold, a);
}
// the joint halves' partner exchange alone (bx_debug_partner)
__global__ void __launch_bounds__(64) partner_kernel(float* out, int lanes) {
  const float v = (float)threadIdx.x;
  out[threadIdx.x] = lanes == 16 ? xh(v) : v;
}
hipError_t debug_partner(float* out64, int lanes, hipStream_t s) {
  hipLaunchKernelGGL(partner_kernel, dim3(1), dim3(64), 0, s, out64, lanes);
  return hipGetLastError();
}
hipError_t debug_stamps(unsigned long long* out, int reset) {
#ifdef BX_STAMPS
  // (reset bit 2: the per-workgroup sums themselves, 4096 x 16)
  return stamps_readback(HIP_SYMBOL(bx_stamp_wave), out, reset, (reset & 4) != 0);
#else
  (void)out;
  (void)reset;
  return hipErrorNotSupported;
#endif
}

}  // namespace bx
