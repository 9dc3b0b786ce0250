// pbd_single.hip — the SINGLE-mode translation unit: the register-hoisted step
// kernels over the bodies of pbd_kernels.hip (built with the max-ILP
// scheduler), their packed / wide / rollout variants and their launchers. The
// item-loop / MULTI / reset kernels: pbd_generic.hip.
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
// K-step launches from single steps
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR env_rollout_kernel(EnvArgs A) {
  env_step_body<L, MODE, F, M, EK, true>(A);
}

// compute units of the current device (the launch runs under the system's
// device scope), cached per device
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

// the variant's kernel of the family KERNEL (generated from the variant list,
// pbd_dispatch.h; single_variant yields listed variants only, so the default
// arm is not reached)
#define BX_SINGLE_CASE(VL, VF, VM, KERNEL, ARGS) \
  case single_key(VL, VF, VM): launch_one<ARGS>(KERNEL<VL, 1, VF, VM>, grid, tpb, lds, s, a); break;
#define BX_DISPATCH_SINGLE(KERNEL, ARGS)                      \
  {                                                           \
    const SingleVariant v = single_variant(L, feat, gw);      \
    switch (single_key(v.L, v.F, v.M)) {                      \
      BX_SINGLE_VARIANTS(BX_SINGLE_CASE, KERNEL, ARGS)        \
      default: return hipErrorInvalidValue;                   \
    }                                                         \
  }

hipError_t launch_system_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                     hipStream_t s, const StepArgs& a) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  BX_DISPATCH_SINGLE(system_step_kernel, StepArgs)
  return hipGetLastError();
}
int single_kernel_feat(int L, int feat, int gw) { return single_variant(L, feat, gw).F; }

// an env kind's own kernels: the K-step rollout, the packed step, the step
template <int F, int M, int EK>
static void launch_env_kind(dim3 grid, int tpb, size_t lds, hipStream_t s, const EnvArgs& a) {
  if (a.n_steps > 1)
    launch_one<EnvArgs>(env_rollout_kernel<16, 1, F, M, EK>, grid, tpb, lds, s, a);
  else if (a.packed)
    launch_one<EnvArgs>(env_step_packed_kernel<16, 1, F, M, EK>, grid, tpb, lds, s, a);
  else
    launch_one<EnvArgs>(env_step_kernel<16, 1, F, M, EK>, grid, tpb, lds, s, a);
}
hipError_t launch_env_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                  hipStream_t s, const EnvArgs& a, int fold) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  // the benchmarked envs get kernels holding only their own env program
  const int k = a.P.kind;
  // (their kernels fold each joint's damping into its actuator's slot: fold
  // bit 0 = every joint j has torque actuator j; the joint-halves kernels
  // also give each side lane its body's copy: bit 1 = the system allows it)
  const bool jb = (fold & 2) != 0;
  // (the Ant kernels resolve contacts on the body lanes, cb_feat: bit 2 = the
  // system's rows allow it; an Ant-kind system without it takes the variant
  // list's all-kinds kernel below)
  const bool ant_ok = jb && ((fold & 4) != 0 || !cb_feat(F_G1 | F_JH));
  if (fold && ant_ok && L == 16 && gw <= 4 && k == BX_ENV_ANT && feat == (F_G1 | F_JH)) {
    // past one wave per SIMD: the register-capped kernels
    const bool wide = (int64_t)grid.x * (tpb / 64 > 0 ? tpb / 64 : 1) > 4 * (int64_t)cu_count();
    // (a packed single step at a wide batch takes the wide rollout kernel)
    if ((a.n_steps > 1 || a.packed) && wide)
      launch_one<EnvArgs>(env_rollout_wide_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a);
    else if (wide)
      launch_one<EnvArgs>(env_step_wide_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a);
    else
      launch_env_kind<F_G1 | F_JH, 4, EK_ANT>(grid, tpb, lds, s, a);
    return hipGetLastError();
  }
  if (fold && L == 16 && gw <= 4 && (k == BX_ENV_HUMANOID || k == BX_ENV_HUMANOID_STANDUP) &&
      feat == (F_SPH | F_G1)) {
    launch_env_kind<F_SPH | F_G1, 4, EK_HUM>(grid, tpb, lds, s, a);
    return hipGetLastError();
  }
  // HalfCheetah: 16 one-way ground rows in slot 1, the feet's capsule-capsule
  // row in slot 2 (F_R2 | F_R2G), joint halves
  constexpr int F_CHEETAH = F_CC | F_TW | F_JH | F_R2 | F_R2G;
  if (fold && jb && L == 16 && gw <= 4 && k == BX_ENV_HALFCHEETAH && (feat & ~F_G1) == F_CHEETAH) {
    launch_env_kind<F_CHEETAH, 4, EK_CHEETAH>(grid, tpb, lds, s, a);
    return hipGetLastError();
  }
  // Pusher: 16 one-way plane rows in slot 1, 7 two-way capsule-capsule rows
  // as contact halves in slot 2, 16-entry contact lists, joint halves, the
  // damping folded (no body copies: F_C16)
  constexpr int F_PUSHER = F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G;
  if (fold && L == 16 && k == BX_ENV_PUSHER && (feat & ~F_G1) == F_PUSHER) {
    if (gw <= 4) launch_env_kind<F_PUSHER, 4, EK_PUSHER>(grid, tpb, lds, s, a);
    else launch_env_kind<F_PUSHER, 8, EK_PUSHER>(grid, tpb, lds, s, a);
    return hipGetLastError();
  }
  // HumanoidStandup: the Humanoid system lying down, 22 ground rows (F_R2)
  if (fold && L == 16 && (k == BX_ENV_HUMANOID || k == BX_ENV_HUMANOID_STANDUP) &&
      feat == (F_SPH | F_G1 | F_R2)) {
    if (a.packed && a.n_steps <= 1)
      launch_one<EnvArgs>(env_step_packed_kernel<16, 1, F_SPH | F_G1 | F_R2, 8, EK_HUM>, grid, tpb, lds, s, a);
    else
      launch_one<EnvArgs>(env_step_kernel<16, 1, F_SPH | F_G1 | F_R2, 8, EK_HUM>, grid, tpb, lds, s, a);
    return hipGetLastError();
  }
  // every other env's Env.step (one packed step): the one-step kernels, whose
  // first loads need no header
  if (a.packed && a.n_steps <= 1) {
    BX_DISPATCH_SINGLE(env_step_packed_kernel, EnvArgs)
    return hipGetLastError();
  }
  BX_DISPATCH_SINGLE(env_step_kernel, EnvArgs)
  return hipGetLastError();
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
