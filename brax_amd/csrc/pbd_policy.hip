// pbd_policy.hip — the closed-loop rollout's translation unit: the K-step
// rollout kernels of pbd_single.hip with the policy action source
// (env_step_body's POL, pbd_kernels.hip), their launcher, and the standard
// normal fill that reproduces their noise (bx_normal_slabs). Built with
// pbd_single.hip's flags; the kernels of that unit are not touched.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_dispatch.h"
#include "pbd_kernels.hip"
#include "pbd_launch.h"

namespace bx {

template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) BX_STEP_ATTR
env_policy_rollout_kernel(EnvArgs A, PolArgs Q) {
  env_step_body<L, MODE, F, M, EK, true, false, true>(A, Q);
}
// the Ant kernel held to 256 registers, as env_rollout_wide_kernel
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_policy_rollout_wide_kernel(EnvArgs A, PolArgs Q) {
  env_step_body<L, MODE, F, M, EK, true, false, true>(A, Q);
}

static void launch_pol(void (*k)(EnvArgs, PolArgs), dim3 grid, int tpb, size_t lds, hipStream_t s,
                       const EnvArgs& a, const PolArgs& q) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(tpb), lds, s, a, q);
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

#define BX_POLICY_CASE(VL, VF, VM, UNUSED) \
  case single_key(VL, VF, VM): launch_pol(env_policy_rollout_kernel<VL, 1, VF, VM>, grid, tpb, lds, s, a, q); break;

// the selection of launch_env_step_single (pbd_single.hip) for a K-step
// launch: the env kinds' own kernels where their conditions hold, else the
// variant list's
hipError_t launch_env_policy_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                    hipStream_t s, const EnvArgs& a, const PolArgs& q, int fold) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  const int k = a.P.kind;
  const bool jb = (fold & 2) != 0;
  const bool ant_ok = jb && ((fold & 4) != 0 || !cb_feat(F_G1 | F_JH));
  if (fold && ant_ok && L == 16 && gw <= 4 && k == BX_ENV_ANT && feat == (F_G1 | F_JH)) {
    const bool wide = (int64_t)grid.x * (tpb / 64 > 0 ? tpb / 64 : 1) > 4 * (int64_t)cu_count();
    if (wide)
      launch_pol(env_policy_rollout_wide_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, q);
    else
      launch_pol(env_policy_rollout_kernel<16, 1, F_G1 | F_JH, 4, EK_ANT>, grid, tpb, lds, s, a, q);
    return hipGetLastError();
  }
  constexpr int F_CHEETAH = F_CC | F_TW | F_JH | F_R2 | F_R2G;
  if (fold && jb && L == 16 && gw <= 4 && k == BX_ENV_HALFCHEETAH && (feat & ~F_G1) == F_CHEETAH) {
    launch_pol(env_policy_rollout_kernel<16, 1, F_CHEETAH, 4, EK_CHEETAH>, grid, tpb, lds, s, a, q);
    return hipGetLastError();
  }
  constexpr int F_PUSHER = F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G;
  if (fold && L == 16 && k == BX_ENV_PUSHER && (feat & ~F_G1) == F_PUSHER) {
    if (gw <= 4) launch_pol(env_policy_rollout_kernel<16, 1, F_PUSHER, 4, EK_PUSHER>, grid, tpb, lds, s, a, q);
    else launch_pol(env_policy_rollout_kernel<16, 1, F_PUSHER, 8, EK_PUSHER>, grid, tpb, lds, s, a, q);
    return hipGetLastError();
  }
  const SingleVariant v = single_variant(L, feat, gw);
  switch (single_key(v.L, v.F, v.M)) {
    BX_SINGLE_VARIANTS(BX_POLICY_CASE, 0)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the kernels' noise on its own: out[s * slab_n + j] = normal_at(seed, offset
// + epoch * epoch_stride + s * slab_stride + 2 j)
__global__ void normal_slabs_kernel(float* out, int64_t slab_n, int64_t n, uint64_t seed,
                                    uint64_t offset, uint64_t slab_stride,
                                    const int64_t* __restrict__ epoch, uint64_t epoch_stride) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t e = epoch ? (uint64_t)epoch[0] : 0ull;
  const int64_t sl = i / slab_n, j = i - sl * slab_n;
  out[i] = normal_at(seed, offset + e * epoch_stride + (uint64_t)sl * slab_stride + 2u * (uint64_t)j);
}
hipError_t launch_normal_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                               uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                               uint64_t epoch_stride, hipStream_t s) {
  const int64_t n = slab_n * n_slabs;
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(normal_slabs_kernel, grid, dim3(256), 0, s, out, slab_n, n, seed, offset,
                     slab_stride, epoch, epoch_stride);
  return hipGetLastError();
}

}  // namespace bx
