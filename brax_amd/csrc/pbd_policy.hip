// pbd_policy.hip — the closed-loop rollout's translation unit: the K-step
// rollout kernels of pbd_single.hip with the policy action source
// (env_step_body's POL, pbd_kernels.hip), their family for the env launcher
// (launch_env_family, pbd_launch.h, over pbd_dispatch.h's decision), and the
// standard normal fill that reproduces their noise (bx_normal_slabs). Built
// with pbd_single.hip's flags; the kernels of that unit are not touched.
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
// the Ant kernel held to 256 registers, as env_rollout_wide_kernel (ZH off:
// with the frozen side in registers it spilled 5 VGPRs, 24 B of scratch)
template <int L, int MODE, int F, int M, int EK = EK_ANY>
__global__ void __launch_bounds__(L > 64 ? L : 64) __attribute__((amdgpu_waves_per_eu(2)))
env_policy_rollout_wide_kernel(EnvArgs A, PolArgs Q) {
  env_step_body<L, MODE, F, M, EK, true, false, true, false, false, false>(A, Q);
}

BX_ENV_FAMILY(PolicyFamily, FAM_POLICY, env_policy_rollout_kernel, env_policy_rollout_wide_kernel)
hipError_t launch_env_policy_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                    hipStream_t s, const EnvArgs& a, const PolArgs& q, int fold) {
  return launch_env_family<PolicyFamily>(L, feat, gw, tpb, n_envs, lds, s, fold, a, q);
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
