// train_kernels.hip — the learner side: kernels that consume a trajectory.
// Its own translation unit with its own flags (Makefile): IEEE float32, no
// finite-math assumptions and no contraction, because bx_compute_gae promises
// the bits of the same lines run as separate elementwise operations, NaN and
// Inf included. It includes none of the step kernels' headers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_launch.h"

namespace bx {

// Generalised advantage estimation (include/brax_amd.h bx_compute_gae): one
// lane per env walks its sequence backwards. The recurrence is a chain of
// dependent float32 operations, but its inputs are not: a lane issues the 4 x
// GAE_CHUNK loads of a chunk of steps first and runs the chain on registers,
// so a chunk costs one memory round trip, not one per step. 8 steps x 4
// inputs are 32 registers of the 64 a wave may hold at full occupancy
// (profiles/gae_code_object.txt); nothing goes through LDS. Consecutive lanes
// are consecutive envs: time-major arrays coalesce, [B, T] views do not (each
// lane then reads its own row; the chunk's loads still overlap).
__global__ void __launch_bounds__(64) compute_gae_kernel(GaeArgs A) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= A.B) return;
  const float* __restrict__ rw = A.reward.ptr + e * A.reward.env_stride;
  const float* __restrict__ dn = A.done.ptr + e * A.done.env_stride;
  const float* __restrict__ tr = A.truncation.ptr + e * A.truncation.env_stride;
  const float* __restrict__ va = A.values.ptr + e * A.values.env_stride;
  float* __restrict__ vs = A.vs.ptr + e * A.vs.env_stride;
  float* __restrict__ ad = A.adv.ptr + e * A.adv.env_stride;
  const int64_t rw_t = A.reward.time_stride, dn_t = A.done.time_stride,
                tr_t = A.truncation.time_stride, va_t = A.values.time_stride,
                vs_t = A.vs.time_stride, ad_t = A.adv.time_stride;
  const float scale = A.reward_scaling, discount = A.discount, lambda = A.lambda;
  float v_next = A.bootstrap[e];
  float vs_next = v_next;
  float acc = 0.f;
  // steps hi - 1 .. hi - GAE_CHUNK of each chunk, the first chunk at the end
  // of the sequence; the last chunk may reach below step 0: those slots load
  // step 0 again (in bounds) and are not computed
  for (int64_t hi = A.T; hi > 0; hi -= GAE_CHUNK) {
    float r_[GAE_CHUNK], d_[GAE_CHUNK], t_[GAE_CHUNK], v_[GAE_CHUNK];
#pragma unroll
    for (int i = 0; i < GAE_CHUNK; ++i) {
      const int64_t t = hi - 1 - i < 0 ? 0 : hi - 1 - i;
      r_[i] = rw[t * rw_t];
      d_[i] = dn[t * dn_t];
      t_[i] = tr[t * tr_t];
      v_[i] = va[t * va_t];
    }
#pragma unroll
    for (int i = 0; i < GAE_CHUNK; ++i) {
      const int64_t t = hi - 1 - i;
      if (t < 0) break;
      const float v = v_[i];
      const float r = r_[i] * scale;
      const float mask = 1.f - t_[i];
      const float term = d_[i] * mask;
      const float g = discount * (1.f - term);
      const float delta = ((r + g * v_next) - v) * mask;
      acc = delta + ((g * mask) * lambda) * acc;
      const float vs_t_ = acc + v;
      const float adv = ((r + g * vs_next) - v) * mask;
      vs[t * vs_t] = vs_t_;
      ad[t * ad_t] = adv;
      v_next = v;
      vs_next = vs_t_;
    }
  }
}

hipError_t launch_compute_gae(const GaeArgs& a, hipStream_t s) {
  dim3 grid((unsigned)((a.B + 63) / 64));
  hipLaunchKernelGGL(compute_gae_kernel, grid, dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace bx
