// optim_kernels.hip — the fused optimiser step (include/brax_amd.h
// bx_adam_step): Adam for up to BX_OPT_MAX_TENSORS tensors, and the soft target
// update of those that carry a target, in ONE launch. train_kernels.hip's
// flags: IEEE float32, no finite-math assumptions and no contraction, since the
// target update promises the bits of three separate elementwise operations. It
// includes none of the other units' headers.
//
// A workgroup of OPT_BLOCK lanes owns OPT_CHUNK consecutive elements of one
// tensor. Which tensor is a function of blockIdx.x alone: a binary search of
// the chunk counts' prefix sums, which arrive with the tensor table in the
// kernel's arguments, so the search and the table row are scalar loads and
// every branch on them is wave-uniform. Where all of a tensor's pointers are
// 16-byte aligned a lane takes 4 consecutive elements in one 16-byte access per
// array; otherwise a lane takes elements lane, lane + 256, ... a float at a
// time. Both forms run the same operations on an element: the same bits. The
// last chunk of a tensor is masked: no lane loads or stores at or past n.
//
// Purely elementwise: no LDS, no atomics, no cross-lane operation. A
// non-finite value stays in its element.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "optim_launch.h"

namespace bx {

namespace {

// one element's Adam step (the header's four lines, each operation rounded
// to float32 on its own)
__device__ __forceinline__ void adam_element(const OptArgs& A, float step_size, float g, float& p,
                                             float& m, float& v) {
#pragma clang fp contract(off)
  m = m + (g - m) * A.one_minus_beta1;
  v = v * A.beta2 + (g * g) * A.one_minus_beta2;
  const float denom = sqrtf(v) / A.bc2_sqrt + A.eps;
  p = p - step_size * (m / denom);
}

__device__ __forceinline__ float target_element(float t, float p, float one_minus_tau, float tau) {
#pragma clang fp contract(off)
  const float a = t * one_minus_tau;
  const float b = p * tau;
  return a + b;
}

__device__ __forceinline__ void scalar_element(const OptArgs& A, const OptTensor& T, int64_t i) {
  float p = T.p[i], m = T.m[i], v = T.v[i];
  adam_element(A, T.step_size, T.g[i], p, m, v);
  T.p[i] = p;
  T.m[i] = m;
  T.v[i] = v;
  if (T.target) T.target[i] = target_element(T.target[i], p, T.one_minus_tau, T.tau);
}

}  // namespace

__global__ void __launch_bounds__(OPT_BLOCK) adam_step_kernel(const OptArgs A) {
  // the tensor of this workgroup: the last k with first[k] <= blockIdx.x
  const int32_t wg = (int32_t)blockIdx.x;
  int lo = 0, hi = A.n_tensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.first[mid] <= wg) lo = mid;
    else hi = mid;
  }
  const OptTensor& T = A.t[lo];
  const int64_t base = (int64_t)(wg - A.first[lo]) * OPT_CHUNK;
  const int64_t n = T.n;
  if (T.vec) {
    const int64_t i = base + (int64_t)threadIdx.x * OPT_VEC;
    if (i + OPT_VEC <= n) {
      float4 p = *reinterpret_cast<const float4*>(T.p + i);
      const float4 g = *reinterpret_cast<const float4*>(T.g + i);
      float4 m = *reinterpret_cast<const float4*>(T.m + i);
      float4 v = *reinterpret_cast<const float4*>(T.v + i);
      adam_element(A, T.step_size, g.x, p.x, m.x, v.x);
      adam_element(A, T.step_size, g.y, p.y, m.y, v.y);
      adam_element(A, T.step_size, g.z, p.z, m.z, v.z);
      adam_element(A, T.step_size, g.w, p.w, m.w, v.w);
      *reinterpret_cast<float4*>(T.p + i) = p;
      *reinterpret_cast<float4*>(T.m + i) = m;
      *reinterpret_cast<float4*>(T.v + i) = v;
      if (T.target) {
        float4 t = *reinterpret_cast<const float4*>(T.target + i);
        t.x = target_element(t.x, p.x, T.one_minus_tau, T.tau);
        t.y = target_element(t.y, p.y, T.one_minus_tau, T.tau);
        t.z = target_element(t.z, p.z, T.one_minus_tau, T.tau);
        t.w = target_element(t.w, p.w, T.one_minus_tau, T.tau);
        *reinterpret_cast<float4*>(T.target + i) = t;
      }
    } else {
      // the tensor's last 1 .. 3 elements (at most one lane of the tensor)
      for (int64_t j = i; j < n; ++j) scalar_element(A, T, j);
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < OPT_VEC; ++r) {
    const int64_t i = base + r * OPT_BLOCK + threadIdx.x;
    if (i < n) scalar_element(A, T, i);
  }
}

const char* opt_check_scalars(double beta1, double beta2, float eps) {
  // (written so that a NaN fails too)
  if (!(beta1 >= 0.0 && beta1 < 1.0)) return "beta1 outside [0, 1)";
  if (!(beta2 >= 0.0 && beta2 < 1.0)) return "beta2 outside [0, 1)";
  if (!(eps >= 0.f)) return "negative eps";
  return nullptr;
}

void opt_set_scalars(OptArgs& a, int64_t step, double beta1, double beta2, float eps) {
  a.one_minus_beta1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.one_minus_beta2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
  a.eps = eps;
}

void opt_set_tensor(OptTensor& d, float lr, float tau, int64_t step, double beta1) {
  d.step_size = (float)((double)lr / (1.0 - pow(beta1, (double)step)));
  d.tau = tau;
  d.one_minus_tau = (float)(1.0 - (double)tau);
}

hipError_t launch_adam_step(const OptArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)a.first[a.n_tensors]), dim3(OPT_BLOCK), 0, s,
                     a);
  return hipGetLastError();
}

}  // namespace bx
