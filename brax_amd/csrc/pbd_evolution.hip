// pbd_evolution.hip — the optimiser side of the evolution agents, with the
// parameter noise regenerated on chip: bx_population_perturb writes the
// population's rows and bx_population_delta sums weight x noise, both from
// normal_at (pbd_kernels.hip), so no (P, n_params) noise array exists. Built
// with pbd_policy.hip's flags: the noise bits are logf / cosf as that unit
// compiles them, the bits bx_normal_slabs writes. No step kernel is
// instantiated here.
#define BX_TU_FAST
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_kernels.hip"
#include "pbd_launch.h"

namespace bx {

// eps[p, j] of the population noise
__device__ __forceinline__ float pop_eps(uint64_t seed, uint64_t offset, int64_t p, int64_t n,
                                         int64_t j) {
  return normal_at(seed, offset + 2u * ((uint64_t)p * (uint64_t)n + (uint64_t)j));
}

// theta[j] +- sigma eps in float64, the product and the sum each rounded on
// their own, then one float32 rounding: `PolicyPopulation.perturb_`'s torch
// expression
__device__ __forceinline__ void perturbed(float th, double sigma, float eps, float& plus,
                                          float& minus) {
#pragma clang fp contract(off)
  const double step = sigma * (double)eps;
  const double t = (double)th;
  plus = (float)(t + step);
  minus = (float)(t - step);
}
// acc + w eps and acc + x in float64, every operation rounded on its own
__device__ __forceinline__ double weighted_add(double acc, float w, float eps) {
#pragma clang fp contract(off)
  const double term = (double)w * (double)eps;
  return acc + term;
}
__device__ __forceinline__ double plain_add(double acc, double x) {
#pragma clang fp contract(off)
  return acc + x;
}

// one lane per four consecutive parameters of one direction: lane l of a
// wave writes the 16 bytes after lane l - 1's. VEC: rows 16-byte aligned
// (base and stride), so a full quad is one 16-byte store; the last quad of a
// row that n does not fill, and every quad without VEC, store word by word
// (the stride padding is never written)
template <bool VEC>
__global__ void __launch_bounds__(256)
population_perturb_kernel(float* __restrict__ rows, const float* __restrict__ theta,
                          const uint8_t* __restrict__ frozen, int64_t P, int64_t n, int64_t stride,
                          int64_t quads, double sigma, uint64_t seed, uint64_t offset,
                          int antithetic) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * quads) return;
  const int64_t p = i / quads, j0 = (i - p * quads) * 4;
  float a[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t j = j0 + k;
    a[k] = b[k] = 0.f;
    if (j < n) {
      const float th = theta[j];
      a[k] = b[k] = th;
      if (!frozen || !frozen[j]) perturbed(th, sigma, pop_eps(seed, offset, p, n, j), a[k], b[k]);
    }
  }
  float* ra = rows + p * stride + j0;
  float* rb = rows + (P + p) * stride + j0;
  if (VEC && j0 + 4 <= n) {
    *reinterpret_cast<float4*>(ra) = make_float4(a[0], a[1], a[2], a[3]);
    if (antithetic) *reinterpret_cast<float4*>(rb) = make_float4(b[0], b[1], b[2], b[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < n) {
        ra[k] = a[k];
        if (antithetic) rb[k] = b[k];
      }
  }
}

hipError_t launch_population_perturb(float* rows, const float* theta, const uint8_t* frozen,
                                     int64_t P, int64_t n, int64_t stride, double sigma,
                                     uint64_t seed, uint64_t offset, int antithetic,
                                     hipStream_t s) {
  const int64_t quads = (n + 3) / 4;
  const bool vec = ((uintptr_t)rows & 15) == 0 && (stride & 3) == 0;
  dim3 grid((unsigned)((P * quads + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(population_perturb_kernel<true>, grid, dim3(256), 0, s, rows, theta, frozen,
                       P, n, stride, quads, sigma, seed, offset, antithetic);
  else
    hipLaunchKernelGGL(population_perturb_kernel<false>, grid, dim3(256), 0, s, rows, theta,
                       frozen, P, n, stride, quads, sigma, seed, offset, antithetic);
  return hipGetLastError();
}

// sum over the directions of chunk blockIdx.y (BX_POPULATION_DELTA_CHUNK of
// them, ascending) of w[p] eps[p, j] in float64, one lane per j: consecutive
// lanes take consecutive j, and w[p] is uniform over the workgroup. A zero
// weight is skipped by its bits (eps is finite, so the skipped term is an
// exact zero; no floating-point compare, so a NaN weight is never skipped
// under the unit's finite-math flags). One chunk: the float32 result goes
// straight to `out`; more: the partial goes to part[chunk * n + j].
__global__ void __launch_bounds__(256)
population_delta_kernel(float* __restrict__ out, double* __restrict__ part,
                        const float* __restrict__ w, const uint8_t* __restrict__ frozen, int64_t P,
                        int64_t n, uint64_t seed, uint64_t offset) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t c = blockIdx.y;
  const int64_t p0 = c * BX_POPULATION_DELTA_CHUNK;
  const int64_t p1 = p0 + BX_POPULATION_DELTA_CHUNK < P ? p0 + BX_POPULATION_DELTA_CHUNK : P;
  double acc = 0.;
  if (!frozen || !frozen[j]) {
    for (int64_t p = p0; p < p1; ++p) {
      const float wp = w[p];
      if ((__float_as_uint(wp) & 0x7fffffffu) == 0u) continue;
      acc = weighted_add(acc, wp, pop_eps(seed, offset, p, n, j));
    }
  }
  if (part) part[c * n + j] = acc;
  else out[j] = (float)acc;
}

// the chunk partials of one j in ascending chunk order, then the one float32
// rounding
__global__ void __launch_bounds__(256)
population_delta_sum_kernel(float* __restrict__ out, const double* __restrict__ part, int64_t n,
                            int64_t chunks) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double acc = part[j];
  for (int64_t c = 1; c < chunks; ++c) acc = plain_add(acc, part[c * n + j]);
  out[j] = (float)acc;
}

hipError_t launch_population_delta(float* out, const float* w, const uint8_t* frozen, int64_t P,
                                   int64_t n, uint64_t seed, uint64_t offset, double* part,
                                   hipStream_t s) {
  const int64_t chunks = (P + BX_POPULATION_DELTA_CHUNK - 1) / BX_POPULATION_DELTA_CHUNK;
  const unsigned gx = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(population_delta_kernel, dim3(gx, (unsigned)chunks), dim3(256), 0, s, out,
                     chunks > 1 ? part : nullptr, w, frozen, P, n, seed, offset);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || chunks == 1) return e;
  hipLaunchKernelGGL(population_delta_sum_kernel, dim3(gx), dim3(256), 0, s, out, part, n, chunks);
  return hipGetLastError();
}

}  // namespace bx
