// bx_mix.h — the counter RNG's 64-bit mix, shared by the step kernels'
// uniform_at (pbd_kernels.hip) and the replay sampler (replay_kernels.hip):
// one copy of the constants, nothing else in here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bx {

// splitmix64's finaliser over (seed, counter i), all 64 bits
// (in two parts for a caller that steps the counter: start is linear in i, so
// start(seed, i + d) = start(seed, i) + d)
__host__ __device__ __forceinline__ uint64_t mix64_start(uint64_t seed, uint64_t i) {
  return seed * 0x9E3779B97F4A7C15ull + i + 0x632BE59BD9B4E019ull;
}
__host__ __device__ __forceinline__ uint64_t mix64_finish(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t i) {
  return mix64_finish(mix64_start(seed, i));
}

}  // namespace bx
