// replay_kernels.hip — the off-policy learner's replay queue: a batch of
// transitions into the ring, and a uniform sample out of it, one launch each
// (include/brax_amd.h bx_replay_insert / bx_replay_sample). Both kernels only
// move 32-bit words; its own translation unit with train_kernels.hip's flags,
// and it includes none of the step kernels' headers (bx_mix.h is the counter
// RNG's mix alone).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bx_mix.h"
#include "replay_launch.h"

namespace bx {

namespace {

constexpr int REPLAY_WAVES = 4;  // waves of a workgroup, each on rows of its own
// 64-word pieces of a row a lane loads before it stores the first: a row of
// up to 256 words (Ant's is 185) is one round trip, not one per piece
constexpr int REPLAY_CHUNK = 4;
constexpr unsigned REPLAY_MAX_BLOCKS = 4096;  // rows past them: grid stride

// Every pointer here is device memory. A field's row pointer is rebuilt from
// integer arithmetic, which loses that fact; the address space restores it,
// so the accesses are global loads and stores, not flat ones.
typedef __attribute__((address_space(1))) uint32_t gword;

// this wave's first row and the launch's row stride, as uniform values
__device__ __forceinline__ int64_t wave_index() {
  return (int64_t)blockIdx.x * REPLAY_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// the field table at batch row r: word w of the row lives at word(w)[w],
// the row pointer of the last field f with off[f] <= w. A lane reaches its
// own by adding the steps between consecutive fields' row pointers that lie
// at or below its word: the steps are uniform (scalar registers), so the
// table needs no memory, and a lane's choice is 7 compares and masked adds.
struct FieldRow {
  uint64_t first, step[BX_FIELDS_MAX];
  __device__ __forceinline__ FieldRow(const ReplayArgs& A, int64_t r) {
    uint64_t prev = first = (uint64_t)(A.base[0] + r * A.stride[0]);
#pragma unroll
    for (int f = 1; f < BX_FIELDS_MAX; ++f) {
      const uint64_t p = (uint64_t)(A.base[f] + r * A.stride[f]);
      step[f] = p - prev;
      prev = p;
    }
  }
  __device__ __forceinline__ gword* word(const ReplayArgs& A, int w) const {
    uint64_t q = first;
#pragma unroll
    for (int f = 1; f < BX_FIELDS_MAX; ++f) q += w >= A.off[f] ? step[f] : 0;
    return (gword*)q + w;
  }
};

// one row between the ring (row `ring_row`, contiguous) and the batch's fields; lanes
// along the row's words, so the ring side is one coalesced run and each field
// is one. TO_RING: fields -> ring (insert), else ring -> fields (sample).
template <bool TO_RING>
__device__ __forceinline__ void move_row(const ReplayArgs& A, int64_t ring_row, const FieldRow& fr,
                                         int lane) {
  gword* __restrict__ ring = (gword*)(uint64_t)A.data + ring_row * A.row_words;
  for (int w0 = 0; w0 < A.row_words; w0 += 64 * REPLAY_CHUNK) {
    uint32_t v[REPLAY_CHUNK];
#pragma unroll
    for (int i = 0; i < REPLAY_CHUNK; ++i) {
      const int w = w0 + i * 64 + lane;
      if (w < A.row_words) v[i] = TO_RING ? *fr.word(A, w) : ring[w];
    }
#pragma unroll
    for (int i = 0; i < REPLAY_CHUNK; ++i) {
      const int w = w0 + i * 64 + lane;
      if (w < A.row_words) {
        if (TO_RING) ring[w] = v[i];
        else *fr.word(A, w) = v[i];
      }
    }
  }
}

}  // namespace

// batch row r -> ring row (position + r) mod capacity; 0 <= position <
// capacity and r < n <= capacity (bx_replay_insert checks), so one
// subtraction wraps
__global__ void __launch_bounds__(64 * REPLAY_WAVES) replay_insert_kernel(ReplayArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * REPLAY_WAVES;
  for (int64_t r = wave_index(); r < A.n; r += waves) {
    int64_t d = A.position + r;
    if (d >= A.capacity) d -= A.capacity;
    move_row<true>(A, d, FieldRow(A, r), lane);
  }
}

// sample j <- ring row (position - size + k) mod capacity, k = mulhi64(mix64(
// seed, offset + j), size) < size; 1 <= size <= capacity and 0 <= position <
// capacity (bx_replay_sample checks), so the sum is in [-capacity, capacity)
// and one addition wraps. The draw is the wave's own scalar arithmetic.
__global__ void __launch_bounds__(64 * REPLAY_WAVES) replay_sample_kernel(ReplayArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * REPLAY_WAVES;
  for (int64_t j = wave_index(); j < A.n; j += waves) {
    const uint64_t z = mix64(A.seed, A.offset + (uint64_t)j);
    const uint64_t k = __umul64hi(z, (uint64_t)A.size);
    int64_t row = A.position - A.size + (int64_t)k;
    if (row < 0) row += A.capacity;
    if (A.idx_out && lane == 0) A.idx_out[j] = row;
    move_row<false>(A, row, FieldRow(A, j), lane);
  }
}

static dim3 replay_grid(int64_t n) {
  const int64_t blocks = (n + REPLAY_WAVES - 1) / REPLAY_WAVES;
  return dim3((unsigned)(blocks < REPLAY_MAX_BLOCKS ? blocks : REPLAY_MAX_BLOCKS));
}

hipError_t launch_replay_insert(const ReplayArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(replay_insert_kernel, replay_grid(a.n), dim3(64 * REPLAY_WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_replay_sample(const ReplayArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(replay_sample_kernel, replay_grid(a.n), dim3(64 * REPLAY_WAVES), 0, s, a);
  return hipGetLastError();
}

}  // namespace bx
