// replay_launch.h — the replay queue's launchers (replay_kernels.hip), apart
// from pbd_launch.h so the step kernels' units do not depend on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

namespace bx {

// One launch's arguments: the ring and the batch's field table, every value
// uniform over the launch. off[f] is the first row word of field f, off[f] =
// row_words for f >= n_fields (no word selects such a field); base[f] is the
// field's pointer moved back by off[f] floats, so word w of batch row r lives
// at base[f] + r * stride[f] + w.
struct ReplayArgs {
  float* data;
  int64_t capacity, position, size, n;
  uint64_t seed, offset;
  int64_t* idx_out;
  int32_t row_words;
  int32_t off[BX_FIELDS_MAX];
  float* base[BX_FIELDS_MAX];
  int64_t stride[BX_FIELDS_MAX];
};

hipError_t launch_replay_insert(const ReplayArgs& a, hipStream_t s);
hipError_t launch_replay_sample(const ReplayArgs& a, hipStream_t s);

}  // namespace bx
