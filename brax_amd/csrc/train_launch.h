// train_launch.h — the learner-side kernels' launchers (train_kernels.hip),
// apart from pbd_launch.h so the step kernels' units do not depend on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

namespace bx {

// bx_compute_gae's arguments (include/brax_amd.h)
struct GaeArgs {
  int64_t T, B;
  bx_seq reward, done, truncation, values, vs, adv;
  const float* bootstrap;
  float reward_scaling, discount, lambda;
};

// time steps whose inputs one lane loads before it runs their dependent chain
constexpr int GAE_CHUNK = 8;

hipError_t launch_compute_gae(const GaeArgs& a, hipStream_t s);

}  // namespace bx
