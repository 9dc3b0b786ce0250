// optim_launch.h — the fused optimiser step's launcher (optim_kernels.hip),
// apart from the other launch headers so no other unit depends on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

namespace bx {

// lanes of one workgroup (4 waves)
constexpr int OPT_BLOCK = 256;
// elements of one tensor that one workgroup owns: one 16-byte access per lane
// and array. At PPO's 290 k parameters that is 290 workgroups on 256 CUs with
// five independent loads in flight per lane, and a bias of a few hundred
// elements costs one workgroup; a larger chunk would only lengthen the
// dependent chain inside the one launch whose fixed cost is what is paid.
constexpr int OPT_VEC = 4;
constexpr int OPT_CHUNK = OPT_BLOCK * OPT_VEC;

// one non-empty tensor as the kernel reads it
struct OptTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* target;  // null: no target update
  int64_t n;
  float step_size;      // (float)(lr / (1 - beta1^step))
  float tau;
  float one_minus_tau;  // (float)(1 - tau), the difference taken in double
  int32_t vec;          // every pointer 16-byte aligned: the 16-byte path
};

// bx_adam_step's table, passed by value with the launch: the non-empty
// tensors and the prefix sums of their chunk counts (first[k] is tensor k's
// first workgroup, first[n_tensors] the grid)
struct OptArgs {
  OptTensor t[BX_OPT_MAX_TENSORS];
  int32_t first[BX_OPT_MAX_TENSORS + 1];
  int32_t n_tensors;
  float one_minus_beta1;  // (float)(1 - beta1)
  float beta2;            // (float)beta2
  float one_minus_beta2;  // (float)(1 - beta2)
  float bc2_sqrt;         // (float)sqrt(1 - beta2^step)
  float eps;
};

inline int64_t opt_chunks(int64_t n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

// The host's share of the arithmetic, in optim_kernels.hip's unit (IEEE flags:
// NaN comparisons hold and a double division is a division). The check
// returns null or why the scalars are refused.
const char* opt_check_scalars(double beta1, double beta2, float eps);
void opt_set_scalars(OptArgs& a, int64_t step, double beta1, double beta2, float eps);
void opt_set_tensor(OptTensor& d, float lr, float tau, int64_t step, double beta1);

// the one launch, on `s`; a.first[a.n_tensors] >= 1
hipError_t launch_adam_step(const OptArgs& a, hipStream_t s);

}  // namespace bx
