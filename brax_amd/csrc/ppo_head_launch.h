// ppo_head_launch.h — the PPO loss head's launchers (ppo_head_kernels.hip),
// apart from the other launch headers so no other unit depends on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

namespace bx {

// lanes of one workgroup (4 waves): an env each in the scan workgroups, a
// (t, env) row each in the row workgroups
constexpr int PPO_HEAD_BLOCK = 256;
// time steps whose inputs one lane loads before it runs their dependent chain
// (bx_compute_gae's GAE_CHUNK, restated)
constexpr int PPO_HEAD_CHUNK = 8;
// doubles one scan workgroup leaves: the count, mean and centred square sum
// of its advantages, and the sum of its squared value errors
constexpr int PPO_HEAD_SCAN_PART = 4;

// bx_ppo_head's arguments (include/brax_amd.h) and the workspace's parts
struct PpoHeadArgs {
  int64_t T, B, A;
  bx_seq logits, baseline, raw, eps, log_prob, reward, done, truncation;
  const float* bootstrap;
  float reward_scaling, discount, lambda, clip_lo, clip_hi, entropy_cost, min_std;
  int32_t normalize;
  float* losses;
  bx_seq dlogits, dbaseline;
  bx_seq vs, adv;  // a null ptr: not wanted
  int64_t scan_groups, row_groups;
  double* scan_part;  // (scan_groups, PPO_HEAD_SCAN_PART)
  double* row_part;   // (row_groups,): the rows' entropy sums
  float* w_adv;       // (T, B) contiguous: the un-normalised advantages
  float* w_rho;       // (T, B) contiguous: exp(log-prob - behaviour log-prob)
};

inline int64_t ppo_head_groups(int64_t n) { return (n + PPO_HEAD_BLOCK - 1) / PPO_HEAD_BLOCK; }

// the doubles first (8-byte aligned in a 16-byte aligned workspace), the
// total rounded up to 16 bytes
inline int64_t ppo_head_workspace_bytes(int64_t T, int64_t B) {
  const int64_t doubles = ppo_head_groups(B) * PPO_HEAD_SCAN_PART + ppo_head_groups(T * B);
  return (8 * doubles + 4 * 2 * T * B + 15) / 16 * 16;
}

// fills the workspace pointers and group counts of `a` from a.T and a.B
inline void ppo_head_carve(PpoHeadArgs& a, void* workspace) {
  a.scan_groups = ppo_head_groups(a.B);
  a.row_groups = ppo_head_groups(a.T * a.B);
  a.scan_part = (double*)workspace;
  a.row_part = a.scan_part + a.scan_groups * PPO_HEAD_SCAN_PART;
  a.w_adv = (float*)(a.row_part + a.row_groups);
  a.w_rho = a.w_adv + a.T * a.B;
}

// the two launches, in order on `s`
hipError_t launch_ppo_head(const PpoHeadArgs& a, hipStream_t s);

}  // namespace bx
