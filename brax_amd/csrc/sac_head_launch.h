// sac_head_launch.h — the SAC loss heads' launchers (sac_head_kernels.hip),
// apart from the other launch headers so no other unit depends on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

namespace bx {

// lanes of one workgroup (4 waves): a row each in sample, losses and
// sample_backward, an element each in prep
constexpr int SAC_HEAD_BLOCK = 256;
// doubles one row workgroup of the losses launch leaves: its rows' sums of the
// critic's squared errors, the actor's terms and the alpha terms
constexpr int SAC_HEAD_PART = 3;
// workgroups of the prep launch at most (each strides over the elements)
constexpr int64_t SAC_HEAD_PREP_GROUPS = 1 << 16;

struct SacPrepArgs {
  int64_t B, O, A;
  const float *obs, *next_obs, *action;
  int64_t obs_pitch, next_obs_pitch, action_pitch;
  const float *mean, *std;  // both null: no normaliser
  float *x_cur, *x_next, *x_pi;
  int64_t x_pitch;
};

struct SacSampleArgs {
  int64_t B, A;
  int32_t n_jobs;
  float min_std;
  bx_sac_sample_job job[BX_SAC_MAX_JOBS];
};

struct SacLossesArgs {
  int64_t B;
  int32_t C;
  const float *lp_alpha, *lp_next, *lp_pi;
  bx_sac_q q;
  const float *reward, *discount, *truncation;
  int64_t reward_stride, discount_stride, truncation_stride;
  const float* log_alpha;
  float reward_scaling, discounting, target_entropy;
  float* g_lp;
  double* part;  // (groups, SAC_HEAD_PART)
};

struct SacBackwardArgs {
  int64_t B, A;
  int32_t C;
  float min_std;
  const float *logits, *eps, *g_lp;
  int64_t logits_pitch, eps_pitch;
  bx_sac_daction da;
  float* dlogits;
  int64_t dlogits_pitch;
  const double* part;  // the losses launch's partials
  float* losses;       // (3,): critic, actor, alpha
  float* dlog_alpha;
};

constexpr int64_t sac_head_groups(int64_t n) { return (n + SAC_HEAD_BLOCK - 1) / SAC_HEAD_BLOCK; }

// the losses launch's partials, which the sample_backward launch sums: the
// total rounded up to 16 bytes
inline int64_t sac_head_workspace_bytes(int64_t B) {
  return (8 * SAC_HEAD_PART * sac_head_groups(B) + 15) / 16 * 16;
}

// one launch each on `s`
hipError_t launch_sac_prep(const SacPrepArgs& a, hipStream_t s);
hipError_t launch_sac_sample(const SacSampleArgs& a, hipStream_t s);
hipError_t launch_sac_losses(const SacLossesArgs& a, hipStream_t s);
hipError_t launch_sac_sample_backward(const SacBackwardArgs& a, hipStream_t s);

}  // namespace bx
