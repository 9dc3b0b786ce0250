// pbd_launch.h — host-side launch entry points of the step kernels' units and
// phase_kernels.hip, and the one launcher of the env launch units
// (launch_env_family over the decisions of pbd_dispatch.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"
#include "pbd_dispatch.h"
#include "pbd_layout.h"

namespace bx {

struct StepArgs {
  const uint32_t* blob;
  int64_t n_envs;
  bx_qp qin, qout;
  const float* act;
  int64_t act_stride, act_width;
  bx_info info;
  // MULTI: the contacts of a pass's penetrating rows past MCBUF (env e's at
  // movf + e * (R - MCBUF) * MOVF_W; null when R <= MCBUF)
  float* movf;
};
struct EnvArgs {
  const uint32_t* blob;
  int64_t n_envs;
  bx_env_params P;
  bx_env_state in, out;
  const float* act;
  int64_t act_stride, act_width;
  // consecutive env steps per launch (bx_env_rollout_packed; <= 1: one step):
  // step t's action rows at act + t * act_step, its outputs at the out
  // pointers + t * out_step floats (rng + t * rng_step)
  int32_t n_steps;
  int64_t act_step, out_step, rng_step;
  // on-device action draws (bx_env_rollout_random; draw = 0: read act): step
  // t's action a of env e is uniform_at(draw_seed, draw_offset + t * draw_step
  // + e * act_width + a, draw_lo, draw_hi), the same bits as bx_uniform_slabs;
  // recorded at act_out[(t * n_envs + e) * act_width + a] when act_out is set
  int32_t draw;
  int32_t packed;  // the outputs are the packed block layout (bx_env_*_packed / rollouts)
  uint64_t draw_seed, draw_offset, draw_step;
  float draw_lo, draw_hi;
  float* act_out;
  // SINGLE mode: blob + o_lane (the lane image), so the one-step kernels
  // issue its loads before the header arrives (last: the other kernels'
  // argument offsets stay as they were)
  const uint32_t* lane_img;
  // the blob's header, for the one-step kernels: read from the arguments,
  // which the kernel holds at its start, instead of one more dependent load
  // from the blob
  BlobHdr hdr;
};
// the policy action source of the env_policy_rollout kernels
// (bx_env_rollout_policy): step t's action row is an MLP of the env's current
// observation, held in LDS between steps. The workgroup's policy area starts
// lds_off words into its LDS: the staged parameters (stage != 0: n_params
// words, padded to 4), then per env obs_words | buf_words | buf_words (the
// observation row and two activation buffers)
struct PolArgs {
  const float* params;  // layer l: W (width[l], width[l+1]) row-major, then b (width[l+1])
  const float* mean;    // (obs_size) or null
  const float* std;
  const float* obs_in;  // (B, obs_size): step 0's observation
  float* raw_out;       // (K, B, A) or null
  float* logp_out;      // (K, B) or null
  int32_t n_layers, act_fn, det, stage;
  int32_t width[BX_POLICY_MAX_LAYERS + 1];  // width[0] = obs_size
  int32_t n_params, lds_off, obs_words, buf_words;
  float min_std;
  uint64_t seed, offset, step;
};
// the evaluation kernels' sums (bx_env_eval_policy / bx_env_eval_packed):
// (M + 3, B) float32, rows = the M metric sums in the env's metric order, the
// reward sum, active_episodes, episode_steps. On chip each env of the
// workgroup holds `words` floats (those M + 3 and the step's M metrics)
// starting lds_off words into the workgroup's LDS
struct EvalArgs {
  const float* in;  // null: a fresh evaluation (zero sums, active 1, steps 0)
  float* out;       // may be `in`
  int32_t lds_off, words;
};
// the population kernels' extras (bx_env_eval_population, pbd_pop.hip): env e
// evaluates the parameter row at PolArgs.params + e * param_stride (0: one
// shared row). On chip each env of the workgroup holds `words` floats starting
// lds_off words into the workgroup's LDS: the observation moments S1 (O) |
// S2 (O) | count (mom_out non-null), then at row_off the env's staged row
// (stage != 0: n_params words, padded to 4)
struct PopArgs {
  const float* mom_in;  // (B, 2 O + 1) or null (zeros)
  float* mom_out;       // may be mom_in; null: no moments
  int64_t param_stride;
  int32_t head, stage, lds_off, words, row_off;
  float reward_shift;
};
struct InfoArgs {
  const uint32_t* blob;
  int64_t n_envs;
  bx_qp q;
  bx_info info;
  int kind, obs_size, obs_flags;
  float coef[8];  // the env's bx_env_params.coef (body indices of the obs programs)
  const float* act;
  int64_t act_stride, act_width;
  float* obs;
  float* angle;  // joint angles (B, D) and velocities (B, D), or null
  float* angvel;
  // reset: env scalars written as zeros (null = skip)
  float* zero_reward;
  float* zero_done;
  float* zero_steps;
  float* zero_trunc;
  float* zero_metrics;
  int n_metrics;
};
struct ResetArgs {
  const uint32_t* blob;
  int64_t n_envs;
  const float* angle;
  const float* vel;
  bx_qp out;
  // gen = 1: angle = default_angle + U(seed, g*2D + k), vel = U(seed, g*2D + D + k)
  // with g = env_offset + e and U uniform in [-scale, scale) (angle/vel unused);
  // seeds non-null: env e uses (seeds[e], k) and (seeds[e], D + k)
  int gen;
  uint64_t seed;
  int64_t env_offset;
  const uint64_t* seeds;
  float scale;
  // gen = 1: the env kind's reset program (bx_env_reset) and its coef
  int kind;
  float coef[8];
  uint32_t* rng_out;  // UR5E / FETCH / GRASP: the per-env streams (or null)
};

// one kernel launch (the translation units' launchers)
template <typename... Args>
static void launch_one(void (*k)(Args...), dim3 grid, int tpb, size_t lds, hipStream_t s, const Args&... a) {
  // tpb threads per workgroup (a multiple of L, <= 64): 64 / L envs share a
  // wavefront by default; 32 halves that (twice the waves for one batch)
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(tpb), lds, s, a...);
}
// the SINGLE-mode grid: tpb / L envs per workgroup
inline dim3 single_grid(int L, int tpb, int64_t n_envs) {
  const int epb = tpb / L;
  return dim3((unsigned)((n_envs + epb - 1) / epb));
}
// compute units of the current device (the launch runs under the system's
// device scope), cached per device
inline int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cached[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// One env launch of a unit's kernel family Fam: the env kind's own kernel
// where kind_variant (pbd_dispatch.h) grants one, Ant's wide twin past one
// wave per SIMD, else the variant list's (single_variant yields listed
// variants only, so its default arm is not reached). Both switches are
// generated from the lists, so nothing is selected without being
// instantiated, and a family instantiates no kind kernel it does not have.
// Fam states what differs between the units: `id` (its EnvFamily) and
//   template <int L, int F, int M, int EK> static auto kernel(const EnvArgs&, bool wide)
// the instantiation's kernel for this launch; x: its kernels' arguments
// after EnvArgs
#define BX_KIND_CASE(VF, VM, VEK, UNUSED)                                                     \
  case kind_key(VF, VM, VEK):                                                                 \
    if constexpr (family_has(Fam::id, VEK)) {                                                 \
      const bool wide = VEK == EK_ANT && ant_wide(grid.x, tpb, cu_count());                   \
      launch_one(Fam::template kernel<16, VF, VM, VEK>(a, wide), grid, tpb, lds, s, a, x...); \
      return hipGetLastError();                                                               \
    }                                                                                         \
    break;
#define BX_VARIANT_CASE(VL, VF, VM, UNUSED)                                                 \
  case single_key(VL, VF, VM):                                                              \
    launch_one(Fam::template kernel<VL, VF, VM, EK_ANY>(a, false), grid, tpb, lds, s, a, x...); \
    break;
template <class Fam, typename... Extra>
static hipError_t launch_env_family(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                    hipStream_t s, int fold, const EnvArgs& a, const Extra&... x) {
  const dim3 grid = single_grid(L, tpb, n_envs);
  const KindVariant k = kind_variant(Fam::id, L, feat, gw, a.P.kind, fold);
  switch (kind_key(k.F, k.M, k.EK)) {
    BX_KIND_VARIANTS(BX_KIND_CASE, 0)
    default: break;
  }
  const SingleVariant v = single_variant(L, feat, gw);
  switch (single_key(v.L, v.F, v.M)) {
    BX_SINGLE_VARIANTS(BX_VARIANT_CASE, 0)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// the family of a rollout kernel template and its wide twin
#define BX_ENV_FAMILY(NAME, ID, KERNEL, WIDE_KERNEL)                 \
  struct NAME {                                                      \
    static constexpr EnvFamily id = ID;                              \
    template <int L, int F, int M, int EK>                           \
    static auto kernel(const EnvArgs&, bool wide) {                  \
      if constexpr (EK == EK_ANT)                                    \
        if (wide) return &WIDE_KERNEL<L, 1, F, M, EK>;               \
      return &KERNEL<L, 1, F, M, EK>;                                \
    }                                                                \
  };

// SINGLE-mode step kernels (fast-reciprocal translation unit)
hipError_t launch_system_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                     hipStream_t s, const StepArgs& a);
// the env launch units (SINGLE mode only), launch_env_family each; fold: the
// plan's fold_bits. Steps and open-loop K-step rollouts (pbd_single.hip)
hipError_t launch_env_step_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                  hipStream_t s, const EnvArgs& a, int fold);
// the K-step rollout with the policy action source (pbd_policy.hip)
hipError_t launch_env_policy_single(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                    hipStream_t s, const EnvArgs& a, const PolArgs& q, int fold);
hipError_t launch_normal_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                               uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                               uint64_t epoch_stride, hipStream_t s);
// the evolution agents' perturbation and weighted noise sum, the noise
// regenerated on chip (pbd_evolution.hip); part: chunks x n doubles
hipError_t launch_population_perturb(float* rows, const float* theta, const uint8_t* frozen,
                                     int64_t P, int64_t n, int64_t stride, double sigma,
                                     uint64_t seed, uint64_t offset, int antithetic, hipStream_t s);
hipError_t launch_population_delta(float* out, const float* w, const uint8_t* frozen, int64_t P,
                                   int64_t n, uint64_t seed, uint64_t offset, double* part,
                                   hipStream_t s);
// whole evaluations (env_step_body's EVL): the policy form (pbd_eval.hip) and
// the open-loop form (pbd_eval_open.hip)
hipError_t launch_env_eval_policy(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                  hipStream_t s, const EnvArgs& a, const PolArgs& q,
                                  const EvalArgs& v, int fold);
hipError_t launch_env_eval_open(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                hipStream_t s, const EnvArgs& a, const EvalArgs& v, int fold);
// one episode per perturbed policy (env_step_body's POP; pbd_pop.hip)
hipError_t launch_env_eval_population(int L, int feat, int gw, int tpb, int64_t n_envs, size_t lds,
                                      hipStream_t s, const EnvArgs& a, const PolArgs& q,
                                      const EvalArgs& v, const PopArgs& n, int fold);
// MULTI-mode step kernel (large pbd scenes, L = 128 or 256 threads per env;
// jh: the joint halves)
hipError_t launch_system_step_multi(int L, int jh, int64_t n_envs, size_t lds, hipStream_t s,
                                    const StepArgs& a);
// item-loop step kernels (generic translation unit)
hipError_t launch_system_step_generic(int L, int mode, int feat, int tpb, int64_t n_envs, size_t lds,
                                      hipStream_t s, const StepArgs& a);
hipError_t launch_env_step_generic(int L, int mode, int feat, int tpb, int64_t n_envs, size_t lds,
                                   hipStream_t s, const EnvArgs& a);
hipError_t launch_info_obs(int L, int64_t n_envs, size_t lds, hipStream_t s, const InfoArgs& a);
hipError_t launch_default_qp(int64_t n_envs, size_t lds, hipStream_t s, const ResetArgs& a);
hipError_t launch_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, float lo, float hi,
                          hipStream_t s);
hipError_t launch_uniform_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                                uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                                uint64_t epoch_stride, float lo, float hi, hipStream_t s);

hipError_t debug_stamps(unsigned long long* out, int reset);
hipError_t debug_partner(float* out64, int lanes, hipStream_t s);
hipError_t debug_mstamps(unsigned long long* out, int reset);  // MULTI mode (item-loop TU)
hipError_t launch_phase(int which, const uint32_t* blob, int N, int64_t B, int64_t plane,
                        const float* in, float* out, const float* aux, int64_t aux_plane,
                        hipStream_t s);
hipError_t launch_capsule_plane(const uint32_t* blob, int R, int64_t B, int64_t plane,
                                const float* in, float* out, int64_t out_plane, hipStream_t s);

}  // namespace bx
