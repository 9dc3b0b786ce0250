// bx_capi_env.cpp — the C ABI's env side (include/brax_amd.h): the env kinds'
// sizes and checks, the env launch path with its LDS planners (the policy, the
// evaluation and the population layouts), and the env entry points.
#include <algorithm>

#include "bx_capi_common.h"
#include "pbd_launch.h"

using namespace bx;

// the step reads actions through jp.take-style clipped indices (jumpy.py:151):
// any positive width is valid, 0 only when the system reads no action
int bx::check_act(const bx_system* S, const float* act, int64_t act_stride, int64_t act_width) {
  const bool reads = S->hdr.K > 0 || S->hdr.NF > 0;
  if (act_width < 0 || act_stride < 0) return fail("negative action width or stride");
  if (reads && (!act || act_width == 0)) return fail("null or empty action");
  return 0;
}

namespace {

// obs / metric widths of each env kind's layer (the kernel's obs_elem and
// reward code), from the system's shape: ant.py:257-282, humanoid.py:282-334,
// half_cheetah.py:200-214, humanoid_standup.py:249-289
int env_sizes(const bx_system* S, const bx_env_params* P, int* obs, int* met) {
  const BlobHdr& H = S->hdr;
  const int D = H.D, N = H.N;
  const bool xy = (P->obs_flags & BX_OBS_XY) != 0;
  if (P->obs_flags & ~BX_OBS_XY) return fail("unknown obs_flags bits");
  switch (P->kind) {
    case BX_ENV_ANT:
      *obs = 1 + 4 + D + 3 + 3 + D + (P->coef[7] != 0.f ? 6 * N : 0) + (xy ? 2 : 0);
      *met = 10;
      return 0;
    case BX_ENV_HUMANOID:
    case BX_ENV_HUMANOID_STANDUP: {
      if (xy && P->kind == BX_ENV_HUMANOID_STANDUP)
        return fail("HumanoidStandup has no current-position observation option");
      int qfrc = 0;
      for (int a = 0; a < H.K; a++) {
        int j = (int)S->words[H.o_act + a * ACT_STRIDE + A_JOINT];
        qfrc += (int)S->words[H.o_joint + j * JOINT_STRIDE + J_DOF];
      }
      *obs = 1 + 4 + D + 3 + 3 + D + 15 * (N - 1) + qfrc + (xy ? 2 : 0);
      *met = P->kind == BX_ENV_HUMANOID ? 9 : 2;
      return 0;
    }
    case BX_ENV_HOPPER:
    case BX_ENV_WALKER2D:
      // (x,) z, ang_y, joint angles, vel x, vel z, ang y, joint vels (hopper.py:231-246)
      *obs = (xy ? 2 : 1) + 1 + D + 3 + D;
      *met = 5;
      return 0;
    case BX_ENV_INVERTED_PENDULUM:  // cart x, joint angles, cart vel x, joint vels
      if (xy) return fail("this env has no current-position observation option");
      *obs = 2 + 2 * D;
      *met = 0;
      return 0;
    case BX_ENV_INVERTED_DOUBLE_PENDULUM:  // cart x, sin, cos, cart vel x, joint vels
      if (xy) return fail("this env has no current-position observation option");
      *obs = 2 + 3 * D;
      *met = 0;
      return 0;
    case BX_ENV_ACROBOT:  // joint angles, joint vels
      if (xy) return fail("this env has no current-position observation option");
      *obs = 2 * D;
      *met = 4;
      return 0;
    case BX_ENV_REACHER:
    case BX_ENV_REACHERANGLE:  // cos, sin, target xy, tip vel xy, tip - target
      if (xy) return fail("this env has no current-position observation option");
      if (P->kind == BX_ENV_REACHERANGLE && H.A > 2)
        return fail("ReacherAngle's action map holds at most 2 actions");
      *obs = 2 * D + 7;
      *met = 2;
      return 0;
    case BX_ENV_SWIMMER:  // (x, y,) ang z, joint angles, vel x, vel y, ang z, joint vels
      if (N != 4) return fail("Swimmer's drag program takes 3 segments and a floor");
      *obs = (xy ? 3 : 1) + D + 3 + D;
      *met = 8;
      return 0;
    case BX_ENV_PUSHER:  // joint angles, joint vels, tip, object, goal positions
      if (xy) return fail("this env has no current-position observation option");
      *obs = 2 * D + 9;
      *met = 3;
      return 0;
    case BX_ENV_UR5E:
    case BX_ENV_FETCH:  // fwd, up, |target|, target dir, local pos, local vel, contacts
      if (xy) return fail("this env has no current-position observation option");
      *obs = 10 + 7 * N;
      *met = P->kind == BX_ENV_UR5E ? 3 : 5;
      return 0;
    case BX_ENV_GRASP:  // object, target, local pos / vel, hand and object terms, contacts
      if (xy) return fail("this env has no current-position observation option");
      if (N < 16) return fail("Grasp's reward reads the contacts of bodies 3, 9, 12 and 15");
      *obs = 1 + 3 + 1 + 3 + 6 * N + 3 + 3 + 1 + 1 + 3 + 1 + N;
      *met = 5;
      return 0;
    case BX_ENV_HALFCHEETAH:
      *obs = 3 + D + 3 + D + (xy ? 1 : 0);
      *met = 4;
      return 0;
  }
  return fail("unknown env kind");
}

int check_env(const bx_system* S, const bx_env_params* P) {
  int obs = 0, met = 0;
  if (env_sizes(S, P, &obs, &met)) return 1;
  if (P->obs_size != obs)
    return fail("obs_size " + std::to_string(P->obs_size) + " != " + std::to_string(obs) +
                " for this env kind and system");
  if (P->n_metrics != met)
    return fail("n_metrics " + std::to_string(P->n_metrics) + " != " + std::to_string(met) +
                " for this env kind");
  return 0;
}

int check_draw(const bx_system* S, const bx_env_params* env, int64_t act_width) {
  if (act_width <= 0) return fail("on-device draws need act_width >= 1");
  // env programs that read the raw action row themselves (the pre-step
  // action maps, the humanoid qfrc observation)
  const int k = env->kind;
  if (k == BX_ENV_REACHERANGLE || k == BX_ENV_SWIMMER || k == BX_ENV_GRASP ||
      k == BX_ENV_HUMANOID || k == BX_ENV_HUMANOID_STANDUP)
    return fail("this env kind's program reads the action row itself: draw with bx_uniform_slabs");
  if (act_width > S->hdr.act_read)
    return fail("on-device draws stage the whole action row: act_width exceeds the row the system stages");
  return 0;
}

// the packed entry points' buffers: the state read, and the blocks written
// (one per step of the launch)
struct PackedIO {
  const float *qp_in, *done_in, *steps_in;
  const uint32_t* rng_in;
  float* out;
  uint32_t* rng_out;
};
// the action rows read: step t's at act + t * act_step (on chip: the width alone)
struct ActSource {
  const float* rows = nullptr;
  int64_t stride = 0, step = 0, width = 0;
};
struct DrawSpec {  // bx_env_rollout_random's on-device action draws
  uint64_t seed = 0, offset = 0, step = 0;
  float lo = 0.f, hi = 0.f;
};
// what an env launch has beyond the plain step, each entry point filling in
// what it uses: the steps of one launch, the action source (rows in memory, or
// made on chip by the draws or the policy, recorded at act_out), the
// evaluation's sums, the population's extras, and the whole workgroup's
// dynamic LDS where those kernels lay out words past the system's areas
struct EnvLaunch {
  int32_t n_steps = 1;
  ActSource act;
  bool on_chip = false;
  DrawSpec draw;
  float* act_out = nullptr;
  const PolArgs* pol = nullptr;
  const EvalArgs* evl = nullptr;
  const PopArgs* pop = nullptr;
  size_t lds = 0;
  // the packed block layout (env_step_packed): floats between two steps' outputs
  bool packed = false;
  int64_t out_step = 0, rng_step = 0;
  void make_on_chip(int64_t act_width, float* record) {
    act.width = act_width;
    on_chip = true;
    act_out = record;
  }
};

int env_step_impl(bx_system* S, const bx_env_params* env, int64_t n_envs, const bx_env_state* in,
                  const bx_env_state* out, void* stream, const EnvLaunch& x) {
  if (!S || !env || !in || !out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (check_env(S, env)) return 1;
  // an empty batch is a no-op (its buffers, the action included, may be null)
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if (x.on_chip ? check_draw(S, env, x.act.width) : check_act(S, x.act.rows, x.act.stride, x.act.width))
    return 1;
  if (!qp_ok(in->qp) || !qp_ok(out->qp)) return fail("null qp field");
  if (!in->done || !out->done || !out->reward || !out->obs) return fail("null env buffer");
  if (env->auto_reset && (!qp_ok(env->first_qp) || !env->first_obs))
    return fail("auto_reset needs first_qp and first_obs");
  if (env->kind == BX_ENV_GRASP && !env->act_map) return fail("Grasp needs its action map");
  if (env->kind == BX_ENV_GRASP && x.act.width > S->hdr.xact_words)
    return fail("action wider than the env program's action buffer");
  if ((env->kind == BX_ENV_UR5E || env->kind == BX_ENV_FETCH || env->kind == BX_ENV_GRASP) &&
      (!in->rng || !out->rng))
    return fail("the target envs need the per-env rng stream (in and out)");
  if (env->episode_length > 0 && (!out->steps || !out->truncation))
    return fail("episode wrapper needs steps and truncation buffers");
  EnvArgs a{};
  a.blob = S->blob;
  a.lane_img = S->blob + S->hdr.o_lane;
  a.hdr = S->hdr;
  a.n_envs = n_envs;
  a.P = *env;
  a.in = *in;
  a.out = *out;
  a.act = x.act.rows;
  a.act_stride = x.act.stride;
  a.act_width = x.act.width;
  a.n_steps = x.n_steps;
  a.act_step = x.act.step;
  a.out_step = x.out_step;
  a.rng_step = x.rng_step;
  a.packed = x.packed ? 1 : 0;
  a.draw = x.on_chip ? 1 : 0;  // (the policies draw nothing: their draw_* stay zero)
  a.draw_seed = x.draw.seed;
  a.draw_offset = x.draw.offset;
  a.draw_step = x.draw.step;
  a.draw_lo = x.draw.lo;
  a.draw_hi = x.draw.hi;
  a.act_out = x.act_out;
  const int fold = fold_bits(S->fold, S->jb, S->cb);
  hipStream_t s = as_stream(stream);
  if (x.pop)  // (policy_plan and eval_plan admit SINGLE-mode systems only)
    HIP_OK(launch_env_eval_population(S->L, S->feat, S->gw, S->tpb, n_envs, x.lds, s, a, *x.pol, *x.evl,
                                      *x.pop, fold));
  else if (x.evl && x.pol)
    HIP_OK(launch_env_eval_policy(S->L, S->feat, S->gw, S->tpb, n_envs, x.lds, s, a, *x.pol, *x.evl, fold));
  else if (x.evl)
    HIP_OK(launch_env_eval_open(S->L, S->feat, S->gw, S->tpb, n_envs, x.lds, s, a, *x.evl, fold));
  else if (x.pol)
    HIP_OK(launch_env_policy_single(S->L, S->feat, S->gw, S->tpb, n_envs, x.lds, s, a, *x.pol, fold));
  else if (S->mode == 1)
    HIP_OK(launch_env_step_single(S->L, S->feat, S->gw, S->tpb, n_envs, step_lds(S), s, a, fold));
  else if (S->mode == 3)  // MULTI-mode systems step envs with the item-loop kernel
    HIP_OK(launch_env_step_generic(S->L, 0, S->feat, S->tpb, n_envs, (size_t)S->hdr.env_words * 4, s, a));
  else
    HIP_OK(launch_env_step_generic(S->L, S->mode, S->feat, S->tpb, n_envs, step_lds(S), s, a));
  return 0;
}

int env_step_packed(bx_system* S, const bx_env_params* env, int64_t n_envs, const PackedIO& io,
                    void* stream, EnvLaunch x) {
  if (!S || !env) return fail("null argument");
  if (n_envs <= 0) {
    if (check_env(S, env)) return 1;
    return n_envs == 0 ? 0 : fail("negative n_envs");
  }
  if (!io.qp_in || !io.out) return fail("null argument");
  const int64_t N = S->hdr.N, B = n_envs;
  auto packed = [es = N * 16](float* b) {
    return bx_qp{{b, es, 16}, {b + 3, es, 16}, {b + 7, es, 16}, {b + 10, es, 16}};
  };
  bx_env_state in{};
  in.qp = packed(const_cast<float*>(io.qp_in));
  in.done = const_cast<float*>(io.done_in);
  in.steps = const_cast<float*>(io.steps_in);
  in.rng = const_cast<uint32_t*>(io.rng_in);
  bx_env_state o{};
  o.qp = packed(io.out);
  float* p = io.out + B * N * 16;
  o.obs = p;
  p += B * env->obs_size;
  o.reward = p;
  o.done = p + B;
  o.steps = p + 2 * B;
  o.truncation = p + 3 * B;
  o.metrics = env->n_metrics > 0 ? p + 4 * B : nullptr;
  o.rng = io.rng_out;
  // one step's output block: qp | obs | reward, done, steps, truncation | metrics
  x.packed = true;
  x.out_step = B * (N * 16 + env->obs_size + 4 + env->n_metrics);
  x.rng_step = B;
  return env_step_impl(S, env, n_envs, &in, &o, stream, x);
}

// bx_env_rollout_policy's descriptor checked against its limits and laid out
// in the workgroup's LDS past the envs' areas: Q's shape fields and *lds (the
// launch's dynamic LDS); the parameters are staged while the workgroup stays
// within a quarter of the compute unit's 160 KiB (the 4,096-env launch's four
// one-wave workgroups per compute unit stay co-resident)
// (identity: the population kernels' identity head, the last layer A wide;
// no_stage: never stage the shared copy, the population's rows differ per env)
int policy_plan(const bx_system* S, const bx_env_params* env, const bx_policy* p,
                int64_t act_width, PolArgs* Q, size_t* lds, bool identity, bool no_stage) {
  if (!p) return fail("null policy");
  if (S->mode != 1) return fail("the policy rollout needs a SINGLE-mode system");
  if (!p->params || ((uintptr_t)p->params & 15)) return fail("policy parameters: null or not 16-byte aligned");
  if (p->n_layers < 1 || p->n_layers > BX_POLICY_MAX_LAYERS)
    return fail("policy: 1.." + std::to_string(BX_POLICY_MAX_LAYERS) + " layers");
  if (!activation_ok(p->activation)) return fail("policy: unknown activation");
  if ((p->obs_mean == nullptr) != (p->obs_std == nullptr)) return fail("policy: obs_mean and obs_std go together");
  if (env->obs_size < 1 || env->obs_size > BX_POLICY_MAX_OBS)
    return fail("policy: obs_size beyond " + std::to_string(BX_POLICY_MAX_OBS));
  if (!(p->min_std >= 0.f)) return fail("policy: negative min_std");
  const int A = (int)act_width;
  int64_t np = 0;
  int wmax = std::max(env->obs_size, 2 * A);
  Q->width[0] = env->obs_size;
  for (int l = 0; l < p->n_layers; l++) {
    const int w = p->width[l];
    if (w < 1 || w > BX_POLICY_MAX_WIDTH)
      return fail("policy: layer widths 1.." + std::to_string(BX_POLICY_MAX_WIDTH));
    np += (int64_t)(Q->width[l] + 1) * w;
    Q->width[l + 1] = w;
    wmax = std::max(wmax, w);
  }
  const int last = p->width[p->n_layers - 1];
  if (identity) {
    if (last != A) return fail("population: the identity head's last layer is action_size wide");
  } else if (last != 2 * A && !(last == A && p->deterministic))
    return fail("policy: the last layer is 2 x action_size wide (action_size when deterministic)");
  Q->params = p->params;
  Q->mean = p->obs_mean;
  Q->std = p->obs_std;
  Q->n_layers = p->n_layers;
  Q->act_fn = p->activation;
  Q->det = p->deterministic ? 1 : 0;
  Q->min_std = p->min_std;
  Q->n_params = (int32_t)np;
  Q->obs_words = (env->obs_size + 3) & ~3;
  Q->buf_words = (wmax + 3) & ~3;
  const size_t base = (step_lds(S) + 15) & ~(size_t)15;
  const size_t envs = (size_t)(S->tpb / S->L) * (Q->obs_words + 2 * Q->buf_words) * 4;
  const size_t staged = (size_t)((np + 3) & ~(int64_t)3) * 4;
  Q->lds_off = (int32_t)(base / 4);
  Q->stage = (!no_stage && base + envs + staged <= 40 * 1024) ? 1 : 0;
  *lds = base + envs + (Q->stage ? staged : 0);
  if (*lds > 160 * 1024) return fail("policy: the workgroup's LDS exceeds 160 KiB");
  return 0;
}

// the policy entry points' shared prelude (bx_env_rollout_policy,
// bx_env_eval_policy, bx_env_eval_population): their first checks in their
// order and the plan into *q and *lds (policy_inputs adds the rest).
// population: bx_env_eval_population's checks, which come before the plans
int policy_prelude(const bx_system* S, const bx_env_params* env, int32_t n_steps,
                   const bx_policy* policy, PolArgs* q, size_t* lds, bool population = false,
                   const bx_population* pop = nullptr) {
  if (!S || !env) return fail("null argument");
  if (n_steps < 0) return fail("negative n_steps");
  if (!policy) return fail("null policy");
  if (population) {
    if (!pop) return fail("null population");
    if (pop->head != BX_HEAD_NORMAL_TANH && pop->head != BX_HEAD_IDENTITY)
      return fail("population: unknown head");
  }
  const int64_t A = policy->action_size;
  return check_env(S, env) || check_draw(S, env, A) ||
         policy_plan(S, env, policy, A, q, lds, population && pop->head == BX_HEAD_IDENTITY,
                     population && pop->param_stride != 0);
}
void policy_inputs(PolArgs* q, const float* obs_in, uint64_t seed, uint64_t offset, uint64_t step) {
  q->obs_in = obs_in;
  q->seed = seed;
  q->offset = offset;
  q->step = step;
}

// the evaluation kernels' on-chip words laid out past `base` bytes of the
// workgroup's LDS (the system's areas, or the policy's): per env the M + 3
// evaluation words and the step's M metrics
int eval_plan(const bx_system* S, const bx_env_params* env, size_t base, EvalArgs* V, size_t* lds) {
  if (S->mode != 1) return fail("the evaluation kernels need a SINGLE-mode system");
  base = (base + 15) & ~(size_t)15;
  V->lds_off = (int32_t)(base / 4);
  V->words = (2 * env->n_metrics + 3 + 3) & ~3;
  *lds = base + (size_t)(S->tpb / S->L) * V->words * 4;
  if (*lds > 160 * 1024) return fail("evaluation: the workgroup's LDS exceeds 160 KiB");
  return 0;
}

// the env half of an observation launch's arguments
InfoArgs info_env_args(const bx_system* S, const bx_env_params* env, int64_t n_envs, const bx_qp& qp) {
  InfoArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.q = qp;
  a.kind = env->kind;
  a.obs_size = env->obs_size;
  a.obs_flags = env->obs_flags;
  for (int k = 0; k < 8; k++) a.coef[k] = env->coef[k];
  return a;
}

}  // namespace

extern "C" {

int bx_env_step(bx_system* S, const bx_env_params* env, int64_t n_envs, const bx_env_state* in,
                const float* act, int64_t act_stride, int64_t act_width, const bx_env_state* out,
                void* stream) {
  EnvLaunch x;
  x.act = {act, act_stride, 0, act_width};
  return env_step_impl(S, env, n_envs, in, out, stream, x);
}

int bx_env_step_packed(bx_system* S, const bx_env_params* env, int64_t n_envs,
                       const float* qp_in, const float* done_in, const float* steps_in,
                       const uint32_t* rng_in, const float* act, int64_t act_stride,
                       int64_t act_width, float* out, uint32_t* rng_out, void* stream) {
  EnvLaunch x;
  x.act = {act, act_stride, 0, act_width};
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_rollout_packed(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                          const float* qp_in, const float* done_in, const float* steps_in,
                          const uint32_t* rng_in, const float* act, int64_t act_stride,
                          int64_t act_step_stride, int64_t act_width, float* out,
                          uint32_t* rng_out, void* stream) {
  if (n_steps < 0) return fail("negative n_steps");
  if (n_steps == 0) return S && env ? check_env(S, env) : fail("null argument");
  if (act_step_stride < 0) return fail("negative action step stride");
  EnvLaunch x;
  x.n_steps = n_steps;
  x.act = {act, act_stride, act_step_stride, act_width};
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_rollout_random(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                          const float* qp_in, const float* done_in, const float* steps_in,
                          const uint32_t* rng_in, uint64_t seed, uint64_t offset,
                          uint64_t step_stride, float lo, float hi, int64_t act_width,
                          float* act_out, float* out, uint32_t* rng_out, void* stream) {
  if (!S || !env) return fail("null argument");
  if (n_steps < 0) return fail("negative n_steps");
  if (check_env(S, env) || check_draw(S, env, act_width)) return 1;
  if (n_steps == 0) return 0;
  EnvLaunch x;
  x.n_steps = n_steps;
  x.make_on_chip(act_width, act_out);
  x.draw = {seed, offset, step_stride, lo, hi};
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_rollout_policy(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                          const float* qp_in, const float* obs_in, const float* done_in,
                          const float* steps_in, const uint32_t* rng_in, const bx_policy* policy,
                          uint64_t seed, uint64_t offset, uint64_t step_stride, float* act_out,
                          float* raw_out, float* logp_out, float* out, uint32_t* rng_out,
                          void* stream) {
  PolArgs q{};
  EnvLaunch x;
  if (policy_prelude(S, env, n_steps, policy, &q, &x.lds)) return 1;
  if (n_steps == 0) return 0;
  if (n_envs > 0 && !obs_in) return fail("null obs_in");
  policy_inputs(&q, obs_in, seed, offset, step_stride);
  q.raw_out = raw_out;
  q.logp_out = logp_out;
  x.n_steps = n_steps;
  x.make_on_chip(policy->action_size, act_out);
  x.pol = &q;
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_eval_policy(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                       const float* qp_in, const float* obs_in, const float* done_in,
                       const float* steps_in, const uint32_t* rng_in, const bx_policy* policy,
                       uint64_t seed, uint64_t offset, uint64_t step_stride, const float* eval_in,
                       float* out, float* eval_out, uint32_t* rng_out, void* stream) {
  PolArgs q{};
  EvalArgs v{};
  EnvLaunch x;
  size_t pol_lds = 0;
  if (policy_prelude(S, env, n_steps, policy, &q, &pol_lds) || eval_plan(S, env, pol_lds, &v, &x.lds))
    return 1;
  if (n_steps == 0) return 0;
  if (n_envs > 0 && !obs_in) return fail("null obs_in");
  if (n_envs > 0 && !eval_out) return fail("null eval_out");
  policy_inputs(&q, obs_in, seed, offset, step_stride);
  v.in = eval_in;
  v.out = eval_out;
  x.n_steps = n_steps;
  x.make_on_chip(policy->action_size, nullptr);
  x.pol = &q;
  x.evl = &v;
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_eval_population(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                           const float* qp_in, const float* obs_in, const float* done_in,
                           const float* steps_in, const uint32_t* rng_in, const bx_policy* policy,
                           uint64_t seed, uint64_t offset, uint64_t step_stride,
                           const float* eval_in, float* out, float* eval_out, uint32_t* rng_out,
                           bx_population* pop, void* stream) {
  PolArgs q{};
  EvalArgs v{};
  PopArgs n{};
  size_t pol_lds = 0, ev_lds = 0;
  if (policy_prelude(S, env, n_steps, policy, &q, &pol_lds, true, pop) ||
      eval_plan(S, env, pol_lds, &v, &ev_lds))
    return 1;
  const int64_t stride = pop->param_stride;
  if (stride != 0 && (stride < q.n_params || (stride & 3)))
    return fail("population: param_stride must be 0 or a multiple of 4 floats no smaller than n_params (" +
                std::to_string(q.n_params) + ")");
  // the population's words past the evaluation's: per env the moments, then
  // the env's row when every env's fits within policy_plan's 40 KiB
  const size_t epb = (size_t)(S->tpb / S->L);
  const size_t base = (ev_lds + 15) & ~(size_t)15;
  const int mom_words = pop->mom_out ? (2 * env->obs_size + 1 + 3) & ~3 : 0;
  const int row_words = (q.n_params + 3) & ~3;
  n.stage = (stride != 0 && !(pop->flags & BX_POP_NO_STAGE) &&
             base + epb * (size_t)(mom_words + row_words) * 4 <= 40 * 1024) ? 1 : 0;
  n.lds_off = (int32_t)(base / 4);
  n.row_off = mom_words;
  n.words = mom_words + (n.stage ? row_words : 0);
  const size_t lds = base + epb * (size_t)n.words * 4;
  if (lds > 160 * 1024) return fail("population: the workgroup's LDS exceeds 160 KiB");
  pop->staged = n.stage;
  pop->lds_bytes = (int32_t)lds;
  if (n_steps == 0) return 0;
  if (n_envs > 0 && !obs_in) return fail("null obs_in");
  if (n_envs > 0 && !eval_out) return fail("null eval_out");
  policy_inputs(&q, obs_in, seed, offset, step_stride);
  if (pop->head == BX_HEAD_IDENTITY) q.det = 1;  // (no noise is drawn; the head returns before reading it)
  v.in = eval_in;
  v.out = eval_out;
  n.mom_in = pop->mom_in;
  n.mom_out = pop->mom_out;
  n.param_stride = stride;
  n.head = pop->head;
  n.reward_shift = pop->reward_shift;
  EnvLaunch x;
  x.n_steps = n_steps;
  x.make_on_chip(policy->action_size, nullptr);
  x.pol = &q;
  x.evl = &v;
  x.pop = &n;
  x.lds = lds;  // (the whole workgroup's, the population's words included)
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_eval_packed(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                       const float* qp_in, const float* done_in, const float* steps_in,
                       const uint32_t* rng_in, const float* act, int64_t act_stride,
                       int64_t act_step_stride, int64_t act_width, const float* eval_in, float* out,
                       float* eval_out, uint32_t* rng_out, void* stream) {
  if (!S || !env) return fail("null argument");
  if (n_steps < 0) return fail("negative n_steps");
  EvalArgs v{};
  EnvLaunch x;
  if (check_env(S, env) || eval_plan(S, env, step_lds(S), &v, &x.lds)) return 1;
  if (n_steps == 0) return 0;
  if (act_step_stride < 0) return fail("negative action step stride");
  if (n_envs > 0 && !eval_out) return fail("null eval_out");
  v.in = eval_in;
  v.out = eval_out;
  x.n_steps = n_steps;
  x.act = {act, act_stride, act_step_stride, act_width};
  x.evl = &v;
  return env_step_packed(S, env, n_envs, {qp_in, done_in, steps_in, rng_in, out, rng_out}, stream, x);
}

int bx_env_sizes(bx_system* S, const bx_env_params* env, int32_t* obs_size, int32_t* n_metrics) {
  if (!S || !env || !obs_size || !n_metrics) return fail("null argument");
  int o = 0, m = 0;
  if (env_sizes(S, env, &o, &m)) return 1;
  *obs_size = o;
  *n_metrics = m;
  return 0;
}

int bx_env_observe(bx_system* S, const bx_env_params* env, int64_t n_envs, const bx_qp* qp,
                   const float* act, int64_t act_stride, int64_t act_width, float* obs,
                   void* stream) {
  if (!S || !env || !qp || !obs) return fail("null argument");
  DEVICE_SCOPE(S);
  if (check_env(S, env)) return 1;
  if (act_width < 0 || act_stride < 0) return fail("negative action width or stride");
  if ((env->kind == BX_ENV_HUMANOID || env->kind == BX_ENV_HUMANOID_STANDUP) && S->hdr.K > 0 &&
      (!act || act_width == 0))
    return fail("the humanoid observation reads the action (qfrc_actuator)");
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  InfoArgs a = info_env_args(S, env, n_envs, *qp);
  a.act = act;
  a.act_stride = act_stride;
  a.act_width = act_width;
  a.obs = obs;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, as_stream(stream), a));
  return 0;
}

int bx_env_reset(bx_system* S, const bx_env_params* env, int64_t n_envs, uint64_t seed,
                 int64_t env_offset, const uint64_t* env_seeds, float noise_scale,
                 const bx_env_state* out, void* stream) {
  if (!S || !env || !out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (S->hdr.o_base == 0) return fail("system was created without a reset descriptor");
  if (check_env(S, env)) return 1;
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if (env_offset < 0) return fail("negative env_offset");
  if (!(noise_scale >= 0.f)) return fail("noise_scale must be >= 0");
  if (!qp_ok(out->qp) || !out->obs || !out->reward || !out->done) return fail("null env buffer");
  if (env->n_metrics > 0 && !out->metrics) return fail("null metrics buffer");
  ResetArgs r{};
  r.blob = S->blob;
  r.n_envs = n_envs;
  r.out = out->qp;
  r.gen = 1;
  r.seed = seed;
  r.env_offset = env_offset;
  r.seeds = env_seeds;
  r.scale = noise_scale;
  r.kind = env->kind;
  for (int k = 0; k < 8; k++) r.coef[k] = env->coef[k];
  r.rng_out = out->rng;
  // the bodies a reset program places must exist (coef holds their indices)
  auto body_ok = [&](float x) { return x >= 0.f && x < (float)S->hdr.N && x == (float)(int)x; };
  if ((env->kind == BX_ENV_REACHER || env->kind == BX_ENV_REACHERANGLE) && !body_ok(env->coef[0]))
    return fail("reacher reset: coef[0] must be the target body");
  if (env->kind == BX_ENV_PUSHER &&
      !(body_ok(env->coef[1]) && body_ok(env->coef[2]) && body_ok(env->coef[3])))
    return fail("pusher reset: coef[1..3] must be the object, goal and table bodies");
  if (env->kind == BX_ENV_PUSHER && S->hdr.num_joint_dof < 4)
    return fail("pusher reset: the last 4 dofs get no velocity noise; the system has fewer");
  if ((env->kind == BX_ENV_UR5E || env->kind == BX_ENV_FETCH) && !body_ok(env->coef[1]))
    return fail("target env reset: coef[1] must be the target body");
  if ((env->kind == BX_ENV_UR5E || env->kind == BX_ENV_FETCH || env->kind == BX_ENV_GRASP) &&
      !out->rng)
    return fail("the target envs' reset writes their per-env rng stream: out->rng is null");
  hipStream_t s = as_stream(stream);
  HIP_OK(launch_default_qp(n_envs, S->lds_reset, s, r));
  // _get_obs(qp, info, jp.zeros(action_size)): a null action reads as zeros
  InfoArgs a = info_env_args(S, env, n_envs, out->qp);
  a.obs = out->obs;
  a.zero_reward = out->reward;
  a.zero_done = out->done;
  a.zero_steps = out->steps;
  a.zero_trunc = out->truncation;
  a.zero_metrics = out->metrics;
  a.n_metrics = env->n_metrics;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, s, a));
  return 0;
}

}  // extern "C"
