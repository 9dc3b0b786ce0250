// bx_capi.cpp — the C ABI (include/brax_amd.h): descriptor -> device blob,
// argument validation, and stream-ordered kernel launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/brax_amd.h"
#include "bx_blob.h"
#include "mlp_launch.h"
#include "optim_launch.h"
#include "ppo_head_launch.h"
#include "pbd_features.h"
#include "pbd_launch.h"
#include "pbd_layout.h"
#include "replay_launch.h"
#include "train_launch.h"

using namespace bx;

namespace {

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return 1;
}

#define HIP_OK(expr)                                                       \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

}  // namespace

// a system: its plan and blob words (bx_blob.h) and their copy on its device
struct bx_system : bx::Plan {
  int device = 0;
  uint32_t* blob = nullptr;
  float* movf = nullptr;  // MULTI: the penetrating contacts past MCBUF, per env (grown on demand)
  int64_t movf_envs = 0;
  // the overflow buffers that growth superseded: an earlier launch or a graph
  // captured at a smaller batch may still hold them, so they live until destroy
  std::vector<float*> movf_old;

  // frees every overflow buffer, the current one and the superseded ones
  hipError_t free_movf() {
    hipError_t e = hipSuccess;
    for (float* p : movf_old) {
      hipError_t f = hipFree(p);
      if (e == hipSuccess) e = f;
    }
    movf_old.clear();
    if (movf) {
      hipError_t f = hipFree(movf);
      if (e == hipSuccess) e = f;
    }
    movf = nullptr;
    movf_envs = 0;
    return e;
  }
};

namespace {

// the host half of a system (bx_blob.cpp), with this process's A/B knobs
int build_blob(const bx_desc* d, const bx_reset_desc* r, bx_system* S) {
  std::string err;
  if (build_plan(d, r, plan_knobs_from_env(), S, &err)) return fail(err);
  return 0;
}

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Every entry point that touches device memory runs with the system's device
// current and restores the caller's afterwards (HIP launches go to the current
// device; a process may hold systems on several GPUs).
struct DeviceScope {
  int prev = -1, want;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int d) : want(d) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != want) err = hipSetDevice(want);
  }
  ~DeviceScope() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
};
#define DEVICE_SCOPE(S)                                                             \
  DeviceScope _dev((S)->device);                                                    \
  if (_dev.err != hipSuccess) return fail(std::string("device ") + std::to_string((S)->device) + \
                                          ": " + hipGetErrorString(_dev.err))

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

size_t step_lds(const bx_system* S) {
  if (S->mode == 3) return (size_t)S->hdr.env_words_m * 4;
  size_t b = (size_t)(S->tpb / S->L) * S->hdr.env_words * 4;
  if (S->mode == 2) b += (size_t)S->hdr.const_words * 4;
  return b;
}

bool field_ok(const bx_field& f) { return f.ptr != nullptr; }
bool qp_ok(const bx_qp& q) {
  return field_ok(q.pos) && field_ok(q.rot) && field_ok(q.vel) && field_ok(q.ang);
}

}  // namespace

extern "C" {

int bx_abi_version(void) { return BX_ABI_VERSION; }

const char* bx_last_error(void) { return g_err.c_str(); }

int bx_device_count(int* count) {
  HIP_OK(hipGetDeviceCount(count));
  return 0;
}

int bx_system_create(const bx_desc* desc, const bx_reset_desc* reset, int device, bx_system** out) {
  if (!desc || !out) return fail("null argument");
  bx_system* S = new bx_system();
  S->device = device;
  if (int rc = build_blob(desc, reset, S)) {
    delete S;
    return rc;
  }
  DeviceScope dev(device);
  hipError_t e = dev.err;
  if (e == hipSuccess) e = hipMalloc(&S->blob, S->words.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(S->blob, S->words.data(), S->words.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    std::string m = std::string("device setup: ") + hipGetErrorString(e);
    (void)S->free_movf();
    if (S->blob) (void)hipFree(S->blob);
    delete S;
    return fail(m);
  }
  *out = S;
  return 0;
}

int bx_system_destroy(bx_system* S) {
  if (!S) return 0;
  if (S->blob || S->movf || !S->movf_old.empty()) {
    DEVICE_SCOPE(S);
    HIP_OK(S->free_movf());
    if (S->blob) HIP_OK(hipFree(S->blob));
  }
  delete S;
  return 0;
}

// the host half of bx_system_create: the kernel plan of a descriptor (no device)
int bx_system_plan(const bx_desc* desc, const bx_reset_desc* reset, int32_t* mode,
                   int32_t* lanes, int32_t* lds_bytes) {
  if (!desc || !mode || !lanes || !lds_bytes) return fail("null argument");
  bx_system S;
  if (int rc = build_blob(desc, reset, &S)) return rc;
  *mode = S.mode;
  *lanes = S.L;
  *lds_bytes = (int32_t)step_lds(&S);
  return 0;
}

// and the blob itself with the whole plan (no device): what the fingerprints
// of tests/test_blob_fingerprint.py pin
int bx_system_blob(const bx_desc* desc, const bx_reset_desc* reset, uint32_t* words,
                   int64_t capacity, int64_t* n_words, int32_t plan[8]) {
  if (!desc || !n_words || !plan) return fail("null argument");
  bx_system S;
  if (int rc = build_blob(desc, reset, &S)) return rc;
  const int64_t n = (int64_t)S.words.size();
  *n_words = n;
  const int32_t p[8] = {S.mode, S.L, (int32_t)step_lds(&S), S.feat, S.gw, S.fold, S.jb, S.cb};
  std::memcpy(plan, p, sizeof(p));
  if (words) {
    if (capacity < n)
      return fail("blob capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " words");
    std::memcpy(words, S.words.data(), (size_t)n * 4);
  }
  return 0;
}

int bx_system_lanes(bx_system* S) { return S ? S->L : 0; }
int bx_system_env_lanes(bx_system* S) {
  return S ? S->L : 0;
}
int bx_system_lds_bytes(bx_system* S) { return S ? (int)step_lds(S) : 0; }

int bx_system_set_single(bx_system* S, int on) {
  if (!S) return fail("null system");
  if (on && (!S->single_ok || S->L != S->min_L)) return fail("system does not fit the single-item-per-lane kernel");
  S->mode = on ? 1 : 0;
  return 0;
}

int bx_system_set_variant(bx_system* S, int lanes, int mode) {
  if (!S) return fail("null system");
  if (lanes != 16 && lanes != 32 && lanes != 64 && lanes != 128 && lanes != 256)
    return fail("lanes must be 16, 32, 64, 128 or 256");
  if (mode < 0 || mode > 3) return fail("mode must be 0 (global), 1 (single), 2 (lds) or 3 (multi)");
  if (mode == 1 && (!S->single_ok || lanes < S->min_L || lanes > 64 || lanes > S->hdr.L))
    return fail("system does not fit the single-item-per-lane kernel at that width");
  if (mode == 3 && (!S->multi_ok || (lanes != 256 && !(lanes == 128 && S->hdr.multi_L == 128))))
    return fail("system does not fit the MULTI-mode kernel at that width (128 or 256 lanes)");
  int old_L = S->L, old_m = S->mode, old_t = S->tpb;
  S->L = lanes;
  S->mode = mode;
  if (lanes > 64) S->tpb = lanes;
  else if (S->tpb > 64 || S->tpb % lanes) S->tpb = 64;
  if (step_lds(S) > 160 * 1024) {
    S->L = old_L;
    S->mode = old_m;
    S->tpb = old_t;
    return fail("variant exceeds the LDS budget");
  }
  return 0;
}

int bx_system_set_block(bx_system* S, int threads) {
  if (!S) return fail("null system");
  if (threads < S->L || threads > (S->L > 64 ? S->L : 64) || threads % S->L)
    return fail("threads must be a multiple of the lanes per env, at most 64 (or the lanes "
                "per env past 64)");
  int old = S->tpb;
  S->tpb = threads;
  if (step_lds(S) > 160 * 1024) {
    S->tpb = old;
    return fail("block exceeds the LDS budget");
  }
  return 0;
}

// the step reads actions through jp.take-style clipped indices (jumpy.py:151):
// any positive width is valid, 0 only when the system reads no action
static int check_act(const bx_system* S, const float* act, int64_t act_stride, int64_t act_width) {
  const bool reads = S->hdr.K > 0 || S->hdr.NF > 0;
  if (act_width < 0 || act_stride < 0) return fail("negative action width or stride");
  if (reads && (!act || act_width == 0)) return fail("null or empty action");
  return 0;
}

int bx_system_step(bx_system* S, int64_t n_envs, const bx_qp* qin, const float* act,
                   int64_t act_stride, int64_t act_width, const bx_qp* qout, const bx_info* info,
                   void* stream) {
  if (!S || !qin || !qout) return fail("null argument");
  DEVICE_SCOPE(S);
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if (!qp_ok(*qin) || !qp_ok(*qout)) return fail("null qp field");
  if (check_act(S, act, act_stride, act_width)) return 1;
  StepArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.qin = *qin;
  a.qout = *qout;
  a.act = act;
  a.act_stride = act_stride;
  a.act_width = act_width;
  if (info) a.info = *info;
  if (S->mode == 3 && S->hdr.R > MCBUF && S->movf_envs < n_envs) {
    // the overflow contacts (a pass with more than MCBUF penetrating rows):
    // grown to this batch once; a capture cannot allocate. The buffer is
    // scratch, written before it is read within a step, so growth copies
    // nothing and waits for nothing: the new allocation serves this launch and
    // the later ones, and the superseded one is kept until bx_system_destroy,
    // because launches in flight and graphs captured at the smaller batch hold
    // its address. Batches that double keep at most about twice the largest
    // buffer; nothing ever shrinks.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(as_stream(stream), &cs));
    if (cs != hipStreamCaptureStatusNone)
      return fail("MULTI overflow buffer: step the batch once before capturing it");
    float* grown = nullptr;
    HIP_OK(hipMalloc(&grown, (size_t)n_envs * (S->hdr.R - MCBUF) * MOVF_W * 4));
    if (S->movf) S->movf_old.push_back(S->movf);
    S->movf = grown;
    S->movf_envs = n_envs;
  }
  a.movf = S->movf;
  if (S->mode == 1)
    HIP_OK(launch_system_step_single(S->L, S->feat, S->gw, S->tpb, n_envs, step_lds(S), as_stream(stream), a));
  else if (S->mode == 3)
    HIP_OK(launch_system_step_multi(S->L, S->hdr.o_mjh ? 1 : 0, n_envs, step_lds(S), as_stream(stream), a));
  else
    HIP_OK(launch_system_step_generic(S->L, S->mode, S->feat, S->tpb, n_envs, step_lds(S), as_stream(stream), a));
  return 0;
}

// bx_env_step over n_steps consecutive steps in one launch (bx_env_rollout_packed):
// step t reads act + t * act_step and writes the out pointers + t * out_step
struct DrawSpec {  // bx_env_rollout_random's on-device action draws
  uint64_t seed, offset, step;
  float lo, hi;
  float* act_out;
};
static int check_draw(const bx_system* S, const bx_env_params* env, int64_t act_width) {
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

// what an env launch has beyond the plain step, each entry point filling in
// what it uses: on-device action draws, the policy action source, the
// evaluation's sums, the population's extras, and the whole workgroup's
// dynamic LDS where those kernels lay out words past the system's areas
struct EnvLaunch {
  const DrawSpec* draw = nullptr;
  const PolArgs* pol = nullptr;
  const EvalArgs* evl = nullptr;
  const PopArgs* pop = nullptr;
  size_t lds = 0;
};
static int env_step_impl(bx_system* S, const bx_env_params* env, int64_t n_envs,
                         const bx_env_state* in, const float* act, int64_t act_stride,
                         int64_t act_width, const bx_env_state* out, void* stream,
                         int32_t n_steps, int64_t act_step, int64_t out_step, int64_t rng_step,
                         bool packed = false, const EnvLaunch& x = {}) {
  const DrawSpec* draw = x.draw;
  if (!S || !env || !in || !out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (check_env(S, env)) return 1;
  // an empty batch is a no-op (its buffers, the action included, may be null)
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if ((draw || x.pol) ? check_draw(S, env, act_width) : check_act(S, act, act_stride, act_width)) return 1;
  if (!qp_ok(in->qp) || !qp_ok(out->qp)) return fail("null qp field");
  if (!in->done || !out->done || !out->reward || !out->obs) return fail("null env buffer");
  if (env->auto_reset && (!qp_ok(env->first_qp) || !env->first_obs))
    return fail("auto_reset needs first_qp and first_obs");
  if (env->kind == BX_ENV_GRASP && !env->act_map) return fail("Grasp needs its action map");
  if (env->kind == BX_ENV_GRASP && act_width + 0 > S->hdr.xact_words)
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
  a.act = act;
  a.act_stride = act_stride;
  a.act_width = act_width;
  a.n_steps = n_steps;
  a.act_step = act_step;
  a.out_step = out_step;
  a.rng_step = rng_step;
  a.packed = packed ? 1 : 0;
  if (draw) {
    a.draw = 1;
    a.draw_seed = draw->seed;
    a.draw_offset = draw->offset;
    a.draw_step = draw->step;
    a.draw_lo = draw->lo;
    a.draw_hi = draw->hi;
    a.act_out = draw->act_out;
  }
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
    HIP_OK(launch_env_step_generic(S->L, 0, S->feat, S->tpb, n_envs,
                                   (size_t)S->hdr.env_words * 4, as_stream(stream), a));
  else
    HIP_OK(launch_env_step_generic(S->L, S->mode, S->feat, S->tpb, n_envs, step_lds(S), as_stream(stream), a));
  return 0;
}

int bx_env_step(bx_system* S, const bx_env_params* env, int64_t n_envs, const bx_env_state* in,
                const float* act, int64_t act_stride, int64_t act_width, const bx_env_state* out,
                void* stream) {
  return env_step_impl(S, env, n_envs, in, act, act_stride, act_width, out, stream, 1, 0, 0, 0);
}

static int env_step_packed(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                           const float* qp_in, const float* done_in, const float* steps_in,
                           const uint32_t* rng_in, const float* act, int64_t act_stride,
                           int64_t act_step, int64_t act_width, float* out, uint32_t* rng_out,
                           void* stream, const EnvLaunch& x = {}) {
  if (!S || !env) return fail("null argument");
  if (n_envs <= 0) {
    if (check_env(S, env)) return 1;
    return n_envs == 0 ? 0 : fail("negative n_envs");
  }
  if (!qp_in || !out) return fail("null argument");
  const int64_t N = S->hdr.N, B = n_envs;
  auto packed = [&](float* base) {
    bx_qp q;
    const int64_t es = N * 16;
    q.pos = bx_field{base, es, 16};
    q.rot = bx_field{base + 3, es, 16};
    q.vel = bx_field{base + 7, es, 16};
    q.ang = bx_field{base + 10, es, 16};
    return q;
  };
  bx_env_state in{};
  in.qp = packed(const_cast<float*>(qp_in));
  in.done = const_cast<float*>(done_in);
  in.steps = const_cast<float*>(steps_in);
  in.rng = const_cast<uint32_t*>(rng_in);
  bx_env_state o{};
  o.qp = packed(out);
  float* p = out + B * N * 16;
  o.obs = p;
  p += B * env->obs_size;
  o.reward = p;
  o.done = p + B;
  o.steps = p + 2 * B;
  o.truncation = p + 3 * B;
  o.metrics = env->n_metrics > 0 ? p + 4 * B : nullptr;
  o.rng = rng_out;
  // one step's output block: qp | obs | reward, done, steps, truncation | metrics
  const int64_t block = B * (N * 16 + env->obs_size + 4 + env->n_metrics);
  return env_step_impl(S, env, n_envs, &in, act, act_stride, act_width, &o, stream, n_steps,
                       act_step, block, B, true, x);
}

int bx_env_step_packed(bx_system* S, const bx_env_params* env, int64_t n_envs,
                       const float* qp_in, const float* done_in, const float* steps_in,
                       const uint32_t* rng_in, const float* act, int64_t act_stride,
                       int64_t act_width, float* out, uint32_t* rng_out, void* stream) {
  return env_step_packed(S, env, n_envs, 1, qp_in, done_in, steps_in, rng_in, act, act_stride, 0,
                         act_width, out, rng_out, stream);
}

int bx_env_rollout_packed(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                          const float* qp_in, const float* done_in, const float* steps_in,
                          const uint32_t* rng_in, const float* act, int64_t act_stride,
                          int64_t act_step_stride, int64_t act_width, float* out,
                          uint32_t* rng_out, void* stream) {
  if (n_steps < 0) return fail("negative n_steps");
  if (n_steps == 0) return S && env ? check_env(S, env) : fail("null argument");
  if (act_step_stride < 0) return fail("negative action step stride");
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, act,
                         act_stride, act_step_stride, act_width, out, rng_out, stream);
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
  const DrawSpec d{seed, offset, step_stride, lo, hi, act_out};
  EnvLaunch x;
  x.draw = &d;
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, nullptr, 0, 0,
                         act_width, out, rng_out, stream, x);
}

// bx_env_rollout_policy's descriptor checked against its limits and laid out
// in the workgroup's LDS past the envs' areas: Q's shape fields and *lds (the
// launch's dynamic LDS); the parameters are staged while the workgroup stays
// within a quarter of the compute unit's 160 KiB (the 4,096-env launch's four
// one-wave workgroups per compute unit stay co-resident)
// (identity: the population kernels' identity head, the last layer A wide;
// no_stage: never stage the shared copy, the population's rows differ per env)
static int policy_plan(const bx_system* S, const bx_env_params* env, const bx_policy* p,
                       int64_t act_width, PolArgs* Q, size_t* lds, bool identity = false,
                       bool no_stage = false) {
  if (!p) return fail("null policy");
  if (S->mode != 1) return fail("the policy rollout needs a SINGLE-mode system");
  if (!p->params || ((uintptr_t)p->params & 15)) return fail("policy parameters: null or not 16-byte aligned");
  if (p->n_layers < 1 || p->n_layers > BX_POLICY_MAX_LAYERS)
    return fail("policy: 1.." + std::to_string(BX_POLICY_MAX_LAYERS) + " layers");
  if (p->activation != BX_POLICY_SWISH && p->activation != BX_POLICY_RELU && p->activation != BX_POLICY_TANH)
    return fail("policy: unknown activation");
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
// order, the plan into *q and *lds, and the launch's observation and noise
// arguments. population: bx_env_eval_population's descriptor checks, which
// come before the plans
static int policy_prelude(const bx_system* S, const bx_env_params* env, int32_t n_steps,
                          const bx_policy* policy, const float* obs_in, uint64_t seed,
                          uint64_t offset, uint64_t step_stride, PolArgs* q, size_t* lds,
                          bool population = false, const bx_population* pop = nullptr) {
  if (!S || !env) return fail("null argument");
  if (n_steps < 0) return fail("negative n_steps");
  if (!policy) return fail("null policy");
  if (population) {
    if (!pop) return fail("null population");
    if (pop->head != BX_HEAD_NORMAL_TANH && pop->head != BX_HEAD_IDENTITY)
      return fail("population: unknown head");
  }
  const int64_t A = policy->action_size;
  if (check_env(S, env) || check_draw(S, env, A) ||
      policy_plan(S, env, policy, A, q, lds, population && pop->head == BX_HEAD_IDENTITY,
                  population && pop->param_stride != 0))
    return 1;
  q->obs_in = obs_in;
  q->seed = seed;
  q->offset = offset;
  q->step = step_stride;
  return 0;
}

int bx_env_rollout_policy(bx_system* S, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                          const float* qp_in, const float* obs_in, const float* done_in,
                          const float* steps_in, const uint32_t* rng_in, const bx_policy* policy,
                          uint64_t seed, uint64_t offset, uint64_t step_stride, float* act_out,
                          float* raw_out, float* logp_out, float* out, uint32_t* rng_out,
                          void* stream) {
  PolArgs q{};
  EnvLaunch x;
  if (policy_prelude(S, env, n_steps, policy, obs_in, seed, offset, step_stride, &q, &x.lds)) return 1;
  if (n_steps == 0) return 0;
  if (n_envs > 0 && !obs_in) return fail("null obs_in");
  q.raw_out = raw_out;
  q.logp_out = logp_out;
  const DrawSpec d{0, 0, 0, 0.f, 0.f, act_out};
  x.draw = &d;
  x.pol = &q;
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, nullptr, 0, 0,
                         policy->action_size, out, rng_out, stream, x);
}

// the evaluation kernels' on-chip words laid out past `base` bytes of the
// workgroup's LDS (the system's areas, or the policy's): per env the M + 3
// evaluation words and the step's M metrics
static int eval_plan(const bx_system* S, const bx_env_params* env, size_t base, EvalArgs* V,
                     size_t* lds) {
  if (S->mode != 1) return fail("the evaluation kernels need a SINGLE-mode system");
  base = (base + 15) & ~(size_t)15;
  V->lds_off = (int32_t)(base / 4);
  V->words = (2 * env->n_metrics + 3 + 3) & ~3;
  *lds = base + (size_t)(S->tpb / S->L) * V->words * 4;
  if (*lds > 160 * 1024) return fail("evaluation: the workgroup's LDS exceeds 160 KiB");
  return 0;
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
  if (policy_prelude(S, env, n_steps, policy, obs_in, seed, offset, step_stride, &q, &pol_lds) ||
      eval_plan(S, env, pol_lds, &v, &x.lds))
    return 1;
  if (n_steps == 0) return 0;
  if (n_envs > 0 && !obs_in) return fail("null obs_in");
  if (n_envs > 0 && !eval_out) return fail("null eval_out");
  v.in = eval_in;
  v.out = eval_out;
  const DrawSpec d{0, 0, 0, 0.f, 0.f, nullptr};
  x.draw = &d;
  x.pol = &q;
  x.evl = &v;
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, nullptr, 0, 0,
                         policy->action_size, out, rng_out, stream, x);
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
  if (policy_prelude(S, env, n_steps, policy, obs_in, seed, offset, step_stride, &q, &pol_lds, true, pop) ||
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
  if (pop->head == BX_HEAD_IDENTITY) q.det = 1;  // (no noise is drawn; the head returns before reading it)
  v.in = eval_in;
  v.out = eval_out;
  n.mom_in = pop->mom_in;
  n.mom_out = pop->mom_out;
  n.param_stride = stride;
  n.head = pop->head;
  n.reward_shift = pop->reward_shift;
  const DrawSpec d{0, 0, 0, 0.f, 0.f, nullptr};
  EnvLaunch x;
  x.draw = &d;
  x.pol = &q;
  x.evl = &v;
  x.pop = &n;
  x.lds = lds;  // (the whole workgroup's, the population's words included)
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, nullptr, 0, 0,
                         policy->action_size, out, rng_out, stream, x);
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
  x.evl = &v;
  return env_step_packed(S, env, n_envs, n_steps, qp_in, done_in, steps_in, rng_in, act,
                         act_stride, act_step_stride, act_width, out, rng_out, stream, x);
}

int bx_system_info(bx_system* S, int64_t n_envs, const bx_qp* qp, const bx_info* info, void* stream) {
  if (!S || !qp || !info) return fail("null argument");
  DEVICE_SCOPE(S);
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  InfoArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.q = *qp;
  a.info = *info;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, as_stream(stream), a));
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
  InfoArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.q = *qp;
  a.kind = env->kind;
  a.obs_size = env->obs_size;
  a.obs_flags = env->obs_flags;
  for (int k = 0; k < 8; k++) a.coef[k] = env->coef[k];
  a.act = act;
  a.act_stride = act_stride;
  a.act_width = act_width;
  a.obs = obs;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, as_stream(stream), a));
  return 0;
}

int bx_system_joint_angles(bx_system* S, int64_t n_envs, const bx_qp* qp, float* angle,
                           float* vel, void* stream) {
  if (!S || !qp) return fail("null argument");
  DEVICE_SCOPE(S);
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if (S->hdr.D == 0) return 0;
  if (!angle || !vel) return fail("null angle or velocity buffer");
  InfoArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.q = *qp;
  a.angle = angle;
  a.angvel = vel;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, as_stream(stream), a));
  return 0;
}

int bx_env_sizes(bx_system* S, const bx_env_params* env, int32_t* obs_size, int32_t* n_metrics) {
  if (!S || !env || !obs_size || !n_metrics) return fail("null argument");
  int o = 0, m = 0;
  if (env_sizes(S, env, &o, &m)) return 1;
  *obs_size = o;
  *n_metrics = m;
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
  HIP_OK(launch_default_qp(n_envs, S->lds_reset, as_stream(stream), r));
  InfoArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.q = out->qp;
  a.kind = env->kind;
  a.obs_size = env->obs_size;
  a.obs_flags = env->obs_flags;
  for (int k = 0; k < 8; k++) a.coef[k] = env->coef[k];
  a.obs = out->obs;
  // _get_obs(qp, info, jp.zeros(action_size)): a null action reads as zeros
  a.act = nullptr;
  a.act_width = 0;
  a.zero_reward = out->reward;
  a.zero_done = out->done;
  a.zero_steps = out->steps;
  a.zero_trunc = out->truncation;
  a.zero_metrics = out->metrics;
  a.n_metrics = env->n_metrics;
  HIP_OK(launch_info_obs(S->L, n_envs, S->lds_env, as_stream(stream), a));
  return 0;
}

int bx_system_default_qp(bx_system* S, int64_t n_envs, const float* joint_angle,
                         const float* joint_velocity, const bx_qp* qp_out, void* stream) {
  if (!S || !qp_out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (S->hdr.o_base == 0) return fail("system was created without a reset descriptor");
  if (n_envs <= 0) return n_envs == 0 ? 0 : fail("negative n_envs");
  if (S->hdr.num_joint_dof > 0 && (!joint_angle || !joint_velocity)) return fail("null joint arrays");
  ResetArgs a{};
  a.blob = S->blob;
  a.n_envs = n_envs;
  a.angle = joint_angle;
  a.vel = joint_velocity;
  a.out = *qp_out;
  HIP_OK(launch_default_qp(n_envs, S->lds_reset, as_stream(stream), a));
  return 0;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int bx_phase(bx_system* S, int which, int64_t n_envs, int64_t plane, const float* in, float* out,
             const float* aux, int64_t aux_plane, void* stream) {
  if (!S || !in || !out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (which < 0 || which > 2) return fail("unknown phase");
  if (n_envs <= 0 || n_envs % 4) return fail("n_envs must be a positive multiple of 4");
  const int64_t N = S->hdr.N;
  if (N * n_envs >= (int64_t)1 << 32) return fail("too many bodies for one phase launch");
  if (plane < N * n_envs || plane % 4) return fail("plane stride must be >= N*n_envs and a multiple of 4");
  if (which >= 1 && (!aux || aux_plane % 4 || aux_plane < N * n_envs)) return fail("bad aux planes");
  if (!aligned16(in) || !aligned16(out) || (aux && !aligned16(aux))) return fail("SoA bases must be 16-byte aligned");
  HIP_OK(launch_phase(which, S->blob, (int)N, n_envs, plane, in, out, aux, aux_plane, as_stream(stream)));
  return 0;
}

int bx_phase_capsule_plane(bx_system* S, int64_t n_envs, int64_t plane, const float* in, float* out,
                           int64_t out_plane, void* stream) {
  if (!S || !in || !out) return fail("null argument");
  DEVICE_SCOPE(S);
  if (n_envs <= 0 || n_envs % 4) return fail("n_envs must be a positive multiple of 4");
  const int64_t N = S->hdr.N, R = S->hdr.R;
  if (plane < N * n_envs || plane % 4) return fail("plane stride must be >= N*n_envs and a multiple of 4");
  if (out_plane < R * n_envs || out_plane % 4) return fail("out plane stride must be >= R*n_envs");
  if (!aligned16(in) || !aligned16(out)) return fail("SoA bases must be 16-byte aligned");
  if (R == 0) return 0;
  HIP_OK(launch_capsule_plane(S->blob, (int)R, n_envs, plane, in, out, out_plane, as_stream(stream)));
  return 0;
}

int bx_debug_partner(float* out64, int lanes, void* stream) {
  if (!out64) return fail("null argument");
  if (lanes != 16) return fail("lanes must be 16 (the revolute joint halves' exchange)");
  HIP_OK(debug_partner(out64, lanes, as_stream(stream)));
  return 0;
}

int bx_debug_stamps(unsigned long long* out, int reset) {
  // bit 1 of reset selects the MULTI-mode stamps (BX_MSTAMPS build)
  // bit 2: the per-workgroup sums (4096 x 16 entries) instead of the totals
  if (reset & 2) HIP_OK(debug_mstamps(out, reset & 1));
  else HIP_OK(debug_stamps(out, reset));
  return 0;
}

int bx_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, float lo, float hi, void* stream) {
  return bx_uniform_slabs(out, n, 1, seed, offset, 0, nullptr, 0, lo, hi, stream);
}

int bx_uniform_epoch(float* out, int64_t n, uint64_t seed, uint64_t offset, const int64_t* epoch,
                     uint64_t epoch_stride, float lo, float hi, void* stream) {
  if (!epoch && n > 0) return fail("null epoch counter");
  return bx_uniform_slabs(out, n, 1, seed, offset, 0, epoch, epoch_stride, lo, hi, stream);
}

int bx_uniform_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed, uint64_t offset,
                     uint64_t slab_stride, const int64_t* epoch, uint64_t epoch_stride, float lo,
                     float hi, void* stream) {
  if (slab_n < 0 || n_slabs < 0) return fail("negative size");
  if (slab_n == 0 || n_slabs == 0) return 0;
  if (slab_n > INT64_MAX / n_slabs || slab_n * n_slabs > ((int64_t)1 << 40))
    return fail("too many elements for one draw");
  if (!out) return fail("null output");
  // no system handle here: launch on the device that owns the stream (the
  // caller's current device for the null stream)
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_uniform_slabs(out, slab_n, n_slabs, seed, offset, slab_stride, epoch, epoch_stride,
                              lo, hi, st));
  return 0;
}

int bx_normal_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed, uint64_t offset,
                    uint64_t slab_stride, const int64_t* epoch, uint64_t epoch_stride, void* stream) {
  if (slab_n < 0 || n_slabs < 0) return fail("negative size");
  if (slab_n == 0 || n_slabs == 0) return 0;
  if (slab_n > INT64_MAX / n_slabs || slab_n * n_slabs > ((int64_t)1 << 40))
    return fail("too many elements for one draw");
  if (!out) return fail("null output");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_normal_slabs(out, slab_n, n_slabs, seed, offset, slab_stride, epoch, epoch_stride, st));
  return 0;
}

int bx_compute_gae(int64_t n_steps, int64_t n_envs, const bx_seq* reward, const bx_seq* done,
                   const bx_seq* truncation, const bx_seq* values, const float* bootstrap,
                   const bx_seq* vs, const bx_seq* advantages, float reward_scaling, float discount,
                   float lambda, void* stream) {
  if (!reward || !done || !truncation || !values || !vs || !advantages) return fail("null argument");
  if (n_steps < 1) return fail("n_steps must be >= 1");
  if (n_envs < 0) return fail("negative n_envs");
  if (n_envs > ((int64_t)1 << 31)) return fail("too many envs for one launch");
  if (n_envs == 0) return 0;
  if (!reward->ptr || !done->ptr || !truncation->ptr || !values->ptr || !bootstrap || !vs->ptr ||
      !advantages->ptr)
    return fail("null argument");
  // (a zero stride on an input broadcasts one row or column; on an output
  // every step or env would write the same element)
  for (const bx_seq* o : {vs, advantages})
    if ((n_steps > 1 && o->time_stride == 0) || (n_envs > 1 && o->env_stride == 0))
      return fail("zero stride on an output");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  GaeArgs a{};
  a.T = n_steps;
  a.B = n_envs;
  a.reward = *reward;
  a.done = *done;
  a.truncation = *truncation;
  a.values = *values;
  a.vs = *vs;
  a.adv = *advantages;
  a.bootstrap = bootstrap;
  a.reward_scaling = reward_scaling;
  a.discount = discount;
  a.lambda = lambda;
  HIP_OK(launch_compute_gae(a, st));
  return 0;
}

int bx_population_perturb(float* rows, const float* theta, int64_t n_directions, int64_t n_params,
                          int64_t stride, double sigma, uint64_t seed, uint64_t offset,
                          int antithetic, const uint8_t* frozen, void* stream) {
  if (!rows || !theta) return fail("null argument");
  if (n_directions < 1) return fail("n_directions must be >= 1");
  if (n_params < 1) return fail("n_params must be >= 1");
  if (stride < n_params) return fail("stride below n_params");
  if (n_params > ((int64_t)1 << 40) / n_directions) return fail("too many samples for one launch");
  if (stride > ((int64_t)1 << 41) / n_directions) return fail("stride too large");
  const int64_t members = antithetic ? 2 * n_directions : n_directions;
  const uintptr_t r0 = (uintptr_t)rows, r1 = r0 + (size_t)((members - 1) * stride + n_params) * 4;
  const uintptr_t t0 = (uintptr_t)theta, t1 = t0 + (size_t)n_params * 4;
  if (r0 < t1 && t0 < r1) return fail("rows overlap theta");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_population_perturb(rows, theta, frozen, n_directions, n_params, stride, sigma, seed,
                                   offset, antithetic ? 1 : 0, st));
  return 0;
}

int bx_population_delta(float* out, const float* weights, int64_t n_directions, int64_t n_params,
                        uint64_t seed, uint64_t offset, const uint8_t* frozen, void* workspace,
                        int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (n_directions < 1) return fail("n_directions must be >= 1");
  if (n_params < 1) return fail("n_params must be >= 1");
  if (n_params > ((int64_t)1 << 40) / n_directions) return fail("too many samples for one launch");
  const int64_t chunks = (n_directions + BX_POPULATION_DELTA_CHUNK - 1) / BX_POPULATION_DELTA_CHUNK;
  const int64_t need = chunks * n_params * (int64_t)sizeof(double);
  if (!workspace) {  // the size query
    *workspace_bytes = need;
    return 0;
  }
  if (!out || !weights) return fail("null argument");
  if (*workspace_bytes < need)
    return fail("workspace of " + std::to_string(*workspace_bytes) + " bytes, " +
                std::to_string(need) + " needed");
  if ((uintptr_t)workspace & 7) return fail("workspace not 8-byte aligned");
  if (chunks > 65535) return fail("too many directions for one launch");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_population_delta(out, weights, frozen, n_directions, n_params, seed, offset,
                                 (double*)workspace, st));
  return 0;
}

namespace {

// the checks bx_replay_insert and bx_replay_sample share, and the kernels'
// field table: prefix offsets, and each field's pointer moved back by its
// offset so a row word indexes it directly
int replay_args(const float* data, int64_t capacity, int64_t row_words, int64_t position,
                int64_t n, const bx_fields* f, ReplayArgs* a) {
  if (!data || !f) return fail("null argument");
  if (f->n_fields < 0 || f->n_fields > BX_FIELDS_MAX)
    return fail("n_fields " + std::to_string(f->n_fields) + " outside 0.." +
                std::to_string(BX_FIELDS_MAX));
  if (capacity < 1) return fail("capacity must be >= 1");
  if (row_words < 0 || row_words > (1 << 24)) return fail("row_words outside 0..2^24");
  if (capacity > ((int64_t)1 << 40) / (row_words ? row_words : 1)) return fail("ring too large");
  if (position < 0 || position >= capacity) return fail("position outside the ring");
  int64_t total = 0;
  for (int k = 0; k < f->n_fields; ++k) {
    if (f->width[k] < 0 || f->width[k] > (1 << 24)) return fail("field width outside 0..2^24");
    total += f->width[k];
  }
  if (total != row_words)
    return fail("field widths sum to " + std::to_string(total) + ", row_words is " +
                std::to_string(row_words));
  int64_t sum = 0;
  for (int k = 0; k < f->n_fields; ++k) {
    if (!f->ptr[k]) return fail("null field pointer");
    a->off[k] = (int32_t)sum;
    a->base[k] = (float*)((uintptr_t)f->ptr[k] - (uintptr_t)sum * sizeof(float));
    a->stride[k] = f->row_stride[k];
    sum += f->width[k];
  }
  for (int k = f->n_fields; k < BX_FIELDS_MAX; ++k) {  // selected by no word
    a->off[k] = (int32_t)row_words;
    a->base[k] = nullptr;
    a->stride[k] = 0;
  }
  a->data = const_cast<float*>(data);
  a->capacity = capacity;
  a->position = position;
  a->row_words = (int32_t)row_words;
  a->n = n;
  return 0;
}

}  // namespace

int bx_replay_insert(float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t n_rows, const bx_fields* src, void* stream) {
  if (n_rows < 0) return fail("negative n_rows");
  if (n_rows == 0) return 0;
  ReplayArgs a{};
  if (replay_args(data, capacity, row_words, position, n_rows, src, &a)) return 1;
  if (n_rows > capacity)
    return fail("n_rows " + std::to_string(n_rows) + " above the capacity " +
                std::to_string(capacity));
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_replay_insert(a, st));
  return 0;
}

int bx_replay_sample(const float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t size, int64_t n_samples, uint64_t seed, uint64_t offset,
                     const bx_fields* dst, int64_t* idx_out, void* stream) {
  if (n_samples < 0) return fail("negative n_samples");
  if (n_samples == 0) return 0;
  ReplayArgs a{};
  if (replay_args(data, capacity, row_words, position, n_samples, dst, &a)) return 1;
  if (size < 1 || size > capacity)
    return fail("size " + std::to_string(size) + " outside 1.." + std::to_string(capacity));
  a.size = size;
  a.seed = seed;
  a.offset = offset;
  a.idx_out = idx_out;
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_replay_sample(a, st));
  return 0;
}

namespace {

// the checks bx_mlp_forward and bx_mlp_backward share, and the kernels' form
// of the network (the hidden layers' column offsets in `saved` and `dz`)
int mlp_args(const bx_mlp* net, int64_t rows, int64_t x_stride, MlpNet* m) {
  if (!net) return fail("null argument");
  if (net->n_layers < 1 || net->n_layers > BX_MLP_MAX_LAYERS)
    return fail("n_layers " + std::to_string(net->n_layers) + " outside 1.." +
                std::to_string(BX_MLP_MAX_LAYERS));
  if (net->activation != BX_POLICY_SWISH && net->activation != BX_POLICY_RELU &&
      net->activation != BX_POLICY_TANH)
    return fail("unknown activation " + std::to_string(net->activation));
  if (rows < 0) return fail("negative rows");
  if (rows > ((int64_t)1 << 31)) return fail("too many rows for one launch");
  m->n_layers = net->n_layers;
  m->activation = net->activation;
  int hidden = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    const int in = net->in[l], out = net->out[l];
    if (out < 1 || out > BX_MLP_MAX_WIDTH)
      return fail("layer " + std::to_string(l) + ": width " + std::to_string(out) +
                  " outside 1.." + std::to_string(BX_MLP_MAX_WIDTH));
    if (l == 0 && (in < 1 || in > BX_MLP_MAX_IN))
      return fail("input width " + std::to_string(in) + " outside 1.." +
                  std::to_string(BX_MLP_MAX_IN));
    if (l > 0 && in != net->out[l - 1])
      return fail("layer " + std::to_string(l) + ": in " + std::to_string(in) +
                  " != the previous out " + std::to_string(net->out[l - 1]));
    if (!net->w[l] || !net->b[l]) return fail("null weight or bias");
    m->in[l] = in;
    m->out[l] = out;
    m->w[l] = net->w[l];
    m->b[l] = net->b[l];
    m->off[l] = hidden;
    if (l + 1 < net->n_layers) hidden += out;
  }
  m->hidden = hidden;
  if (x_stride < net->in[0])
    return fail("x_stride " + std::to_string(x_stride) + " below the input width " +
                std::to_string(net->in[0]));
  return 0;
}

}  // namespace

int bx_mlp_sizes(int32_t* mlp_bytes, int32_t* grads_bytes) {
  if (!mlp_bytes || !grads_bytes) return fail("null argument");
  *mlp_bytes = (int32_t)sizeof(bx_mlp);
  *grads_bytes = (int32_t)sizeof(bx_mlp_grads);
  return 0;
}

int bx_mlp_forward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride, float* y,
                   float* saved, void* stream) {
  MlpNet m{};
  if (mlp_args(net, rows, x_stride, &m)) return 1;
  if (rows == 0) return 0;
  if (!x || !y) return fail("null argument");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_mlp_forward(m, rows, x, x_stride, y, saved, st));
  return 0;
}

int bx_mlp_backward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride,
                    const float* saved, const float* dy, float* dx, const bx_mlp_grads* grads,
                    void* workspace, int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  MlpNet m{};
  if (mlp_args(net, rows, x_stride, &m)) return 1;
  const int64_t need = std::max<int64_t>(16, 4 * rows * (int64_t)m.hidden);
  if (!workspace) {  // the size query
    *workspace_bytes = need;
    return 0;
  }
  if (rows == 0) return 0;
  if (!x || !dy) return fail("null argument");
  if (m.n_layers > 1 && !saved) return fail("null saved with hidden layers");
  if (*workspace_bytes < need)
    return fail("workspace of " + std::to_string(*workspace_bytes) + " bytes, " +
                std::to_string(need) + " needed");
  if ((uintptr_t)workspace & 15) return fail("workspace not 16-byte aligned");
  MlpGrads g{};
  if (grads)
    for (int l = 0; l < m.n_layers; ++l) {
      g.dw[l] = grads->dw[l];
      g.db[l] = grads->db[l];
    }
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_mlp_backward(m, g, rows, x, x_stride, saved, dy, dx, (float*)workspace, st));
  return 0;
}

int bx_ppo_head(int64_t n_steps, int64_t n_envs, int64_t n_actions, const bx_seq* logits,
                const bx_seq* baseline, const float* bootstrap, const bx_seq* raw_action,
                const bx_seq* eps, const bx_seq* log_prob, const bx_seq* reward,
                const bx_seq* done, const bx_seq* truncation, float reward_scaling, float discount,
                float lambda, double clipping_epsilon, float entropy_cost, float min_std,
                int normalize_advantage, float* losses, const bx_seq* dlogits,
                const bx_seq* dbaseline, const bx_seq* vs, const bx_seq* advantages,
                void* workspace, int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (n_steps < 1) return fail("n_steps must be >= 1");
  if (n_actions < 1) return fail("n_actions must be >= 1");
  if (n_envs < 0) return fail("negative n_envs");
  if (n_actions > ((int64_t)1 << 20)) return fail("too many actions");
  if (n_steps > ((int64_t)1 << 31) || n_envs > ((int64_t)1 << 31) ||
      n_steps * n_envs > ((int64_t)1 << 31))
    return fail("too many rows for one launch");
  const int64_t need = ppo_head_workspace_bytes(n_steps, n_envs);
  if (!workspace) {  // the size query
    *workspace_bytes = need;
    return 0;
  }
  if (n_envs == 0) return 0;
  const bx_seq* in[] = {logits, baseline, raw_action, eps, log_prob, reward, done, truncation};
  for (const bx_seq* q : in)
    if (!q || !q->ptr) return fail("null argument");
  if (!bootstrap || !losses || !dlogits || !dlogits->ptr || !dbaseline || !dbaseline->ptr)
    return fail("null argument");
  const bx_seq none{nullptr, 0, 0};
  if (!vs) vs = &none;
  if (!advantages) advantages = &none;
  // (a zero stride on an input broadcasts one row or column; on an output
  // every step or env would write the same element)
  for (const bx_seq* o : {dlogits, dbaseline, vs, advantages})
    if (o->ptr && ((n_steps > 1 && o->time_stride == 0) || (n_envs > 1 && o->env_stride == 0)))
      return fail("zero stride on an output");
  if (*workspace_bytes < need)
    return fail("workspace of " + std::to_string(*workspace_bytes) + " bytes, " +
                std::to_string(need) + " needed");
  if ((uintptr_t)workspace & 15) return fail("workspace not 16-byte aligned");
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  PpoHeadArgs a{};
  a.T = n_steps;
  a.B = n_envs;
  a.A = n_actions;
  a.logits = *logits;
  a.baseline = *baseline;
  a.raw = *raw_action;
  a.eps = *eps;
  a.log_prob = *log_prob;
  a.reward = *reward;
  a.done = *done;
  a.truncation = *truncation;
  a.bootstrap = bootstrap;
  a.reward_scaling = reward_scaling;
  a.discount = discount;
  a.lambda = lambda;
  a.clip_lo = (float)(1.0 - clipping_epsilon);
  a.clip_hi = (float)(1.0 + clipping_epsilon);
  a.entropy_cost = entropy_cost;
  a.min_std = min_std;
  a.normalize = normalize_advantage != 0;
  a.losses = losses;
  a.dlogits = *dlogits;
  a.dbaseline = *dbaseline;
  a.vs = *vs;
  a.adv = *advantages;
  ppo_head_carve(a, workspace);
  HIP_OK(launch_ppo_head(a, st));
  return 0;
}

int bx_opt_sizes(int32_t* tensor_bytes) {
  if (!tensor_bytes) return fail("null argument");
  *tensor_bytes = (int32_t)sizeof(bx_opt_tensor);
  return 0;
}

int bx_adam_step(const bx_opt_tensor* t, int32_t n_tensors, int64_t step, double beta1,
                 double beta2, float eps, void* stream) {
  if (!t) return fail("null tensor table");
  if (n_tensors < 1 || n_tensors > BX_OPT_MAX_TENSORS)
    return fail("n_tensors " + std::to_string(n_tensors) + " outside 1.." +
                std::to_string(BX_OPT_MAX_TENSORS));
  if (step < 1) return fail("step must be >= 1 (the count after this step)");
  // (the range checks and the double arithmetic live in optim_kernels.hip,
  // whose flags keep NaN comparisons and IEEE division; this unit's do not)
  if (const char* why = opt_check_scalars(beta1, beta2, eps)) return fail(why);
  OptArgs a{};
  int64_t groups = 0;
  int k = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const bx_opt_tensor& s = t[i];
    if (s.n < 0) return fail("tensor " + std::to_string(i) + ": negative n");
    if (s.n == 0) continue;
    if (!s.p || !s.g || !s.m || !s.v)
      return fail("tensor " + std::to_string(i) + ": null p, g, m or v");
    OptTensor& d = a.t[k];
    d.p = s.p;
    d.g = s.g;
    d.m = s.m;
    d.v = s.v;
    d.target = s.target;
    d.n = s.n;
    opt_set_tensor(d, s.lr, s.tau, step, beta1);
    const uintptr_t bits = (uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v |
                           (uintptr_t)s.target;
    d.vec = (bits & 15) == 0;
    a.first[k] = (int32_t)groups;
    groups += opt_chunks(s.n);
    if (groups > (int64_t)0x7fffffff) return fail("too many elements for one launch");
    ++k;
  }
  if (k == 0) return 0;
  a.first[k] = (int32_t)groups;
  a.n_tensors = k;
  opt_set_scalars(a, step, beta1, beta2, eps);
  int dev = -1;
  hipStream_t st = as_stream(stream);
  if (st) HIP_OK(hipStreamGetDevice(st, &dev));
  else HIP_OK(hipGetDevice(&dev));
  DeviceScope scope(dev);
  if (scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(scope.err));
  HIP_OK(launch_adam_step(a, st));
  return 0;
}

}  // extern "C"
