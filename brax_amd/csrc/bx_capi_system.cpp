// bx_capi_system.cpp — the C ABI's system side (include/brax_amd.h): the error
// string, a system's lifecycle and plan, bx_system_step, the state readers,
// the phase kernels and the debug entry points.
#include <cstring>

#include "bx_capi_common.h"
#include "pbd_launch.h"

using namespace bx;

namespace {

thread_local std::string g_err;

// the host half of a system (bx_blob.cpp), with this process's A/B knobs
int build_blob(const bx_desc* d, const bx_reset_desc* r, bx_system* S) {
  std::string err;
  if (build_plan(d, r, plan_knobs_from_env(), S, &err)) return fail(err);
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int bx::fail(const std::string& m) {
  g_err = m;
  return 1;
}

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
int bx_system_env_lanes(bx_system* S) { return S ? S->L : 0; }
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

}  // extern "C"
