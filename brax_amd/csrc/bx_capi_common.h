// bx_capi_common.h — what the C ABI's units (bx_capi_system.cpp, _env, _learn)
// share: the error string, the device scopes, a system's host side and the
// checks more than one unit makes. Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/brax_amd.h"
#include "bx_blob.h"

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

namespace bx {

// sets this thread's bx_last_error() and returns 1 (bx_capi_system.cpp)
int fail(const std::string& m);

#define HIP_OK(expr)                                                       \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

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
// Without a system handle: declares hipStream_t st and scopes the device that
// owns the stream (the caller's current device for the null stream)
#define STREAM_SCOPE(stream, st)                                                   \
  hipStream_t st = as_stream(stream);                                              \
  int _sdev = -1;                                                                  \
  if (st) HIP_OK(hipStreamGetDevice(st, &_sdev));                                  \
  else HIP_OK(hipGetDevice(&_sdev));                                               \
  DeviceScope _scope(_sdev);                                                       \
  if (_scope.err != hipSuccess) return fail(std::string("device: ") + hipGetErrorString(_scope.err))

// the dynamic LDS of a system's step kernels, per workgroup
inline size_t step_lds(const bx_system* S) {
  if (S->mode == 3) return (size_t)S->hdr.env_words_m * 4;
  size_t b = (size_t)(S->tpb / S->L) * S->hdr.env_words * 4;
  if (S->mode == 2) b += (size_t)S->hdr.const_words * 4;
  return b;
}

inline bool qp_ok(const bx_qp& q) { return q.pos.ptr && q.rot.ptr && q.vel.ptr && q.ang.ptr; }

// the action row of bx_system_step and bx_env_step (bx_capi_env.cpp)
int check_act(const bx_system* S, const float* act, int64_t act_stride, int64_t act_width);

// the BX_POLICY_* activation codes (bx_policy and bx_mlp)
inline bool activation_ok(int a) {
  return a == BX_POLICY_SWISH || a == BX_POLICY_RELU || a == BX_POLICY_TANH;
}

}  // namespace bx
