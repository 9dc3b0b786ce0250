// pbd_generic.hip — the item-loop translation unit over the bodies of
// pbd_kernels.hip (large scenes, legacy_spring, the extended contact
// functions), with the MULTI-mode, info, reset and RNG kernels and their
// launchers. Built with fast reciprocal division as the SINGLE-mode unit by
// default (GENERIC_PRECISE=1: IEEE).
#define BX_TU_GENERIC
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbd_kernels.hip"
#include "pbd_launch.h"
#include "pbd_stamps.h"

namespace bx {

// the MULTI kernel held to 256 registers per lane (VGPRs + AGPRs): two waves
// per SIMD. Past 256 (round 4: the row image's b-slot index took it to
// 256 + 4) one wave per SIMD fits and the CU holds half the envs: Ant
// Mountain(4) at 2,048 envs ran 1.8x slower (tools/multi_occ.py). At L = 128
// threads per env (two waves) four envs share a CU, when their LDS tail
// fits 40 KB (the compact contact slots, bx_capi.cpp)
template <int L, int JH = 0>
__global__ void __launch_bounds__(L) __attribute__((amdgpu_waves_per_eu(2)))
system_step_multi_kernel(StepArgs A) {
  system_step_body<L, MODE_MULTI, F_CC | F_TW | JH, 1>(A);
}

// System.info contact part + optional Env._get_obs of the same state (reset)
template <int L>
__global__ void __launch_bounds__(L > 64 ? L : 64) info_obs_kernel(InfoArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Cst c{A.blob};
  BlobHdr H = *reinterpret_cast<const BlobHdr*>(A.blob);
  const int lane = threadIdx.x % L;
  const int le = threadIdx.x / L;
  const int64_t e = (int64_t)blockIdx.x * (blockDim.x / L) + le;
  const bool valid = e < A.n_envs;
  Env E = carve(smem + le * H.env_words, H);
  if (valid) {
    for (int b = lane; b < H.N; b += L) load_qp_global(A.q, e, b, E.qp + b * QP_STRIDE);
  } else {
    for (int b = lane; b < H.N; b += L) {
      float* s = E.qp + b * QP_STRIDE;
      for (int k = 0; k < 13; k++) s[k] = k == 3 ? 1.f : 0.f;
    }
  }
  esync<L>();
  if (A.angle) {  // Joint.angle_vel only
    joint_angles<L>(c, H, E, lane);
    esync<L>();
    if (valid)
      for (int i = lane; i < H.D; i += L) {
        A.angle[e * H.D + i] = E.ang[i];
        A.angvel[e * H.D + i] = E.ang[H.D + i];
      }
    return;
  }
  pbd_info<L>(c, H, E, lane);
  if (valid) {
    for (int b = lane; b < H.N; b += L) {
      const float* acc = E.acc + b * ACC_STRIDE;
      const bx_info& I = A.info;
      if (I.contact_vel.ptr) {
        float* p = I.contact_vel.ptr + e * I.contact_vel.env_stride + b * I.contact_vel.body_stride;
        p[0] = acc[ACC_ICV]; p[1] = acc[ACC_ICV + 1]; p[2] = acc[ACC_ICV + 2];
      }
      if (I.contact_ang.ptr) {
        float* p = I.contact_ang.ptr + e * I.contact_ang.env_stride + b * I.contact_ang.body_stride;
        p[0] = acc[ACC_ICA]; p[1] = acc[ACC_ICA + 1]; p[2] = acc[ACC_ICA + 2];
      }
    }
  }
  if (A.obs) {
    const float* act = valid && A.act ? A.act + e * A.act_stride : nullptr;
    env_observe<L>(c, H, E, lane, A.kind, A.obs_flags, A.obs_size, act, (int)A.act_width,
                   valid ? A.obs + e * A.obs_size : nullptr, A.coef);
  }
  // reset: reward, done, steps, truncation and metrics start at zero
  // (ant.py:205-219, wrappers.py:94-97)
  if (valid) {
    if (lane == 0) {
      if (A.zero_reward) A.zero_reward[e] = 0.f;
      if (A.zero_done) A.zero_done[e] = 0.f;
      if (A.zero_steps) A.zero_steps[e] = 0.f;
      if (A.zero_trunc) A.zero_trunc[e] = 0.f;
    }
    if (A.zero_metrics)
      for (int i = lane; i < A.n_metrics; i += L) A.zero_metrics[e * A.n_metrics + i] = 0.f;
  }
}

// System.default_qp (system.py:112-242): one thread per env (reset path)
__global__ void __launch_bounds__(64) default_qp_kernel(ResetArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Cst c{A.blob};
  BlobHdr H = *reinterpret_cast<const BlobHdr*>(A.blob);
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= A.n_envs) return;
  float* q = smem + threadIdx.x * H.N * 13;  // per-thread scratch: N x 13
  const int N = H.N, D = H.num_joint_dof;
  for (int b = 0; b < N; b++)
    for (int k = 0; k < 13; k++) q[b * 13 + k] = c.f(H.o_base + b * 13 + k);
  const float* ja = A.gen ? nullptr : A.angle + e * D;
  const float* jv = A.gen ? nullptr : A.vel + e * D;
  // Env.reset draws (gen = 1), keyed by the global env id g (W draws per
  // env: (seed, g * W + k)) or by the env's own key (seeds[e], k):
  //   default (ant.py:200-203 ...): qpos = default + U[-s, s) at k = dof,
  //     qvel = U[-s, s) at k = D + dof (W = 2D)
  //   REACHER, REACHERANGLE (reacher.py:157-160): qpos noise U[-.1, .1),
  //     qvel U[-.005, .005), then the target's two draws at 2D, 2D + 1
  //   PUSHER (pusher.py:178-195): default angles, qvel U[-.005, .005) on the
  //     first D - 4 dofs (k = dof), the object's two draws at D - 4, D - 3
  //   UR5E, FETCH (ur5e.py:41-46): default pose at rest, the target's two
  //     draws at 0, 1;  GRASP (grasp.py:54-70): default pose at rest
  const int kind = A.gen ? A.kind : 0;
  int W = 2 * D;
  float as = A.scale, vs = A.scale;
  int nvel = D;
  if (kind == BX_ENV_REACHER || kind == BX_ENV_REACHERANGLE) {
    W = 2 * D + 2; as = .1f; vs = .005f;
  } else if (kind == BX_ENV_PUSHER) {
    W = D - 4 + 2; as = 0.f; vs = .005f; nvel = D - 4;
  } else if (kind == BX_ENV_UR5E || kind == BX_ENV_FETCH) {
    W = 2; as = 0.f; vs = 0.f; nvel = 0;
  } else if (kind == BX_ENV_GRASP) {
    W = 0; as = 0.f; vs = 0.f; nvel = 0;
  }
  const int voff = kind == BX_ENV_PUSHER ? 0 : D;  // pusher's qvel draws come first
  const uint64_t seed = A.seeds ? A.seeds[e] : A.seed;
  const uint64_t g0 = A.seeds ? 0ull : (uint64_t)(A.env_offset + e) * (uint64_t)W;
  for (int f = 0; f < H.n_fk; f++) {
    int o = H.o_fk + f * FK_STRIDE;
    float a3[3], v3_[3];
    for (int l = 0; l < 3; l++) {
      int ix = c.i(o + FK_IDX + l);
      if (A.gen) {
        a3[l] = ix < 0 ? 0.f
                : c.f(H.o_dangle + ix) + (as > 0.f ? uniform_at(seed, g0 + ix, -as, as) : 0.f);
        v3_[l] = ix >= 0 && ix < nvel ? uniform_at(seed, g0 + voff + ix, -vs, vs) : 0.f;
      } else {
        a3[l] = ix >= 0 ? ja[ix] : 0.f;
        v3_[l] = ix >= 0 ? jv[ix] : 0.f;
      }
    }
    q4 jr{c.f(o + FK_ROT), c.f(o + FK_ROT + 1), c.f(o + FK_ROT + 2), c.f(o + FK_ROT + 3)};
    q4 rot{c.f(o + FK_REF), c.f(o + FK_REF + 1), c.f(o + FK_REF + 2), c.f(o + FK_REF + 3)};
    v3 axes[3] = {rotate(mk(1.f, 0.f, 0.f), jr), rotate(mk(0.f, 1.f, 0.f), jr),
                  rotate(mk(0.f, 0.f, 1.f), jr)};
    v3 lang = axes[0] * v3_[0] + axes[1] * v3_[1] + axes[2] * v3_[2];
    for (int l = 0; l < 3; l++) {
      v3 ax = rotate(axes[l], rot);
      rot = quat_mul(quat_rot_axis(ax, a3[l]), rot);
    }
    int bp = c.i(o + FK_BP), bc = c.i(o + FK_BC);
    float* sp = q + bp * 13;
    float* sc = q + bc * 13;
    q4 prot = ld4(sp + 3);
    q4 wr = quat_mul(prot, rot);
    v3 lp = c.f3(o + FK_OFFP) - rotate(c.f3(o + FK_OFFC), rot);
    v3 wp = ld3(sp) + rotate(lp, prot);
    v3 wa = rotate(lang, prot);
    st3(sc, wp);
    st4(sc + 3, wr);
    st3(sc + 10, wa);
  }
  // bodies.min_z per root group, then lift (system.py:213-240)
  for (int g = 0; g < H.n_root_groups; g++) {
    float zmin = 3.4028235e38f;
    for (int b = 0; b < N; b++) {
      if (c.i(H.o_rgroup + b) != g) continue;
      float bz = 3.4028235e38f;
      for (int p = c.i(H.o_zoff + b), pe = c.i(H.o_zoff + b + 1); p < pe; p++) {
        int o = H.o_zpt + p * 4;
        v3 w = rotate(c.f3(o), ld4(q + b * 13 + 3));
        float z = q[b * 13 + 2] + w.z - c.f(o + 3);
        bz = fminf(bz, z);
      }
      if (c.i(H.o_zero + b)) bz = fminf(bz, 0.f);
      zmin = fminf(zmin, bz);
    }
    for (int b = 0; b < N; b++) {
      if (c.i(H.o_rgroup + b) != g) continue;
      q[b * 13 + 0] = q[b * 13 + 0] - zmin * 0.f;
      q[b * 13 + 1] = q[b * 13 + 1] - zmin * 0.f;
      q[b * 13 + 2] = q[b * 13 + 2] - zmin * 1.f;
    }
  }
  // the bodies the env's reset places after default_qp (index_update of
  // qp.pos, so after the lift): the reachers' target (reacher.py:212-221,
  // reacherangle.py:102-113: radius .2 u, sqrt(u) for ReacherAngle), the
  // pusher's object in its .17 disc, goal and table (pusher.py:181-201), the
  // target envs' target on their ring (ur5e.py:117-125, fetch.py:124-134)
  const float twopi = 3.14159265358979323846f * 2.f;
  if (kind == BX_ENV_REACHER || kind == BX_ENV_REACHERANGLE) {
    const float u0 = uniform_at(seed, g0 + 2 * D, 0.f, 1.f);
    const float u1 = uniform_at(seed, g0 + 2 * D + 1, 0.f, 1.f);
    const float dist = .2f * (kind == BX_ENV_REACHERANGLE ? sqrtf(u0) : u0);
    const float an = twopi * u1;
    float* t = q + (int)A.coef[0] * 13;
    t[0] = dist * cosf(an);
    t[1] = dist * sinf(an);
    t[2] = .01f;
  } else if (kind == BX_ENV_PUSHER) {
    float x = uniform_at(seed, g0 + D - 4, -.3f, 0.f);
    float y = uniform_at(seed, g0 + D - 3, -.2f, .2f);
    const float nrm = sqrtf(x * x + y * y);
    const float sc = nrm > .17f ? .17f / nrm : 1.f;
    float* ob = q + (int)A.coef[1] * 13;
    ob[0] = sc * x;
    ob[1] = sc * y;
    ob[2] = .05f;
    float* gl = q + (int)A.coef[2] * 13;
    gl[0] = .45f; gl[1] = .05f; gl[2] = .05f;
    float* tb = q + (int)A.coef[3] * 13;
    tb[0] = 0.f; tb[1] = 0.f; tb[2] = 0.f;
  } else if (kind == BX_ENV_UR5E || kind == BX_ENV_FETCH) {
    const float u0 = uniform_at(seed, g0, 0.f, 1.f), u1 = uniform_at(seed, g0 + 1, 0.f, 1.f);
    const float rr = A.coef[2] + A.coef[3] * u0;
    const float an = twopi * u1;
    float* t = q + (int)A.coef[1] * 13;
    t[0] = rr * cosf(an);
    t[1] = rr * sinf(an);
    t[2] = A.coef[4];
  }
  // the target envs' per-env stream (info['rng']): a hash of (seed, global
  // env id), or of the env's own key
  if (A.rng_out && (kind == BX_ENV_UR5E || kind == BX_ENV_FETCH || kind == BX_ENV_GRASP)) {
    const uint64_t id = A.seeds ? 0ull : (uint64_t)(A.env_offset + e);
    int64_t z = (int64_t)(id * 0x9E3779B97F4A7C15ull + (seed & 0x7FFFFFFFFFFFFFFFull));
    z = (int64_t)((uint64_t)(z ^ (z >> 31)) * 0x94D049BB133111EBull);
    A.rng_out[e] = (uint32_t)(z ^ (z >> 29));
  }
  for (int b = 0; b < N; b++) store_qp_global(A.out, e, b, q + b * 13);
}

// counter-based uniform fill: splitmix64 of (seed, index) -> [lo, hi)
__global__ void uniform_kernel(float* out, int64_t n, uint64_t seed, uint64_t offset, float lo,
                               float hi) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = uniform_at(seed, (uint64_t)i + offset, lo, hi);
}

// the same fill over n_slabs slabs of slab_n elements with their own offsets,
// advanced by a device-resident epoch counter: out[s * slab_n + j] =
// U(seed, offset + epoch * epoch_stride + s * slab_stride + j). A
// graph-captured rollout draws the action slabs of all its K steps in one
// launch and still draws fresh slabs per replay (the counter is bumped inside
// the graph); epoch null reads as 0
__global__ void uniform_slabs_kernel(float* out, int64_t slab_n, int64_t n, uint64_t seed,
                                     uint64_t offset, uint64_t slab_stride,
                                     const int64_t* __restrict__ epoch, uint64_t epoch_stride,
                                     float lo, float hi) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t e = epoch ? (uint64_t)epoch[0] : 0ull;
  const int64_t sl = i / slab_n, j = i - sl * slab_n;
  out[i] = uniform_at(seed, offset + e * epoch_stride + (uint64_t)sl * slab_stride + (uint64_t)j,
                      lo, hi);
}

// item-loop kernels: a lean instantiation (F_LEAN) where the system allows,
// else every feature
#define BX_DISPATCH_GENERIC(KERNEL, ARGS)                                           \
  const bool lean = (feat & (F_SPH | F_ANGLE | F_FORCE | F_X)) == 0;                \
  switch (L * 8 + mode * 2 + (lean ? 1 : 0)) {                                      \
    case 16 * 8 + 0: case 16 * 8 + 1: launch_one<ARGS>(KERNEL<16, 0, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 16 * 8 + 4: case 16 * 8 + 5: launch_one<ARGS>(KERNEL<16, 2, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 32 * 8 + 0: case 32 * 8 + 1: launch_one<ARGS>(KERNEL<32, 0, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 32 * 8 + 4: case 32 * 8 + 5: launch_one<ARGS>(KERNEL<32, 2, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 64 * 8 + 0: launch_one<ARGS>(KERNEL<64, 0, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 64 * 8 + 1: launch_one<ARGS>(KERNEL<64, 0, F_LEAN, 8>, grid, tpb, lds, s, a); break; \
    case 64 * 8 + 4: case 64 * 8 + 5: launch_one<ARGS>(KERNEL<64, 2, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 128 * 8 + 0: launch_one<ARGS>(KERNEL<128, 0, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 128 * 8 + 1: launch_one<ARGS>(KERNEL<128, 0, F_LEAN, 8>, grid, tpb, lds, s, a); break; \
    case 256 * 8 + 0: launch_one<ARGS>(KERNEL<256, 0, F_GEN, 8>, grid, tpb, lds, s, a); break; \
    case 256 * 8 + 1: launch_one<ARGS>(KERNEL<256, 0, F_LEAN, 8>, grid, tpb, lds, s, a); break; \
    default: return hipErrorInvalidValue;                                           \
  }

hipError_t launch_system_step_generic(int L, int mode, int feat, int tpb, int64_t n_envs, size_t lds,
                                      hipStream_t s, const StepArgs& a) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  BX_DISPATCH_GENERIC(system_step_kernel, StepArgs)
  return hipGetLastError();
}
hipError_t launch_env_step_generic(int L, int mode, int feat, int tpb, int64_t n_envs, size_t lds,
                                   hipStream_t s, const EnvArgs& a) {
  const int epb = tpb / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  BX_DISPATCH_GENERIC(env_step_kernel, EnvArgs)
  return hipGetLastError();
}
hipError_t launch_system_step_multi(int L, int jh, int64_t n_envs, size_t lds, hipStream_t s,
                                    const StepArgs& a) {
  dim3 grid((unsigned)n_envs);
  switch (L * 2 + (jh ? 1 : 0)) {
    case 128 * 2: launch_one<StepArgs>(system_step_multi_kernel<128>, grid, 128, lds, s, a); break;
    case 128 * 2 + 1: launch_one<StepArgs>(system_step_multi_kernel<128, F_JH>, grid, 128, lds, s, a); break;
    case 256 * 2: launch_one<StepArgs>(system_step_multi_kernel<256>, grid, 256, lds, s, a); break;
    case 256 * 2 + 1: launch_one<StepArgs>(system_step_multi_kernel<256, F_JH>, grid, 256, lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_info_obs(int L, int64_t n_envs, size_t lds, hipStream_t s, const InfoArgs& a) {
  int epb = L > 64 ? 1 : 64 / L;
  dim3 grid((unsigned)((n_envs + epb - 1) / epb));
  if (L == 128) launch_one<InfoArgs>(info_obs_kernel<128>, grid, 128, lds, s, a);
  else if (L == 256) launch_one<InfoArgs>(info_obs_kernel<256>, grid, 256, lds, s, a);
  else if (L == 16) launch_one<InfoArgs>(info_obs_kernel<16>, grid, 64, lds, s, a);
  else if (L == 32) launch_one<InfoArgs>(info_obs_kernel<32>, grid, 64, lds, s, a);
  else launch_one<InfoArgs>(info_obs_kernel<64>, grid, 64, lds, s, a);
  return hipGetLastError();
}
hipError_t debug_mstamps(unsigned long long* out, int reset) {
#ifdef BX_MSTAMPS
  return stamps_readback(HIP_SYMBOL(bx_mstamp_wave), out, reset, false);
#else
  (void)out;
  (void)reset;
  return hipErrorNotSupported;
#endif
}
hipError_t launch_default_qp(int64_t n_envs, size_t lds, hipStream_t s, const ResetArgs& a) {
  dim3 grid((unsigned)((n_envs + 63) / 64));
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)default_qp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(default_qp_kernel, grid, dim3(64), lds, s, a);
  return hipGetLastError();
}
hipError_t launch_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, float lo, float hi,
                          hipStream_t s) {
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(uniform_kernel, grid, dim3(256), 0, s, out, n, seed, offset, lo, hi);
  return hipGetLastError();
}
hipError_t launch_uniform_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                                uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                                uint64_t epoch_stride, float lo, float hi, hipStream_t s) {
  const int64_t n = slab_n * n_slabs;
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(uniform_slabs_kernel, grid, dim3(256), 0, s, out, slab_n, n, seed, offset,
                     slab_stride, epoch, epoch_stride, lo, hi);
  return hipGetLastError();
}

}  // namespace bx
