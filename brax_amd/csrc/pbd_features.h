// pbd_features.h — the compile-time switches of the step kernels: the feature
// mask F, the env-program kind EK, the kernel mode and the limit-row slots,
// with the predicates that read them. The enums are plain C++ (pbd_dispatch.h
// and host programs include them without HIP); the device predicates exist
// under hipcc only.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace bx {

// ---------------------------------------------------------------------------
// compile-time feature mask: kernels specialised for a system only carry the
// joint / actuator / contact kinds it uses (Ant: revolute + torque + one-way
// capsule-plane), which keeps dead paths out of the register allocation.
// ---------------------------------------------------------------------------
enum { F_SPH = 1, F_ANGLE = 2, F_CC = 4, F_TW = 8, F_FORCE = 16, F_ALL = 31 };
// F_G1 (outside F_ALL): every body's contact rows come from one collider
// group, so the per-group normalisation needs one accumulator
enum { F_G1 = 32 };
// F_X (outside F_ALL): the extended contact functions (height map, clipped
// plane, capsule-mesh, box-box SAT), item-loop kernels only. F_GEN: every
// feature, the item-loop kernels' general instantiation.
enum { F_X = 64, F_GEN = F_ALL | F_X };
// F_JH: the joint halves (joint_apply_half)
enum { F_JH = 128 };
// F_R2 (outside F_ALL, SINGLE mode at 16 lanes): 17-32 contact rows, lane l
// owning rows l and l + 16 (its second row's constants from the lane image's
// LI_ROW2 words)
enum { F_R2 = 256 };
// F_C16 (outside F_ALL, SINGLE mode): contact gather lists of up to 16
// entries (Pusher's wrist: 15 rows), the joint / actuator lists <= M
enum { F_C16 = 512 };
// F_R2G (with F_R2): the host put every one-way capsule-plane row in the
// lanes' first slot and every two-way capsule-capsule row in the second, so
// each slot's passes are compiled for its one contact function
enum { F_R2G = 1024 };
// F_CCO (kernel-internal): every row this code path sees is a two-way
// capsule-capsule row (F_R2G's second slot)
enum { F_CCO = 2048 };
// F_LEAN: the item-loop kernels' lean instantiation (revolute joints, torque
// actuators, capsule-plane / capsule-capsule rows one- or two-way, no forces:
// Ant Mountain, the culled scenes)
enum { F_LEAN = F_CC | F_TW };

// CB (contact on body lanes): the feature sets whose body-copy kernels (JB,
// pbd_step_single) resolve each body's one contact row on the body's own
// lanes: joint halves, one collider group, one-way capsule-plane rows only,
// one row slot and no forces (the Ant env kernels). The host admits a system
// to such a kernel only when its rows fit (bx_blob.cpp cb_rows_ok).
// A/B switch -DBX_NO_CB: the same kernels with the row-lane passes.
constexpr bool cb_feat(int F) {
#if defined(BX_NO_CB)
  return false;
#else
  return (F & F_JH) != 0 && (F & F_G1) != 0 &&
         (F & (F_CC | F_TW | F_R2 | F_C16 | F_FORCE | F_SPH)) == 0;
#endif
}

// CBH (the CB kernels): the frozen plane side of the lane's row (its pose and
// the plane normal rotate((0, 0, 1), rot)) read from LDS once per launch and
// after an AutoReset instead of in every collision pass, and the frozen
// bodies' records written once per launch instead of every step.
// A/B switch -DBX_NO_CBH: the CB passes with their per-pass loads.
constexpr bool cbh_feat(int F) {
#if defined(BX_NO_CBH)
  return false;
#else
  return cb_feat(F);
#endif
}

#if defined(__HIPCC__)
template <int F, int M> __device__ __forceinline__ constexpr int cl_width() {
  return (F & F_C16) ? 16 : M;
}
template <int F> __device__ __forceinline__ bool is_rev(int type) {
  if constexpr ((F & F_SPH) == 0) return true; else return type == 1;
}
template <int F> __device__ __forceinline__ bool is_torque(int type) {
  if constexpr ((F & F_ANGLE) == 0) return true; else return type == 0;
}
template <int F> __device__ __forceinline__ bool is_plane(int fn) {
  if constexpr ((F & F_CCO) != 0) return false;
  else if constexpr ((F & F_CC) == 0) return true; else return fn == 0;
}
// the F_R2G kernels' two-way slot runs as contact halves (HALF: a row's a
// side on lane k, its b side on lane k + 8; the host places them so)
template <int F> __device__ __forceinline__ constexpr bool HALF() {
  return (F & F_CCO) != 0 && (F & F_R2G) != 0;
}
template <int F> __device__ __forceinline__ bool is_oneway(int ow) {
  if constexpr ((F & F_CCO) != 0) return false;
  else if constexpr ((F & F_TW) == 0) return true; else return ow != 0;
}
#endif  // __HIPCC__

// the LDS-staged joint limit rows' first slots (ld_lim)
enum { LIM_G0 = 0, LIM_G1 = 2, LIM_G2 = 4, LIM_SLOTS = 6 };

// env-program specialisation: the hot env kinds get step kernels holding
// only their own env code (EK_ANT, EK_HUM: Humanoid and HumanoidStandup,
// EK_CHEETAH: HalfCheetah); EK_ANY carries every kind, chosen at run time
// (EK_PUSHER: Pusher, round 6: its 50 substeps with the damping folded)
enum { EK_ANY = 0, EK_ANT = 1, EK_HUM = 2, EK_CHEETAH = 3, EK_PUSHER = 4 };

// kernel variants: MODE_GLOBAL (constants read from the HBM blob inside the
// loops), MODE_SINGLE (constants hoisted to registers), MODE_LDS (the blob's
// constant part copied to LDS once per workgroup, read there inside the loops)
enum { MODE_GLOBAL = 0, MODE_SINGLE = 1, MODE_LDS = 2, MODE_MULTI = 3 };

}  // namespace bx
