// pbd_dispatch.h — which SINGLE-mode kernel instantiation a system runs.
//
// single_variant() is the decision, BX_SINGLE_VARIANTS the list of (lanes,
// features, gather width) that exist. The launchers' switches are generated
// from the list (pbd_launch.h), so a variant cannot be selected without
// being instantiated; the host asks the same function which kernel a system
// gets (bx_blob.cpp sizes the staged limit rows by its F_SPH bit).
// Single mode at 16 lanes is specialised per feature set and gather width.
//
// kind_variant() is the same for the env kinds with kernels of their own
// (BX_KIND_VARIANTS), asked first by every env launch unit (EnvFamily);
// ant_wide() and step_kernel() are the two choices left after it. Plain host
// C++: tests/dispatch_grid.cpp prints the decisions without HIP.
#pragma once
#include <stdint.h>

#include "../../include/brax_amd.h"
#include "pbd_features.h"

namespace bx {

struct SingleVariant {
  int L, F, M;
};

// 16 lanes, <= 16 contact rows: the system's features -> the kernel's
inline int single16_feat(int feat) {
  switch (feat) {
    case 0: return 0;
    case F_SPH: return F_SPH;
    case F_G1: return F_G1;
    case F_SPH | F_G1: return F_SPH | F_G1;
    case F_CC | F_TW:
    case F_CC | F_TW | F_G1: return F_CC | F_TW;
    case F_G1 | F_JH: return F_G1 | F_JH;
    case F_JH: return F_JH;
    case F_CC | F_TW | F_JH:
    case F_CC | F_TW | F_G1 | F_JH: return F_CC | F_TW | F_JH;
    default: return F_ALL;
  }
}
// F_R2 systems (17-32 rows at 16 lanes): HalfCheetah (capsule-capsule,
// two-way, joint halves), Fetch (box corners, one group), HumanoidStandup
// (spherical, one group), else every feature
inline int single16_r2_feat(int feat) {
  if (feat & F_C16) {
    if ((feat & ~(F_R2 | F_C16 | F_G1 | F_R2G)) != (F_CC | F_TW | F_JH)) return F_ALL | F_R2 | F_C16;
    return F_CC | F_TW | F_JH | F_R2 | F_C16 | (feat & F_R2G);
  }
  switch (feat & ~F_R2) {
    case F_CC | F_TW | F_JH | F_R2G:
    case F_CC | F_TW | F_G1 | F_JH | F_R2G: return F_CC | F_TW | F_JH | F_R2 | F_R2G;
    case F_CC | F_TW | F_JH:
    case F_CC | F_TW | F_G1 | F_JH: return F_CC | F_TW | F_JH | F_R2;
    case F_G1: return F_G1 | F_R2;
    case F_SPH | F_G1: return F_SPH | F_G1 | F_R2;
    default: return F_ALL | F_R2;
  }
}
// the instantiation of (lanes, system features, gather width)
inline SingleVariant single_variant(int L, int feat, int gw) {
  const int M = gw <= 4 ? 4 : 8;
  if (L == 16 && (feat & F_R2)) return {16, single16_r2_feat(feat), M};
  if (L == 16 && (feat & F_C16)) return {16, F_ALL | F_C16, M};
  if (L == 16) return {16, single16_feat(feat), M};
  if (L == 32) return {32, F_ALL, 8};
  return {64, F_ALL, 8};
}

// every instantiated variant: X(L, F, M, ...) once each
#define BX_SINGLE16_VARIANTS(X, M, ...)                     \
  X(16, 0, M, __VA_ARGS__)                                  \
  X(16, F_SPH, M, __VA_ARGS__)                              \
  X(16, F_G1, M, __VA_ARGS__)                               \
  X(16, F_SPH | F_G1, M, __VA_ARGS__)                       \
  X(16, F_CC | F_TW, M, __VA_ARGS__)                        \
  X(16, F_G1 | F_JH, M, __VA_ARGS__)                        \
  X(16, F_JH, M, __VA_ARGS__)                               \
  X(16, F_CC | F_TW | F_JH, M, __VA_ARGS__)                 \
  X(16, F_ALL, M, __VA_ARGS__)                              \
  X(16, F_ALL | F_C16, M, __VA_ARGS__)                      \
  X(16, F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G, M, __VA_ARGS__) \
  X(16, F_CC | F_TW | F_JH | F_R2 | F_C16, M, __VA_ARGS__)  \
  X(16, F_ALL | F_R2 | F_C16, M, __VA_ARGS__)               \
  X(16, F_CC | F_TW | F_JH | F_R2 | F_R2G, M, __VA_ARGS__)  \
  X(16, F_CC | F_TW | F_JH | F_R2, M, __VA_ARGS__)          \
  X(16, F_G1 | F_R2, M, __VA_ARGS__)                        \
  X(16, F_SPH | F_G1 | F_R2, M, __VA_ARGS__)                \
  X(16, F_ALL | F_R2, M, __VA_ARGS__)
#define BX_SINGLE_VARIANTS(X, ...)         \
  BX_SINGLE16_VARIANTS(X, 4, __VA_ARGS__)  \
  BX_SINGLE16_VARIANTS(X, 8, __VA_ARGS__)  \
  X(32, F_ALL, 8, __VA_ARGS__)             \
  X(64, F_ALL, 8, __VA_ARGS__)

// a variant as a switch label (F < 4096, M <= 8)
constexpr int single_key(int L, int F, int M) { return (L << 16) | (F << 4) | M; }

// ---------------------------------------------------------------------------
// the env kinds' own kernels
// ---------------------------------------------------------------------------
// what bx_blob.cpp's plan allows the env kernels (the launchers' `fold`):
// FOLD_DAMPING = every joint j has torque actuator j, so the kind kernels fold
// each joint's damping into its actuator's slot (no kind kernel without it);
// FOLD_BODY_COPIES = the joint-halves kernels may give each side lane its
// body's copy; FOLD_CONTACT_ON_BODY = the system's rows allow the Ant kernels'
// contacts on the body lanes (cb_feat)
enum { FOLD_DAMPING = 1, FOLD_BODY_COPIES = 2, FOLD_CONTACT_ON_BODY = 4 };
constexpr int fold_bits(bool damping, bool body_copies, bool contact_on_body) {
  return damping ? (FOLD_DAMPING | (body_copies ? FOLD_BODY_COPIES : 0) |
                    (contact_on_body ? FOLD_CONTACT_ON_BODY : 0))
                 : 0;
}

// the kind kernels' feature masks. HalfCheetah: 16 one-way ground rows in slot
// 1, the feet's capsule-capsule row in slot 2 (F_R2 | F_R2G), joint halves.
// Pusher: 16 one-way plane rows in slot 1, 7 two-way capsule-capsule rows as
// contact halves in slot 2, 16-entry contact lists, joint halves (no body
// copies: F_C16). HumanoidStandup: the Humanoid system lying down, 22 ground
// rows (F_R2)
enum {
  F_ENV_ANT = F_G1 | F_JH,
  F_ENV_HUM = F_SPH | F_G1,
  F_ENV_CHEETAH = F_CC | F_TW | F_JH | F_R2 | F_R2G,
  F_ENV_PUSHER = F_CC | F_TW | F_JH | F_R2 | F_C16 | F_R2G,
  F_ENV_STANDUP = F_SPH | F_G1 | F_R2
};
// every kind kernel (16 lanes): X(F, M, EK, ...) once each
#define BX_KIND_VARIANTS(X, ...)             \
  X(F_ENV_ANT, 4, EK_ANT, __VA_ARGS__)       \
  X(F_ENV_HUM, 4, EK_HUM, __VA_ARGS__)       \
  X(F_ENV_CHEETAH, 4, EK_CHEETAH, __VA_ARGS__) \
  X(F_ENV_PUSHER, 4, EK_PUSHER, __VA_ARGS__) \
  X(F_ENV_PUSHER, 8, EK_PUSHER, __VA_ARGS__) \
  X(F_ENV_STANDUP, 8, EK_HUM, __VA_ARGS__)

// the env launch units. The policy, eval-policy and population units have no
// EK_HUM kernels (check_draw refuses those kinds on the host); a Humanoid
// system that reached them would take the variant list
enum EnvFamily { FAM_STEP, FAM_POLICY, FAM_EVAL_POLICY, FAM_EVAL_OPEN, FAM_POPULATION };
constexpr bool family_has(EnvFamily fam, int EK) {
  return EK != EK_HUM || fam == FAM_STEP || fam == FAM_EVAL_OPEN;
}

struct KindVariant {
  int F, M, EK;  // EK_ANY: no kind kernel, the variant list's (single_variant)
};
constexpr int kind_key(int F, int M, int EK) { return (EK << 16) | (F << 4) | M; }

// the kind kernel of (lanes, system features, gather width, env kind, fold
// bits) in the family, or EK_ANY. An Ant-kind system whose rows do not allow
// the contacts on the body lanes takes the variant list's all-kinds kernel
inline KindVariant kind_variant(EnvFamily fam, int L, int feat, int gw, int kind, int fold) {
  const KindVariant none{0, 0, EK_ANY};
  if (!fold || L != 16) return none;
  const bool jb = (fold & FOLD_BODY_COPIES) != 0, cb = (fold & FOLD_CONTACT_ON_BODY) != 0;
  const bool hum = (kind == BX_ENV_HUMANOID || kind == BX_ENV_HUMANOID_STANDUP) && family_has(fam, EK_HUM);
  const int M = gw <= 4 ? 4 : 8;
  if (kind == BX_ENV_ANT && feat == F_ENV_ANT && M == 4 && jb && (cb || !cb_feat(F_ENV_ANT)))
    return {F_ENV_ANT, 4, EK_ANT};
  if (hum && feat == F_ENV_HUM && M == 4) return {F_ENV_HUM, 4, EK_HUM};
  if (kind == BX_ENV_HALFCHEETAH && (feat & ~F_G1) == F_ENV_CHEETAH && M == 4 && jb)
    return {F_ENV_CHEETAH, 4, EK_CHEETAH};
  if (kind == BX_ENV_PUSHER && (feat & ~F_G1) == F_ENV_PUSHER) return {F_ENV_PUSHER, M, EK_PUSHER};
  if (hum && feat == F_ENV_STANDUP) return {F_ENV_STANDUP, 8, EK_HUM};
  return none;
}

// the Ant kernels past one wave per SIMD take their register-capped "wide"
// twins (amdgpu_waves_per_eu(2)): tpb threads per workgroup on cus compute units
inline bool ant_wide(int64_t workgroups, int tpb, int cus) {
  return workgroups * (tpb / 64 > 0 ? tpb / 64 : 1) > 4 * (int64_t)cus;
}

// FAM_STEP's kernels (pbd_single.hip) and its choice among them for a launch
// of n_steps steps, packed outputs or not: the kind kernels run K-step
// launches under the rollout name, except the lying-down HumanoidStandup's;
// a packed single step takes the one-step packed kernel, whose first loads
// need no header (at a wide Ant batch: the wide rollout kernel)
enum StepKernel { K_STEP, K_STEP_PACKED, K_ROLLOUT, K_STEP_WIDE, K_ROLLOUT_WIDE };
constexpr bool has_rollout_kernel(int F, int EK) { return EK != EK_ANY && F != F_ENV_STANDUP; }
inline StepKernel step_kernel(KindVariant v, bool wide, int n_steps, bool packed) {
  if (v.EK == EK_ANT && wide) return (n_steps > 1 || packed) ? K_ROLLOUT_WIDE : K_STEP_WIDE;
  if (has_rollout_kernel(v.F, v.EK) && n_steps > 1) return K_ROLLOUT;
  return packed && n_steps <= 1 ? K_STEP_PACKED : K_STEP;
}

}  // namespace bx
