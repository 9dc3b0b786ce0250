// pbd_dispatch.h — which SINGLE-mode kernel instantiation a system runs.
//
// single_variant() is the decision, BX_SINGLE_VARIANTS the list of (lanes,
// features, gather width) that exist. The launchers' switches are generated
// from the list (pbd_single.hip), so a variant cannot be selected without
// being instantiated; the host asks the same function which kernel a system
// gets (single_kernel_feat: bx_capi.cpp sizes the staged limit rows by it).
// Single mode at 16 lanes is specialised per feature set and gather width.
#pragma once
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

}  // namespace bx
