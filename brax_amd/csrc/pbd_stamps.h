// pbd_stamps.h — in-kernel phase stamps (diagnostic builds only).
//
// A stamp reads the wave's clock between two scheduling barriers and adds the
// time since the previous stamp to an accumulator slot. Four families, each
// keeping its slot meanings (tools/stamps.py, pstamps.py, mstamps.py,
// wave_spread.py):
//   -DBX_STAMPS   BX_STAMP(0..9): pbd_step_single's phases; BX_KSTAMP(10..14):
//                 the env step kernel's parts; with -DBX_PSTAMPS its prologue
//                 too (BX_PSTAMP(5..9), the pbd phases then not written);
//                 with -DBX_OSTAMPS the observation's parts (BX_OST(5..9))
//   -DBX_MSTAMPS  BX_MSTAMP(0..14): pbd_step_multi's phases, of which
//                 BX_NSTAMP(12..14) are the NearNeighbors picks' parts
//   -DBX_PHASE_MARKS  the SINGLE stamp points as assembly comments
//                 (tools/phase_mix.py), no timing
// Each family exists in one translation unit only: the SINGLE-mode unit
// (BX_TU_FAST) has BX_STAMPS / BX_PSTAMPS / BX_OSTAMPS, the item-loop unit
// (BX_TU_GENERIC) has BX_MSTAMPS. In the default build every stamp expands to
// nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#if !defined(BX_TU_FAST)
#undef BX_STAMPS
#endif
#if !defined(BX_TU_GENERIC)
#undef BX_MSTAMPS
#endif

// the one stamp: _d = the clock's advance since `last`, handed to `use`
#define BX_STAMP_START(last) \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(last)::"memory")
#define BX_STAMP_BODY(last, use)                                                   \
  do {                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                             \
    unsigned long long _t;                                                         \
    BX_STAMP_START(_t);                                                            \
    __builtin_amdgcn_sched_barrier(0);                                             \
    const unsigned long long _d = _t - (last);                                     \
    (last) = _t;                                                                   \
    use;                                                                           \
  } while (0)
#define BX_NO_STAMP do {} while (0)

namespace bx {

#ifdef BX_STAMPS
// per-workgroup accumulators (no atomics: contended atomics inside the timed
// windows distort them); summed on the host by debug_stamps
__device__ unsigned long long bx_stamp_wave[4096][16];
#define BX_STAMP(k) BX_STAMP_BODY(st_last, st_acc[k] += _d)
// kernel-level stamps (env_step_kernel): slots 10..14; with BX_PSTAMPS the
// prologue's parts too (slots 5..9, BX_KSTAMP(5..9); the pbd phases' slots
// 0..9 are then not written)
#define BX_KSTAMP_DECL                                                             \
  unsigned long long kst_last, kst_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};       \
  BX_STAMP_START(kst_last);
#define BX_KSTAMP(k)                                                               \
  BX_STAMP_BODY(kst_last, kst_acc[(k) - 5] += _d;                                  \
                if ((k) == 14 && threadIdx.x == 0)                                 \
                  for (int _i = BX_KSLOT0; _i < 10; _i++)                          \
                    bx_stamp_wave[blockIdx.x & 4095][5 + _i] += kst_acc[_i])
#if defined(BX_PSTAMPS)
#define BX_KSLOT0 0
#define BX_PSTAMP(k) BX_KSTAMP(k)
#else
#define BX_KSLOT0 5
#define BX_PSTAMP(k) BX_NO_STAMP
#endif
#elif defined(BX_PHASE_MARKS)
// static per-phase instruction mix (diagnostic, tools/phase_mix.py): the
// stamp points as assembly comments the scheduler does not move code across
#define BX_STAMP(k)                                                                \
  do {                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                             \
    asm volatile(";BXPHASE " #k ::: "memory");                                     \
    __builtin_amdgcn_sched_barrier(0);                                             \
  } while (0)
#define BX_KSTAMP_DECL
#define BX_KSTAMP(k) BX_STAMP(k)
#define BX_PSTAMP(k) BX_NO_STAMP
#else
#define BX_STAMP(k) BX_NO_STAMP
#define BX_KSTAMP_DECL
#define BX_KSTAMP(k) BX_NO_STAMP
#define BX_PSTAMP(k) BX_NO_STAMP
#endif

#if defined(BX_OSTAMPS) && defined(BX_TU_FAST)
// (diagnostic: the observation's parts into stamp slots 5..9)
#define BX_OST_DECL                                                                \
  unsigned long long ost_last;                                                     \
  BX_STAMP_START(ost_last);
#define BX_OST(k) \
  BX_STAMP_BODY(ost_last, if (threadIdx.x == 0) bx_stamp_wave[blockIdx.x & 4095][k] += _d)
#else
#define BX_OST_DECL
#define BX_OST(k) BX_NO_STAMP
#endif

#ifdef BX_MSTAMPS
// MULTI-mode phase stamps of each workgroup's first wave (diagnostic build)
__device__ unsigned long long bx_mstamp_wave[4096][16];
#define BX_MSTAMP(k) BX_STAMP_BODY(ms_last, ms_acc[k] += _d)
// (the MULTI stamps build splits the picks' phases into slots 12-14 of the
// caller's accumulators)
#define BX_NSTAMP(k)                                                               \
  do {                                                                             \
    if (nsa) BX_STAMP_BODY(*nsl, nsa[k] += _d);                                    \
  } while (0)
#else
#define BX_MSTAMP(k) BX_NO_STAMP
#define BX_NSTAMP(k) BX_NO_STAMP
#endif

#if defined(BX_STAMPS) || defined(BX_MSTAMPS)
// debug_stamps / debug_mstamps: a family's per-workgroup sums read back. out
// gets the 16 slots summed over the workgroups, or with raw the 4096 x 16
// sums themselves; reset zeroes the device accumulators
static hipError_t stamps_readback(const void* sym, unsigned long long* out, int reset, bool raw) {
  static unsigned long long host[4096][16];
  hipError_t e = hipMemcpyFromSymbol(host, sym, sizeof(host));
  if (raw) {
    memcpy(out, host, sizeof(host));
    return e;
  }
  for (int k = 0; k < 16; k++) {
    out[k] = 0;
    for (int w = 0; w < 4096; w++) out[k] += host[w][k];
  }
  if (e == hipSuccess && reset) {
    memset(host, 0, sizeof(host));
    e = hipMemcpyToSymbol(sym, host, sizeof(host));
  }
  return e;
}
#endif

}  // namespace bx
