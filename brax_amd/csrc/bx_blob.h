// bx_blob.h — the host blob builder: descriptor -> the device blob's words and
// the kernel plan (mode, lanes, features, LDS). Plain C++17, no HIP: bx_capi_system.cpp
// copies the words to the device and launches by the plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/brax_amd.h"
#include "pbd_features.h"
#include "pbd_layout.h"

namespace bx {

// the builder's A/B knobs (each env variable set to a non-zero integer)
struct PlanKnobs {
  bool no_joint_halves;  // BX_NO_JOINT_HALVES: one lane per joint
  bool no_r2;            // BX_NO_R2: 17-32-row systems stay at 32 lanes
  bool no_multi_jh;      // BX_NO_MULTI_JH: the MULTI kernel without its joint halves
  bool no_jb;            // BX_NO_JB: no body copies (the kinds take the all-kinds kernel)
  bool debug;            // BX_PLAN_DEBUG: print the plan to stderr
};
PlanKnobs plan_knobs_from_env();  // the only getenv calls of the builder

struct Plan {
  BlobHdr hdr{};
  std::vector<uint32_t> words;  // the blob, hdr first
  int L = 16;       // lanes per env
  int min_L = 16;
  int mode = 0;     // MODE_GLOBAL / MODE_SINGLE / MODE_LDS / MODE_MULTI
  int feat = F_ALL;  // the F_* this system uses
  int gw = 8;       // gather width (max per-body list length, 4 or 8)
  int tpb = 64;     // threads per workgroup of the step kernels (multiple of L)
  int fold = 0;     // every joint j has torque actuator j (the Ant / Humanoid env kernels)
  int jb = 0;       // the joint-halves env kernels may own body copies (JB, bx_blob.cpp)
  int cb = 0;       // and may resolve each body's contact row on its lanes (CB, bx_blob.cpp)
  bool single_ok = false;
  bool multi_ok = false;  // MODE_MULTI (3): large pbd scenes, 128 or 256 threads per env
  size_t lds_env = 0;    // bytes per block for the per-env kernels
  size_t lds_reset = 0;  // bytes per block for default_qp
};

// A pure function of (desc, reset, knobs); reset may be null. Returns 0, or 1
// with the reason in *err.
int build_plan(const bx_desc* desc, const bx_reset_desc* reset, const PlanKnobs& knobs,
               Plan* plan, std::string* err);

}  // namespace bx
