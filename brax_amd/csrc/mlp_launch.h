// mlp_launch.h — the learner MLP kernels' launchers (mlp_kernels.hip), apart
// from pbd_launch.h and train_launch.h so no other unit depends on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"
#include "../../include/brax_amd_mlp_group.h"

namespace bx {

// rows of one workgroup's tile (the M of v_mfma_f32_32x32x2_f32) and the
// widest activation row the tile's LDS image holds
constexpr int MLP_TILE_ROWS = 32;
constexpr int MLP_TILE_COLS = BX_MLP_MAX_WIDTH;
// the LDS image's row pitch in floats: 16-byte rows, and 4 past a multiple of
// the bank count so the rows' 16-byte reads spread over the banks
constexpr int MLP_LDS_PITCH = MLP_TILE_COLS + 4;
// the gradient launch: waves of one workgroup (each sums its own slice of the
// rows), and the (in, out) tile of dW one workgroup owns
constexpr int MLP_GRAD_WAVES = 8;
constexpr int MLP_GRAD_TILE_IN = 32;
constexpr int MLP_GRAD_TILE_OUT = 64;

// one network as the kernels take it: bx_mlp plus the hidden layers' column
// offsets in the (rows, hidden) arrays `saved` and `dz`
struct MlpNet {
  int32_t n_layers, activation;
  int32_t in[BX_MLP_MAX_LAYERS], out[BX_MLP_MAX_LAYERS];
  int32_t off[BX_MLP_MAX_LAYERS];  // of layer l < n_layers - 1
  int32_t hidden;                  // sum of the hidden layers' widths
  const float* w[BX_MLP_MAX_LAYERS];
  const float* b[BX_MLP_MAX_LAYERS];
};

struct MlpGrads {
  float* dw[BX_MLP_MAX_LAYERS];
  float* db[BX_MLP_MAX_LAYERS];
  // the first workgroup of layer l in the gradient launch's grid, and the total
  int32_t first[BX_MLP_MAX_LAYERS + 1];
};

// The group launches' member tables, carried in the kernel arguments: each
// member is a complete problem of its own. `first` is the members' prefix
// table over the launch's workgroups (the entries past the last member hold
// the total). A member that takes no part in a launch is not in its table.
struct MlpForwardMember {
  MlpNet net;
  int64_t rows;
  const float* x;
  int64_t x_stride;
  float* y;
  float* saved;
};
struct MlpBackwardMember {
  MlpNet net;
  int64_t rows;
  const float* saved;
  const float* dy;
  float* dx;
  float* dz;
  uint32_t vec_mask;
};
struct MlpGradMember {
  MlpNet net;
  MlpGrads grads;
  int64_t rows;
  const float* x;
  int64_t x_stride;
  const float* saved;
  const float* dy;
  const float* dz;
};
struct MlpGroupForward {
  int32_t first[BX_MLP_MAX_GROUP + 1];
  MlpForwardMember m[BX_MLP_MAX_GROUP];
};
struct MlpGroupBackward {
  int32_t first[BX_MLP_MAX_GROUP + 1];
  MlpBackwardMember m[BX_MLP_MAX_GROUP];
};
struct MlpGroupGrad {
  int32_t first[BX_MLP_MAX_GROUP + 1];
  MlpGradMember m[BX_MLP_MAX_GROUP];
};
// HIP's limit on a launch's arguments
static_assert(sizeof(MlpGroupForward) <= 4096, "forward group arguments above 4 KB");
static_assert(sizeof(MlpGroupBackward) <= 4096, "backward group arguments above 4 KB");
static_assert(sizeof(MlpGroupGrad) <= 4096, "gradient group arguments above 4 KB");

hipError_t launch_mlp_forward(const MlpNet& net, int64_t rows, const float* x, int64_t x_stride,
                              float* y, float* saved, hipStream_t s);
// launch (i): the reverse chain (dz of the hidden layers to `dz`, dx when not
// null); launch (ii): every wanted dW and db. Each is skipped when it has
// nothing to write.
hipError_t launch_mlp_backward(const MlpNet& net, MlpGrads& grads, int64_t rows, const float* x,
                               int64_t x_stride, const float* saved, const float* dy, float* dx,
                               float* dz, hipStream_t s);
// The same launches for n <= BX_MLP_MAX_GROUP members at once: one forward
// launch; at most one launch (i) and one launch (ii). A member with rows = 0
// contributes no workgroups, one with a null dy takes no part in the backward
// launches; dx[i] is member i's input gradient or null.
hipError_t launch_mlp_group_forward(const MlpForwardMember* members, int n, hipStream_t s);
hipError_t launch_mlp_group_backward(MlpGradMember* members, float* const* dx, int n,
                                     hipStream_t s);

}  // namespace bx
