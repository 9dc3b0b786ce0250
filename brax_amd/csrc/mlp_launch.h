// mlp_launch.h — the learner MLP kernels' launchers (mlp_kernels.hip), apart
// from pbd_launch.h and train_launch.h so no other unit depends on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brax_amd.h"

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

hipError_t launch_mlp_forward(const MlpNet& net, int64_t rows, const float* x, int64_t x_stride,
                              float* y, float* saved, hipStream_t s);
// launch (i): the reverse chain (dz of the hidden layers to `dz`, dx when not
// null); launch (ii): every wanted dW and db. Each is skipped when it has
// nothing to write.
hipError_t launch_mlp_backward(const MlpNet& net, MlpGrads& grads, int64_t rows, const float* x,
                               int64_t x_stride, const float* saved, const float* dy, float* dx,
                               float* dz, hipStream_t s);

}  // namespace bx
