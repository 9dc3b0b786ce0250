// mlp_kernels.hip — the learners' MLPs: a whole network forward in one launch
// and backward in two (include/brax_amd.h bx_mlp_forward / bx_mlp_backward).
// Its own translation unit with BASEFLAGS alone (Makefile): IEEE float32, no
// finite-math assumptions, so NaN and Inf propagate as the chained torch form
// has them. It includes none of the step kernels' headers.
//
// Every product runs on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a
// k-ordered fmaf chain, so nothing here is a precision decision). Its
// fragments, lane l = 32 h + c:
//   A: one float, A[row c][k = h];  B: one float, B[k = h][column c]
//   C/D: 16 floats, register r is D[row (r & 3) + 8 (r >> 2) + 4 h][column c]
// A workgroup of the forward and of launch (i) owns MLP_TILE_ROWS = 32 rows:
// the MFMA's whole M. The tile's activations live in ONE LDS image of 32 x
// 260 floats (33,280 B) for the whole launch: a layer's outputs are complete
// in the accumulators before the image is overwritten with them, so no second
// buffer is needed. The four waves split a layer's output columns in tiles of
// 32 (wave w owns tiles w and w + 4), so every weight is read by exactly one
// lane of the workgroup, straight from global memory into the B operand with
// no LDS staging; all workgroups read the same addresses, which L2 serves.
// The K loop walks groups of 8: lane half h takes k = 8 g + 4 h + s in MFMA s
// = 0..3, so a lane reads its four A values as one 16-byte LDS read, and the
// next group's B values are requested before the current group's MFMAs.
// Columns past a layer's width are zero in the image and read as zero from
// the weights (a guard, not a load), so padding contributes exact zeros even
// where the data holds NaN or Inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_launch.h"

namespace bx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TM = MLP_TILE_ROWS;
constexpr int LDW = MLP_LDS_PITCH;
constexpr int GW = MLP_GRAD_WAVES;

// the activation as the chained form computes it (torch: relu is a select
// that lets NaN through, silu is x / (1 + exp(-x)))
__device__ __forceinline__ float act_fwd(int kind, float z) {
  if (kind == BX_POLICY_RELU) return z <= 0.f ? 0.f : z;
  if (kind == BX_POLICY_TANH) return tanhf(z);
  return z / (1.f + expf(-z));
}

// g * act'(z), as torch's backward formulas: relu selects (a NaN g at z <= 0
// gives 0), silu is g * (s * (1 + z * (1 - s))), tanh is g * (1 - t * t)
__device__ __forceinline__ float act_bwd(int kind, float z, float g) {
  if (kind == BX_POLICY_RELU) return z <= 0.f ? 0.f : g;
  if (kind == BX_POLICY_TANH) {
    const float t = tanhf(z);
    return g * (1.f - t * t);
  }
  const float s = 1.f / (1.f + expf(-z));
  return g * (s * (1.f + z * (1.f - s)));
}

__device__ __forceinline__ int round_up8(int n) { return (n + 7) & ~7; }

// The four B values of lane (h, c) for one group: W is (in, out) row-major
// with `ldw` = out. Plain: B[k][j] = W[k][j], k over `in`. TR: B[k][j] =
// W[j][k], k over `out` (the backward chain's dz . W^T); its four k are one
// 16-byte load when `vec` (out a multiple of 4 and W 16-byte aligned).
template <bool TR>
__device__ __forceinline__ f32x4 load_b(const float* __restrict__ W, int ldw, int K, int N, int k,
                                        int j, bool vec) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (j >= N) return b;
  if (TR) {
    const float* p = W + (int64_t)j * ldw + k;
    if (vec) {
      if (k < K) b = *(const f32x4*)p;
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (k + s < K) b[s] = p[s];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (k + s < K) b[s] = W[(int64_t)(k + s) * ldw + j];
  }
  return b;
}

// acc[t] += image[32 x kext] . B[:, tile t] for this wave's two column tiles
// n_base + 32 (wave + 4 t) of an N-column product. `kofs` is the global k of
// the image's column 0 (the first layer walks its input in chunks). No
// barrier inside: a wave without a tile below N returns at once.
template <bool TR>
__device__ __forceinline__ void gemm_tile(f32x16 (&acc)[2], const float* image, int kext,
                                          const float* __restrict__ W, int ldw, int kofs, int K,
                                          int N, int n_base, bool vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int n0 = n_base + 32 * wave, n1 = n0 + 128;
  if (n0 >= N) return;
  const bool on1 = n1 < N;  // wave-uniform
  const float* arow = image + c * LDW + 4 * h;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 b0 = load_b<TR>(W, ldw, K, N, kofs + 4 * h, n0 + c, vec);
  f32x4 b1 = on1 ? load_b<TR>(W, ldw, K, N, kofs + 4 * h, n1 + c, vec) : zero;
  for (int k = 0; k < kext; k += 8) {
    f32x4 nb0 = zero, nb1 = zero;
    if (k + 8 < kext) {
      nb0 = load_b<TR>(W, ldw, K, N, kofs + k + 8 + 4 * h, n0 + c, vec);
      if (on1) nb1 = load_b<TR>(W, ldw, K, N, kofs + k + 8 + 4 * h, n1 + c, vec);
    }
    const f32x4 a = *(const f32x4*)(arow + k);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[s], acc[0], 0, 0, 0);
      if (on1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[s], acc[1], 0, 0, 0);
    }
    b0 = nb0;
    b1 = nb1;
  }
}

// rows row0 .. row0 + 31 of a (rows, width) array with row pitch `pitch` into
// the image's columns 0 .. round_up8(width) - 1, zeros outside the array
__device__ __forceinline__ void fill_image(float* image, const float* __restrict__ src,
                                           int64_t pitch, int64_t row0, int64_t rows, int width) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wp = round_up8(width);
  for (int r = wave * (TM / 4); r < (wave + 1) * (TM / 4); ++r) {
    const bool in_rows = row0 + r < rows;
    for (int col = lane; col < wp; col += 64)
      image[r * LDW + col] = in_rows && col < width ? src[(row0 + r) * pitch + col] : 0.f;
  }
}

__device__ __forceinline__ void clear(f32x16 (&acc)[2]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
}

// ---- forward: every layer of a 32-row tile in one launch ------------------------------------

// (the tile bodies are __device__ functions: the single-network kernels and
// the group kernels below run the same code on a tile, in the same order)
__device__ __forceinline__ void forward_tile(const MlpNet& net, int64_t rows,
                                             const float* __restrict__ x, int64_t x_stride,
                                             float* __restrict__ y, float* __restrict__ saved,
                                             float* image, int64_t row0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int L = net.n_layers, kind = net.activation;
  for (int l = 0; l < L; ++l) {
    const int K = net.in[l], N = net.out[l];
    const float* __restrict__ W = net.w[l];
    f32x16 acc[2];
    clear(acc);
    if (l == 0) {
      // the input may be wider than the image: chunks of 256 columns, the
      // accumulators carried across them
      for (int c0 = 0; c0 < K; c0 += MLP_TILE_COLS) {
        const int kc = K - c0 < MLP_TILE_COLS ? K - c0 : MLP_TILE_COLS;
        if (c0) __syncthreads();  // the previous chunk's reads
        fill_image(image, x + c0, x_stride, row0, rows, kc);
        __syncthreads();
        gemm_tile<false>(acc, image, round_up8(kc), W, N, c0, K, N, 0, false);
      }
    } else {
      gemm_tile<false>(acc, image, round_up8(K), W, N, 0, K, N, 0, false);
    }
    __syncthreads();  // every wave has read the layer's input
    const bool last = l + 1 == L;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n0 = 32 * (wave + 4 * t);
      if (n0 >= N) continue;
      const int col = n0 + c;
      const bool in_cols = col < N;
      const float bias = in_cols ? net.b[l][col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float z = acc[t][r] + bias;
        const bool live = in_cols && row0 + row < rows;
        if (last) {
          if (live) y[(row0 + row) * N + col] = z;
        } else {
          if (live && saved) saved[(row0 + row) * net.hidden + net.off[l] + col] = z;
          image[row * LDW + col] = in_cols ? act_fwd(kind, z) : 0.f;
        }
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) mlp_forward_kernel(MlpNet net, int64_t rows,
                                                          const float* __restrict__ x,
                                                          int64_t x_stride, float* __restrict__ y,
                                                          float* __restrict__ saved) {
  __shared__ __attribute__((aligned(16))) float image[TM * LDW];
  forward_tile(net, rows, x, x_stride, y, saved, image, (int64_t)blockIdx.x * TM);
}

// A group launch: workgroup b belongs to the member m with first[m] <= b <
// first[m + 1] (the walk mlp_grad_kernel does over its layers) and is that
// member's tile b - first[m]. The member table travels in the kernel
// arguments.
__global__ void __launch_bounds__(256) mlp_group_forward_kernel(MlpGroupForward g) {
  __shared__ __attribute__((aligned(16))) float image[TM * LDW];
  int m = 0;
  while ((int)blockIdx.x >= g.first[m + 1]) ++m;
  const MlpForwardMember& M = g.m[m];
  forward_tile(M.net, M.rows, M.x, M.x_stride, M.y, M.saved, image,
               (int64_t)((int)blockIdx.x - g.first[m]) * TM);
}

// ---- backward (i): the reverse chain of a 32-row tile ----------------------------------------
// The image holds dz_l (dy for the last layer). g = dz_l . W_l^T is the
// gradient of layer l - 1's activations; dz_{l-1} = g * act'(z_{l-1}) goes to
// the workspace (rows, hidden) for launch (ii) and back into the image. With
// `dx` the chain ends in dz_0 . W_0^T, 256 columns of the input at a time.

__device__ __forceinline__ void backward_tile(const MlpNet& net, int64_t rows,
                                              const float* __restrict__ saved,
                                              const float* __restrict__ dy, float* __restrict__ dx,
                                              float* __restrict__ dz, uint32_t vec_mask,
                                              float* image, int64_t row0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int L = net.n_layers, kind = net.activation;
  fill_image(image, dy, net.out[L - 1], row0, rows, net.out[L - 1]);
  __syncthreads();
  for (int l = L - 1; l >= 1; --l) {
    const int K = net.out[l], N = net.in[l];
    f32x16 acc[2];
    clear(acc);
    gemm_tile<true>(acc, image, round_up8(K), net.w[l], K, 0, K, N, 0, (vec_mask >> l) & 1);
    __syncthreads();  // every wave has read dz_l
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n0 = 32 * (wave + 4 * t);
      if (n0 >= N) continue;
      const int col = n0 + c;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool live = col < N && row0 + row < rows;
        float d = 0.f;
        if (live) {
          const int64_t at = (row0 + row) * net.hidden + net.off[l - 1] + col;
          d = act_bwd(kind, saved[at], acc[t][r]);
          dz[at] = d;
        }
        image[row * LDW + col] = d;
      }
    }
    __syncthreads();
  }
  if (!dx) return;
  const int K = net.out[0], N = net.in[0];
  for (int nb = 0; nb < N; nb += MLP_TILE_COLS) {
    f32x16 acc[2];
    clear(acc);
    gemm_tile<true>(acc, image, round_up8(K), net.w[0], K, 0, K, N, nb, vec_mask & 1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = nb + 32 * (wave + 4 * t) + c;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row0 + row < rows) dx[(row0 + row) * N + col] = acc[t][r];
      }
    }
  }
}

__global__ void __launch_bounds__(256) mlp_backward_kernel(MlpNet net, int64_t rows,
                                                           const float* __restrict__ saved,
                                                           const float* __restrict__ dy,
                                                           float* __restrict__ dx,
                                                           float* __restrict__ dz, uint32_t vec_mask) {
  __shared__ __attribute__((aligned(16))) float image[TM * LDW];
  backward_tile(net, rows, saved, dy, dx, dz, vec_mask, image, (int64_t)blockIdx.x * TM);
}

__global__ void __launch_bounds__(256) mlp_group_backward_kernel(MlpGroupBackward g) {
  __shared__ __attribute__((aligned(16))) float image[TM * LDW];
  int m = 0;
  while ((int)blockIdx.x >= g.first[m + 1]) ++m;
  const MlpBackwardMember& M = g.m[m];
  backward_tile(M.net, M.rows, M.saved, M.dy, M.dx, M.dz, M.vec_mask, image,
                (int64_t)((int)blockIdx.x - g.first[m]) * TM);
}

// ---- backward (ii): every layer's dW and db in one grouped launch ----------------------------
// A workgroup owns one (32 in, 64 out) tile of one layer's dW = a^T . dz, the
// sum running over the rows. Its 8 waves each sum one contiguous slice of the
// rows (the rows are the MFMA's k: lane half h takes row r0 + h), reading a
// (recomputed from the saved pre-activations, or x for layer 0) and dz
// straight from global memory, consecutive lanes on consecutive columns. The
// 8 partial tiles are then summed through LDS in wave order, and db (the
// column sums of the dz values the lanes already hold) likewise in the
// workgroups of the first in-tile. No floating-point atomics: the order of
// every sum depends on (rows, shapes) alone.

// (`block` is the workgroup's index among the network's own)
__device__ __forceinline__ void grad_tile(const MlpNet& net, const MlpGrads& G, int64_t rows,
                                          const float* __restrict__ x, int64_t x_stride,
                                          const float* __restrict__ saved,
                                          const float* __restrict__ dy,
                                          const float* __restrict__ dz, float* red, int block) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int L = net.n_layers, kind = net.activation;
  int l = 0;
  while (block >= G.first[l + 1]) ++l;
  const int K = net.in[l], N = net.out[l];
  const int n_out_tiles = (N + MLP_GRAD_TILE_OUT - 1) / MLP_GRAD_TILE_OUT;
  const int tile = block - G.first[l];
  const int mt = tile / n_out_tiles, nt = tile % n_out_tiles;
  float* __restrict__ dw = G.dw[l];
  float* __restrict__ db = mt == 0 ? G.db[l] : nullptr;
  const float* __restrict__ A = l == 0 ? x : saved + net.off[l - 1];
  const int64_t a_pitch = l == 0 ? x_stride : net.hidden;
  const bool a_act = l != 0;
  const float* __restrict__ B = l == L - 1 ? dy : dz + net.off[l];
  const int64_t b_pitch = l == L - 1 ? N : net.hidden;
  const int i = MLP_GRAD_TILE_IN * mt + c;
  const int j0 = MLP_GRAD_TILE_OUT * nt + c, j1 = j0 + 32;
  const bool on_a = dw && i < K, on0 = j0 < N, on1 = j1 < N;
  const bool tile1 = MLP_GRAD_TILE_OUT * nt + 32 < N;  // workgroup-uniform
  // the waves' row slices: an even number of rows each
  const int64_t slice = (((rows + GW - 1) / GW) + 1) & ~(int64_t)1;
  const int64_t lo = wave * slice;
  const int64_t hi = lo + slice < rows ? lo + slice : rows;
  f32x16 acc[2];
  clear(acc);
  float bs0 = 0.f, bs1 = 0.f;
  // 4 k-steps (8 rows) a trip: their 12 loads are issued before the first use
  for (int64_t r0 = lo; r0 < hi; r0 += 8) {
    float a[4], b0[4], b1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = r0 + 2 * u + h;
      const bool in_rows = r < hi;
      a[u] = on_a && in_rows ? A[r * a_pitch + i] : 0.f;
      b0[u] = on0 && in_rows ? B[r * b_pitch + j0] : 0.f;
      b1[u] = on1 && in_rows ? B[r * b_pitch + j1] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // (a zero outside the array stays a zero: act(0) is 0 for all three)
      if (a_act) a[u] = act_fwd(kind, a[u]);
      if (dw) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b0[u], acc[0], 0, 0, 0);
        if (tile1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b1[u], acc[1], 0, 0, 0);
      }
      bs0 += b0[u];
      bs1 += b1[u];
    }
  }
  if (dw) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t == 1 && !tile1) break;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[t][r];
      __syncthreads();
      // wave v sums registers 2 v and 2 v + 1 of the 8 partial tiles
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int r = 2 * wave + q;
        float sum = red[r * 64 + lane];
        for (int w = 1; w < GW; ++w) sum += red[(w * 16 + r) * 64 + lane];
        const int row = MLP_GRAD_TILE_IN * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int col = MLP_GRAD_TILE_OUT * nt + 32 * t + c;
        if (row < K && col < N) dw[(int64_t)row * N + col] = sum;
      }
    }
  }
  if (db) {
    __syncthreads();
    red[(wave * 2 + 0) * 64 + lane] = bs0;
    red[(wave * 2 + 1) * 64 + lane] = bs1;
    __syncthreads();
    if (threadIdx.x < 64) {
      const int t = lane >> 5;
      float sum = 0.f;
      for (int w = 0; w < GW; ++w) {
        const float part = red[(w * 2 + t) * 64 + c] + red[(w * 2 + t) * 64 + 32 + c];
        sum = w == 0 ? part : sum + part;
      }
      const int col = MLP_GRAD_TILE_OUT * nt + 32 * t + c;
      if (col < N) db[col] = sum;
    }
  }
}

__global__ void __launch_bounds__(64 * GW) mlp_grad_kernel(MlpNet net, MlpGrads G, int64_t rows,
                                                           const float* __restrict__ x,
                                                           int64_t x_stride,
                                                           const float* __restrict__ saved,
                                                           const float* __restrict__ dy,
                                                           const float* __restrict__ dz) {
  __shared__ float red[GW * 16 * 64];
  grad_tile(net, G, rows, x, x_stride, saved, dy, dz, red, (int)blockIdx.x);
}

__global__ void __launch_bounds__(64 * GW) mlp_group_grad_kernel(MlpGroupGrad g) {
  __shared__ float red[GW * 16 * 64];
  int m = 0;
  while ((int)blockIdx.x >= g.first[m + 1]) ++m;
  const MlpGradMember& M = g.m[m];
  grad_tile(M.net, M.grads, M.rows, M.x, M.x_stride, M.saved, M.dy, M.dz, red,
            (int)blockIdx.x - g.first[m]);
}

}  // namespace

hipError_t launch_mlp_forward(const MlpNet& net, int64_t rows, const float* x, int64_t x_stride,
                              float* y, float* saved, hipStream_t s) {
  dim3 grid((unsigned)((rows + TM - 1) / TM));
  hipLaunchKernelGGL(mlp_forward_kernel, grid, dim3(256), 0, s, net, rows, x, x_stride, y, saved);
  return hipGetLastError();
}

namespace {

// launch (ii)'s plan for one network: G.first, and the workgroups it takes;
// *hidden_grads when a hidden layer's gradient is wanted (launch (i) must run)
int plan_grads(const MlpNet& net, MlpGrads& G, bool* hidden_grads) {
  const int L = net.n_layers;
  int total = 0;
  *hidden_grads = false;
  for (int l = 0; l < L; ++l) {
    G.first[l] = total;
    if (!G.dw[l] && !G.db[l]) continue;
    if (l + 1 < L) *hidden_grads = true;
    const int in_tiles = G.dw[l] ? (net.in[l] + MLP_GRAD_TILE_IN - 1) / MLP_GRAD_TILE_IN : 1;
    total += in_tiles * ((net.out[l] + MLP_GRAD_TILE_OUT - 1) / MLP_GRAD_TILE_OUT);
  }
  for (int l = L; l <= BX_MLP_MAX_LAYERS; ++l) G.first[l] = total;
  return total;
}

// which layers' transposed weight rows take 16-byte loads
uint32_t vec_layers(const MlpNet& net) {
  uint32_t vec_mask = 0;
  for (int l = 0; l < net.n_layers; ++l)
    if (net.out[l] % 4 == 0 && ((uintptr_t)net.w[l] & 15) == 0) vec_mask |= 1u << l;
  return vec_mask;
}

int row_tiles(int64_t rows) { return (int)((rows + TM - 1) / TM); }

}  // namespace

hipError_t launch_mlp_backward(const MlpNet& net, MlpGrads& G, int64_t rows, const float* x,
                               int64_t x_stride, const float* saved, const float* dy, float* dx,
                               float* dz, hipStream_t s) {
  bool hidden_grads = false;
  const int total = plan_grads(net, G, &hidden_grads);
  if (dx || hidden_grads) {
    hipLaunchKernelGGL(mlp_backward_kernel, dim3((unsigned)row_tiles(rows)), dim3(256), 0, s, net,
                       rows, saved, dy, dx, dz, vec_layers(net));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (total) {
    hipLaunchKernelGGL(mlp_grad_kernel, dim3((unsigned)total), dim3(64 * GW), 0, s, net, G, rows, x,
                       x_stride, saved, dy, dz);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_mlp_group_forward(const MlpForwardMember* members, int n, hipStream_t s) {
  MlpGroupForward g{};
  int total = 0, k = 0;
  for (int i = 0; i < n; ++i) {
    if (members[i].rows == 0) continue;
    g.first[k] = total;
    g.m[k++] = members[i];
    total += row_tiles(members[i].rows);
  }
  for (int i = k; i <= BX_MLP_MAX_GROUP; ++i) g.first[i] = total;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(mlp_group_forward_kernel, dim3((unsigned)total), dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_mlp_group_backward(MlpGradMember* members, float* const* dx, int n,
                                     hipStream_t s) {
  MlpGroupBackward b{};
  MlpGroupGrad g{};
  int chain_total = 0, grad_total = 0, kb = 0, kg = 0;
  for (int i = 0; i < n; ++i) {
    MlpGradMember& M = members[i];
    if (M.rows == 0 || !M.dy) continue;
    bool hidden_grads = false;
    const int tiles = plan_grads(M.net, M.grads, &hidden_grads);
    if (dx[i] || hidden_grads) {
      b.first[kb] = chain_total;
      MlpBackwardMember& B = b.m[kb++];
      B.net = M.net;
      B.rows = M.rows;
      B.saved = M.saved;
      B.dy = M.dy;
      B.dx = dx[i];
      B.dz = const_cast<float*>(M.dz);
      B.vec_mask = vec_layers(M.net);
      chain_total += row_tiles(M.rows);
    }
    if (tiles) {
      g.first[kg] = grad_total;
      g.m[kg++] = M;
      grad_total += tiles;
    }
  }
  for (int i = kb; i <= BX_MLP_MAX_GROUP; ++i) b.first[i] = chain_total;
  for (int i = kg; i <= BX_MLP_MAX_GROUP; ++i) g.first[i] = grad_total;
  if (chain_total) {
    hipLaunchKernelGGL(mlp_group_backward_kernel, dim3((unsigned)chain_total), dim3(256), 0, s, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (grad_total) {
    hipLaunchKernelGGL(mlp_group_grad_kernel, dim3((unsigned)grad_total), dim3(64 * GW), 0, s, g);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace bx
