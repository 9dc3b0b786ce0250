// ppo_head_kernels.hip — the PPO loss head (include/brax_amd.h bx_ppo_head):
// everything of `ppo_loss` between the networks' outputs and the scalar loss,
// with its gradients in logits and baseline, in TWO launches. train_kernels.hip's
// flags: IEEE float32, no finite-math assumptions and no contraction. It
// includes none of the other units' headers; the GAE recurrence is restated.
//
// Launch 1 has two kinds of workgroup. A scan workgroup gives each lane one env
// and runs compute_gae_kernel's chain over it (the same operations in the same
// order: the same bits), leaves the advantages in the workspace, writes
// dbaseline, and leaves its advantages' (count, mean, centred square sum) and
// its squared value errors' sum. A row workgroup gives each lane one (t, env)
// row, sums the row's log-prob and entropy over the actions, leaves rho in the
// workspace and its rows' entropy sum.
//
// Launch 2: every workgroup first combines the scan workgroups' moments into the
// advantages' mean and standard deviation (Chan's pairwise update, not the
// one-pass sum of squares). Workgroup 0 then sums the surrogate over all rows
// and the partials of launch 1 into losses[4]; workgroup 1 + k writes the
// dlogits of rows 256 k .. 256 k + 255, an action at a time.
//
// Every cross-row sum is float64, lane-strided in ascending order, then a
// butterfly over the wave's lanes and the workgroup's 4 waves in wave order:
// its order is a function of (T, B, A) alone. No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppo_head_launch.h"

namespace bx {

namespace {

constexpr float LOG_2 = 0.69314718055994530942f;
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;
constexpr int WAVES = PPO_HEAD_BLOCK / 64;

// the sum of `v` over the workgroup, the same value in every lane; every lane
// of the workgroup calls it
__device__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();  // (the previous call's reads of lds)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = lds[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s += lds[w];
  return s;
}

// torch's softplus (beta 1, threshold 20) and its derivative
__device__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ float softplus_grad(float x) {
  if (x > 20.f) return 1.f;
  const float e = expf(x);
  return e / (e + 1.f);
}
// brax_amd/envs/policy.py tanh_log_det
__device__ float tanh_log_det(float x) { return 2.f * ((LOG_2 - x) - softplus(-2.f * x)); }

// torch.minimum: a NaN on either side is the result
__device__ float minimum(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? a : b;
}

// The advantages' mean and the divisor std + 1e-8 from the scan workgroups'
// moments; (0, 1) without normalisation. Every lane of the workgroup calls it.
__device__ void advantage_moments(const PpoHeadArgs& A, double* lds, float* mean, float* divisor) {
  if (!A.normalize) {
    *mean = 0.f;
    *divisor = 1.f;
    return;
  }
  const double n = (double)A.T * (double)A.B;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < A.scan_groups; k += PPO_HEAD_BLOCK)
    s += A.scan_part[k * PPO_HEAD_SCAN_PART] * A.scan_part[k * PPO_HEAD_SCAN_PART + 1];
  const double m = block_sum(s, lds) / n;
  double q = 0.0;
  for (int64_t k = threadIdx.x; k < A.scan_groups; k += PPO_HEAD_BLOCK) {
    const double d = A.scan_part[k * PPO_HEAD_SCAN_PART + 1] - m;
    q += A.scan_part[k * PPO_HEAD_SCAN_PART + 2] + A.scan_part[k * PPO_HEAD_SCAN_PART] * (d * d);
  }
  const double var = block_sum(q, lds) / n;
  *mean = (float)m;
  *divisor = (float)sqrt(var) + 1e-8f;
}

// one row's surrogate term min(rho A, clamp(rho) A) and, in *weight, the
// factor of A in its derivative in rho as autograd's minimum and clamp give
// it (a tie of the minimum gives each side a half; the clamp passes a
// gradient on the closed interval)
__device__ float surrogate(float rho, float adv, float lo, float hi, float* weight) {
  const float clamped = rho < lo ? lo : (rho > hi ? hi : rho);
  const float s1 = rho * adv, s2 = clamped * adv;
  const float w1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
  const float w2 = s2 < s1 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
  *weight = w1 + ((rho >= lo && rho <= hi) ? w2 : 0.f);
  return minimum(s1, s2);
}

}  // namespace

__global__ void __launch_bounds__(PPO_HEAD_BLOCK) ppo_head_forward_kernel(PpoHeadArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[WAVES];
  const int64_t N = A.T * A.B;
  if ((int64_t)blockIdx.x < A.scan_groups) {
    // ---- a scan workgroup: one lane per env ----
    const int64_t e = (int64_t)blockIdx.x * PPO_HEAD_BLOCK + threadIdx.x;
    const bool valid = e < A.B;
    double sum_a = 0.0, sum_v = 0.0;
    if (valid) {
      const float* __restrict__ rw = A.reward.ptr + e * A.reward.env_stride;
      const float* __restrict__ dn = A.done.ptr + e * A.done.env_stride;
      const float* __restrict__ tr = A.truncation.ptr + e * A.truncation.env_stride;
      const float* __restrict__ va = A.baseline.ptr + e * A.baseline.env_stride;
      // the outputs' step T - 1; each walks down a step at a time
      float* vs = A.vs.ptr ? A.vs.ptr + e * A.vs.env_stride + (A.T - 1) * A.vs.time_stride : nullptr;
      float* ad = A.adv.ptr ? A.adv.ptr + e * A.adv.env_stride + (A.T - 1) * A.adv.time_stride
                            : nullptr;
      float* db = A.dbaseline.ptr + e * A.dbaseline.env_stride + (A.T - 1) * A.dbaseline.time_stride;
      float* wa = A.w_adv + (A.T - 1) * A.B + e;
      const int64_t rw_t = A.reward.time_stride, dn_t = A.done.time_stride,
                    tr_t = A.truncation.time_stride, va_t = A.baseline.time_stride;
      const float scale = A.reward_scaling, discount = A.discount, lambda = A.lambda;
      const float db_coef = (float)(-0.5 / (double)N);
      float v_next = A.bootstrap[e];
      float vs_next = v_next;
      float acc = 0.f;
      // compute_gae_kernel's loop: steps hi - 1 .. hi - CHUNK of each chunk;
      // slots below step 0 load step 0 again (in bounds) and are not computed
      for (int64_t hi = A.T; hi > 0; hi -= PPO_HEAD_CHUNK) {
        float r_[PPO_HEAD_CHUNK], d_[PPO_HEAD_CHUNK], t_[PPO_HEAD_CHUNK], v_[PPO_HEAD_CHUNK];
#pragma unroll
        for (int i = 0; i < PPO_HEAD_CHUNK; ++i) {
          const int64_t t = hi - 1 - i < 0 ? 0 : hi - 1 - i;
          r_[i] = rw[t * rw_t];
          d_[i] = dn[t * dn_t];
          t_[i] = tr[t * tr_t];
          v_[i] = va[t * va_t];
        }
#pragma unroll
        for (int i = 0; i < PPO_HEAD_CHUNK; ++i) {
          const int64_t t = hi - 1 - i;
          if (t < 0) break;
          const float v = v_[i];
          const float r = r_[i] * scale;
          const float mask = 1.f - t_[i];
          const float term = d_[i] * mask;
          const float g = discount * (1.f - term);
          const float delta = ((r + g * v_next) - v) * mask;
          acc = delta + ((g * mask) * lambda) * acc;
          const float vs_t_ = acc + v;
          const float adv = ((r + g * vs_next) - v) * mask;
          if (vs) *vs = vs_t_, vs -= A.vs.time_stride;
          if (ad) *ad = adv, ad -= A.adv.time_stride;
          *wa = adv, wa -= A.B;
          const float v_error = vs_t_ - v;
          *db = v_error * db_coef, db -= A.dbaseline.time_stride;
          sum_a += (double)adv;
          sum_v += (double)(v_error * v_error);
          v_next = v;
          vs_next = vs_t_;
        }
      }
    }
    const int64_t first = (int64_t)blockIdx.x * PPO_HEAD_BLOCK;
    const int64_t envs = A.B - first < PPO_HEAD_BLOCK ? A.B - first : PPO_HEAD_BLOCK;
    const double n = (double)A.T * (double)envs;
    const double mean = block_sum(sum_a, lds) / n;
    double m2 = 0.0;
    if (valid)  // (this lane's own stores)
      for (int64_t t = 0; t < A.T; ++t) {
        const double d = (double)A.w_adv[t * A.B + e] - mean;
        m2 += d * d;
      }
    m2 = block_sum(m2, lds);
    sum_v = block_sum(sum_v, lds);
    if (threadIdx.x == 0) {
      double* part = A.scan_part + (int64_t)blockIdx.x * PPO_HEAD_SCAN_PART;
      part[0] = n;
      part[1] = mean;
      part[2] = m2;
      part[3] = sum_v;
    }
    return;
  }
  // ---- a row workgroup: one lane per (t, env) ----
  const int64_t group = (int64_t)blockIdx.x - A.scan_groups;
  const int64_t i = group * PPO_HEAD_BLOCK + threadIdx.x;
  double row_h = 0.0;
  if (i < N) {
    const int64_t t = i / A.B, e = i % A.B;
    const float* __restrict__ lg = A.logits.ptr + t * A.logits.time_stride + e * A.logits.env_stride;
    const float* __restrict__ rw = A.raw.ptr + t * A.raw.time_stride + e * A.raw.env_stride;
    const float* __restrict__ ep = A.eps.ptr + t * A.eps.time_stride + e * A.eps.env_stride;
    double lp = 0.0, h = 0.0;
    for (int64_t a = 0; a < A.A; ++a) {
      const float loc = lg[a], raw = rw[a];
      const float scale = softplus(lg[A.A + a]) + A.min_std;
      const float log_scale = logf(scale);
      const float z = (raw - loc) / scale;
      lp += (double)(((((-0.5f * z) * z) - HALF_LOG_2PI) - log_scale) - tanh_log_det(raw));
      h += (double)((0.5f + (HALF_LOG_2PI + log_scale)) + tanh_log_det(loc + scale * ep[a]));
    }
    const float old = A.log_prob.ptr[t * A.log_prob.time_stride + e * A.log_prob.env_stride];
    A.w_rho[i] = expf((float)lp - old);
    row_h = (double)(float)h;
  }
  row_h = block_sum(row_h, lds);
  if (threadIdx.x == 0) A.row_part[group] = row_h;
}

__global__ void __launch_bounds__(PPO_HEAD_BLOCK) ppo_head_backward_kernel(PpoHeadArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[WAVES];
  const int64_t N = A.T * A.B;
  float mean, divisor;
  advantage_moments(A, lds, &mean, &divisor);
  if (blockIdx.x == 0) {
    // ---- the losses ----
    double p = 0.0, h = 0.0, v = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += PPO_HEAD_BLOCK) {
      float w;
      p += (double)surrogate(A.w_rho[i], (A.w_adv[i] - mean) / divisor, A.clip_lo, A.clip_hi, &w);
    }
    for (int64_t k = threadIdx.x; k < A.row_groups; k += PPO_HEAD_BLOCK) h += A.row_part[k];
    for (int64_t k = threadIdx.x; k < A.scan_groups; k += PPO_HEAD_BLOCK)
      v += A.scan_part[k * PPO_HEAD_SCAN_PART + 3];
    p = block_sum(p, lds);
    h = block_sum(h, lds);
    v = block_sum(v, lds);
    if (threadIdx.x == 0) {
      const double n = (double)N;
      const float policy_loss = -(float)(p / n);
      const float v_loss = ((float)(v / n) * 0.5f) * 0.5f;
      const float entropy_loss = A.entropy_cost * -(float)(h / n);
      A.losses[0] = (policy_loss + v_loss) + entropy_loss;
      A.losses[1] = policy_loss;
      A.losses[2] = v_loss;
      A.losses[3] = entropy_loss;
    }
    return;
  }
  // ---- the rows' gradients ----
  const int64_t i = ((int64_t)blockIdx.x - 1) * PPO_HEAD_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int64_t t = i / A.B, e = i % A.B;
  const float inv_n = (float)(1.0 / (double)N);
  const float rho = A.w_rho[i];
  const float adv = (A.w_adv[i] - mean) / divisor;
  float weight;
  surrogate(rho, adv, A.clip_lo, A.clip_hi, &weight);
  // d loss / d log-prob and d loss / d entropy of this row
  const float c_lp = -inv_n * ((adv * weight) * rho);
  const float c_h = -(A.entropy_cost * inv_n);
  const float* __restrict__ lg = A.logits.ptr + t * A.logits.time_stride + e * A.logits.env_stride;
  const float* __restrict__ rw = A.raw.ptr + t * A.raw.time_stride + e * A.raw.env_stride;
  const float* __restrict__ ep = A.eps.ptr + t * A.eps.time_stride + e * A.eps.env_stride;
  float* __restrict__ dl = A.dlogits.ptr + t * A.dlogits.time_stride + e * A.dlogits.env_stride;
  for (int64_t a = 0; a < A.A; ++a) {
    const float loc = lg[a], s = lg[A.A + a], eps = ep[a];
    const float scale = softplus(s) + A.min_std;
    const float z = (rw[a] - loc) / scale;
    const float th = tanhf(loc + scale * eps);
    const float d_loc = c_lp * (z / scale) + c_h * (-2.f * th);
    const float d_scale = c_lp * ((z * z - 1.f) / scale) + c_h * (1.f / scale - (2.f * eps) * th);
    dl[a] = d_loc;
    dl[A.A + a] = d_scale * softplus_grad(s);
  }
}

hipError_t launch_ppo_head(const PpoHeadArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ppo_head_forward_kernel, dim3((unsigned)(a.scan_groups + a.row_groups)),
                     dim3(PPO_HEAD_BLOCK), 0, s, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(ppo_head_backward_kernel, dim3((unsigned)(1 + a.row_groups)),
                     dim3(PPO_HEAD_BLOCK), 0, s, a);
  return hipGetLastError();
}

}  // namespace bx
