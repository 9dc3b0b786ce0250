// sac_head_kernels.hip — the SAC loss heads (include/brax_amd.h bx_sac_head_*):
// everything of a SAC gradient step between the networks, in FOUR launches.
// train_kernels.hip's flags: IEEE float32, no finite-math assumptions and no
// contraction. It includes none of the other units' headers.
//
//   prep             an element per lane (strided): the three critic inputs'
//                    observation columns, (obs - mean) / std as two float32
//                    operations (losses.normalize's bits), and X_cur's actions
//   sample           a row per lane, a job per blockIdx.y: tanh(raw) and the
//                    row's NormalTanh log-prob
//   losses           a row per lane: the Bellman target, the critics' errors,
//                    the minimal critic, the rows' gradients; each workgroup
//                    leaves its rows' three sums as doubles
//   sample_backward  a row per lane: the sample's closed-form backward into
//                    dlogits; one more workgroup sums the losses launch's
//                    partials into losses[3] and dlog_alpha
//
// Every cross-row sum is float64: a butterfly over the wave's lanes, the
// workgroup's 4 waves in wave order, the workgroups' partials lane-strided in
// ascending order. Its order is a function of B alone. No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sac_head_launch.h"

namespace bx {

namespace {

constexpr float LOG_2 = 0.69314718055994530942f;
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;
constexpr int WAVES = SAC_HEAD_BLOCK / 64;

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

}  // namespace

__global__ void __launch_bounds__(SAC_HEAD_BLOCK) sac_head_prep_kernel(SacPrepArgs P) {
#pragma clang fp contract(off)
  const int64_t W = P.O + P.A, N = P.B * W;
  const int64_t step = (int64_t)gridDim.x * SAC_HEAD_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * SAC_HEAD_BLOCK + threadIdx.x; i < N; i += step) {
    const int64_t row = i / W, col = i % W;
    if (col < P.O) {
      float o = P.obs[row * P.obs_pitch + col], n = P.next_obs[row * P.next_obs_pitch + col];
      if (P.mean) {
        const float m = P.mean[col], s = P.std[col];
        o = (o - m) / s;
        n = (n - m) / s;
      }
      P.x_cur[row * P.x_pitch + col] = o;
      P.x_pi[row * P.x_pitch + col] = o;
      P.x_next[row * P.x_pitch + col] = n;
    } else {
      P.x_cur[row * P.x_pitch + col] = P.action[row * P.action_pitch + (col - P.O)];
    }
  }
}

__global__ void __launch_bounds__(SAC_HEAD_BLOCK) sac_head_sample_kernel(SacSampleArgs S) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * SAC_HEAD_BLOCK + threadIdx.x;
  if (row >= S.B) return;
  const bx_sac_sample_job& J = S.job[blockIdx.y];
  const float* __restrict__ lg = J.logits + row * J.logits_pitch;
  const float* __restrict__ ep = J.eps + row * J.eps_pitch;
  float* __restrict__ act = J.action ? J.action + row * J.action_pitch : nullptr;
  double lp = 0.0;
  for (int64_t a = 0; a < S.A; ++a) {
    const float loc = lg[a];
    const float scale = softplus(lg[S.A + a]) + S.min_std;
    const float raw = loc + scale * ep[a];
    const float z = (raw - loc) / scale;
    lp += (double)(((((-0.5f * z) * z) - HALF_LOG_2PI) - logf(scale)) - tanh_log_det(raw));
    if (act) act[a] = tanhf(raw);
  }
  J.log_prob[row] = (float)lp;
}

__global__ void __launch_bounds__(SAC_HEAD_BLOCK) sac_head_losses_kernel(SacLossesArgs L) {
#pragma clang fp contract(off)
  __shared__ double lds[WAVES];
  const int64_t row = (int64_t)blockIdx.x * SAC_HEAD_BLOCK + threadIdx.x;
  double sum_c = 0.0, sum_p = 0.0, sum_a = 0.0;
  if (row < L.B) {
    const float alpha = expf(*L.log_alpha);
    const float inv_b = (float)(1.0 / (double)L.B);
    const float inv_bc = (float)(1.0 / ((double)L.B * (double)L.C));
    // torch.min over the critics: a NaN is the result; a tie goes to the lowest c
    float next_min = L.q.next_q[0][row], pi_min = L.q.q_pi[0][row];
    int pi_arg = 0;
    for (int c = 1; c < L.C; ++c) {
      const float n = L.q.next_q[c][row], p = L.q.q_pi[c][row];
      if (next_min == next_min && (n < next_min || n != n)) next_min = n;
      if (pi_min == pi_min && (p < pi_min || p != p)) pi_min = p, pi_arg = c;
    }
    // ---- critic ----
    const float next_v = next_min - alpha * L.lp_next[row];
    const float y = L.reward[row * L.reward_stride] * L.reward_scaling +
                    (L.discount[row * L.discount_stride] * L.discounting) * next_v;
    const float mask = 1.f - L.truncation[row * L.truncation_stride];
    for (int c = 0; c < L.C; ++c) {
      const float e = (L.q.q_old[c][row] - y) * mask;
      sum_c += (double)(e * e);
      L.q.dq_old[c][row] = (e * mask) * inv_bc;
    }
    // ---- actor ----
    sum_p = (double)(alpha * L.lp_pi[row] - pi_min);
    for (int c = 0; c < L.C; ++c) L.q.dq_pi[c][row] = c == pi_arg ? -inv_b : 0.f;
    L.g_lp[row] = alpha * inv_b;
    // ---- alpha ----
    sum_a = (double)(alpha * (-L.lp_alpha[row] - L.target_entropy));
  }
  sum_c = block_sum(sum_c, lds);
  sum_p = block_sum(sum_p, lds);
  sum_a = block_sum(sum_a, lds);
  if (threadIdx.x == 0) {
    double* part = L.part + (int64_t)blockIdx.x * SAC_HEAD_PART;
    part[0] = sum_c;
    part[1] = sum_p;
    part[2] = sum_a;
  }
}

__global__ void __launch_bounds__(SAC_HEAD_BLOCK) sac_head_sample_backward_kernel(SacBackwardArgs K) {
#pragma clang fp contract(off)
  __shared__ double lds[WAVES];
  const int64_t groups = sac_head_groups(K.B);
  if ((int64_t)blockIdx.x == groups) {
    // ---- the losses, from the losses launch's partials ----
    double c = 0.0, p = 0.0, a = 0.0;
    for (int64_t k = threadIdx.x; k < groups; k += SAC_HEAD_BLOCK) {
      c += K.part[k * SAC_HEAD_PART];
      p += K.part[k * SAC_HEAD_PART + 1];
      a += K.part[k * SAC_HEAD_PART + 2];
    }
    c = block_sum(c, lds);
    p = block_sum(p, lds);
    a = block_sum(a, lds);
    if (threadIdx.x == 0) {
      const double n = (double)K.B;
      K.losses[0] = 0.5f * (float)(c / (n * (double)K.C));
      K.losses[1] = (float)(p / n);
      K.losses[2] = (float)(a / n);
      // alpha's derivative in log_alpha is alpha: the loss's own value
      *K.dlog_alpha = K.losses[2];
    }
    return;
  }
  const int64_t row = (int64_t)blockIdx.x * SAC_HEAD_BLOCK + threadIdx.x;
  if (row >= K.B) return;
  const float* __restrict__ lg = K.logits + row * K.logits_pitch;
  const float* __restrict__ ep = K.eps + row * K.eps_pitch;
  float* __restrict__ dl = K.dlogits + row * K.dlogits_pitch;
  const float g = K.g_lp[row];
  for (int64_t a = 0; a < K.A; ++a) {
    const float loc = lg[a], s = lg[K.A + a], eps = ep[a];
    const float scale = softplus(s) + K.min_std;
    const float th = tanhf(loc + scale * eps);
    float da = K.da.ptr[0][row * K.da.pitch[0] + a];
    for (int c = 1; c < K.C; ++c) da += K.da.ptr[c][row * K.da.pitch[c] + a];
    const float u = g * (2.f * th) + da * (1.f - th * th);
    const float d_scale = u * eps - g / scale;
    dl[a] = u;
    dl[K.A + a] = d_scale * softplus_grad(s);
  }
}

hipError_t launch_sac_prep(const SacPrepArgs& a, hipStream_t s) {
  int64_t groups = sac_head_groups(a.B * (a.O + a.A));
  if (groups > SAC_HEAD_PREP_GROUPS) groups = SAC_HEAD_PREP_GROUPS;
  hipLaunchKernelGGL(sac_head_prep_kernel, dim3((unsigned)groups), dim3(SAC_HEAD_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sac_sample(const SacSampleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sac_head_sample_kernel, dim3((unsigned)sac_head_groups(a.B), (unsigned)a.n_jobs),
                     dim3(SAC_HEAD_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sac_losses(const SacLossesArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sac_head_losses_kernel, dim3((unsigned)sac_head_groups(a.B)),
                     dim3(SAC_HEAD_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sac_sample_backward(const SacBackwardArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sac_head_sample_backward_kernel, dim3((unsigned)(sac_head_groups(a.B) + 1)),
                     dim3(SAC_HEAD_BLOCK), 0, s, a);
  return hipGetLastError();
}

}  // namespace bx
