// bx_capi_learn.cpp — the C ABI's learner side (include/brax_amd.h): the RNG
// slabs, GAE, the evolution agents' perturbation and update, the replay queue,
// the MLPs, the PPO and SAC loss heads and the optimiser step, none on a system
#include <algorithm>
#include <initializer_list>
#include <string>

#include "bx_capi_common.h"
#include "mlp_launch.h"
#include "optim_launch.h"
#include "pbd_launch.h"  // (the slab and evolution launchers)
#include "ppo_head_launch.h"
#include "replay_launch.h"
#include "sac_head_launch.h"
#include "train_launch.h"

using namespace bx;

namespace {

// the slab entry points' sizes and output: false when the call is over, with
// its result in *rc (an empty draw, whose output may be null, or a refusal)
bool slabs_to_draw(const float* out, int64_t slab_n, int64_t n_slabs, int* rc) {
  *rc = 0;
  if (slab_n < 0 || n_slabs < 0) *rc = fail("negative size");
  else if (slab_n == 0 || n_slabs == 0) return false;
  else if (slab_n > INT64_MAX / n_slabs || slab_n * n_slabs > ((int64_t)1 << 40))
    *rc = fail("too many elements for one draw");
  else if (!out) *rc = fail("null output");
  return *rc == 0;
}

// (a zero stride on an input broadcasts one row or column; on an output every
// step or env would write the same element); null outputs are skipped
int check_out_strides(std::initializer_list<const bx_seq*> outs, int64_t n_steps, int64_t n_envs) {
  for (const bx_seq* o : outs)
    if (o->ptr && ((n_steps > 1 && o->time_stride == 0) || (n_envs > 1 && o->env_stride == 0)))
      return fail("zero stride on an output");
  return 0;
}

// the workspace protocol: a null workspace asks for the size (true: written);
// one given must hold `need` bytes at an `align`-byte address
bool size_query(const void* workspace, int64_t* bytes, int64_t need) {
  if (!workspace) *bytes = need;
  return !workspace;
}
int check_workspace(const void* workspace, int64_t bytes, int64_t need, int align) {
  if (bytes < need)
    return fail("workspace of " + std::to_string(bytes) + " bytes, " + std::to_string(need) + " needed");
  if ((uintptr_t)workspace & (uintptr_t)(align - 1))
    return fail("workspace not " + std::to_string(align) + "-byte aligned");
  return 0;
}

// the checks bx_replay_insert and bx_replay_sample share, and the kernels'
// field table: prefix offsets, and each field's pointer moved back by its
// offset so a row word indexes it directly
int replay_args(const float* data, int64_t capacity, int64_t row_words, int64_t position,
                int64_t n, const bx_fields* f, ReplayArgs* a) {
  if (!data || !f) return fail("null argument");
  if (f->n_fields < 0 || f->n_fields > BX_FIELDS_MAX)
    return fail("n_fields " + std::to_string(f->n_fields) + " outside 0.." +
                std::to_string(BX_FIELDS_MAX));
  if (capacity < 1) return fail("capacity must be >= 1");
  if (row_words < 0 || row_words > (1 << 24)) return fail("row_words outside 0..2^24");
  if (capacity > ((int64_t)1 << 40) / (row_words ? row_words : 1)) return fail("ring too large");
  if (position < 0 || position >= capacity) return fail("position outside the ring");
  int64_t total = 0;
  for (int k = 0; k < f->n_fields; ++k) {
    if (f->width[k] < 0 || f->width[k] > (1 << 24)) return fail("field width outside 0..2^24");
    total += f->width[k];
  }
  if (total != row_words)
    return fail("field widths sum to " + std::to_string(total) + ", row_words is " +
                std::to_string(row_words));
  int64_t sum = 0;
  for (int k = 0; k < f->n_fields; ++k) {
    if (!f->ptr[k]) return fail("null field pointer");
    a->off[k] = (int32_t)sum;
    a->base[k] = (float*)((uintptr_t)f->ptr[k] - (uintptr_t)sum * sizeof(float));
    a->stride[k] = f->row_stride[k];
    sum += f->width[k];
  }
  for (int k = f->n_fields; k < BX_FIELDS_MAX; ++k) {  // selected by no word
    a->off[k] = (int32_t)row_words;
    a->base[k] = nullptr;
    a->stride[k] = 0;
  }
  a->data = const_cast<float*>(data);
  a->capacity = capacity;
  a->position = position;
  a->row_words = (int32_t)row_words;
  a->n = n;
  return 0;
}

// the checks bx_mlp_forward and bx_mlp_backward share, and the kernels' form
// of the network (the hidden layers' column offsets in `saved` and `dz`)
int mlp_args(const bx_mlp* net, int64_t rows, int64_t x_stride, MlpNet* m) {
  if (!net) return fail("null argument");
  if (net->n_layers < 1 || net->n_layers > BX_MLP_MAX_LAYERS)
    return fail("n_layers " + std::to_string(net->n_layers) + " outside 1.." +
                std::to_string(BX_MLP_MAX_LAYERS));
  if (!activation_ok(net->activation))
    return fail("unknown activation " + std::to_string(net->activation));
  if (rows < 0) return fail("negative rows");
  if (rows > ((int64_t)1 << 31)) return fail("too many rows for one launch");
  m->n_layers = net->n_layers;
  m->activation = net->activation;
  int hidden = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    const int in = net->in[l], out = net->out[l];
    if (out < 1 || out > BX_MLP_MAX_WIDTH)
      return fail("layer " + std::to_string(l) + ": width " + std::to_string(out) +
                  " outside 1.." + std::to_string(BX_MLP_MAX_WIDTH));
    if (l == 0 && (in < 1 || in > BX_MLP_MAX_IN))
      return fail("input width " + std::to_string(in) + " outside 1.." +
                  std::to_string(BX_MLP_MAX_IN));
    if (l > 0 && in != net->out[l - 1])
      return fail("layer " + std::to_string(l) + ": in " + std::to_string(in) +
                  " != the previous out " + std::to_string(net->out[l - 1]));
    if (!net->w[l] || !net->b[l]) return fail("null weight or bias");
    m->in[l] = in;
    m->out[l] = out;
    m->w[l] = net->w[l];
    m->b[l] = net->b[l];
    m->off[l] = hidden;
    if (l + 1 < net->n_layers) hidden += out;
  }
  m->hidden = hidden;
  if (x_stride < net->in[0])
    return fail("x_stride " + std::to_string(x_stride) + " below the input width " +
                std::to_string(net->in[0]));
  return 0;
}

// what bx_mlp_forward refuses after mlp_args (rows > 0), and bx_mlp_backward
// likewise: the single and the group entry points make the same checks
int mlp_forward_ptrs(const float* x, const float* y) {
  if (!x || !y) return fail("null argument");
  return 0;
}
int64_t mlp_workspace_need(const MlpNet& m, int64_t rows) {
  return std::max<int64_t>(16, 4 * rows * (int64_t)m.hidden);
}
int mlp_backward_ptrs(const MlpNet& m, const float* x, const float* saved, const float* dy,
                      const void* workspace, int64_t bytes, int64_t need) {
  if (!x || !dy) return fail("null argument");
  if (m.n_layers > 1 && !saved) return fail("null saved with hidden layers");
  return check_workspace(workspace, bytes, need, 16);
}
void mlp_grads(const MlpNet& m, const bx_mlp_grads* grads, MlpGrads* g) {
  if (grads)
    for (int l = 0; l < m.n_layers; ++l) {
      g->dw[l] = grads->dw[l];
      g->db[l] = grads->db[l];
    }
}

// a group's members: the count, and the last refusal as member i's
int mlp_group_count(const bx_mlp_member* members, int32_t n_members) {
  if (!members) return fail("null argument");
  if (n_members < 1 || n_members > BX_MLP_MAX_GROUP)
    return fail("n_members " + std::to_string(n_members) + " outside 1.." +
                std::to_string(BX_MLP_MAX_GROUP));
  return 0;
}
int member_fail(int i) {
  return fail("member " + std::to_string(i) + ": " + std::string(bx_last_error()));
}
// the arrays a group launch writes: no two members may name the same one (a
// member has at most dx, its workspace and a dw and a db per layer)
struct MlpWritten {
  struct Entry { const void* p; int member; const char* what; };
  Entry entries[BX_MLP_MAX_GROUP * (2 + 2 * BX_MLP_MAX_LAYERS)];
  int n = 0;
  int add(const void* p, int member, const char* what) {
    if (!p) return 0;
    for (int k = 0; k < n; ++k)
      if (entries[k].p == p && entries[k].member != member)
        return fail("members " + std::to_string(entries[k].member) + " and " +
                    std::to_string(member) + " write the same array (" + entries[k].what + ", " +
                    what + ")");
    entries[n++] = {p, member, what};
    return 0;
  }
};

// the SAC heads' shared checks: the row count, then the action count
int sac_rows(int64_t n_rows) {
  if (n_rows < 0) return fail("negative n_rows");
  if (n_rows > ((int64_t)1 << 31)) return fail("too many rows for one launch");
  return 0;
}
int sac_actions(int64_t n_actions) {
  if (n_actions < 1) return fail("n_actions must be >= 1");
  if (n_actions > ((int64_t)1 << 20)) return fail("too many actions");
  return 0;
}
int sac_critics(int32_t n_critics) {
  if (n_critics < 1 || n_critics > BX_SAC_MAX_CRITICS)
    return fail("n_critics " + std::to_string(n_critics) + " outside 1.." +
                std::to_string(BX_SAC_MAX_CRITICS));
  return 0;
}
int sac_pitch(const char* name, int64_t pitch, int64_t width) {
  if (pitch < width)
    return fail(std::string(name) + " " + std::to_string(pitch) + " below the row width " +
                std::to_string(width));
  return 0;
}

}  // namespace

extern "C" {

int bx_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, float lo, float hi, void* stream) {
  return bx_uniform_slabs(out, n, 1, seed, offset, 0, nullptr, 0, lo, hi, stream);
}

int bx_uniform_epoch(float* out, int64_t n, uint64_t seed, uint64_t offset, const int64_t* epoch,
                     uint64_t epoch_stride, float lo, float hi, void* stream) {
  if (!epoch && n > 0) return fail("null epoch counter");
  return bx_uniform_slabs(out, n, 1, seed, offset, 0, epoch, epoch_stride, lo, hi, stream);
}

int bx_uniform_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed, uint64_t offset,
                     uint64_t slab_stride, const int64_t* epoch, uint64_t epoch_stride, float lo,
                     float hi, void* stream) {
  int rc = 0;
  if (!slabs_to_draw(out, slab_n, n_slabs, &rc)) return rc;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_uniform_slabs(out, slab_n, n_slabs, seed, offset, slab_stride, epoch, epoch_stride,
                              lo, hi, st));
  return 0;
}

int bx_normal_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed, uint64_t offset,
                    uint64_t slab_stride, const int64_t* epoch, uint64_t epoch_stride, void* stream) {
  int rc = 0;
  if (!slabs_to_draw(out, slab_n, n_slabs, &rc)) return rc;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_normal_slabs(out, slab_n, n_slabs, seed, offset, slab_stride, epoch, epoch_stride, st));
  return 0;
}

int bx_compute_gae(int64_t n_steps, int64_t n_envs, const bx_seq* reward, const bx_seq* done,
                   const bx_seq* truncation, const bx_seq* values, const float* bootstrap,
                   const bx_seq* vs, const bx_seq* advantages, float reward_scaling, float discount,
                   float lambda, void* stream) {
  if (!reward || !done || !truncation || !values || !vs || !advantages) return fail("null argument");
  if (n_steps < 1) return fail("n_steps must be >= 1");
  if (n_envs < 0) return fail("negative n_envs");
  if (n_envs > ((int64_t)1 << 31)) return fail("too many envs for one launch");
  if (n_envs == 0) return 0;
  if (!reward->ptr || !done->ptr || !truncation->ptr || !values->ptr || !bootstrap || !vs->ptr ||
      !advantages->ptr)
    return fail("null argument");
  if (check_out_strides({vs, advantages}, n_steps, n_envs)) return 1;
  STREAM_SCOPE(stream, st);
  GaeArgs a{};
  a.T = n_steps;
  a.B = n_envs;
  a.reward = *reward;
  a.done = *done;
  a.truncation = *truncation;
  a.values = *values;
  a.vs = *vs;
  a.adv = *advantages;
  a.bootstrap = bootstrap;
  a.reward_scaling = reward_scaling;
  a.discount = discount;
  a.lambda = lambda;
  HIP_OK(launch_compute_gae(a, st));
  return 0;
}

int bx_population_perturb(float* rows, const float* theta, int64_t n_directions, int64_t n_params,
                          int64_t stride, double sigma, uint64_t seed, uint64_t offset,
                          int antithetic, const uint8_t* frozen, void* stream) {
  if (!rows || !theta) return fail("null argument");
  if (n_directions < 1) return fail("n_directions must be >= 1");
  if (n_params < 1) return fail("n_params must be >= 1");
  if (stride < n_params) return fail("stride below n_params");
  if (n_params > ((int64_t)1 << 40) / n_directions) return fail("too many samples for one launch");
  if (stride > ((int64_t)1 << 41) / n_directions) return fail("stride too large");
  const int64_t members = antithetic ? 2 * n_directions : n_directions;
  const uintptr_t r0 = (uintptr_t)rows, r1 = r0 + (size_t)((members - 1) * stride + n_params) * 4;
  const uintptr_t t0 = (uintptr_t)theta, t1 = t0 + (size_t)n_params * 4;
  if (r0 < t1 && t0 < r1) return fail("rows overlap theta");
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_population_perturb(rows, theta, frozen, n_directions, n_params, stride, sigma, seed,
                                   offset, antithetic ? 1 : 0, st));
  return 0;
}

int bx_population_delta(float* out, const float* weights, int64_t n_directions, int64_t n_params,
                        uint64_t seed, uint64_t offset, const uint8_t* frozen, void* workspace,
                        int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (n_directions < 1) return fail("n_directions must be >= 1");
  if (n_params < 1) return fail("n_params must be >= 1");
  if (n_params > ((int64_t)1 << 40) / n_directions) return fail("too many samples for one launch");
  const int64_t chunks = (n_directions + BX_POPULATION_DELTA_CHUNK - 1) / BX_POPULATION_DELTA_CHUNK;
  const int64_t need = chunks * n_params * (int64_t)sizeof(double);
  if (size_query(workspace, workspace_bytes, need)) return 0;
  if (!out || !weights) return fail("null argument");
  if (check_workspace(workspace, *workspace_bytes, need, 8)) return 1;
  if (chunks > 65535) return fail("too many directions for one launch");
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_population_delta(out, weights, frozen, n_directions, n_params, seed, offset,
                                 (double*)workspace, st));
  return 0;
}

int bx_replay_insert(float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t n_rows, const bx_fields* src, void* stream) {
  if (n_rows < 0) return fail("negative n_rows");
  if (n_rows == 0) return 0;
  ReplayArgs a{};
  if (replay_args(data, capacity, row_words, position, n_rows, src, &a)) return 1;
  if (n_rows > capacity)
    return fail("n_rows " + std::to_string(n_rows) + " above the capacity " +
                std::to_string(capacity));
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_replay_insert(a, st));
  return 0;
}

int bx_replay_sample(const float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t size, int64_t n_samples, uint64_t seed, uint64_t offset,
                     const bx_fields* dst, int64_t* idx_out, void* stream) {
  if (n_samples < 0) return fail("negative n_samples");
  if (n_samples == 0) return 0;
  ReplayArgs a{};
  if (replay_args(data, capacity, row_words, position, n_samples, dst, &a)) return 1;
  if (size < 1 || size > capacity)
    return fail("size " + std::to_string(size) + " outside 1.." + std::to_string(capacity));
  a.size = size;
  a.seed = seed;
  a.offset = offset;
  a.idx_out = idx_out;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_replay_sample(a, st));
  return 0;
}

int bx_mlp_sizes(int32_t* mlp_bytes, int32_t* grads_bytes) {
  if (!mlp_bytes || !grads_bytes) return fail("null argument");
  *mlp_bytes = (int32_t)sizeof(bx_mlp);
  *grads_bytes = (int32_t)sizeof(bx_mlp_grads);
  return 0;
}

int bx_mlp_forward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride, float* y,
                   float* saved, void* stream) {
  MlpNet m{};
  if (mlp_args(net, rows, x_stride, &m)) return 1;
  if (rows == 0) return 0;
  if (mlp_forward_ptrs(x, y)) return 1;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_mlp_forward(m, rows, x, x_stride, y, saved, st));
  return 0;
}

int bx_mlp_backward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride,
                    const float* saved, const float* dy, float* dx, const bx_mlp_grads* grads,
                    void* workspace, int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  MlpNet m{};
  if (mlp_args(net, rows, x_stride, &m)) return 1;
  const int64_t need = mlp_workspace_need(m, rows);
  if (size_query(workspace, workspace_bytes, need)) return 0;
  if (rows == 0) return 0;
  if (mlp_backward_ptrs(m, x, saved, dy, workspace, *workspace_bytes, need)) return 1;
  MlpGrads g{};
  mlp_grads(m, grads, &g);
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_mlp_backward(m, g, rows, x, x_stride, saved, dy, dx, (float*)workspace, st));
  return 0;
}

int bx_mlp_group_sizes(int32_t* member_bytes) {
  if (!member_bytes) return fail("null argument");
  *member_bytes = (int32_t)sizeof(bx_mlp_member);
  return 0;
}

int bx_mlp_group_forward(const bx_mlp_member* members, int32_t n_members, void* stream) {
  if (mlp_group_count(members, n_members)) return 1;
  MlpForwardMember table[BX_MLP_MAX_GROUP] = {};
  MlpWritten written;
  int n = 0;
  for (int i = 0; i < n_members; ++i) {
    const bx_mlp_member& s = members[i];
    MlpForwardMember& d = table[n];
    if (mlp_args(s.net, s.rows, s.x_stride, &d.net)) return member_fail(i);
    if (s.rows == 0) continue;
    if (mlp_forward_ptrs(s.x, s.y)) return member_fail(i);
    if (written.add(s.y, i, "y") || written.add(s.saved, i, "saved")) return 1;
    d.rows = s.rows;
    d.x = s.x;
    d.x_stride = s.x_stride;
    d.y = s.y;
    d.saved = s.saved;
    ++n;
  }
  if (n == 0) return 0;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_mlp_group_forward(table, n, st));
  return 0;
}

int bx_mlp_group_backward(bx_mlp_member* members, int32_t n_members, int32_t query, void* stream) {
  if (mlp_group_count(members, n_members)) return 1;
  MlpGradMember table[BX_MLP_MAX_GROUP] = {};
  float* dx[BX_MLP_MAX_GROUP] = {};
  MlpWritten written;
  int n = 0;
  for (int i = 0; i < n_members; ++i) {
    bx_mlp_member& s = members[i];
    MlpGradMember& d = table[n];
    d = MlpGradMember{};
    if (mlp_args(s.net, s.rows, s.x_stride, &d.net)) return member_fail(i);
    const int64_t need = mlp_workspace_need(d.net, s.rows);
    if (query) {
      s.workspace_bytes = need;
      continue;
    }
    if (s.rows == 0 || !s.dy) continue;
    if (mlp_backward_ptrs(d.net, s.x, s.saved, s.dy, s.workspace, s.workspace_bytes, need))
      return member_fail(i);
    mlp_grads(d.net, s.grads, &d.grads);
    if (written.add(s.dx, i, "dx") || written.add(s.workspace, i, "workspace")) return 1;
    for (int l = 0; l < d.net.n_layers; ++l)
      if (written.add(d.grads.dw[l], i, "dw") || written.add(d.grads.db[l], i, "db")) return 1;
    d.rows = s.rows;
    d.x = s.x;
    d.x_stride = s.x_stride;
    d.saved = s.saved;
    d.dy = s.dy;
    d.dz = (const float*)s.workspace;
    dx[n] = s.dx;
    ++n;
  }
  if (n == 0) return 0;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_mlp_group_backward(table, dx, n, st));
  return 0;
}

int bx_ppo_head(int64_t n_steps, int64_t n_envs, int64_t n_actions, const bx_seq* logits,
                const bx_seq* baseline, const float* bootstrap, const bx_seq* raw_action,
                const bx_seq* eps, const bx_seq* log_prob, const bx_seq* reward,
                const bx_seq* done, const bx_seq* truncation, float reward_scaling, float discount,
                float lambda, double clipping_epsilon, float entropy_cost, float min_std,
                int normalize_advantage, float* losses, const bx_seq* dlogits,
                const bx_seq* dbaseline, const bx_seq* vs, const bx_seq* advantages,
                void* workspace, int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (n_steps < 1) return fail("n_steps must be >= 1");
  if (n_actions < 1) return fail("n_actions must be >= 1");
  if (n_envs < 0) return fail("negative n_envs");
  if (n_actions > ((int64_t)1 << 20)) return fail("too many actions");
  if (n_steps > ((int64_t)1 << 31) || n_envs > ((int64_t)1 << 31) ||
      n_steps * n_envs > ((int64_t)1 << 31))
    return fail("too many rows for one launch");
  const int64_t need = ppo_head_workspace_bytes(n_steps, n_envs);
  if (size_query(workspace, workspace_bytes, need)) return 0;
  if (n_envs == 0) return 0;
  const bx_seq* in[] = {logits, baseline, raw_action, eps, log_prob, reward, done, truncation};
  for (const bx_seq* q : in)
    if (!q || !q->ptr) return fail("null argument");
  if (!bootstrap || !losses || !dlogits || !dlogits->ptr || !dbaseline || !dbaseline->ptr)
    return fail("null argument");
  const bx_seq none{nullptr, 0, 0};
  if (!vs) vs = &none;
  if (!advantages) advantages = &none;
  if (check_out_strides({dlogits, dbaseline, vs, advantages}, n_steps, n_envs)) return 1;
  if (check_workspace(workspace, *workspace_bytes, need, 16)) return 1;
  STREAM_SCOPE(stream, st);
  PpoHeadArgs a{};
  a.T = n_steps;
  a.B = n_envs;
  a.A = n_actions;
  a.logits = *logits;
  a.baseline = *baseline;
  a.raw = *raw_action;
  a.eps = *eps;
  a.log_prob = *log_prob;
  a.reward = *reward;
  a.done = *done;
  a.truncation = *truncation;
  a.bootstrap = bootstrap;
  a.reward_scaling = reward_scaling;
  a.discount = discount;
  a.lambda = lambda;
  a.clip_lo = (float)(1.0 - clipping_epsilon);
  a.clip_hi = (float)(1.0 + clipping_epsilon);
  a.entropy_cost = entropy_cost;
  a.min_std = min_std;
  a.normalize = normalize_advantage != 0;
  a.losses = losses;
  a.dlogits = *dlogits;
  a.dbaseline = *dbaseline;
  a.vs = *vs;
  a.adv = *advantages;
  ppo_head_carve(a, workspace);
  HIP_OK(launch_ppo_head(a, st));
  return 0;
}

int bx_sac_head_prep(int64_t n_rows, int64_t n_obs, int64_t n_actions, const float* obs,
                     int64_t obs_pitch, const float* next_obs, int64_t next_obs_pitch,
                     const float* action, int64_t action_pitch, const float* mean,
                     const float* std, float* x_cur, float* x_next, float* x_pi, int64_t x_pitch,
                     void* stream) {
  if (sac_rows(n_rows)) return 1;
  if (n_obs < 1) return fail("n_obs must be >= 1");
  if (n_obs > ((int64_t)1 << 20)) return fail("too many observations");
  if (sac_actions(n_actions)) return 1;
  if (n_rows == 0) return 0;
  if (!obs || !next_obs || !action || !x_cur || !x_next || !x_pi) return fail("null argument");
  if (!mean != !std) return fail("one of mean and std is null");
  if (sac_pitch("obs_pitch", obs_pitch, n_obs) || sac_pitch("next_obs_pitch", next_obs_pitch, n_obs) ||
      sac_pitch("action_pitch", action_pitch, n_actions) ||
      sac_pitch("x_pitch", x_pitch, n_obs + n_actions))
    return 1;
  STREAM_SCOPE(stream, st);
  SacPrepArgs a{};
  a.B = n_rows;
  a.O = n_obs;
  a.A = n_actions;
  a.obs = obs;
  a.next_obs = next_obs;
  a.action = action;
  a.obs_pitch = obs_pitch;
  a.next_obs_pitch = next_obs_pitch;
  a.action_pitch = action_pitch;
  a.mean = mean;
  a.std = std;
  a.x_cur = x_cur;
  a.x_next = x_next;
  a.x_pi = x_pi;
  a.x_pitch = x_pitch;
  HIP_OK(launch_sac_prep(a, st));
  return 0;
}

int bx_sac_head_sample(int64_t n_rows, int64_t n_actions, const bx_sac_sample_job* jobs,
                       int32_t n_jobs, float min_std, void* stream) {
  if (sac_rows(n_rows) || sac_actions(n_actions)) return 1;
  if (n_jobs < 1 || n_jobs > BX_SAC_MAX_JOBS)
    return fail("n_jobs " + std::to_string(n_jobs) + " outside 1.." + std::to_string(BX_SAC_MAX_JOBS));
  if (n_rows == 0) return 0;
  if (!jobs) return fail("null argument");
  SacSampleArgs a{};
  for (int k = 0; k < n_jobs; ++k) {
    const bx_sac_sample_job& j = jobs[k];
    if (!j.logits || !j.eps || !j.log_prob)
      return fail("job " + std::to_string(k) + ": null logits, eps or log_prob");
    if (sac_pitch("logits_pitch", j.logits_pitch, 2 * n_actions) ||
        sac_pitch("eps_pitch", j.eps_pitch, n_actions) ||
        (j.action && sac_pitch("action_pitch", j.action_pitch, n_actions)))
      return 1;
    a.job[k] = j;
  }
  a.B = n_rows;
  a.A = n_actions;
  a.n_jobs = n_jobs;
  a.min_std = min_std;
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_sac_sample(a, st));
  return 0;
}

int bx_sac_head_losses(int64_t n_rows, int32_t n_critics, const float* lp_alpha,
                       const float* lp_next, const float* lp_pi, const bx_sac_q* q,
                       const float* reward, int64_t reward_stride, const float* discount,
                       int64_t discount_stride, const float* truncation,
                       int64_t truncation_stride, const float* log_alpha, float reward_scaling,
                       float discounting, float target_entropy, float* g_lp, void* workspace,
                       int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (sac_rows(n_rows) || sac_critics(n_critics)) return 1;
  const int64_t need = sac_head_workspace_bytes(n_rows);
  if (size_query(workspace, workspace_bytes, need)) return 0;
  if (n_rows == 0) return 0;
  if (!lp_alpha || !lp_next || !lp_pi || !q || !reward || !discount || !truncation || !log_alpha ||
      !g_lp)
    return fail("null argument");
  for (int c = 0; c < n_critics; ++c)
    if (!q->q_old[c] || !q->next_q[c] || !q->q_pi[c] || !q->dq_old[c] || !q->dq_pi[c])
      return fail("critic " + std::to_string(c) + ": null pointer");
  if (check_workspace(workspace, *workspace_bytes, need, 16)) return 1;
  STREAM_SCOPE(stream, st);
  SacLossesArgs a{};
  a.B = n_rows;
  a.C = n_critics;
  a.lp_alpha = lp_alpha;
  a.lp_next = lp_next;
  a.lp_pi = lp_pi;
  a.q = *q;
  a.reward = reward;
  a.discount = discount;
  a.truncation = truncation;
  a.reward_stride = reward_stride;
  a.discount_stride = discount_stride;
  a.truncation_stride = truncation_stride;
  a.log_alpha = log_alpha;
  a.reward_scaling = reward_scaling;
  a.discounting = discounting;
  a.target_entropy = target_entropy;
  a.g_lp = g_lp;
  a.part = (double*)workspace;
  HIP_OK(launch_sac_losses(a, st));
  return 0;
}

int bx_sac_head_sample_backward(int64_t n_rows, int64_t n_actions, int32_t n_critics,
                                const float* logits, int64_t logits_pitch, const float* eps,
                                int64_t eps_pitch, const float* g_lp, const bx_sac_daction* da,
                                float min_std, float* dlogits, int64_t dlogits_pitch,
                                float* losses, float* dlog_alpha, void* workspace,
                                int64_t* workspace_bytes, void* stream) {
  if (!workspace_bytes) return fail("null argument");
  if (sac_rows(n_rows) || sac_actions(n_actions) || sac_critics(n_critics)) return 1;
  const int64_t need = sac_head_workspace_bytes(n_rows);
  if (size_query(workspace, workspace_bytes, need)) return 0;
  if (n_rows == 0) return 0;
  if (!logits || !eps || !g_lp || !da || !dlogits || !losses || !dlog_alpha)
    return fail("null argument");
  if (sac_pitch("logits_pitch", logits_pitch, 2 * n_actions) ||
      sac_pitch("eps_pitch", eps_pitch, n_actions) ||
      sac_pitch("dlogits_pitch", dlogits_pitch, 2 * n_actions))
    return 1;
  for (int c = 0; c < n_critics; ++c) {
    if (!da->ptr[c]) return fail("critic " + std::to_string(c) + ": null pointer");
    if (sac_pitch("daction pitch", da->pitch[c], n_actions)) return 1;
  }
  if (check_workspace(workspace, *workspace_bytes, need, 16)) return 1;
  STREAM_SCOPE(stream, st);
  SacBackwardArgs a{};
  a.B = n_rows;
  a.A = n_actions;
  a.C = n_critics;
  a.min_std = min_std;
  a.logits = logits;
  a.eps = eps;
  a.g_lp = g_lp;
  a.logits_pitch = logits_pitch;
  a.eps_pitch = eps_pitch;
  a.da = *da;
  a.dlogits = dlogits;
  a.dlogits_pitch = dlogits_pitch;
  a.part = (const double*)workspace;
  a.losses = losses;
  a.dlog_alpha = dlog_alpha;
  HIP_OK(launch_sac_sample_backward(a, st));
  return 0;
}

int bx_opt_sizes(int32_t* tensor_bytes) {
  if (!tensor_bytes) return fail("null argument");
  *tensor_bytes = (int32_t)sizeof(bx_opt_tensor);
  return 0;
}

int bx_adam_step(const bx_opt_tensor* t, int32_t n_tensors, int64_t step, double beta1,
                 double beta2, float eps, void* stream) {
  if (!t) return fail("null tensor table");
  if (n_tensors < 1 || n_tensors > BX_OPT_MAX_TENSORS)
    return fail("n_tensors " + std::to_string(n_tensors) + " outside 1.." +
                std::to_string(BX_OPT_MAX_TENSORS));
  if (step < 1) return fail("step must be >= 1 (the count after this step)");
  // (the range checks and the double arithmetic live in optim_kernels.hip,
  // whose flags keep NaN comparisons and IEEE division; this unit's do not)
  if (const char* why = opt_check_scalars(beta1, beta2, eps)) return fail(why);
  OptArgs a{};
  int64_t groups = 0;
  int k = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const bx_opt_tensor& s = t[i];
    if (s.n < 0) return fail("tensor " + std::to_string(i) + ": negative n");
    if (s.n == 0) continue;
    if (!s.p || !s.g || !s.m || !s.v)
      return fail("tensor " + std::to_string(i) + ": null p, g, m or v");
    OptTensor& d = a.t[k];
    d.p = s.p;
    d.g = s.g;
    d.m = s.m;
    d.v = s.v;
    d.target = s.target;
    d.n = s.n;
    opt_set_tensor(d, s.lr, s.tau, step, beta1);
    const uintptr_t bits = (uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v |
                           (uintptr_t)s.target;
    d.vec = (bits & 15) == 0;
    a.first[k] = (int32_t)groups;
    groups += opt_chunks(s.n);
    if (groups > (int64_t)0x7fffffff) return fail("too many elements for one launch");
    ++k;
  }
  if (k == 0) return 0;
  a.first[k] = (int32_t)groups;
  a.n_tensors = k;
  opt_set_scalars(a, step, beta1, beta2, eps);
  STREAM_SCOPE(stream, st);
  HIP_OK(launch_adam_step(a, st));
  return 0;
}

}  // extern "C"
