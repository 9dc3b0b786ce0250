// bx_blob.cpp — build_plan: a descriptor's device blob and kernel plan, as a
// sequence of stages over one context (PlanCtx). The stages run in the blob's
// allocation order: every B.alloc below, the 16-byte alignment pads included,
// is pinned by tests/golden/blob_fingerprints.json.
#include "bx_blob.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "pbd_dispatch.h"

namespace bx {

PlanKnobs plan_knobs_from_env() {
  auto on = [](const char* name) { return getenv(name) && atoi(getenv(name)); };
  return {on("BX_NO_JOINT_HALVES"), on("BX_NO_R2"), on("BX_NO_MULTI_JH"), on("BX_NO_JB"),
          getenv("BX_PLAN_DEBUG") != nullptr};
}

namespace {

uint32_t fbits(double x) {
  float f = (float)x;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// a joint limit l (radians, as the record holds it in float) as the kernels
// test it (pbd_layout.h LL_*): its pseudo-angle (pbd_math.h pseudo_angle, a
// monotone stand-in for atan2 over (-pi, pi]; +-3 at or past +-pi, where no
// angle is out of range) and its cosine / sine, in double
void limit_trig(float lf, double* p, double* c, double* s) {
  const double l = lf;
  *c = std::cos(l);
  *s = std::sin(l);
  if (l <= -M_PI) *p = -3.0;
  else if (l >= M_PI) *p = 3.0;
  else {
    const double r = std::fabs(*c) + std::fabs(*s), t = r > 0 ? *c / r : 1.0;
    *p = *s >= 0 ? 1.0 - t : t - 1.0;
  }
}

// the smallest half float >= x (0 < x <= 65504), as its bits
uint16_t half_up(double x) {
  const int E = std::max(std::ilogb(x), -14);  // x = 1.m 2^E, or subnormal at E = -14
  // (a mantissa that rounds up to 2048 carries into the exponent)
  return (uint16_t)(((E + 14) << 10) + (int)std::ceil(std::ldexp(x, 10 - E)));
}

struct Builder {
  std::vector<uint32_t> w;
  int alloc(int n) {
    int o = (int)w.size();
    w.resize(w.size() + (size_t)std::max(n, 0), 0u);
    return o;
  }
  void align16() { alloc((4 - (int)w.size() % 4) % 4); }  // 16-byte aligned groups
  void f(int o, double x) { w[o] = fbits(x); }
  void i(int o, int x) { w[o] = (uint32_t)x; }
};

// a lane image in the blob (the SINGLE lane image, the MULTI joint halves):
// word w of lane l at o + (w / 4) * 4 * lanes + 4 * l + w % 4
struct Image {
  Builder& B;
  int o, lanes;
  void operator()(int lane, int w, uint32_t v) const {
    B.w[o + (w / 4) * 4 * lanes + 4 * lane + w % 4] = v;
  }
};

typedef std::vector<std::vector<int>> Lists;
const int HB = 8;  // the joint halves' half width (lanes per side)

struct PlanCtx {
  const bx_desc* d;
  const bx_reset_desc* r;
  const PlanKnobs& knobs;
  std::string* err;
  const int N, J, K, R, G;
  Builder B;
  BlobHdr H{};
  Lists jl, al, cl;  // per body: joint, actuator and contact gather lists
  // derived scalars
  int D = 0;                // joint angle dofs
  int max_btask = 0;        // MULTI gather tasks of one body
  size_t mx = 0, mx_ja = 0;  // longest gather list; longest joint / actuator list
  int max_groups = 0;       // collider groups on one body
  bool xcol = false;        // extended contact functions run in the item-loop kernel
  bool c16 = false, single_shape = false, r2 = false, r2g = false, mtab_ok = false, mjh = false;
  int L = 16;               // lanes per env (SINGLE / item loops)
  int off = 0, tail_m = 0, jlim_at = 0;  // LDS words carved; where the mode tails / limit rows start
  // the MULTI row tables: distinct collidables and materials, and each row's
  std::vector<std::array<uint32_t, 8>> cens;
  std::vector<std::array<uint32_t, 4>> mats;
  std::vector<int> row_cen, row_mat;
  std::vector<int> slot1, slot2;  // F_R2: the row of each lane's two slots, or -1

  PlanCtx(const bx_desc* d_, const bx_reset_desc* r_, const PlanKnobs& k, std::string* e)
      : d(d_), r(r_), knobs(k), err(e), N(d_->n_bodies), J(d_->n_joints), K(d_->n_actuators),
        R(d_->n_rows), G(d_->n_groups), jl(std::max(N, 0)), al(std::max(N, 0)), cl(std::max(N, 0)) {}

  int fail(const char* m) {
    *err = m;
    return 1;
  }
  int carve(int n) {
    int o = off;
    off += (n + 3) & ~3;
    return o;
  }
  // the width the SINGLE kernels gather the joint / actuator lists by (and the
  // contact list, unless F_C16 gives it 16)
  int gather_width() const { return (c16 ? mx_ja : mx) <= 4 ? 4 : 8; }

  // the stages, in build_plan's order (an int is a status: 1 with *err set)
  int validate();
  void pack_bodies_joints_actuators(), pack_rows_groups_forces(), gather_lists(), multi_tasks();
  int reset_tables();
  void shape_limits(), dedupe_row_tables(), lds_head(), lds_multi_tail(), lds_item_tail(), mode_fits();
  void multi_row_tables(), row_slots(), multi_joint_halves(), single_lane_image();
  int system_feat() const;
  int decide(Plan* P);
  // and the records they share
  void img_joint(const Image& put, int lane, int base, int j) const;
  void img_lim(const Image& put, int lane, int base, int j, int row) const;
  void img_act(const Image& put, int lane, int base, int a) const;
  int img_side(const Image& put, int lane, int base, int j, bool child) const;
  void img_body(const Image& put, int lane, int base, int b) const;
  void row_words(int x, uint32_t* out) const;
};

int PlanCtx::validate() {
  if (N <= 0) return fail("descriptor has no bodies");
  if (d->dynamics_mode != BX_DYN_PBD && d->dynamics_mode != BX_DYN_LEGACY_SPRING)
    return fail("unknown dynamics mode");
  if (d->substeps <= 0) return fail("substeps must be positive");
  for (int j = 0; j < J; j++) {
    if (d->joint_body_p[j] < 0 || d->joint_body_p[j] >= N || d->joint_body_c[j] < 0 ||
        d->joint_body_c[j] >= N)
      return fail("joint body index out of range");
    if (d->joint_type[j] != BX_JOINT_REVOLUTE && d->joint_type[j] != BX_JOINT_SPHERICAL &&
        !(d->joint_type[j] == BX_JOINT_UNIVERSAL && d->dynamics_mode == BX_DYN_LEGACY_SPRING))
      return fail("unsupported joint type");
    if (d->dynamics_mode == BX_DYN_LEGACY_SPRING &&
        (!d->joint_stiffness || !d->joint_spring_damping || !d->joint_limit_strength))
      return fail("legacy_spring descriptor needs joint stiffness, spring damping and limit strength");
  }
  for (int a = 0; a < K; a++) {
    if (d->act_joint[a] < 0 || d->act_joint[a] >= J) return fail("actuator joint out of range");
    for (int l = 0; l < 3; l++)
      if (d->act_index[3 * a + l] >= d->action_size) return fail("actuator index out of range");
  }
  for (int x = 0; x < R; x++) {
    if (d->row_body_a[x] < 0 || d->row_body_a[x] >= N || d->row_body_b[x] < 0 ||
        d->row_body_b[x] >= N)
      return fail("contact row body out of range");
    if (d->row_group[x] < 0 || d->row_group[x] >= G) return fail("contact row group out of range");
    int fn = d->col_fn[d->row_group[x]];
    if (fn < BX_COL_CAPSULE_PLANE || fn > BX_COL_HULL_HULL) return fail("unsupported contact function");
    if (fn == BX_COL_HULL_HULL) {
      if (!d->hull_vert || !d->hull_face || !d->hull_norm) return fail("hull rows need the hull arrays");
      for (int k = 0; k < 2; k++) {
        int hx = (int)d->row_ext[16 * x + k];
        if (hx < 0 || hx >= d->n_hull) return fail("hull row index out of range");
      }
      int e = (int)d->row_ext[16 * x + 2];
      if (e < 0 || e > 3) return fail("hull row contact index out of range");
    }
    if (fn >= BX_COL_HEIGHTMAP && !d->row_ext) return fail("extended contact rows need row_ext");
    if (fn == BX_COL_HEIGHTMAP) {
      if (!d->row_hm || !d->hm_data) return fail("height map rows need row_hm and hm_data");
      int off = d->row_hm[2 * x], m = d->row_hm[2 * x + 1];
      if (m < 2 || off < 0 || (int64_t)off + (int64_t)m * m > d->n_hm)
        return fail("height map row out of range");
    }
  }
  for (int f = 0; f < d->n_forces; f++) {
    if (d->force_body[f] < 0 || d->force_body[f] >= N) return fail("force body out of range");
    if (d->force_type[f] != BX_FORCE_THRUSTER && d->force_type[f] != BX_FORCE_TWISTER)
      return fail("unknown force type");
    if (f > 0 && d->force_type[f] < d->force_type[f - 1])
      return fail("forces must be ordered Thrusters, then Twisters");
  }
  if (G >= 128) return fail("too many collider groups");
  // rows of a group are contiguous; a culled group's rows are in flat order
  for (int x = 1; x < R; x++)
    if (d->row_group[x] < d->row_group[x - 1]) return fail("contact rows must be grouped");
  for (int g = 0; g < G; g++) {
    if (d->col_cutoff[g] < 0) return fail("negative collider cutoff");
    if (d->col_cutoff[g] == 0) continue;
    if (d->col_fn[g] != BX_COL_CAPSULE_CAPSULE) return fail("culling is capsule-capsule only");
    int n = 0, last = -1;
    for (int x = 0; x < R; x++) {
      if (d->row_group[x] != g) continue;
      // a masked cell ranks after every allowed one: only where cutoff needs it
      if (d->row_flat[x] <= last) return fail("culled rows must be in increasing flat order");
      last = d->row_flat[x];
      n++;
    }
    if (d->col_cutoff[g] > n) return fail("collider cutoff exceeds the group's rows");
  }
  if (d->row_nn_masked)
    for (int x = 0; x < R; x++)
      if (d->row_nn_masked[x] && !d->col_cutoff[d->row_group[x]])
        return fail("masked NearNeighbors rows belong to culled groups");
  if (2 * R >= (1 << 24)) return fail("too many contact rows");
  return 0;
}

// the header's scalars and the body, joint and actuator records
void PlanCtx::pack_bodies_joints_actuators() {
  B.alloc((int)(sizeof(BlobHdr) / 4));
  H.N = N; H.J = J; H.K = K; H.R = R; H.G = G; H.A = d->action_size; H.substeps = d->substeps;
  H.num_joint_dof = d->num_joint_dof;
  H.h = (float)d->h;
  H.dt = (float)d->dt;
  // integrators.py:87,91 — exp(damping * dt) of Python doubles, one constant
  H.vexp = (float)std::exp(d->velocity_damping * d->h);
  H.aexp = (float)std::exp(d->angular_damping * d->h);
  H.spring = d->dynamics_mode == BX_DYN_LEGACY_SPRING ? 1 : 0;
  H.gx = (float)d->gravity[0]; H.gy = (float)d->gravity[1]; H.gz = (float)d->gravity[2];

  H.o_body = B.alloc(N * BODY_STRIDE);
  for (int b = 0; b < N; b++) {
    int o = H.o_body + b * BODY_STRIDE;
    B.f(o + BODY_MASS, d->body_mass[b]);
    for (int k = 0; k < 3; k++) {
      B.f(o + BODY_I + k, d->body_inv_inertia[3 * b + k]);
      B.f(o + BODY_PM + k, d->pos_mask[3 * b + k]);
      B.f(o + BODY_RM + k, d->rot_mask[3 * b + k]);
    }
    for (int k = 0; k < 4; k++) B.f(o + BODY_QM + k, d->quat_mask[4 * b + k]);
  }
  H.o_joint = B.alloc(J * JOINT_STRIDE);
  for (int j = 0; j < J; j++) {
    int o = H.o_joint + j * JOINT_STRIDE;
    int type = d->joint_type[j];
    // angle_vel dofs (joints.py:218-225): the free dofs of a sphericalised
    // group, else every dof of the joint (1 / 2 / 3)
    int nang = d->joint_free_dofs[j] >= 0 ? d->joint_free_dofs[j] : d->joint_dof[j];
    B.i(o + J_TYPE, type);
    B.i(o + J_BP, d->joint_body_p[j]);
    B.i(o + J_BC, d->joint_body_c[j]);
    B.i(o + J_FREE, d->joint_free_dofs[j]);
    B.i(o + J_DOF, d->joint_dof[j]);
    B.i(o + J_ANGLE_OFF, D);
    B.i(o + J_NANGLES, nang);
    D += nang;
    B.f(o + J_DAMP, d->joint_damping[j]);
    B.f(o + J_SP, d->joint_scale_pos[j]);
    B.f(o + J_SA, d->joint_scale_ang[j]);
    for (int k = 0; k < 3; k++) {
      B.f(o + J_OFFP + k, d->joint_off_p[3 * j + k]);
      B.f(o + J_OFFC + k, d->joint_off_c[3 * j + k]);
    }
    for (int k = 0; k < 9; k++) {
      B.f(o + J_AXP + k, d->joint_axis_p[9 * j + k]);
      B.f(o + J_AXC + k, d->joint_axis_c[9 * j + k]);
    }
    for (int k = 0; k < 6; k++) B.f(o + J_LIM + k, d->joint_limit[6 * j + k]);
    // the limit rows' pseudo-angles and cos / sin (J_JLIM, LL_*), from the
    // radians just stored as float
    for (int row = 0; row < 3; row++)
      for (int side = 0; side < 2; side++) {
        float lf;
        std::memcpy(&lf, &B.w[o + J_LIM + 2 * row + side], 4);
        double p, c, sn;
        limit_trig(lf, &p, &c, &sn);
        const int lr = o + J_JLIM + 8 * row;
        B.f(lr + (side ? LL_PHI : LL_PLO), p);
        B.f(lr + (side ? LL_CHI : LL_CLO), c);
        B.f(lr + (side ? LL_SHI : LL_SLO), sn);
      }
    if (d->dynamics_mode == BX_DYN_LEGACY_SPRING) {
      B.f(o + J_STIFF, d->joint_stiffness[j]);
      B.f(o + J_SDAMP, d->joint_spring_damping[j]);
      B.f(o + J_LSTR, d->joint_limit_strength[j]);
    }
  }
  H.D = D;
  H.o_act = B.alloc(K * ACT_STRIDE);
  for (int a = 0; a < K; a++) {
    int o = H.o_act + a * ACT_STRIDE;
    B.i(o + A_TYPE, d->act_type[a]);
    B.i(o + A_JOINT, d->act_joint[a]);
    for (int k = 0; k < 3; k++) B.i(o + A_IDX + k, d->act_index[3 * a + k]);
    B.f(o + A_STR, d->act_strength[a]);
  }
}

// the contact row, height map, hull, collider group and force records
void PlanCtx::pack_rows_groups_forces() {
  H.o_row = B.alloc(R * ROW_STRIDE);
  for (int x = 0; x < R; x++) {
    int o = H.o_row + x * ROW_STRIDE;
    int g = d->row_group[x];
    B.i(o + R_GROUP, g);
    B.i(o + R_A, d->row_body_a[x]);
    B.i(o + R_B, d->row_body_b[x]);
    B.i(o + R_FN, d->col_fn[g]);
    B.i(o + R_ONEWAY, d->col_oneway[g]);
    for (int k = 0; k < 3; k++) {
      B.f(o + R_APOS + k, d->row_a_pos[3 * x + k]);
      B.f(o + R_AEND + k, d->row_a_end[3 * x + k]);
      B.f(o + R_BPOS + k, d->row_b_pos[3 * x + k]);
      B.f(o + R_BEND + k, d->row_b_end[3 * x + k]);
    }
    B.f(o + R_ARAD, d->row_a_radius[x]);
    B.f(o + R_BRAD, d->row_b_radius[x]);
    B.f(o + R_FRIC, d->row_friction[x]);
    B.f(o + R_ELAS, d->row_elasticity[x]);
    B.f(o + R_SCALE, d->col_scale[g]);
    B.f(o + R_THR, d->col_velocity_threshold[g]);
    B.f(o + R_ERP, d->col_baumgarte_erp[g]);
    if (d->row_ext)
      for (int k = 0; k < 16; k++) B.f(o + R_X + k, d->row_ext[16 * x + k]);
    B.i(o + R_NNMASK, d->row_nn_masked && d->row_nn_masked[x] ? 1 : 0);
    B.i(o + R_FLAT, d->col_cutoff[g] ? d->row_flat[x] : -1);
    if (d->col_fn[g] == BX_COL_HEIGHTMAP) {
      B.i(o + R_HM_OFF, d->row_hm[2 * x]);
      B.i(o + R_HM_M, d->row_hm[2 * x + 1]);
    }
  }
  H.o_hm = B.alloc(d->n_hm > 0 ? d->n_hm : 0);
  for (int k = 0; k < d->n_hm; k++) B.f(H.o_hm + k, d->hm_data[k]);
  H.o_hull = B.alloc(d->n_hull > 0 ? d->n_hull * HULL_STRIDE : 0);
  for (int h = 0; h < d->n_hull; h++) {
    int o = H.o_hull + h * HULL_STRIDE;
    for (int k = 0; k < 24; k++) B.f(o + HULL_V + k, d->hull_vert[24 * h + k]);
    for (int k = 0; k < 72; k++) B.f(o + HULL_F + k, d->hull_face[72 * h + k]);
    for (int k = 0; k < 18; k++) B.f(o + HULL_N + k, d->hull_norm[18 * h + k]);
  }
  // collider groups: cutoff, row range, Info base (system.py:36-43 order)
  H.o_group = B.alloc(G * GROUP_STRIDE);
  int info = 0;
  for (int g = 0; g < G; g++) {
    int r0 = R, r1 = 0;
    for (int x = 0; x < R; x++)
      if (d->row_group[x] == g) { r0 = std::min(r0, x); r1 = std::max(r1, x + 1); }
    if (r0 > r1) r0 = r1 = 0;
    int o = H.o_group + g * GROUP_STRIDE;
    B.i(o + G_CUT, d->col_cutoff[g]);
    B.i(o + G_R0, r0);
    B.i(o + G_R1, r1);
    B.i(o + G_INFO, info);
    info += d->col_cutoff[g] ? d->col_cutoff[g] : r1 - r0;
    if (d->col_cutoff[g]) H.n_nn++;
  }
  H.info_rows = info;
  H.NF = d->n_forces;
  H.o_force = B.alloc(d->n_forces * FORCE_STRIDE);
  for (int f = 0; f < d->n_forces; f++) {
    int o = H.o_force + f * FORCE_STRIDE;
    B.i(o + F_TYPE, d->force_type[f]);
    B.i(o + F_BODY, d->force_body[f]);
    for (int k = 0; k < 3; k++) B.i(o + F_IDX + k, d->force_index[3 * f + k]);
    B.f(o + F_STR, d->force_strength[f]);
    B.f(o + F_MASS, d->body_mass[d->force_body[f]]);
  }
}

// gather lists (the reference's segment_sum order: per group, parents then
// children / a-rows then b-rows)
void PlanCtx::gather_lists() {
  for (int j0 = 0; j0 < J;) {
    int g = d->joint_group[j0], j1 = j0;
    while (j1 < J && d->joint_group[j1] == g) j1++;
    for (int j = j0; j < j1; j++) jl[d->joint_body_p[j]].push_back(j);
    for (int j = j0; j < j1; j++) jl[d->joint_body_c[j]].push_back(J + j);
    j0 = j1;
  }
  for (int a0 = 0; a0 < K;) {
    int g = d->act_group[a0], a1 = a0;
    while (a1 < K && d->act_group[a1] == g) a1++;
    for (int a = a0; a < a1; a++) al[d->joint_body_p[d->act_joint[a]]].push_back(a);
    for (int a = a0; a < a1; a++) al[d->joint_body_c[d->act_joint[a]]].push_back(K + a);
    a0 = a1;
  }
  for (int g = 0; g < G; g++) {
    for (int x = 0; x < R; x++)
      if (d->row_group[x] == g) cl[d->row_body_a[x]].push_back(x | (g << 24));
    if (!d->col_oneway[g])
      for (int x = 0; x < R; x++)
        if (d->row_group[x] == g) cl[d->row_body_b[x]].push_back((R + x) | (g << 24));
  }
  auto put_lists = [&](const Lists& L_, int& o_off, int& o_l) {
    o_off = B.alloc(N + 1);
    int tot = 0;
    for (int b = 0; b < N; b++) tot += (int)L_[b].size();
    o_l = B.alloc(tot);
    int k = 0;
    for (int b = 0; b < N; b++) {
      B.i(o_off + b, k);
      for (int v : L_[b]) B.i(o_l + k++, v);
    }
    B.i(o_off + N, k);
  };
  put_lists(jl, H.o_jl_off, H.o_jl);
  put_lists(al, H.o_al_off, H.o_al);
  put_lists(cl, H.o_cl_off, H.o_cl);
}

// MULTI-mode gather tasks: each body's contact list cut, per collider group,
// into runs of <= TASK_W entries (same order); a body's tasks in list order.
// An entry names a row and side (row | side << 15, pbd_layout.h MCAP):
// the kernel finds the side's slot through the row's compact index; the
// padding entry is row R (never indexed); the zero slot is 2 MCAP
void PlanCtx::multi_tasks() {
  H.m_zero = 2 * MCAP;
  auto mslot_of = [&](int s) { return s < R ? s : ((s - R) | 0x8000); };
  Lists task_e;    // row | side << 15
  Lists btask(N);  // task | group << 24
  for (int b = 0; b < N; b++) {
    size_t i = 0;
    while (i < cl[b].size()) {
      const int g = cl[b][i] >> 24;
      std::vector<int> t;
      while (i < cl[b].size() && (cl[b][i] >> 24) == g && (int)t.size() < TASK_W)
        t.push_back(mslot_of(cl[b][i++] & 0xFFFFFF));
      btask[b].push_back((int)task_e.size() | (g << 24));
      task_e.push_back(t);
    }
    max_btask = std::max(max_btask, (int)btask[b].size());
  }
  H.T = (int)task_e.size();
  H.o_task = B.alloc(H.T * TASK_W);
  for (int t = 0; t < H.T; t++)
    for (int k = 0; k < TASK_W; k++)
      B.i(H.o_task + t * TASK_W + k, k < (int)task_e[t].size() ? task_e[t][k] : R);
  H.o_btask = B.alloc(N * BTASK_W);
  for (int b = 0; b < N; b++) {
    // padding: the zero task (index T, a zero partial) in the last group
    const int gl = btask[b].empty() ? 0 : (btask[b].back() >> 24);
    for (int k = 0; k < BTASK_W; k++)
      B.i(H.o_btask + b * BTASK_W + k,
          k < (int)btask[b].size() ? btask[b][k] : (H.T | (gl << 24)));
  }
}

int PlanCtx::reset_tables() {
  if (r) {
    H.n_fk = r->n_fk;
    H.n_root_groups = r->n_root_groups;
    H.o_base = B.alloc(N * 13);
    for (int k = 0; k < N * 13; k++) B.f(H.o_base + k, r->base_qp[k]);
    H.o_fk = B.alloc(r->n_fk * FK_STRIDE);
    for (int f = 0; f < r->n_fk; f++) {
      int o = H.o_fk + f * FK_STRIDE;
      if (r->fk_body_p[f] < 0 || r->fk_body_p[f] >= N || r->fk_body_c[f] < 0 || r->fk_body_c[f] >= N)
        return fail("reset joint body out of range");
      B.i(o + FK_BP, r->fk_body_p[f]);
      B.i(o + FK_BC, r->fk_body_c[f]);
      for (int l = 0; l < 3; l++) {
        int ix = r->fk_dof_index[3 * f + l];
        if (ix >= d->num_joint_dof) return fail("reset dof index out of range");
        B.i(o + FK_IDX + l, ix);
      }
      for (int k = 0; k < 4; k++) {
        B.f(o + FK_ROT + k, r->fk_rot[4 * f + k]);
        B.f(o + FK_REF + k, r->fk_ref[4 * f + k]);
      }
      for (int k = 0; k < 3; k++) {
        B.f(o + FK_OFFP + k, r->fk_off_p[3 * f + k]);
        B.f(o + FK_OFFC + k, r->fk_off_c[3 * f + k]);
      }
    }
    Lists zl(N);
    for (int p = 0; p < r->n_zpts; p++) {
      if (r->zpt_body[p] < 0 || r->zpt_body[p] >= N) return fail("min_z point body out of range");
      zl[r->zpt_body[p]].push_back(p);
    }
    H.o_zoff = B.alloc(N + 1);
    H.o_zpt = B.alloc(r->n_zpts * 4);
    int k = 0;
    for (int b = 0; b < N; b++) {
      B.i(H.o_zoff + b, k);
      for (int p : zl[b]) {
        for (int q = 0; q < 3; q++) B.f(H.o_zpt + 4 * k + q, r->zpt_local[3 * p + q]);
        B.f(H.o_zpt + 4 * k + 3, r->zpt_radius[p]);
        k++;
      }
    }
    B.i(H.o_zoff + N, k);
    H.o_dangle = B.alloc(d->num_joint_dof);
    for (int k = 0; k < d->num_joint_dof; k++)
      B.f(H.o_dangle + k, r->default_angle ? r->default_angle[k] : 0.0);
    H.o_zero = B.alloc(N);
    H.o_rgroup = B.alloc(N);
    for (int b = 0; b < N; b++) {
      B.i(H.o_zero + b, r->body_zero_cand[b]);
      B.i(H.o_rgroup + b, r->body_root_group[b]);
    }
  }
  H.const_words = (((r ? H.o_base : (int)B.w.size())) + 3) & ~3;
  return 0;
}

// the register-hoisted (SINGLE) kernels' shape limits, independent of the
// lane count: gather lists of <= 8 entries, <= 2 collider groups per body,
// the pbd step without culling or the extended contact functions
void PlanCtx::shape_limits() {
  size_t mx_c = 0;
  for (int g = 0; g < G; g++) xcol |= d->col_fn[g] >= BX_COL_HEIGHTMAP;
  for (int b = 0; b < N; b++) {
    mx_ja = std::max({mx_ja, jl[b].size(), al[b].size()});
    mx_c = std::max(mx_c, cl[b].size());
    std::vector<int> gs;
    for (int v : cl[b])
      if (std::find(gs.begin(), gs.end(), v >> 24) == gs.end()) gs.push_back(v >> 24);
    max_groups = std::max(max_groups, (int)gs.size());
  }
  mx = std::max(mx_ja, mx_c);
  // F_C16: a body's contact list may hold up to 16 entries (its joint and
  // actuator lists <= 8), the SINGLE kernels then gather 16 contact slots
  c16 = mx_c > 8 && mx_c <= 16 && mx_ja <= 8;
  single_shape = (mx <= 8 || c16) && max_groups <= 2 && H.n_nn == 0 &&
                 d->dynamics_mode != BX_DYN_LEGACY_SPRING && !xcol;
}

// the MULTI kernel's row tables: the rows' collidables as the distinct
// (body, offset, end, radius) records, whose centres the broad phase and
// the NearNeighbors keys place in the world once per pass (culled scenes:
// once per step) for every row naming them, and from which the contact
// passes assemble a row's geometry in LDS
void PlanCtx::dedupe_row_tables() {
  std::map<std::array<uint32_t, 8>, int> cen_ix;
  row_cen.assign(2 * R, 0);
  // and the rows' impulse constants as the distinct (friction, elasticity,
  // scale, velocity threshold) materials
  std::map<std::array<uint32_t, 4>, int> mat_ix;
  row_mat.assign(R, 0);
  // a record's index in its table, appended where new
  auto intern = [](auto& ix, auto& table, const auto& k) {
    const auto it = ix.emplace(k, (int)table.size());
    if (it.second) table.push_back(k);
    return it.first->second;
  };
  for (int x = 0; x < R; x++) {
    // (the row record's words: the bits the row image carried)
    const uint32_t* w = &B.w[H.o_row + x * ROW_STRIDE];
    for (int side = 0; side < 2; side++) {
      const int o = side ? R_BPOS : R_APOS, oe = side ? R_BEND : R_AEND, orr = side ? R_BRAD : R_ARAD;
      const std::array<uint32_t, 8> k{w[side ? R_B : R_A], w[o], w[o + 1], w[o + 2],
                                      w[oe], w[oe + 1], w[oe + 2], w[orr]};
      row_cen[2 * x + side] = intern(cen_ix, cens, k);
    }
    const std::array<uint32_t, 4> m{w[R_FRIC], w[R_ELAS], w[R_SCALE], w[R_THR]};
    row_mat[x] = intern(mat_ix, mats, m);
  }
  // (past these sizes the scene takes the item-loop kernels: no MULTI tables)
  mtab_ok = cens.size() <= 256 && mats.size() <= 0xFF && R <= 0xFFFF;
  H.n_cen = mtab_ok ? (int)cens.size() : 0;
  H.n_mat = mtab_ok ? (int)mats.size() : 0;
}

// per-env LDS layout: the lanes per env and the regions every mode keeps
void PlanCtx::lds_head() {
  L = std::max({N, J, K, R, 1});
  // an env is one 16/32/64-lane segment of a wave; past 64 items (large
  // scenes) it spreads over a whole 128- or 256-thread workgroup
  L = L <= 16 ? 16 : L <= 32 ? 32 : L <= 64 ? 64 : L <= 128 ? 128 : 256;
  // 17-32 contact rows and <= 16 bodies / joints / actuators: SINGLE mode at
  // 16 lanes with two rows per lane (F_R2: rows l and l + 16), not 32 lanes
  // for the rows alone (HalfCheetah, HumanoidStandup, Fetch)
  r2 = L == 32 && std::max({N, J, K}) <= 16 && R <= 32 && single_shape && !knobs.no_r2;
  if (r2) L = 16;
  H.L = L;
  H.l_qp = carve(N * QP_STRIDE);
  H.l_prev = carve(N * PREV_STRIDE);
  H.l_rb = carve(N * RB_STRIDE);
  // slot regions end with one zero slot (padding target of the gather lists)
  H.l_jslot = carve((2 * J + 1) * SLOT_STRIDE);
  H.l_aslot = carve((2 * K + 1) * ASLOT_STRIDE);
  // the active-row list: culled scenes only (the SINGLE kernels never cull;
  // MULTI's all-pairs scenes need the room)
  H.l_alist = carve(H.n_nn ? H.info_rows : 0);
  H.l_red = carve(64);
  // NearNeighbors: each wave's sorted picks (64-bit keys) when an env spans
  // up to 4 waves (carved with the env-step regions below; the MULTI kernel
  // keeps them in its task-partials region)
  int max_cut = 0;
  for (int g = 0; g < G; g++) max_cut = std::max(max_cut, d->col_cutoff[g]);
  H.nnl_words = 2 * 4 * max_cut;
  // the MULTI (System.step only) tail starts here, over the env step's regions
  tail_m = off;
}

// the contact regions form each mode's tail: the item-loop / SINGLE
// kernels keep per-row data and 12-word slots, MULTI mode keeps the row data
// in registers and needs 6-word slots plus the task partials
void PlanCtx::lds_multi_tail() {
  off = tail_m;
  // the chunk's contact slots (2 MCAP + the zero slot; the Info accumulators
  // alias them after the substeps)
  H.l_mslot = carve(std::max((2 * MCAP + 1) * MSLOT_STRIDE, N * ACC_STRIDE));
  // the task partials; before the passes read them the same words hold the
  // broad phase's near-row list (16-bit), the NearNeighbors pick lists and the
  // serial picks' distances
  H.l_tslot = carve(std::max({(H.T + 1) * TSLOT_STRIDE, (R + 1) / 2, H.nnl_words, H.n_nn ? R : 0}));
  H.l_near = H.l_tslot;
  H.l_cnt = carve(48);
  H.l_nearc = H.l_cnt;
  // the rows' compact contact indices (16-bit, R + 1: the padding row R)
  H.l_sidx = carve((R + 2) / 2);
  // the penetrating rows' contacts, then their rows (16-bit)
  H.l_cbuf = carve(std::max(MCBUF * MCB_W + MCBUF / 2, H.n_nn ? R : 0));
  // the broad phase's row bounds and centres (constants, then world), staged
  // once per launch
  H.l_bimg = carve(BI_WORDS * R);
  H.l_cen = carve(4 * (3 * H.n_cen + H.n_mat + N));
  H.env_words_m = (off + 63) & ~63;
  if (knobs.debug)
    fprintf(stderr,
            "bx plan (words): qp..red %d  mslot %d  tslot %d (T=%d)  cnt+sidx+cbuf %d  bimg %d  "
            "cen %d (n_cen=%d n_mat=%d)  ract %d  alist %d  nnl %d  env_words_m %d (%d B)\n",
            H.l_red + 64, H.l_tslot - H.l_mslot, H.l_cnt - H.l_tslot, H.T, H.l_bimg - H.l_cnt,
            H.l_cen - H.l_bimg, 4 * (3 * H.n_cen + H.n_mat + N), H.n_cen, H.n_mat,
            H.n_nn ? R : 0, H.n_nn ? H.info_rows : 0, H.nnl_words, H.env_words_m, 4 * H.env_words_m);
}

void PlanCtx::lds_item_tail() {
  off = tail_m;
  // env-step regions: joint angles, the env programs' System.step action
  // (swimmer: + drag, grasp: 3 palm actions), the staged action row (every
  // index an actuator or force reads: jp.take clips into the row, so no read
  // lands past these words)
  // (the Info accumulators and the NearNeighbors ranks: the MULTI kernel
  // keeps them in its contact slots / contact buffer, dead when these live)
  H.l_acc = carve(N * ACC_STRIDE);
  H.l_ract = carve(H.n_nn ? R : 0);
  H.l_nnl = carve(H.nnl_words);
  H.l_ang = carve(2 * D);
  H.xact_words = std::max(16, (d->action_size + 12 + 3) & ~3);
  H.l_xact = carve(H.xact_words);
  H.act_read = std::max(d->action_size, 1);
  for (int k = 0; k < 3 * K; k++) H.act_read = std::max(H.act_read, d->act_index[k] + 1);
  for (int k = 0; k < 3 * d->n_forces; k++) H.act_read = std::max(H.act_read, d->force_index[k] + 1);
  H.l_arow = carve(H.act_read);
  H.l_rowd = carve(R * ROWD_STRIDE);
  H.l_cslot = carve((2 * R + 1) * SLOT_STRIDE);
  // SINGLE mode: the spherical kernels' joint limit rows, staged from the
  // lane image once per launch (6 16-byte groups per lane, LIM_SLOTS; sized
  // for this system's L, which bx_system_set_variant keeps)
  // (carved in decide(), once the features say the system's SINGLE kernel reads it)
  jlim_at = off;
  H.l_jlim = 0;
  // envs 64 words apart: with the odd-multiple record strides, the four
  // envs' records of one ds_read_b128 lane group land on distinct bank slots
  H.env_words = (off + 63) & ~63;
}

// which of the SINGLE and MULTI kernels the system fits
void PlanCtx::mode_fits() {
  const bool single_fit = N <= L && J <= L && K <= L && (R <= L || r2) && single_shape &&
                          (mx <= 8 || L == 16);
  // the register-hoisted kernel is the pbd step only; legacy_spring systems
  // run the item-loop kernel
  H.single = single_fit ? 1 : 0;  // F_C16 kernels: 16 lanes
  // MULTI mode: a pbd scene past one wave (256 threads per env), every
  // lane owning <= 1 body / joint / actuator / task and <= MULTI_MR rows
  // (and its LDS tail within one workgroup's 160 KB)
  H.multi = (!H.single && L > 64 && !H.spring && !xcol && N <= 256 && J <= 256 && K <= 256 &&
             H.T <= 2 * 256 && G < 64 && R <= 8 * 256 && mx_ja <= 8 && max_btask <= BTASK_W && mtab_ok &&
             (size_t)H.env_words_m * 4 <= 160 * 1024) ? 1 : 0;
  H.act_same = 1;
  for (int a = 0; a < K; a++)
    if (d->act_joint[a] != a) H.act_same = 0;
}

// a contact row's 32 resolved words (LR_*): its record's geometry and
// constants with the masses / inverse inertias of the bodies it names
void PlanCtx::row_words(int x, uint32_t* out) const {
  const uint32_t* w = &B.w[H.o_row + x * ROW_STRIDE];
  const uint32_t* pa = &B.w[H.o_body + (int)w[R_A] * BODY_STRIDE];
  const uint32_t* pb = &B.w[H.o_body + (int)w[R_B] * BODY_STRIDE];
  const int src[24] = {R_GROUP, R_A, R_B, R_FN, R_ONEWAY, R_APOS, R_APOS + 1, R_APOS + 2,
                       R_AEND, R_AEND + 1, R_AEND + 2, R_ARAD, R_BPOS, R_BPOS + 1, R_BPOS + 2,
                       R_BEND, R_BEND + 1, R_BEND + 2, R_BRAD, R_FRIC, R_ELAS, R_SCALE, R_THR,
                       R_ERP};
  for (int k = 0; k < 24; k++) out[k] = w[src[k]];
  out[LR_MA] = pa[BODY_MASS];
  out[LR_MB] = pb[BODY_MASS];
  for (int k = 0; k < 3; k++) {
    out[LR_IA + k] = pa[BODY_I + k];
    out[LR_IB + k] = pb[BODY_I + k];
  }
}

// the MULTI kernel's row tables (BI_*: bounds / flags per row; collidables,
// materials and bodies after them)
void PlanCtx::multi_row_tables() {
  if (!H.multi || R <= 0) return;
  B.align16();
  // broad-phase bounds (BI_*): reach = |a_end| + |b_end| + radii in double,
  // rounded up to float
  std::vector<uint32_t> bimg(BI_WORDS * R, 0u);
  for (int x = 0; x < R; x++) {
    const int g = d->row_group[x];
    double reach = d->row_a_radius[x] + d->row_b_radius[x];
    double ea = 0, eb = 0;
    for (int k = 0; k < 3; k++) {
      ea += d->row_a_end[3 * x + k] * d->row_a_end[3 * x + k];
      eb += d->row_b_end[3 * x + k] * d->row_b_end[3 * x + k];
    }
    reach += std::sqrt(ea) + std::sqrt(eb);
    // the broad phase compares squared centre distances with (reach +
    // 1e-4)^2, rounded up (the margin far above the fp32 error of the
    // centres; a row it keeps that cannot touch only costs its test)
    const double reach2 = (reach + 1e-4) * (reach + 1e-4);
    // as a half float rounded up (+inf past 65504: always near)
    const uint16_t hb = reach2 <= 65504.0 ? half_up(reach2) : 0x7C00u;
    uint32_t* bw = &bimg[BI_WORDS * x];
    const bool skip = d->col_fn[g] == BX_COL_CAPSULE_CAPSULE;
    const bool cull = d->col_cutoff[g] != 0;
    const bool masked = d->row_nn_masked && d->row_nn_masked[x];
    uint32_t fl = (uint32_t)(skip * BIF_SKIP) | (uint32_t)(cull * BIF_CULL) |
                  (uint32_t)(masked * BIF_MASK) | (uint32_t)((d->col_oneway[g] != 0) * BIF_OW) |
                  ((uint32_t)d->col_fn[g] << BIF_FN_SHIFT) | ((uint32_t)row_mat[x] << BIF_MAT_SHIFT);
    uint32_t info = 0u;
    if (!cull) {
      // the unculled row's Info index (its group's first Info row + its offset)
      const int og = H.o_group + g * GROUP_STRIDE;
      info = (uint32_t)((int)B.w[og + G_INFO] + x - (int)B.w[og + G_R0]);
    }
    bw[BI_W0] = (uint32_t)row_cen[2 * x] | ((uint32_t)row_cen[2 * x + 1] << 8) | (fl << 16);
    bw[BI_W1] = (uint32_t)hb | (info << 16);
  }
  H.o_bimg = B.alloc(BI_WORDS * R);
  for (int k = 0; k < BI_WORDS * R; k++) B.w[H.o_bimg + k] = bimg[k];
  B.align16();
  H.o_cen = B.alloc(8 * H.n_cen + 4 * H.n_mat + 4 * N);
  for (int k = 0; k < H.n_cen; k++)
    for (int i = 0; i < 8; i++) B.w[H.o_cen + 8 * k + i] = cens[k][i];
  const int o_mat = H.o_cen + 8 * H.n_cen, o_bod = o_mat + 4 * H.n_mat;
  for (int k = 0; k < H.n_mat; k++)
    for (int i = 0; i < 4; i++) B.w[o_mat + 4 * k + i] = mats[k][i];
  // the bodies' (mass, inverse inertia), the rows' ma / Ia / mb / Ib
  for (int b = 0; b < N; b++) {
    B.w[o_bod + 4 * b] = B.w[H.o_body + b * BODY_STRIDE + BODY_MASS];
    for (int i = 0; i < 3; i++) B.w[o_bod + 4 * b + 1 + i] = B.w[H.o_body + b * BODY_STRIDE + BODY_I + i];
  }
}

// F_R2: which rows each lane works. Rows of one contact function share a
// slot where they fit (HalfCheetah, Pusher: the plane rows in the first,
// the capsule-capsule rows in the second), so a pass runs one function per
// slot instead of both on every lane; otherwise rows l and l + 16
void PlanCtx::row_slots() {
  slot1.assign(16, -1);
  slot2.assign(16, -1);
  if (!r2) return;
  std::vector<int> pl, other;
  for (int x = 0; x < R; x++)
    (d->col_fn[d->row_group[x]] == BX_COL_CAPSULE_PLANE ? pl : other).push_back(x);
  if (!pl.empty() && !other.empty() && pl.size() <= 16 && other.size() <= 16) {
    // F_R2G: slot 1 one-way capsule-plane, slot 2 two-way capsule-capsule
    r2g = true;
    for (int x : pl) r2g &= d->col_oneway[d->row_group[x]] != 0;
    for (int x : other)
      r2g &= d->col_fn[d->row_group[x]] == BX_COL_CAPSULE_CAPSULE && !d->col_oneway[d->row_group[x]];
    // F_R2G's two-way slot runs as contact halves: row k's a side on lane
    // k, its b side on lane k + 8 (pbd_kernels.hip position_contact_half)
    r2g &= other.size() <= 8;
    for (size_t i = 0; i < pl.size(); i++) slot1[i] = pl[i];
    for (size_t i = 0; i < other.size(); i++) {
      slot2[i] = other[i];
      if (r2g) slot2[i + 8] = other[i];
    }
  } else {
    for (int l = 0; l < 16; l++) {
      slot1[l] = l < R ? l : -1;
      slot2[l] = l + 16 < R ? l + 16 : -1;
    }
  }
}

// records in the lane images' layouts, each word through put(lane, word,
// value): a joint (LJ_*, with its bodies' masses / inverse inertias), its
// limit row `row` (LL_*: pseudo-angles and cos / sin, from J_JLIM), an
// actuator (LA_*), a joint-halves side (LS_* but LS_OWN; returns the body)
void PlanCtx::img_joint(const Image& put, int lane, int base, int j) const {
  if (J == 0) return;
  const uint32_t* s = &B.w[H.o_joint + j * JOINT_STRIDE];
  const int bp = (int)s[J_BP], bc = (int)s[J_BC];
  const uint32_t* p = &B.w[H.o_body + bp * BODY_STRIDE];
  const uint32_t* c = &B.w[H.o_body + bc * BODY_STRIDE];
  const int ints[6] = {J_TYPE, J_BP, J_BC, J_FREE, J_ANGLE_OFF, J_NANGLES};
  for (int k = 0; k < 6; k++) put(lane, base + k, s[ints[k]]);
  put(lane, base + LJ_DAMP, s[J_DAMP]);
  put(lane, base + LJ_SP, s[J_SP]);
  put(lane, base + LJ_SA, s[J_SA]);
  for (int k = 0; k < 3; k++) {
    put(lane, base + LJ_OFFP + k, s[J_OFFP + k]);
    put(lane, base + LJ_OFFC + k, s[J_OFFC + k]);
    put(lane, base + LJ_IP + k, p[BODY_I + k]);
    put(lane, base + LJ_IC + k, c[BODY_I + k]);
  }
  for (int k = 0; k < 9; k++) {
    put(lane, base + LJ_AXP + k, s[J_AXP + k]);
    put(lane, base + LJ_AXC + k, s[J_AXC + k]);
  }
  for (int k = 0; k < 6; k++) put(lane, base + LJ_LIM + k, s[J_LIM + k]);
  put(lane, base + LJ_DOF, s[J_DOF]);
  put(lane, base + LJ_MP, p[BODY_MASS]);
  put(lane, base + LJ_MC, c[BODY_MASS]);
}
void PlanCtx::img_lim(const Image& put, int lane, int base, int j, int row) const {
  if (J == 0) return;
  const uint32_t* s = &B.w[H.o_joint + j * JOINT_STRIDE + J_JLIM + 8 * row];
  for (int k = 0; k < 6; k++) put(lane, base + k, s[k]);
}
void PlanCtx::img_act(const Image& put, int lane, int base, int a) const {
  if (K == 0) return;
  const uint32_t* s = &B.w[H.o_act + a * ACT_STRIDE];
  put(lane, base + LA_TYPE, s[A_TYPE]);
  put(lane, base + LA_JOINT, s[A_JOINT]);
  for (int k = 0; k < 3; k++) put(lane, base + LA_IDX + k, s[A_IDX + k]);
  put(lane, base + LA_STR, s[A_STR]);
}
int PlanCtx::img_side(const Image& put, int lane, int base, int j, bool child) const {
  const uint32_t* s = &B.w[H.o_joint + j * JOINT_STRIDE];
  const int body = (int)s[child ? J_BC : J_BP];
  const uint32_t* bw = &B.w[H.o_body + body * BODY_STRIDE];
  for (int k = 0; k < 3; k++) {
    put(lane, base + LS_OFF + k, s[(child ? J_OFFC : J_OFFP) + k]);
    put(lane, base + LS_AX0 + k, s[(child ? J_AXC : J_AXP) + k]);
    put(lane, base + LS_AX2 + k, s[(child ? J_AXC : J_AXP) + 6 + k]);
    put(lane, base + LS_I + k, bw[BODY_I + k]);
  }
  put(lane, base + LS_M, bw[BODY_MASS]);
  put(lane, base + LS_SG, fbits(child ? -1.0 : 1.0));
  put(lane, base + LS_BODY, (uint32_t)body);
  return body;
}
// a body's record: mass, inverse inertia, pos / rot / quat masks
void PlanCtx::img_body(const Image& put, int lane, int base, int b) const {
  const uint32_t* s = &B.w[H.o_body + b * BODY_STRIDE];
  put(lane, base, s[BODY_MASS]);
  for (int k = 0; k < 3; k++) {
    put(lane, base + 1 + k, s[BODY_I + k]);
    put(lane, base + 4 + k, s[BODY_PM + k]);
    put(lane, base + 7 + k, s[BODY_RM + k]);
  }
  for (int k = 0; k < 4; k++) put(lane, base + 10 + k, s[BODY_QM + k]);
}

// the MULTI kernel's joint halves (MJ_*): revolute joints each driven by
// the torque actuator of its index, <= 128 joints (16 lanes per 8)
void PlanCtx::multi_joint_halves() {
  bool ok = H.multi && J > 0 && J <= 128 && K == J && H.act_same;
  for (int j = 0; j < J; j++) ok = ok && d->joint_type[j] == BX_JOINT_REVOLUTE;
  for (int a = 0; a < K; a++) ok = ok && d->act_type[a] == BX_ACT_TORQUE;
  mjh = ok && !knobs.no_multi_jh;
  // MULTI threads per env: 128 when the bodies, joints (joint halves: two
  // lanes each), actuators and gather tasks (two per lane) fit, so four envs
  // share a CU (two waves each, 256 registers, <= 40 KB of LDS); else 256
  H.multi_L = (N <= 128 && K <= 128 && (mjh ? 2 * J <= 128 : J <= 128) && H.T <= 2 * 128 &&
               R <= 8 * 128) ? 128 : 256;
  if (!mjh) return;
  B.align16();
  H.o_mjh = B.alloc(MJ_W * MJ_LANES);
  const Image putm{B, H.o_mjh, MJ_LANES};
  for (int l = 0; l < MJ_LANES; l++) {
    const int jx = (l >> 4) * 8 + (l & 7);
    const int j = jx < J ? jx : 0;
    img_joint(putm, l, MJ_JOINT, j);
    img_act(putm, l, MJ_ACT, j);
    img_lim(putm, l, MJ_JLIM, j, 0);
    img_side(putm, l, MJ_SIDE, j, (l & 8) != 0);
  }
}

// the SINGLE-mode lane image (pbd_layout.h LI_*): copies of the records
// above, so its words are the same bits the item-loop kernels read; a lane
// without an item of a kind gets item 0's record (as the kernels' clamped
// index did), and zeros where the system has none of that kind
void PlanCtx::single_lane_image() {
  if (!H.single) return;
  B.align16();
  H.o_lane = B.alloc(LANE_W * LANE_IMG_LANES);
  const Image put{B, H.o_lane, LANE_IMG_LANES};
  auto put_list = [&](int lane, int base, const std::vector<int>& v, bool has, uint32_t zero) {
    for (int k = 0; k < 8; k++) put(lane, base + k, has && k < (int)v.size() ? (uint32_t)v[k] : zero);
  };
  auto put_row = [&](int lane, int base, int x) {
    uint32_t rw[32];
    row_words(x >= 0 ? x : 0, rw);
    for (int k = 0; k < 32; k++) put(lane, base + k, rw[k]);
  };
  // joint halves: lane m's side body (the parent of joint m & 7 on lanes
  // 0-7 of each 16, the child on 8-15)
  auto side_body = [&](int m) {
    const int j = m & (HB - 1);
    const uint32_t* s = &B.w[H.o_joint + (j < J ? j : 0) * JOINT_STRIDE];
    return (int)s[(m & HB) ? J_BC : J_BP];
  };
  // CB (cb_rows_ok: at most one row per a body): a body's row, or -1
  std::vector<int> row_of(N, -1);
  for (int x = R - 1; x >= 0; x--) row_of[d->row_body_a[x]] = x;
  for (int l = 0; l < LANE_IMG_LANES; l++) {
    const bool hasB = l < N;
    const int b = hasB ? l : 0;
    img_body(put, l, LI_BODY, b);
    img_joint(put, l, LI_JOINT, l < J ? l : 0);
    img_act(put, l, LI_ACT, l < K ? l : 0);
    const int jh = l & (HB - 1);  // the lane's joint-halves joint
    img_joint(put, l, LI_JOINT_H, jh < J ? jh : 0);
    // the staged limit rows (stage_lim): lane l -> joint l
    img_lim(put, l, LI_JLIM, l < J ? l : 0, 0);
    img_lim(put, l, LI_JLIM12, l < J ? l : 0, 1);
    img_lim(put, l, LI_JLIM12 + 8, l < J ? l : 0, 2);
    img_lim(put, l, LI_JLIM_H, jh < J ? jh : 0, 0);
    if (J > 0) {
      // the joint-halves side: the parent's on lanes 0-7, the child's on
      // 8-15
      const bool child = (l & HB) != 0;
      const int body = img_side(put, l, LI_SIDE_H, jh < J ? jh : 0, child);
      // JB: the side body's record and gather lists; LS_OWN on the lowest
      // lane of the env's 16 whose side is that body
      const bool hasS = jh < J;
      bool own = hasS;
      for (int m = l & ~(2 * HB - 1); m < l; m++)
        if ((m & (HB - 1)) < J && side_body(m) == body) own = false;
      put(l, LI_SIDE_H + LS_OWN, own ? 1u : 0u);
      img_body(put, l, LI_BODY_J, body);
      put_list(l, LI_JL_J, jl[body], hasS, (uint32_t)(2 * J));
      put_list(l, LI_AL_J, al[body], hasS, (uint32_t)(2 * K));
      uint32_t czj = (uint32_t)(2 * R);
      if (hasS && !cl[body].empty()) czj |= (uint32_t)cl[body][0] & 0x7F000000u;
      put_list(l, LI_CL_J, cl[body], hasS, czj);
      // CB: the side body's row (row 0's record where it has none)
      if (R > 0) {
        const int x = hasS ? row_of[body] : -1;
        put_row(l, LI_ROW_J, x);
        put(l, LI_ROW_J + LRJ_HAS, x >= 0 ? 1u : 0u);
      }
    }
    img_act(put, l, LI_ACT_H, jh < K ? jh : 0);
    if (R > 0) {
      put_row(l, LI_ROW, l < R ? l : 0);
      // F_R2: the lane's two rows (slot1[l], slot2[l])
      if (r2 && l < 16) {
        put_row(l, LI_ROW, slot1[l]);
        put_row(l, LI_ROW2, slot2[l]);
        put(l, LI_RIDX, (uint32_t)slot1[l]);
        put(l, LI_RIDX + 1, (uint32_t)slot2[l]);
      }
    }
    put_list(l, LI_JL, jl[b], hasB, (uint32_t)(2 * J));
    put_list(l, LI_AL, al[b], hasB, (uint32_t)(2 * K));
    // contact entries carry their collider group in bits 24..30; the padding
    // entry takes the group of the body's first entry (it adds exact zeros)
    uint32_t cz = (uint32_t)(2 * R);
    if (hasB && !cl[b].empty()) cz |= (uint32_t)cl[b][0] & 0x7F000000u;
    put_list(l, LI_CL, cl[b], hasB, cz);
    // F_C16: entries 8..15 of the contact list
    for (int k = 0; k < 8; k++)
      put(l, LI_CL2 + k, hasB && 8 + k < (int)cl[b].size() ? (uint32_t)cl[b][8 + k] : cz);
  }
}

// the system's feature mask (F_* of pbd_features.h: what its joints,
// actuators, colliders and layout need), which picks its step kernels
int PlanCtx::system_feat() const {
  int f = 0;
  for (int j = 0; j < J; j++) if (d->joint_type[j] != BX_JOINT_REVOLUTE) f |= F_SPH;
  for (int a = 0; a < K; a++) if (d->act_type[a] != BX_ACT_TORQUE) f |= F_ANGLE;
  for (int g = 0; g < G; g++) {
    if (d->col_fn[g] != BX_COL_CAPSULE_PLANE) f |= F_CC;
    if (!d->col_oneway[g]) f |= F_TW;
  }
  if (d->n_forces > 0) f |= F_FORCE;
  if (max_groups <= 1) f |= F_G1;  // one collider group per body
  if (xcol) f |= F_X;              // extended contact functions
  // F_JH (joint halves, SINGLE mode at 16 lanes): <= 8 revolute joints, each
  // driven by the actuator of the same index
  if (H.single && L == 16 && J <= 8 && K <= 8 && H.act_same && !(f & F_SPH) && !knobs.no_joint_halves)
    f |= F_JH;
  if (r2) f |= F_R2;               // two contact rows per lane (SINGLE mode, 16 lanes)
  if (H.single && c16) f |= F_C16;  // 16-entry contact gather lists
  if (r2g) f |= F_R2G;             // one contact function per row slot
  return f;
}

// the plan's decisions: features, gather width, the staged limit rows, mode,
// lanes, fold / JB / CB and the LDS sizes; the header goes into the blob
int PlanCtx::decide(Plan* P) {
  const int f = system_feat();
  // the SINGLE kernel this system launches reads its joints' limit rows
  // from LDS when its feature set carries spherical joints (F_SPH; the
  // all-features instantiations too): carve the rows' region then (6
  // 16-byte groups per lane), not otherwise (Ant keeps its LDS footprint:
  // 32 envs per CU for the 2-wave kernels at 32,768 envs)
  if (H.single && (single_variant(L, f, gather_width()).F & F_SPH)) {
    H.l_jlim = jlim_at;
    H.env_words = (jlim_at + 24 * L + 63) & ~63;
  }
  H.total_words = (int)B.w.size();
  std::memcpy(B.w.data(), &H, sizeof(BlobHdr));

  P->hdr = H;
  P->single_ok = H.single != 0;
  P->min_L = L;
  P->gw = gather_width();
  P->feat = f;
  P->fold = (H.act_same && K == J && J > 0 && !(f & F_ANGLE)) ? 1 : 0;
  // the bodies on a joint side
  std::vector<char> side(N, 0);
  for (int j = 0; j < J; j++) side[d->joint_body_p[j]] = side[d->joint_body_c[j]] = 1;
  // JB's body conditions (the env kernels whose joint-halves lanes own body
  // copies): every body on no joint side is frozen in all dimensions
  // (position, rotation and the quaternion's vector part masks zero) and
  // touches contact rows only as the plane side of one-way rows (its record
  // then never changes and its contact sums are zeros)
  auto jb_bodies_ok = [&]() {
    for (int b = 0; b < N; b++) {
      if (side[b]) continue;
      const uint32_t* bw = &B.w[H.o_body + b * BODY_STRIDE];
      for (int k = 0; k < 3; k++)
        if (bw[BODY_PM + k] != fbits(0.0) || bw[BODY_RM + k] != fbits(0.0)) return false;
      // (the reference's quaternion mask keeps w at 1 for a frozen rotation:
      // integrators.py's [0] + frozen.rotation; the w update is an exact zero)
      for (int k = 1; k < 4; k++)
        if (bw[BODY_QM + k] != fbits(0.0)) return false;
    }
    for (int x = 0; x < R; x++) {
      if (!side[d->row_body_a[x]]) return false;
      if (!side[d->row_body_b[x]] && !d->col_oneway[d->row_group[x]]) return false;
    }
    return true;
  };
  // CB's row conditions (the JB kernels that resolve a body's contact row on
  // the body's own lanes, pbd_features.h cb_feat): one collider group of
  // one-way capsule-plane rows, each against a body on no joint side (frozen
  // under jb_bodies_ok), at most one row per a body
  auto cb_rows_ok = [&]() {
    if (G != 1 || d->col_fn[0] != BX_COL_CAPSULE_PLANE || !d->col_oneway[0]) return false;
    std::vector<int> rows(N, 0);
    for (int x = 0; x < R; x++) {
      if (side[d->row_body_b[x]] || ++rows[d->row_body_a[x]] > 1) return false;
    }
    return true;
  };
  // JB (the Ant / HalfCheetah env kernels: joint halves own body copies):
  // JB's body conditions (jb_bodies_ok) and no forces (they index bodies
  // by lane)
  // (BX_NO_JB=1: off, the Ant / HalfCheetah kinds then take the all-kinds
  // kernel; the GPU tests run that fallback against the goldens too)
  const bool jb = P->fold && (f & F_JH) && !(f & F_FORCE) && L == 16 && !knobs.no_jb && jb_bodies_ok();
  P->jb = jb ? 1 : 0;
  // CB: a JB system whose rows its kernel can resolve on the body lanes
  // (cb_rows_ok). The Ant kind's own kernels are compiled that way
  // (cb_feat), so an Ant-kind system without it takes the all-kinds kernel
  P->cb = (jb && cb_feat(f) && cb_rows_ok()) ? 1 : 0;
  if (knobs.debug)
    fprintf(stderr, "bx plan: fold=%d body_copies=%d contact_on_body=%d\n", P->fold, P->jb, P->cb);
  // the MULTI kernel is instantiated for the lean feature set (revolute,
  // torque, capsule-plane / capsule-capsule, no forces)
  P->multi_ok = H.multi != 0 && (f & (F_SPH | F_ANGLE | F_FORCE | F_X)) == 0;
  P->mode = P->single_ok ? MODE_SINGLE : (P->multi_ok ? MODE_MULTI : MODE_GLOBAL);
  P->words = std::move(B.w);
  P->L = P->multi_ok ? H.multi_L : L;
  P->tpb = P->L > 64 ? P->L : 64;
  P->lds_env = (size_t)(L > 64 ? 1 : 64 / L) * H.env_words * 4;
  P->lds_reset = (size_t)64 * N * 13 * 4;
  if (P->lds_env > 160 * 1024) return fail("system too large for one workgroup's LDS");
  if (r && P->lds_reset > 160 * 1024) return fail("system too large for the reset kernel's LDS");
  return 0;
}

}  // namespace

int build_plan(const bx_desc* desc, const bx_reset_desc* reset, const PlanKnobs& knobs,
               Plan* plan, std::string* err) {
  PlanCtx c(desc, reset, knobs, err);
  if (c.validate()) return 1;
  c.pack_bodies_joints_actuators();
  c.pack_rows_groups_forces();
  c.gather_lists();
  c.multi_tasks();
  if (c.reset_tables()) return 1;
  c.shape_limits();
  c.dedupe_row_tables();
  c.lds_head();
  c.lds_multi_tail();
  c.lds_item_tail();
  c.mode_fits();
  c.multi_row_tables();
  c.row_slots();
  c.multi_joint_halves();
  c.single_lane_image();
  return c.decide(plan);
}

}  // namespace bx
