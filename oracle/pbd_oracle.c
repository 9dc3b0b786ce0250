/*
 * pbd_oracle.c — CPU RESTATEMENT OF THE REFERENCE, TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the reference's position-based-dynamics step
 * (`brax/physics/system.py:254-325`) and the Ant/Humanoid/HalfCheetah env
 * layer, compiled twice: REAL=double (the checker, pinned to the reference's
 * own float64 numpy execution by tests/golden/*.npz) and REAL=float (the CPU
 * baseline timed by bench.py, OpenMP over envs). Only tests/, smoke() and
 * bench.py's cpu_baseline leg may load it; the product path never does.
 *
 * Each function cites the reference file:line it restates. Array layout here
 * is the oracle's own: qp (B,N,13) = pos, rot(wxyz), vel, ang.
 */
#define _USE_MATH_DEFINES
#include <math.h>
#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/brax_amd.h"

#ifndef REAL
#define REAL double
#endif
#ifndef SUF
#define SUF _f64
#endif
#define CAT2(a, b) a##b
#define CAT(a, b) CAT2(a, b)
#define FN(name) CAT(name, SUF)

typedef REAL R;

/* 1: emulate jnp safe_norm's allclose(x, 0) zero guard (jumpy.py:183-189);
 * 0: plain norm, as the numpy backend the goldens come from (jumpy.py:190). */
static int g_safe_guard = 1;

void FN(oracle_set_safe_norm_guard)(int on) { g_safe_guard = on; }

/* width of the action rows the next calls receive (0: action_size); indices
 * are clipped into it like jp.take(mode='clip') (jumpy.py:146-151) */
static int g_act_width = 0;
void FN(oracle_set_act_width)(int w) { g_act_width = w; }
/* GRASP's action map [2, n] (per action min, range; grasp.py:42-52) */
static double g_act_map[2 * 64];
static int g_act_map_n = 0;
void FN(oracle_set_act_map)(const double* m, int n) {
  g_act_map_n = n < 64 ? n : 64;
  for (int i = 0; i < g_act_map_n; i++) { g_act_map[i] = m[i]; g_act_map[64 + i] = m[n + i]; }
}
static inline int take_idx(int i, int w) { return i < 0 ? 0 : (i >= w ? w - 1 : i); }
void FN(oracle_set_threads)(int n) {
#ifdef _OPENMP
  if (n > 0) omp_set_num_threads(n);
#else
  (void)n;
#endif
}
int FN(oracle_max_threads)(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

/* ---------------------------------------------------------------- math --- */
/* brax/math.py and the jumpy helpers it uses */

static inline R dot3(const R* a, const R* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static inline void cross3(const R* a, const R* b, R* o) {
  R x = a[1] * b[2] - a[2] * b[1];
  R y = a[2] * b[0] - a[0] * b[2];
  R z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
static inline R norm3(const R* a) { return (R)sqrt(dot3(a, a)); }
/* jumpy.py:170-192 */
static inline R safe_norm3(const R* a) {
  if (g_safe_guard && fabs((double)a[0]) <= 1e-8 && fabs((double)a[1]) <= 1e-8 &&
      fabs((double)a[2]) <= 1e-8)
    return (R)0;
  return norm3(a);
}
/* math.py:25-40 */
static inline void rotate(const R* v, const R* q, R* o) {
  R s = q[0];
  const R* u = q + 1;
  R uv = dot3(u, v), uu = dot3(u, u);
  R c[3];
  cross3(u, v, c);
  R r0 = 2 * (uv * u[0]) + (s * s - uu) * v[0];
  R r1 = 2 * (uv * u[1]) + (s * s - uu) * v[1];
  R r2 = 2 * (uv * u[2]) + (s * s - uu) * v[2];
  o[0] = r0 + 2 * s * c[0];
  o[1] = r1 + 2 * s * c[1];
  o[2] = r2 + 2 * s * c[2];
}
/* math.py:130-145 */
static inline void quat_mul(const R* u, const R* v, R* o) {
  R w = u[0] * v[0] - u[1] * v[1] - u[2] * v[2] - u[3] * v[3];
  R x = u[0] * v[1] + u[1] * v[0] + u[2] * v[3] - u[3] * v[2];
  R y = u[0] * v[2] - u[1] * v[3] + u[2] * v[0] + u[3] * v[1];
  R z = u[0] * v[3] + u[1] * v[2] - u[2] * v[1] + u[3] * v[0];
  o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
/* math.py:148-170 */
static inline void vec_quat_mul(const R* u, const R* v, R* o) {
  R w = -u[0] * v[1] - u[1] * v[2] - u[2] * v[3];
  R x = u[0] * v[0] + u[1] * v[3] - u[2] * v[2];
  R y = -u[0] * v[3] + u[1] * v[0] + u[2] * v[1];
  R z = u[0] * v[2] - u[1] * v[1] + u[2] * v[0];
  o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
/* math.py:173-187 */
static inline void quat_rot_axis(const R* axis, R angle, R* o) {
  R s = (R)sin(angle / 2), c = (R)cos(angle / 2);
  o[0] = c; o[1] = axis[0] * s; o[2] = axis[1] * s; o[3] = axis[2] * s;
}
/* math.py:190-199 */
static inline void quat_inv(const R* q, R* o) { o[0] = q[0]; o[1] = -q[1]; o[2] = -q[2]; o[3] = -q[3]; }
/* math.py:116-127 */
static inline R signed_angle(const R* axis, const R* ref_p, const R* ref_c) {
  R c[3];
  cross3(ref_p, ref_c, c);
  return (R)atan2(dot3(c, axis), dot3(ref_p, ref_c));
}
static inline R clip(R x, R lo, R hi) { return x < lo ? lo : (x > hi ? hi : x); }
static inline R sgn(R x) { return (R)((x > 0) - (x < 0)); }

/* ----------------------------------------------------------- descriptor --- */
/* the descriptor's float64 constants, cast once to REAL (jit casts the
 * Python-double constants to fp32 the same way) */
typedef struct {
  const bx_desc* d;
  int N, J, K, Rn, G, A, aw, NF;
  R h, g[3], vdamp_exp, adamp_exp;
  R *fstr, *fmass;
  R *mass, *inv_mass, *I, *pos_mask, *rot_mask, *quat_mask;
  R *joff_p, *joff_c, *jax_p, *jax_c, *jlim, *jdamp, *jsp, *jsa;
  R *jstiff, *jsdamp, *jlstr;  /* legacy_spring (spring_joints.py:57-67) */
  int spring;
  R *astr;
  R *gscale, *gthr, *gerp;
  R *ra_pos, *ra_end, *ra_rad, *rb_pos, *rb_end, *rb_rad, *rfric, *relas;
  R *rext, *hm;  /* extended contact functions: row constants (R,16), heightmaps */
  R *hv, *hf, *hn; /* box hulls: corners (H,8,3), quads (H,6,4,3), normals (H,6,3) */
} sysc;

static R* cvt(const double* s, int n) {
  R* o = (R*)malloc(sizeof(R) * (n > 0 ? n : 1));
  for (int i = 0; i < n; i++) o[i] = s ? (R)s[i] : (R)0;
  return o;
}

static void sys_init(sysc* s, const bx_desc* d) {
  s->d = d;
  s->N = d->n_bodies; s->J = d->n_joints; s->K = d->n_actuators;
  s->Rn = d->n_rows; s->G = d->n_groups; s->A = d->action_size;
  s->aw = g_act_width > 0 ? g_act_width : d->action_size;
  s->NF = d->n_forces;
  s->fstr = cvt(d->force_strength, s->NF);
  s->fmass = (R*)malloc(sizeof(R) * (s->NF > 0 ? s->NF : 1));
  for (int f = 0; f < s->NF; f++) s->fmass[f] = (R)d->body_mass[d->force_body[f]];
  s->h = (R)d->h;
  for (int k = 0; k < 3; k++) s->g[k] = (R)d->gravity[k];
  /* integrators.py:87,91: exp(damping * dt) of Python floats -> a constant */
  s->vdamp_exp = (R)exp(d->velocity_damping * d->h);
  s->adamp_exp = (R)exp(d->angular_damping * d->h);
  int N = s->N, J = s->J, Rn = s->Rn;
  s->mass = cvt(d->body_mass, N);
  s->inv_mass = (R*)malloc(sizeof(R) * (N ? N : 1));
  for (int i = 0; i < N; i++) s->inv_mass[i] = (R)(1.0 / d->body_mass[i]);
  s->I = cvt(d->body_inv_inertia, 3 * N);
  s->pos_mask = cvt(d->pos_mask, 3 * N);
  s->rot_mask = cvt(d->rot_mask, 3 * N);
  s->quat_mask = cvt(d->quat_mask, 4 * N);
  s->joff_p = cvt(d->joint_off_p, 3 * J);
  s->joff_c = cvt(d->joint_off_c, 3 * J);
  s->jax_p = cvt(d->joint_axis_p, 9 * J);
  s->jax_c = cvt(d->joint_axis_c, 9 * J);
  s->jlim = cvt(d->joint_limit, 6 * J);
  s->jdamp = cvt(d->joint_damping, J);
  s->jsp = cvt(d->joint_scale_pos, J);
  s->jsa = cvt(d->joint_scale_ang, J);
  s->spring = d->dynamics_mode == BX_DYN_LEGACY_SPRING;
  s->jstiff = cvt(d->joint_stiffness, J);
  s->jsdamp = cvt(d->joint_spring_damping, J);
  s->jlstr = cvt(d->joint_limit_strength, J);
  s->astr = cvt(d->act_strength, s->K);
  s->gscale = cvt(d->col_scale, s->G);
  s->gthr = cvt(d->col_velocity_threshold, s->G);
  s->gerp = cvt(d->col_baumgarte_erp, s->G);
  s->ra_pos = cvt(d->row_a_pos, 3 * Rn);
  s->ra_end = cvt(d->row_a_end, 3 * Rn);
  s->ra_rad = cvt(d->row_a_radius, Rn);
  s->rb_pos = cvt(d->row_b_pos, 3 * Rn);
  s->rb_end = cvt(d->row_b_end, 3 * Rn);
  s->rb_rad = cvt(d->row_b_radius, Rn);
  s->rfric = cvt(d->row_friction, Rn);
  s->relas = cvt(d->row_elasticity, Rn);
  s->rext = cvt(d->row_ext, 16 * Rn);
  s->hm = cvt(d->hm_data, d->n_hm);
  s->hv = cvt(d->hull_vert, 24 * d->n_hull);
  s->hf = cvt(d->hull_face, 72 * d->n_hull);
  s->hn = cvt(d->hull_norm, 18 * d->n_hull);
}

static void sys_free(sysc* s) {
  R** p[] = {&s->mass, &s->inv_mass, &s->I, &s->pos_mask, &s->rot_mask, &s->quat_mask,
             &s->joff_p, &s->joff_c, &s->jax_p, &s->jax_c, &s->jlim, &s->jdamp,
             &s->jsp, &s->jsa, &s->astr, &s->gscale, &s->gthr, &s->gerp,
             &s->ra_pos, &s->ra_end, &s->ra_rad, &s->rb_pos, &s->rb_end,
             &s->rb_rad, &s->rfric, &s->relas, &s->fstr, &s->fmass,
             &s->jstiff, &s->jsdamp, &s->jlstr, &s->rext, &s->hm, &s->hv, &s->hf, &s->hn};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(*p[i]);
}

/* ------------------------------------------------------------ state ------ */
typedef struct { R pos[3], rot[4], vel[3], ang[3]; } body_t;

/* workspace per env */
typedef struct {
  body_t *qp, *qprev, *qrb;
  R *dp_a, *dp_j, *acc;          /* (N,3) angular */
  R *dq_pos, *dq_rot;            /* (N,3),(N,4) */
  R *dp_vel, *dp_ang;            /* (N,3) */
  R *cnt;                        /* (N) */
  R *gpos, *grot, *gvel, *gang;  /* per-group scratch (N,3/4) */
  R *c_pos, *c_norm, *c_pen, *c_vel, *dlam; /* contact rows */
  R *info_c, *info_a;            /* (N,6) accumulators */
  R *sj_v, *sj_a, *info_j;       /* legacy_spring: dp_j (N,3)x2, Info.joint (N,6) */
  int* ract;                     /* (R) NearNeighbors rank, -1 = culled */
} work_t;

static void work_alloc(work_t* w, int N, int Rn) {
  int n = N > 0 ? N : 1, r = Rn > 0 ? Rn : 1;
  w->qp = calloc(n, sizeof(body_t)); w->qprev = calloc(n, sizeof(body_t));
  w->qrb = calloc(n, sizeof(body_t));
  w->dp_a = calloc(3 * n, sizeof(R)); w->dp_j = calloc(3 * n, sizeof(R));
  w->acc = calloc(3 * n, sizeof(R));
  w->dq_pos = calloc(3 * n, sizeof(R)); w->dq_rot = calloc(4 * n, sizeof(R));
  w->dp_vel = calloc(3 * n, sizeof(R)); w->dp_ang = calloc(3 * n, sizeof(R));
  w->cnt = calloc(n, sizeof(R));
  w->gpos = calloc(3 * n, sizeof(R)); w->grot = calloc(4 * n, sizeof(R));
  w->gvel = calloc(3 * n, sizeof(R)); w->gang = calloc(3 * n, sizeof(R));
  w->c_pos = calloc(3 * r, sizeof(R)); w->c_norm = calloc(3 * r, sizeof(R));
  w->c_pen = calloc(r, sizeof(R)); w->c_vel = calloc(3 * r, sizeof(R));
  w->dlam = calloc(r, sizeof(R));
  w->info_c = calloc(6 * n, sizeof(R)); w->info_a = calloc(6 * n, sizeof(R));
  w->ract = calloc(r, sizeof(int));
  w->sj_v = calloc(3 * n, sizeof(R)); w->sj_a = calloc(3 * n, sizeof(R));
  w->info_j = calloc(6 * n, sizeof(R));
}
static void work_free(work_t* w) {
  void* p[] = {w->qp, w->qprev, w->qrb, w->dp_a, w->dp_j, w->acc, w->dq_pos, w->dq_rot,
               w->dp_vel, w->dp_ang, w->cnt, w->gpos, w->grot, w->gvel, w->gang,
               w->c_pos, w->c_norm, w->c_pen, w->c_vel, w->dlam, w->info_c, w->info_a,
               w->ract, w->sj_v, w->sj_a, w->info_j};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
}

static void load_qp(body_t* qp, const R* src, int N) {
  for (int b = 0; b < N; b++) {
    const R* s = src + 13 * b;
    memcpy(qp[b].pos, s, 3 * sizeof(R)); memcpy(qp[b].rot, s + 3, 4 * sizeof(R));
    memcpy(qp[b].vel, s + 7, 3 * sizeof(R)); memcpy(qp[b].ang, s + 10, 3 * sizeof(R));
  }
}
static void store_qp(const body_t* qp, R* dst, int N) {
  for (int b = 0; b < N; b++) {
    R* s = dst + 13 * b;
    memcpy(s, qp[b].pos, 3 * sizeof(R)); memcpy(s + 3, qp[b].rot, 4 * sizeof(R));
    memcpy(s + 7, qp[b].vel, 3 * sizeof(R)); memcpy(s + 10, qp[b].ang, 3 * sizeof(R));
  }
}

/* -------------------------------------------------------------- joints --- */

/* Revolute.axis_angle (joints.py:311-319) / Spherical.axis_angle (:388-415) */
static int axis_angle(const sysc* s, int j, const body_t* p, const body_t* c,
                      R axes[3][3], R ang[3]) {
  const R* axp = s->jax_p + 9 * j;
  const R* axc = s->jax_c + 9 * j;
  if (s->d->joint_type[j] == BX_JOINT_REVOLUTE) {
    R ref_p[3], ref_c[3];
    rotate(axp, p->rot, axes[0]);
    rotate(axp + 6, p->rot, ref_p);
    rotate(axc + 6, c->rot, ref_c);
    ang[0] = signed_angle(axes[0], ref_p, ref_c);
    return 1;
  }
  R a1p[3], a2p[3], a1c[3], a2c[3], a3c[3];
  rotate(axp, p->rot, a1p);
  rotate(axp + 3, p->rot, a2p);
  rotate(axc, c->rot, a1c);
  rotate(axc + 3, c->rot, a2c);
  rotate(axc + 6, c->rot, a3c);
  R lon[3];
  cross3(a3c, a1p, lon);
  R ln = (R)1e-10 + safe_norm3(lon);
  for (int k = 0; k < 3; k++) lon[k] /= ln;
  R psi = signed_angle(a1p, a2p, lon);
  R d11 = dot3(a1p, a1c), d12 = dot3(a1p, a2c);
  R xz[3];
  for (int k = 0; k < 3; k++) xz[k] = d11 * a1c[k] + d12 * a2c[k];
  R xn = (R)1e-10 + safe_norm3(xz);
  for (int k = 0; k < 3; k++) xz[k] /= xn;
  R cb = dot3(xz, a1p);
  R theta = (R)acos(clip(cb, -1, 1)) * sgn(dot3(a1p, a3c));
  R ycn[3] = {-a3c[0], -a3c[1], -a3c[2]};
  R phi = signed_angle(ycn, a2c, lon);
  memcpy(axes[0], a1p, sizeof(a1p));
  memcpy(axes[1], a2c, sizeof(a2c));
  memcpy(axes[2], a3c, sizeof(a3c));
  ang[0] = psi; ang[1] = theta; ang[2] = phi;
  /* spring Universal.axis_angle (spring_joints.py:188-216): (psi, theta) */
  return s->d->joint_type[j] == BX_JOINT_UNIVERSAL ? 2 : 3;
}

/* Joint.apply_angle_update (joints.py:130-152); accumulates into dq (7 per side) */
static void angle_update(const sysc* s, int j, const body_t* p, const body_t* c,
                         const R* dq, R* out_p, R* out_c) {
  int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
  const R* Ip = s->I + 3 * bp;
  const R* Ic = s->I + 3 * bc;
  R th = safe_norm3(dq);
  R n[3];
  for (int k = 0; k < 3; k++) n[k] = dq[k] / (th + (R)1e-6);
  R w1 = n[0] * (Ip[0] * n[0]) + n[1] * (Ip[1] * n[1]) + n[2] * (Ip[2] * n[2]);
  R w2 = n[0] * (Ic[0] * n[0]) + n[1] * (Ic[1] * n[1]) + n[2] * (Ic[2] * n[2]);
  R dl = -th / (w1 + w2 + (R)1e-6);
  R pv[3] = {-dl * n[0], -dl * n[1], -dl * n[2]};
  R t[3], q[4];
  R sa = s->jsa[j];
  for (int k = 0; k < 3; k++) t[k] = Ip[k] * pv[k];
  vec_quat_mul(t, p->rot, q);
  for (int k = 0; k < 4; k++) out_p[3 + k] += sa * ((R)0.5 * q[k]);
  for (int k = 0; k < 3; k++) t[k] = Ic[k] * pv[k];
  vec_quat_mul(t, c->rot, q);
  for (int k = 0; k < 4; k++) out_c[3 + k] += sa * ((R)-0.5 * q[k]);
  /* dq pos is scale_ang * zeros: adds exact zeros */
}

/* Joint.apply_position_update (joints.py:154-195) */
static void position_update(const sysc* s, int j, const body_t* p, const body_t* c,
                            const R* pos_p_w, const R* pos_c_w, R* out_p, R* out_c) {
  int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
  const R* Ip = s->I + 3 * bp;
  const R* Ic = s->I + 3 * bc;
  R dx[3], rp[3], rc[3];
  for (int k = 0; k < 3; k++) {
    dx[k] = pos_p_w[k] - pos_c_w[k];
    rp[k] = pos_p_w[k] - p->pos[k];
    rc[k] = pos_c_w[k] - c->pos[k];
  }
  R cc = safe_norm3(dx);
  R n[3];
  for (int k = 0; k < 3; k++) n[k] = dx[k] / (cc + (R)1e-6);
  R cr1[3], cr2[3];
  cross3(rp, n, cr1);
  cross3(rc, n, cr2);
  R w1 = (R)1 / s->mass[bp] +
         (cr1[0] * (Ip[0] * cr1[0]) + cr1[1] * (Ip[1] * cr1[1]) + cr1[2] * (Ip[2] * cr1[2]));
  R w2 = (R)1 / s->mass[bc] +
         (cr2[0] * (Ic[0] * cr2[0]) + cr2[1] * (Ic[1] * cr2[1]) + cr2[2] * (Ic[2] * cr2[2]));
  R dl = -cc / (w1 + w2 + (R)1e-6);
  R pv[3] = {dl * n[0], dl * n[1], dl * n[2]};
  R sp = s->jsp[j];
  R t[3], u[3], q[4];
  cross3(rp, pv, t);
  for (int k = 0; k < 3; k++) u[k] = Ip[k] * t[k];
  vec_quat_mul(u, p->rot, q);
  for (int k = 0; k < 3; k++) out_p[k] += sp * (pv[k] / s->mass[bp]);
  for (int k = 0; k < 4; k++) out_p[3 + k] += sp * ((R)0.5 * q[k]);
  cross3(rc, pv, t);
  for (int k = 0; k < 3; k++) u[k] = Ic[k] * t[k];
  vec_quat_mul(u, c->rot, q);
  for (int k = 0; k < 3; k++) out_c[k] += sp * (-pv[k] / s->mass[bc]);
  for (int k = 0; k < 4; k++) out_c[3 + k] += sp * ((R)-0.5 * q[k]);
}

/* Revolute.apply_reduced (joints.py:270-309), Spherical (:332-386).
 * out_p/out_c: 7 (pos3, rot4) zero-initialised */
static void joint_apply_one(const sysc* s, int j, const body_t* qp, R* out_p, R* out_c) {
  const bx_desc* d = s->d;
  const body_t* p = &qp[d->joint_body_p[j]];
  const body_t* c = &qp[d->joint_body_c[j]];
  const R* axp = s->jax_p + 9 * j;
  const R* axc = s->jax_c + 9 * j;
  const R* lim = s->jlim + 6 * j;
  R pw[3], cw[3];
  rotate(s->joff_p + 3 * j, p->rot, pw);
  rotate(s->joff_c + 3 * j, c->rot, cw);
  for (int k = 0; k < 3; k++) { pw[k] += p->pos[k]; cw[k] += c->pos[k]; }
  position_update(s, j, p, c, pw, cw, out_p, out_c);
  if (d->joint_type[j] == BX_JOINT_REVOLUTE) {
    R axis[3], ref_p[3], ref_c[3], axis_c[3];
    rotate(axp, p->rot, axis);
    rotate(axp + 6, p->rot, ref_p);
    rotate(axc + 6, c->rot, ref_c);
    R psi = signed_angle(axis, ref_p, ref_c);
    rotate(axc, c->rot, axis_c);
    R dq1[3], dq2[3], fix[4], n1[3];
    cross3(axis, axis_c, dq1);
    R ph = clip(psi, lim[0], lim[1]);
    quat_rot_axis(axis, ph, fix);
    rotate(ref_p, fix, n1);
    cross3(n1, ref_c, dq2);
    /* v_apply over [dq_1, dq_2], summed then added (joints.py:299-307) */
    R ap[2][7] = {{0}}, ac[2][7] = {{0}};
    angle_update(s, j, p, c, dq1, ap[0], ac[0]);
    angle_update(s, j, p, c, dq2, ap[1], ac[1]);
    for (int k = 0; k < 7; k++) {
      out_p[k] += ap[0][k] + ap[1][k];
      out_c[k] += ac[0][k] + ac[1][k];
    }
    return;
  }
  /* Spherical */
  R a1p[3], a2p[3], a1c[3], a2c[3], a3c[3];
  rotate(axp, p->rot, a1p);
  rotate(axp + 3, p->rot, a2p);
  rotate(axc, c->rot, a1c);
  rotate(axc + 3, c->rot, a2c);
  rotate(axc + 6, c->rot, a3c);
  R lon[3];
  cross3(a3c, a1p, lon);
  R ln = (R)1e-6 + safe_norm3(lon);
  for (int k = 0; k < 3; k++) lon[k] /= ln;
  R d11 = dot3(a1p, a1c), d12 = dot3(a1p, a2c);
  R xz[3];
  for (int k = 0; k < 3; k++) xz[k] = d11 * a1c[k] + d12 * a2c[k];
  R xn = (R)1e-6 + safe_norm3(xz);
  for (int k = 0; k < 3; k++) xz[k] /= xn;
  R a2n[3];
  cross3(xz, a1p, a2n);
  R an = (R)1e-6 + safe_norm3(a2n);
  for (int k = 0; k < 3; k++) a2n[k] /= an;
  R sg = sgn(dot3(a1p, a3c));
  R nvec[3][3], n1v[3][3], n2v[3][3];
  for (int k = 0; k < 3; k++) {
    nvec[0][k] = a1p[k]; n1v[0][k] = a2p[k]; n2v[0][k] = lon[k];
    nvec[1][k] = -a2n[k] * sg; n1v[1][k] = a1p[k]; n2v[1][k] = xz[k];
    nvec[2][k] = -(-a3c[k]); n1v[2][k] = lon[k]; n2v[2][k] = a2c[k];
  }
  R acc_p[7] = {0}, acc_c[7] = {0};
  for (int l = 0; l < 3; l++) {
    /* limit_angle (joints.py:343-355) */
    R ph = signed_angle(nvec[l], n1v[l], n2v[l]);
    R lo = lim[2 * l], hi = lim[2 * l + 1];
    R mask = ph < lo ? (R)1 : (R)0;
    mask = ph > hi ? (R)1 : mask;
    ph = clip(ph, lo, hi);
    R fix[4], n1[3], dq[3];
    quat_rot_axis(nvec[l], ph, fix);
    rotate(n1v[l], fix, n1);
    cross3(n1, n2v[l], dq);
    for (int k = 0; k < 3; k++) dq[k] *= mask;
    R ap[7] = {0}, ac[7] = {0};
    angle_update(s, j, p, c, dq, ap, ac);
    for (int k = 0; k < 7; k++) { acc_p[k] += ap[k]; acc_c[k] += ac[k]; }
  }
  for (int k = 0; k < 7; k++) { out_p[k] += acc_p[k]; out_c[k] += acc_c[k]; }
}

/* Joint.apply (joints.py:79-100), summed over joint groups (system.py:272) */
static void joints_apply(const sysc* s, work_t* w) {
  int N = s->N, J = s->J;
  memset(w->dq_pos, 0, sizeof(R) * 3 * N);
  memset(w->dq_rot, 0, sizeof(R) * 4 * N);
  int j0 = 0;
  while (j0 < J) {
    int g = s->d->joint_group[j0], j1 = j0;
    while (j1 < J && s->d->joint_group[j1] == g) j1++;
    memset(w->gpos, 0, sizeof(R) * 3 * N);
    memset(w->grot, 0, sizeof(R) * 4 * N);
    R (*op)[7] = calloc(j1 - j0, sizeof(R[7]));
    R (*oc)[7] = calloc(j1 - j0, sizeof(R[7]));
    for (int j = j0; j < j1; j++) joint_apply_one(s, j, w->qp, op[j - j0], oc[j - j0]);
    /* segment_sum over concat(parents, children) */
    for (int j = j0; j < j1; j++) {
      int b = s->d->joint_body_p[j];
      for (int k = 0; k < 3; k++) w->gpos[3 * b + k] += op[j - j0][k];
      for (int k = 0; k < 4; k++) w->grot[4 * b + k] += op[j - j0][3 + k];
    }
    for (int j = j0; j < j1; j++) {
      int b = s->d->joint_body_c[j];
      for (int k = 0; k < 3; k++) w->gpos[3 * b + k] += oc[j - j0][k];
      for (int k = 0; k < 4; k++) w->grot[4 * b + k] += oc[j - j0][3 + k];
    }
    for (int i = 0; i < 3 * N; i++) w->dq_pos[i] += w->gpos[i];
    for (int i = 0; i < 4 * N; i++) w->dq_rot[i] += w->grot[i];
    free(op); free(oc);
    j0 = j1;
  }
}

/* Joint.damp (joints.py:103-128), per group, summed into dp_j */
static void joints_damp(const sysc* s, work_t* w) {
  int N = s->N, J = s->J;
  memset(w->dp_j, 0, sizeof(R) * 3 * N);
  int j0 = 0;
  while (j0 < J) {
    int g = s->d->joint_group[j0], j1 = j0;
    while (j1 < J && s->d->joint_group[j1] == g) j1++;
    memset(w->gang, 0, sizeof(R) * 3 * N);
    for (int pass = 0; pass < 2; pass++) {
      for (int j = j0; j < j1; j++) {
        int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
        R tq[3];
        for (int k = 0; k < 3; k++)
          tq[k] = (R)-1 * s->jdamp[j] * (w->qp[bp].ang[k] - w->qp[bc].ang[k]);
        if (pass == 0)
          for (int k = 0; k < 3; k++) w->gang[3 * bp + k] += s->I[3 * bp + k] * tq[k];
        else
          for (int k = 0; k < 3; k++) w->gang[3 * bc + k] += -s->I[3 * bc + k] * tq[k];
      }
    }
    for (int i = 0; i < 3 * N; i++) w->dp_j[i] += w->gang[i];
    j0 = j1;
  }
}

/* Actuator.apply + Torque/Angle.apply_reduced (actuators.py:52-112) */
static void actuators_apply(const sysc* s, work_t* w, const R* act) {
  int N = s->N, K = s->K;
  memset(w->dp_a, 0, sizeof(R) * 3 * N);
  int k0 = 0;
  while (k0 < K) {
    int g = s->d->act_group[k0], k1 = k0;
    while (k1 < K && s->d->act_group[k1] == g) k1++;
    memset(w->gang, 0, sizeof(R) * 3 * N);
    R (*tp)[3] = calloc(k1 - k0, sizeof(R[3]));
    R (*tc)[3] = calloc(k1 - k0, sizeof(R[3]));
    for (int a = k0; a < k1; a++) {
      int j = s->d->act_joint[a];
      int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
      R axes[3][3], ang[3];
      int dof = axis_angle(s, j, &w->qp[bp], &w->qp[bc], axes, ang);
      const int32_t* idx = s->d->act_index + 3 * a;
      const R* lim = s->jlim + 6 * j;
      R tq[3] = {0, 0, 0};
      for (int l = 0; l < dof; l++) {
        /* jp.take(act, act_index) * act_mask; take clips -1 to 0 */
        int ai = take_idx(idx[l], s->aw);
        R a_l = act[ai] * (idx[l] >= 0 ? (R)1 : (R)0);
        R t;
        if (s->d->act_type[a] == BX_ACT_TORQUE) {
          t = a_l * s->astr[a] * (R)-1;
          if (ang[l] < lim[2 * l]) t = 0;
          if (ang[l] > lim[2 * l + 1]) t = 0;
        } else {
          R target = clip(a_l * (R)M_PI / (R)180, lim[2 * l], lim[2 * l + 1]);
          t = (target - ang[l]) * s->astr[a];
        }
        for (int k = 0; k < 3; k++) tq[k] += axes[l][k] * t;
      }
      R sgn_p = s->d->act_type[a] == BX_ACT_TORQUE ? (R)1 : (R)-1;
      for (int k = 0; k < 3; k++) {
        tp[a - k0][k] = sgn_p * s->I[3 * bp + k] * tq[k];
        tc[a - k0][k] = -sgn_p * s->I[3 * bc + k] * tq[k];
      }
    }
    for (int a = k0; a < k1; a++) {
      int b = s->d->joint_body_p[s->d->act_joint[a]];
      for (int k = 0; k < 3; k++) w->gang[3 * b + k] += tp[a - k0][k];
    }
    for (int a = k0; a < k1; a++) {
      int b = s->d->joint_body_c[s->d->act_joint[a]];
      for (int k = 0; k < 3; k++) w->gang[3 * b + k] += tc[a - k0][k];
    }
    for (int i = 0; i < 3 * N; i++) w->dp_a[i] += w->gang[i];
    free(tp); free(tc);
    k0 = k1;
  }
}

/* ---------------------------------------------------------- integrator --- */

/* dp_f of body b (forces.py:41-107): Thruster dvel = a * strength / mass,
 * Twister dang = a * strength / mass, segment-summed in application order
 * (Thrusters, then Twisters) */
static void body_forces(const sysc* s, int b, const R* act, R fv[3], R fa[3]) {
  for (int k = 0; k < 3; k++) fv[k] = fa[k] = 0;
  for (int f = 0; f < s->NF; f++) {
    if (s->d->force_body[f] != b) continue;
    for (int k = 0; k < 3; k++) {
      R a = act[take_idx(s->d->force_index[3 * f + k], s->aw)];
      R dv = a * s->fstr[f] / s->fmass[f];
      if (s->d->force_type[f] == BX_FORCE_THRUSTER) fv[k] += dv;
      else fa[k] += dv;
    }
  }
}

/* Euler.update acc (integrators.py:85-93); acc = (dp_a + dp_f) + dp_j
 * (system.py:268-271) */
static void update_acc(const sysc* s, work_t* w, const R* act) {
  for (int b = 0; b < s->N; b++) {
    body_t* q = &w->qp[b];
    R fv[3], fa[3];
    body_forces(s, b, act, fv, fa);
    for (int k = 0; k < 3; k++) {
      R v = s->vdamp_exp * q->vel[k];
      v += (fv[k] + s->g[k]) * s->h;
      v *= s->pos_mask[3 * b + k];
      R acc = (w->dp_a[3 * b + k] + fa[k]) + w->dp_j[3 * b + k];
      R a = s->adamp_exp * q->ang[k];
      a += acc * s->h;
      a *= s->rot_mask[3 * b + k];
      q->vel[k] = v;
      q->ang[k] = a;
    }
  }
}

/* Euler.kinetic (integrators.py:50-68) */
static void kinetic(const sysc* s, work_t* w) {
  for (int b = 0; b < s->N; b++) {
    body_t* q = &w->qp[b];
    for (int k = 0; k < 3; k++) q->pos[k] = q->pos[k] + q->vel[k] * s->h * s->pos_mask[3 * b + k];
    R hq[4] = {0, q->ang[0] * s->rot_mask[3 * b], q->ang[1] * s->rot_mask[3 * b + 1],
               q->ang[2] * s->rot_mask[3 * b + 2]};
    for (int k = 0; k < 4; k++) hq[k] = hq[k] * (R)0.5 * s->h;
    R m[4];
    quat_mul(hq, q->rot, m);
    R r[4];
    for (int k = 0; k < 4; k++) r[k] = q->rot[k] + m[k];
    R n = (R)sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    for (int k = 0; k < 4; k++) q->rot[k] = r[k] / n;
  }
}

/* Euler.update pos (integrators.py:102-110) */
static void update_pos(const sysc* s, work_t* w) {
  for (int b = 0; b < s->N; b++) {
    body_t* q = &w->qp[b];
    for (int k = 0; k < 3; k++) q->pos[k] = q->pos[k] + w->dq_pos[3 * b + k] * s->pos_mask[3 * b + k];
    for (int k = 0; k < 4; k++) q->rot[k] = q->rot[k] + w->dq_rot[4 * b + k] * s->quat_mask[4 * b + k];
  }
}

/* Euler.update vel (integrators.py:96-100) */
static void update_vel(const sysc* s, work_t* w) {
  for (int b = 0; b < s->N; b++) {
    body_t* q = &w->qp[b];
    for (int k = 0; k < 3; k++) {
      q->vel[k] = (q->vel[k] + w->dp_vel[3 * b + k]) * s->pos_mask[3 * b + k];
      q->ang[k] = (q->ang[k] + w->dp_ang[3 * b + k]) * s->rot_mask[3 * b + k];
    }
  }
}

/* Euler.velocity_projection (integrators.py:122-146) */
static void velocity_projection(const sysc* s, work_t* w, const body_t* prev) {
  for (int b = 0; b < s->N; b++) {
    body_t* q = &w->qp[b];
    const body_t* p = &prev[b];
    R n = (R)sqrt(q->rot[0] * q->rot[0] + q->rot[1] * q->rot[1] + q->rot[2] * q->rot[2] +
                  q->rot[3] * q->rot[3]);
    R nr[4];
    for (int k = 0; k < 4; k++) nr[k] = q->rot[k] / n;
    for (int k = 0; k < 3; k++) q->vel[k] = ((q->pos[k] - p->pos[k]) / s->h) * s->pos_mask[3 * b + k];
    R inv[4], dq[4];
    quat_inv(p->rot, inv);
    quat_mul(nr, inv, dq);
    R scale = dq[0] >= 0 ? (R)1 : (R)-1;
    for (int k = 0; k < 3; k++) {
      R a = (R)2 * dq[1 + k] / s->h;
      R sc = scale * s->rot_mask[3 * b + k];
      q->ang[k] = sc * a * s->rot_mask[3 * b + k];
    }
    memcpy(q->rot, nr, sizeof(nr));
  }
}

/* ----------------------------------------------------------- colliders --- */

/* closest_segment_point_and_dist (geometry.py:360-374) */
static R seg_point(const R* a, const R* b, const R* pt, R* out) {
  R ab[3], t[3], v[3];
  for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; t[k] = pt[k] - a[k]; }
  R tt = dot3(t, ab) / (dot3(ab, ab) + (R)1e-6);
  tt = clip(tt, 0, 1);
  for (int k = 0; k < 3; k++) { out[k] = a[k] + tt * ab[k]; v[k] = pt[k] - out[k]; }
  return dot3(v, v);
}

/* _closest_segment_to_segment_points (geometry.py:394-451) */
static void seg_seg(const R* a0, const R* a1, const R* b0, const R* b1, R* ba, R* bb) {
  R da[3], db[3];
  for (int k = 0; k < 3; k++) { da[k] = a1[k] - a0[k]; db[k] = b1[k] - b0[k]; }
  R la = safe_norm3(da);
  la += (R)1e-6 * (R)(la == 0);
  for (int k = 0; k < 3; k++) da[k] /= la;
  R hla = la * (R)0.5;
  R lb = safe_norm3(db);
  lb += (R)1e-6 * (R)(lb == 0);
  for (int k = 0; k < 3; k++) db[k] /= lb;
  R hlb = lb * (R)0.5;
  R am[3], bm[3], tr[3];
  for (int k = 0; k < 3; k++) {
    am[k] = a0[k] + da[k] * hla;
    bm[k] = b0[k] + db[k] * hlb;
    tr[k] = am[k] - bm[k];
  }
  R dadb = dot3(da, db), datr = dot3(da, tr), dbtr = dot3(db, tr);
  R den = 1 - dadb * dadb;
  R ota = (-datr + dadb * dbtr) / (den + (R)1e-6);
  R otb = dbtr + ota * dadb;
  R ta = clip(ota, -hla, hla), tb = clip(otb, -hlb, hlb);
  for (int k = 0; k < 3; k++) { ba[k] = am[k] + da[k] * ta; bb[k] = bm[k] + db[k] * tb; }
  R na[3], nb[3];
  R d1 = seg_point(a0, a1, bb, na);
  R d2 = seg_point(b0, b1, ba, nb);
  if (d1 < d2) { memcpy(ba, na, sizeof(na)); } else { memcpy(bb, nb, sizeof(nb)); }
}

/* closest_segment_point_plane (geometry.py:377-391) */
static void seg_plane(const R* a, const R* b, const R* p0, const R* n, R* out) {
  R ba[3];
  for (int k = 0; k < 3; k++) ba[k] = b[k] - a[k];
  R dd = dot3(p0, n);
  R den = dot3(n, ba);
  R t = (dd - dot3(n, a)) / (den + (R)1e-6);
  t = clip(t, 0, 1);
  for (int k = 0; k < 3; k++) out[k] = a[k] + t * ba[k];
}

/* closest_triangle_point (geometry.py:462-498) */
static void tri_point(const R* p0, const R* p1, const R* p2, const R* pt, R* out) {
  R e0[3], e1[3], dv[3];
  for (int k = 0; k < 3; k++) { e0[k] = p1[k] - p0[k]; e1[k] = p2[k] - p0[k]; dv[k] = pt[k] - p0[k]; }
  R a = dot3(e0, e0), b = dot3(e0, e1), c = dot3(e1, e1);
  R det = a * c - b * b;
  R u = (c * dot3(e0, dv) - b * dot3(e1, dv)) / det;
  R v = (-b * dot3(e0, dv) + a * dot3(e1, dv)) / det;
  int inside = (0 <= u) && (u <= 1) && (0 <= v) && (v <= 1) && (u + v <= 1);
  R cp[3], w[3];
  for (int k = 0; k < 3; k++) { cp[k] = p0[k] + u * e0[k] + v * e1[k]; w[k] = cp[k] - pt[k]; }
  R d0 = dot3(w, w);
  R c1[3], c2[3], c3[3];
  R d1 = seg_point(p0, p1, pt, c1);
  int use0 = (d0 < d1) && inside;
  R best[3];
  for (int k = 0; k < 3; k++) best[k] = use0 ? cp[k] : c1[k];
  R md = use0 ? d0 : d1;
  R d2 = seg_point(p1, p2, pt, c2);
  if (d2 < md) memcpy(best, c2, sizeof(c2));
  md = md < d2 ? md : d2;
  R d3 = seg_point(p2, p0, pt, c3);
  if (d3 < md) memcpy(best, c3, sizeof(c3));
  memcpy(out, best, sizeof(best));
}

/* world velocity difference of a contact point (base.py:126-133) */
static void rel_vel(const body_t* a, const body_t* b, const R* pos, R* vel) {
  R ra[3], rb[3], ca[3], cb[3];
  for (int k = 0; k < 3; k++) { ra[k] = pos[k] - a->pos[k]; rb[k] = pos[k] - b->pos[k]; }
  cross3(a->ang, ra, ca);
  cross3(b->ang, rb, cb);
  for (int k = 0; k < 3; k++) vel[k] = (a->vel[k] + ca[k]) - (b->vel[k] + cb[k]);
}

/* box_heightmap, one corner (colliders.py:699-739). Height indices follow
 * jit: negative indices wrap once, then clamp into the grid. */
static void contact_heightmap(const sysc* s, int r, const body_t* a, const body_t* b, R* pos,
                              R* vel, R* nrm, R* pen) {
  const R* x = s->rext + 16 * r;
  const int off = s->d->row_hm[2 * r], M = s->d->row_hm[2 * r + 1];
  const R cell = x[0];
  R o[3], w[3], rel[3], inv[4], p[3];
  rotate(s->ra_end + 3 * r, a->rot, o);
  cross3(a->ang, o, w);
  for (int k = 0; k < 3; k++) { pos[k] = a->pos[k] + o[k]; vel[k] = a->vel[k] + w[k]; }
  for (int k = 0; k < 3; k++) rel[k] = pos[k] - b->pos[k];
  quat_inv(b->rot, inv);
  rotate(rel, inv, p);
  R u = p[0] / cell, v = p[1] / cell;
  int iu = (int)floor(u), iv = (int)floor(v);
  R du = u - (R)iu, dv = v - (R)iv;
  int lower = (du + dv) < 1;
  R mu = lower ? (R)-1 : (R)1;
  int tu[3] = {iu + (lower ? 0 : 1), iu + (lower ? 1 : 0), iu + (lower ? 0 : 1)};
  int tv[3] = {iv + (lower ? 0 : 1), iv + (lower ? 0 : 1), iv + (lower ? 1 : 0)};
  R h[3];
  for (int k = 0; k < 3; k++) {
    int i = tu[k], j = -tv[k];
    if (i < 0) i += M;
    if (j < 0) j += M;
    i = i < 0 ? 0 : (i >= M ? M - 1 : i);
    j = j < 0 ? 0 : (j >= M ? M - 1 : j);
    h[k] = s->hm[off + i * M + j];
  }
  R raw[3] = {mu * (h[1] - h[0]), mu * (h[2] - h[0]), cell};
  R rn = safe_norm3(raw);
  R n0[3] = {raw[0] / rn, raw[1] / rn, raw[2] / rn};
  R p0[3] = {(R)tu[0] * cell, (R)tv[0] * cell, h[0]};
  R dp[3];
  for (int k = 0; k < 3; k++) dp[k] = p0[k] - p[k];
  *pen = dot3(dp, n0);
  rotate(n0, b->rot, nrm);
}

/* capsule_clippedplane, one capsule end (colliders.py:762-802) */
static void contact_clipped(const sysc* s, int r, const body_t* a, const body_t* b, R* pos,
                            R* vel, R* nrm, R* pen) {
  const R* x = s->rext + 16 * r;
  R e[3], n[3];
  rotate(s->ra_end + 3 * r, a->rot, e);
  for (int k = 0; k < 3; k++) e[k] += a->pos[k];
  rotate(x, b->rot, n);
  R ndir = dot3(a->pos, n) > 0 ? (R)1 : (R)-1;
  for (int k = 0; k < 3; k++) nrm[k] = n[k] * ndir;
  for (int k = 0; k < 3; k++) pos[k] = e[k] - nrm[k] * s->ra_rad[r];
  R rel[3], c[3];
  for (int k = 0; k < 3; k++) rel[k] = pos[k] - a->pos[k];
  cross3(a->ang, rel, c);
  for (int k = 0; k < 3; k++) vel[k] = a->vel[k] + c[k];
  R pp[3], pt[3];
  rotate(x + 9, b->rot, pp);
  for (int k = 0; k < 3; k++) pt[k] = pp[k] + b->pos[k];
  R dp[3];
  for (int k = 0; k < 3; k++) dp[k] = pt[k] - pos[k];
  *pen = dot3(dp, nrm);
  R nx[3], ny[3], nn[3], yn[3], xn[3];
  rotate(x + 3, b->rot, nx);
  rotate(x + 6, b->rot, ny);
  for (int k = 0; k < 3; k++) nn[k] = nrm[k] * ndir;
  cross3(nn, nx, yn);
  cross3(nn, ny, xn);
  for (int k = 0; k < 3; k++) xn[k] = -xn[k];
  R hx = x[12], hy = x[13];
  int front = 0;
  for (int q = 0; q < 4; q++) {
    R sp[3], sn[3], dd[3];
    for (int k = 0; k < 3; k++) {
      sp[k] = q < 2 ? pt[k] + (q == 0 ? nx[k] * hx : -(nx[k] * hx))
                    : pt[k] + (q == 2 ? ny[k] * hy : -(ny[k] * hy));
      sn[k] = q == 0 ? xn[k] : (q == 1 ? -xn[k] : (q == 2 ? yn[k] : -yn[k]));
      dd[k] = pos[k] - sp[k];
    }
    front |= dot3(dd, sn) > (R)1e-6;
  }
  if (front) *pen = -1;
}

/* capsule_mesh, one triangle (colliders.py:822-848; geometry.py:501-541) */
static void contact_capsule_mesh(const sysc* s, int r, const body_t* a, const body_t* b, R* pos,
                                 R* vel, R* nrm, R* pen) {
  const R* x = s->rext + 16 * r;
  R pa[3], ea[3], a0[3], a1[3];
  rotate(s->ra_pos + 3 * r, a->rot, pa);
  rotate(s->ra_end + 3 * r, a->rot, ea);
  for (int k = 0; k < 3; k++) { pa[k] += a->pos[k]; a0[k] = pa[k] + ea[k]; a1[k] = pa[k] - ea[k]; }
  R tn[3], p[3][3];
  rotate(x + 9, b->rot, tn);
  for (int i = 0; i < 3; i++) {
    rotate(x + 3 * i, b->rot, p[i]);
    for (int k = 0; k < 3; k++) p[i][k] += b->pos[k];
  }
  /* closest_segment_triangle_points (geometry.py:501-541) */
  R sp[4][3], tp[4][3], dd[4];
  seg_seg(a0, a1, p[0], p[1], sp[0], tp[0]);
  seg_seg(a0, a1, p[1], p[2], sp[1], tp[1]);
  seg_seg(a0, a1, p[0], p[2], sp[2], tp[2]);
  seg_plane(a0, a1, p[0], tn, sp[3]);
  tri_point(p[0], p[1], p[2], sp[3], tp[3]);
  for (int i = 0; i < 4; i++) {
    R w[3];
    for (int k = 0; k < 3; k++) w[k] = sp[i][k] - tp[i][k];
    dd[i] = dot3(w, w);
  }
  R md = dd[0];
  for (int i = 1; i < 4; i++) md = dd[i] < md ? dd[i] : md;
  R ss[3] = {0, 0, 0}, ts[3] = {0, 0, 0}, cnt = 0;
  for (int i = 0; i < 4; i++) {
    R m = dd[i] == md ? (R)1 : (R)0;
    for (int k = 0; k < 3; k++) { ss[k] += sp[i][k] * m; ts[k] += tp[i][k] * m; }
    cnt += m;
  }
  R pv[3];
  for (int k = 0; k < 3; k++) { ss[k] /= cnt; ts[k] /= cnt; pv[k] = ss[k] - ts[k]; }
  R dist = safe_norm3(pv);
  for (int k = 0; k < 3; k++) nrm[k] = pv[k] / ((R)1e-6 + dist);
  *pen = s->ra_rad[r] - dist;
  memcpy(pos, ts, sizeof(ts));
  rel_vel(a, b, pos, vel);
}

/* ------------------------------------------------ hull_hull (SAT) ------- */

typedef struct { R v[8][3]; R f[6][4][3]; R n[6][3]; } hull_w;

static void hull_world(const sysc* s, int h, const body_t* q, hull_w* w) {
  for (int i = 0; i < 8; i++) {
    rotate(s->hv + 24 * h + 3 * i, q->rot, w->v[i]);
    for (int k = 0; k < 3; k++) w->v[i][k] += q->pos[k];
  }
  for (int f = 0; f < 6; f++) {
    rotate(s->hn + 18 * h + 3 * f, q->rot, w->n[f]);
    for (int i = 0; i < 4; i++) {
      rotate(s->hf + 72 * h + 12 * f + 3 * i, q->rot, w->f[f][i]);
      for (int k = 0; k < 3; k++) w->f[f][i][k] += q->pos[k];
    }
  }
}

/* get_face_support (geometry.py:794-801): max over faces of the min signed
 * distance of the vertices to the face plane; first index on ties */
static R face_support(R (*verts)[3], R (*normals)[3], R (*faces)[4][3], int* idx) {
  R best = 0;
  for (int f = 0; f < 6; f++) {
    R mn = 0;
    for (int v = 0; v < 8; v++) {
      R d[3];
      for (int k = 0; k < 3; k++) d[k] = verts[v][k] - faces[f][0][k];
      R x = dot3(normals[f], d);
      mn = (v == 0 || x < mn) ? x : mn;
    }
    if (f == 0 || mn > best) { best = mn; *idx = f; }
  }
  return best;
}

/* _closest_segment_to_segment_points with the barycentric t (geometry.py:394-451) */
static void seg_seg_t(const R* a0, const R* a1, const R* b0, const R* b1, R* ba, R* bb, R* t_a, R* t_b) {
  R da[3], db[3];
  for (int k = 0; k < 3; k++) { da[k] = a1[k] - a0[k]; db[k] = b1[k] - b0[k]; }
  R la = safe_norm3(da);
  la += (R)1e-6 * (R)(la == 0);
  for (int k = 0; k < 3; k++) da[k] /= la;
  R hla = la * (R)0.5;
  R lb = safe_norm3(db);
  lb += (R)1e-6 * (R)(lb == 0);
  for (int k = 0; k < 3; k++) db[k] /= lb;
  R hlb = lb * (R)0.5;
  R am[3], bm[3], tr[3];
  for (int k = 0; k < 3; k++) { am[k] = a0[k] + da[k] * hla; bm[k] = b0[k] + db[k] * hlb; tr[k] = am[k] - bm[k]; }
  R dadb = dot3(da, db), datr = dot3(da, tr), dbtr = dot3(db, tr);
  R den = 1 - dadb * dadb;
  R ota = (-datr + dadb * dbtr) / (den + (R)1e-6);
  R otb = dbtr + ota * dadb;
  R ta = clip(ota, -hla, hla), tb = clip(otb, -hlb, hlb);
  for (int k = 0; k < 3; k++) { ba[k] = am[k] + da[k] * ta; bb[k] = bm[k] + db[k] * tb; }
  R na[3], nb[3];
  R d1 = seg_point(a0, a1, bb, na);
  R d2 = seg_point(b0, b1, ba, nb);
  if (d1 < d2) { memcpy(ba, na, sizeof(na)); } else { memcpy(bb, nb, sizeof(nb)); }
  *t_a = (ota + hla) / la;
  *t_b = (otb + hlb) / lb;
}

/* _clip_edge_to_planes (geometry.py:580-624) against 4 planes */
static int clip_edge(const R* p0, const R* p1, R (*pp)[3], R (*pn)[3], R out[2][3]) {
  int f0[4], f1[4];
  R cand[4][3];
  for (int j = 0; j < 4; j++) {
    R d0[3], d1[3];
    for (int k = 0; k < 3; k++) { d0[k] = p0[k] - pp[j][k]; d1[k] = p1[k] - pp[j][k]; }
    f0[j] = dot3(d0, pn[j]) > (R)1e-6;
    f1[j] = dot3(d1, pn[j]) > (R)1e-6;
    seg_plane(p0, p1, pp[j], pn[j], cand[j]);
  }
  for (int side = 0; side < 2; side++) {
    const R* a = side == 0 ? p0 : p1;
    const R* b = side == 0 ? p1 : p0;
    const int* fr = side == 0 ? f0 : f1;
    R ab[3];
    for (int k = 0; k < 3; k++) ab[k] = b[k] - a[k];
    int best = 0;
    R bd = 0;
    for (int j = 0; j < 4; j++) {
      R e[3];
      for (int k = 0; k < 3; k++) e[k] = (fr[j] ? cand[j][k] : a[k]) - a[k];
      R dd = dot3(e, ab);
      if (j == 0 || dd > bd) { bd = dd; best = j; }
    }
    for (int k = 0; k < 3; k++) out[side][k] = fr[best] ? cand[best][k] : a[k];
  }
  int any_both = 0;
  for (int j = 0; j < 4; j++) any_both |= f0[j] && f1[j];
  int mask = !any_both;
  if (!mask) { memcpy(out[0], p0, 3 * sizeof(R)); memcpy(out[1], p1, 3 * sizeof(R)); }
  R e1[3], e2[3];
  for (int k = 0; k < 3; k++) { e1[k] = p0[k] - p1[k]; e2[k] = out[0][k] - out[1][k]; }
  if (dot3(e1, e2) < 0) mask = 0;
  return mask;
}

/* _create_sat_contact_manifold + clip (geometry.py:627-747): 4 contacts */
static void sat_manifold(R (*cp)[3], R (*sp)[3], const R* cn, const R* sn, R sign, R pos[4][3],
                         R nrm[4][3], R pen[4]) {
  R c0[4][3], c1[4][3], cpn[4][3], s0[4][3], s1[4][3], spn[4][3];
  for (int i = 0; i < 4; i++) {
    int im = (i + 3) % 4;  /* jp.roll(poly, 1): element i comes from i - 1 */
    R e[3];
    for (int k = 0; k < 3; k++) { c0[i][k] = cp[im][k]; c1[i][k] = cp[i][k]; e[k] = c1[i][k] - c0[i][k]; }
    cross3(cn, e, cpn[i]);
    for (int k = 0; k < 3; k++) { s0[i][k] = sp[im][k]; s1[i][k] = sp[i][k]; e[k] = s1[i][k] - s0[i][k]; }
    cross3(sn, e, spn[i]);
  }
  R pts[16][3];
  int msk[16];
  for (int i = 0; i < 4; i++) {
    R o[2][3];
    int m = clip_edge(s0[i], s1[i], c0, cpn, o);
    memcpy(pts[2 * i], o[0], sizeof(o[0]));
    memcpy(pts[2 * i + 1], o[1], sizeof(o[1]));
    msk[2 * i] = msk[2 * i + 1] = m;
  }
  /* _project_poly_onto_poly_plane of the clipping edge points onto the subject plane */
  R dd = dot3(sp[0], sn), den = dot3(cn, sn);
  R dn = den + (R)1e-6 * (R)(den == 0);
  R c0s[4][3], c1s[4][3];
  for (int i = 0; i < 4; i++) {
    R t0 = (dd - dot3(c0[i], sn)) / dn, t1 = (dd - dot3(c1[i], sn)) / dn;
    for (int k = 0; k < 3; k++) { c0s[i][k] = c0[i][k] + t0 * cn[k]; c1s[i][k] = c1[i][k] + t1 * cn[k]; }
  }
  for (int i = 0; i < 4; i++) {
    R o[2][3];
    int m = clip_edge(c0s[i], c1s[i], s0, spn, o);
    memcpy(pts[8 + 2 * i], o[0], sizeof(o[0]));
    memcpy(pts[8 + 2 * i + 1], o[1], sizeof(o[1]));
    msk[8 + 2 * i] = msk[8 + 2 * i + 1] = m;
  }
  /* reference points: projected onto the clipping plane (math.normalize) */
  R nn = (R)1e-6 + safe_norm3(cn), nh[3], ref[16][3];
  for (int k = 0; k < 3; k++) nh[k] = cn[k] / nn;
  for (int i = 0; i < 16; i++) {
    R d[3];
    for (int k = 0; k < 3; k++) d[k] = pts[i][k] - cp[0][k];
    R dist = dot3(d, nh);
    for (int k = 0; k < 3; k++) ref[i][k] = pts[i][k] - dist * nh[k];
    R ncn[3] = {-cn[0], -cn[1], -cn[2]};
    msk[i] = msk[i] && (dot3(d, ncn) > (R)1e-6);  /* point_in_front_of_plane(p0, -n, pt) */
  }
  /* get_orthogonals (geometry.py:568-577) */
  int ix = 0;
  R ab = cn[0] < 0 ? -cn[0] : cn[0];
  for (int k = 1; k < 3; k++) { R v = cn[k] < 0 ? -cn[k] : cn[k]; if (v > ab) { ab = v; ix = k; } }
  R o1[3] = {1, 1, 1}, o2[3];
  R denom = cn[ix] + (R)1e-6 * (R)(cn[ix] == 0);
  o1[ix] = -(((cn[0] + cn[1]) + cn[2]) - cn[ix]) / denom;
  cross3(cn, o1, o2);
  R dirs[4][3];
  for (int k = 0; k < 3; k++) { dirs[0][k] = o1[k]; dirs[1][k] = -o1[k]; dirs[2][k] = o2[k]; dirs[3][k] = -o2[k]; }
  for (int c = 0; c < 4; c++) {
    int best = 0;
    R bv = 0;
    for (int i = 0; i < 16; i++) {
      R v = dot3(ref[i], dirs[c]) + (msk[i] ? (R)0 : (R)-1e6);
      if (i == 0 || v > bv) { bv = v; best = i; }
    }
    R pd[3];
    for (int k = 0; k < 3; k++) { pos[c][k] = ref[best][k]; pd[k] = pts[best][k] - ref[best][k]; nrm[c][k] = sign * cn[k]; }
    R ncn[3] = {-cn[0], -cn[1], -cn[2]};
    pen[c] = msk[best] ? dot3(pd, ncn) : (R)-1;
  }
}

/* hull_hull (colliders.py:851-888) with sat_hull_hull (geometry.py:750-914):
 * contact e of the pair */
static void contact_hull(const sysc* s, int r, const body_t* a, const body_t* b, R* pos, R* vel,
                         R* nrm, R* pen) {
  const R* x = s->rext + 16 * r;
  const int ha = (int)x[0], hb = (int)x[1], e = (int)x[2];
  hull_w A, B;
  hull_world(s, ha, a, &A);
  hull_world(s, hb, b, &B);
  R origin[3] = {0, 0, 0};
  for (int v = 0; v < 8; v++)
    for (int k = 0; k < 3; k++) origin[k] += A.v[v][k];
  for (int k = 0; k < 3; k++) origin[k] /= 8;
  int i1 = 0, i2 = 0;
  R d1 = face_support(A.v, B.n, B.f, &i1);
  R d2 = face_support(B.v, A.n, A.f, &i2);
  int use_b = d1 > d2;
  R face_dist = use_b ? d1 : d2;
  int fi = use_b ? i1 : i2;
  R (*ref_face)[3] = use_b ? B.f[fi] : A.f[fi];
  R* ref_n = use_b ? B.n[fi] : A.n[fi];
  R sign = use_b ? (R)1 : (R)-1;
  R (*inc_faces)[4][3] = use_b ? A.f : B.f;
  R (*inc_ns)[3] = use_b ? A.n : B.n;
  int ii = 0;
  R bd = 0;
  for (int f = 0; f < 6; f++) {
    R d = dot3(inc_ns[f], ref_n);
    if (f == 0 || d < bd) { bd = d; ii = f; }
  }
  R fpos[4][3], fnrm[4][3], fpen[4];
  sat_manifold(ref_face, inc_faces[ii], ref_n, inc_ns[ii], sign, fpos, fnrm, fpen);
  /* edge axes over every face pair (tile a, repeat b) and edge pair */
  int best = -1;
  R best_v = 0, best_sd = 0, best_ax[3] = {0, 0, 0};
  R ba1[3] = {0}, ba2[3] = {0}, bb1[3] = {0}, bb2[3] = {0};
  for (int kp = 0; kp < 36; kp++) {
    const int fa = kp % 6, fb = kp / 6;
    for (int m = 0; m < 16; m++) {
      const int ea = m % 4, eb = m / 4;
      const R* a1 = A.f[fa][ea];
      const R* a2 = A.f[fa][(ea + 3) % 4];
      const R* b1 = B.f[fb][eb];
      const R* b2 = B.f[fb][(eb + 3) % 4];
      R e1[3], e2[3], ax[3], dv[3];
      for (int k = 0; k < 3; k++) { e1[k] = a1[k] - a2[k]; e2[k] = b1[k] - b2[k]; dv[k] = a1[k] - origin[k]; }
      cross3(e1, e2, ax);
      R sg = dot3(dv, ax) > 0 ? (R)1 : (R)-1;
      for (int k = 0; k < 3; k++) ax[k] *= sg;
      int bad = ax[0] == 0 && ax[1] == 0 && ax[2] == 0;
      R mx = 0;
      for (int v = 0; v < 8; v++) {
        R d[3];
        for (int k = 0; k < 3; k++) d[k] = A.v[v][k] - a1[k];
        R t = dot3(ax, d);
        mx = (v == 0 || t > mx) ? t : mx;
      }
      bad |= mx > 0;
      R am[3], bm[3], dm[3];
      for (int k = 0; k < 3; k++) {
        am[k] = a1[k] + (a2[k] - a1[k]) * (R)0.5;
        bm[k] = b1[k] + (b2[k] - b1[k]) * (R)0.5;
        dm[k] = am[k] - bm[k];
      }
      R aux = -dot3(dm, dm);
      /* get_edge_support: the support vertex of B along -ax */
      int sv = 0;
      R sd = 0;
      for (int v = 0; v < 8; v++) {
        R d[3];
        for (int k = 0; k < 3; k++) d[k] = B.v[v][k] - a1[k];
        R t = dot3(ax, d);
        if (v == 0 || t < sd) { sd = t; sv = v; }
      }
      R s1 = ((b1[0] - B.v[sv][0]) + (b1[1] - B.v[sv][1])) + (b1[2] - B.v[sv][2]);
      R s2 = ((b2[0] - B.v[sv][0]) + (b2[1] - B.v[sv][1])) + (b2[2] - B.v[sv][2]);
      if (!(s1 == 0 || s2 == 0)) bad = 1;
      if (bad) sd = (R)-1e6;
      R val = sd + aux;
      if (best < 0 || val > best_v) {
        best_v = val; best = kp * 16 + m; best_sd = sd;
        memcpy(best_ax, ax, sizeof(ax));
        memcpy(ba1, a1, sizeof(ba1)); memcpy(ba2, a2, sizeof(ba2));
        memcpy(bb1, b1, sizeof(bb1)); memcpy(bb2, b2, sizeof(bb2));
      }
    }
  }
  R edge_dist = best_sd;
  int maybe_edge = edge_dist > face_dist;
  R an = safe_norm3(best_ax), en[3];
  for (int k = 0; k < 3; k++) en[k] = best_ax[k] / an;
  R best_dist = edge_dist > face_dist ? edge_dist : face_dist;
  int has_int = best_dist < 0;
  /* _create_sat_edge_contact */
  R pa[3], pb[3], ta, tb;
  seg_seg_t(ba1, ba2, bb1, bb2, pa, pb, &ta, &tb);
  int valid = has_int && maybe_edge && ta >= 0 && ta <= 1 && tb >= 0 && tb <= 1;
  R edge_pen0 = valid ? -edge_dist : (R)-1;
  if (edge_pen0 > 0) {  /* jp.cond(edge_contact.penetration[0] > 0, edge, face) */
    for (int k = 0; k < 3; k++) { pos[k] = pb[k] + (pa[k] - pb[k]) * (R)0.5; nrm[k] = -en[k]; }
    *pen = e == 0 ? edge_pen0 : (R)-1;
  } else {
    for (int k = 0; k < 3; k++) { pos[k] = fpos[e][k]; nrm[k] = fnrm[e][k]; }
    *pen = fpen[e];
  }
  rel_vel(a, b, pos, vel);
}

/* capsule_plane (colliders.py:744-759) / capsule_capsule (:805-819) and the
 * extended functions above */
static void contact_row(const sysc* s, int r, const body_t* qp, R* pos, R* vel, R* nrm, R* pen) {
  const bx_desc* d = s->d;
  int g = d->row_group[r];
  const body_t* a = &qp[d->row_body_a[r]];
  const body_t* b = &qp[d->row_body_b[r]];
  switch (d->col_fn[g]) {
    case BX_COL_HEIGHTMAP: contact_heightmap(s, r, a, b, pos, vel, nrm, pen); return;
    case BX_COL_CLIPPED_PLANE: contact_clipped(s, r, a, b, pos, vel, nrm, pen); return;
    case BX_COL_CAPSULE_MESH: contact_capsule_mesh(s, r, a, b, pos, vel, nrm, pen); return;
    case BX_COL_HULL_HULL: contact_hull(s, r, a, b, pos, vel, nrm, pen); return;
    default: break;
  }
  if (d->col_fn[g] == BX_COL_CAPSULE_PLANE) {
    R e[3], z[3] = {0, 0, 1};
    rotate(s->ra_end + 3 * r, a->rot, e);
    for (int k = 0; k < 3; k++) e[k] += a->pos[k];
    rotate(z, b->rot, nrm);
    for (int k = 0; k < 3; k++) pos[k] = e[k] - nrm[k] * s->ra_rad[r];
    R rel[3], c[3];
    for (int k = 0; k < 3; k++) rel[k] = pos[k] - a->pos[k];
    cross3(a->ang, rel, c);
    for (int k = 0; k < 3; k++) vel[k] = a->vel[k] + c[k];
    R dpb[3];
    for (int k = 0; k < 3; k++) dpb[k] = b->pos[k] - pos[k];
    *pen = dot3(dpb, nrm);
    return;
  }
  /* _endpoints (colliders.py:660-664) */
  R pa[3], ea[3], pb[3], eb[3];
  rotate(s->ra_pos + 3 * r, a->rot, pa);
  rotate(s->ra_end + 3 * r, a->rot, ea);
  rotate(s->rb_pos + 3 * r, b->rot, pb);
  rotate(s->rb_end + 3 * r, b->rot, eb);
  R a0[3], a1[3], b0[3], b1[3];
  for (int k = 0; k < 3; k++) {
    pa[k] += a->pos[k]; pb[k] += b->pos[k];
    a0[k] = pa[k] + ea[k]; a1[k] = pa[k] - ea[k];
    b0[k] = pb[k] + eb[k]; b1[k] = pb[k] - eb[k];
  }
  R ba[3], bb[3];
  seg_seg(a0, a1, b0, b1, ba, bb);
  R pv[3];
  for (int k = 0; k < 3; k++) pv[k] = ba[k] - bb[k];
  R dist = safe_norm3(pv);
  for (int k = 0; k < 3; k++) nrm[k] = pv[k] / ((R)1e-6 + dist);
  *pen = s->ra_rad[r] + s->rb_rad[r] - dist;
  for (int k = 0; k < 3; k++) pos[k] = (ba[k] + bb[k]) / 2;
  R ra[3], rb[3], ca[3], cb[3];
  for (int k = 0; k < 3; k++) { ra[k] = pos[k] - a->pos[k]; rb[k] = pos[k] - b->pos[k]; }
  cross3(a->ang, ra, ca);
  cross3(b->ang, rb, cb);
  for (int k = 0; k < 3; k++) vel[k] = (a->vel[k] + ca[k]) - (b->vel[k] + cb[k]);
}

static inline R quad_I(const R* I, const R* v) {
  return v[0] * (I[0] * v[0]) + v[1] * (I[1] * v[1]) + v[2] * (I[2] * v[2]);
}

/* One/TwoWay._position_contact (colliders.py:306-377, :495-580).
 * oa/ob: (pos3, rot4) outputs; returns dlambda. */
static R position_contact(const sysc* s, int r, const body_t* qp, const body_t* qprev,
                          const R* cpos, const R* n, R cpen, R* oa, R* ob) {
  const bx_desc* d = s->d;
  int g = d->row_group[r];
  int ia = d->row_body_a[r], ib = d->row_body_b[r];
  const body_t* a = &qp[ia];
  const body_t* b = &qp[ib];
  const body_t* ao = &qprev[ia];
  const body_t* bo = &qprev[ib];
  const R* Ia = s->I + 3 * ia;
  const R* Ib = s->I + 3 * ib;
  R ma = s->mass[ia], mb = s->mass[ib];
  R sc = s->gscale[g];
  R t[3], u[3], q[4];
  for (int k = 0; k < 7; k++) { oa[k] = 0; ob[k] = 0; }
  if (d->col_oneway[g]) {
    R fr = s->rfric[r];
    R pp[3], pc[3], dx[3];
    for (int k = 0; k < 3; k++) {
      pp[k] = cpos[k];
      pc[k] = cpos[k] + n[k] * cpen;
      dx[k] = pp[k] - pc[k];
      pp[k] = pp[k] - a->pos[k];
      pc[k] = pc[k] - b->pos[k];
    }
    R c = dot3(dx, n);
    R cr1[3];
    cross3(pp, n, cr1);
    R w1 = (R)1 / ma + quad_I(Ia, cr1);
    R dl = -c / (w1 + (R)1e-6);
    R cm = c < 0 ? (R)1 : (R)0;
    R pv[3];
    for (int k = 0; k < 3; k++) pv[k] = dl * n[k] * cm;
    cross3(pp, pv, t);
    for (int k = 0; k < 3; k++) u[k] = Ia[k] * t[k];
    vec_quat_mul(u, a->rot, q);
    for (int k = 0; k < 3; k++) oa[k] = sc * (pv[k] / ma);
    for (int k = 0; k < 4; k++) oa[3 + k] = sc * ((R)0.5 * q[k]);
    /* static friction */
    R qi[4], r1[3], rr[3], p1bar[3];
    quat_inv(a->rot, qi);
    for (int k = 0; k < 3; k++) rr[k] = cpos[k] - a->pos[k];
    rotate(rr, qi, r1);
    rotate(r1, ao->rot, p1bar);
    R dp[3];
    for (int k = 0; k < 3; k++) { p1bar[k] += ao->pos[k]; dp[k] = cpos[k] - p1bar[k]; }
    R dpn = dot3(dp, n);
    R dt_[3];
    for (int k = 0; k < 3; k++) dt_[k] = dp[k] - dpn * n[k];
    R c2 = safe_norm3(dt_);
    R n2[3];
    for (int k = 0; k < 3; k++) n2[k] = dt_[k] / (c2 + (R)1e-6);
    cross3(pp, n2, cr1);
    w1 = (R)1 / ma + quad_I(Ia, cr1);
    R dlt = -c2 / (w1 + (R)0);
    R sm = fabs((double)dlt) < fabs((double)(fr * dl)) ? (R)1 : (R)0;
    for (int k = 0; k < 3; k++) pv[k] = dlt * n2[k] * sm * cm;
    cross3(pp, pv, t);
    for (int k = 0; k < 3; k++) u[k] = Ia[k] * t[k];
    vec_quat_mul(u, a->rot, q);
    for (int k = 0; k < 3; k++) oa[k] = oa[k] + sc * (pv[k] / ma);
    for (int k = 0; k < 4; k++) oa[3 + k] = oa[3 + k] + sc * ((R)0.5 * q[k]);
    return dl * cm;
  }
  /* TwoWay */
  R pp[3], pc[3];
  for (int k = 0; k < 3; k++) {
    pp[k] = cpos[k] - n[k] * cpen / 2;
    pc[k] = cpos[k] + n[k] * cpen / 2;
    pp[k] -= a->pos[k];
    pc[k] -= b->pos[k];
  }
  R c = -cpen;
  R cr1[3], cr2[3];
  cross3(pp, n, cr1);
  cross3(pc, n, cr2);
  R w1 = (R)1 / ma + quad_I(Ia, cr1);
  R w2 = (R)1 / mb + quad_I(Ib, cr2);
  R dl = -c / (w1 + w2 + (R)1e-6);
  R cm = c < 0 ? (R)1 : (R)0;
  R pv[3];
  for (int k = 0; k < 3; k++) pv[k] = dl * n[k] * cm;
  cross3(pp, pv, t);
  for (int k = 0; k < 3; k++) u[k] = Ia[k] * t[k];
  vec_quat_mul(u, a->rot, q);
  for (int k = 0; k < 3; k++) oa[k] = sc * (pv[k] / ma);
  for (int k = 0; k < 4; k++) oa[3 + k] = sc * ((R)0.5 * q[k]);
  cross3(pc, pv, t);
  for (int k = 0; k < 3; k++) u[k] = Ib[k] * t[k];
  vec_quat_mul(u, b->rot, q);
  for (int k = 0; k < 3; k++) ob[k] = sc * (-pv[k] / mb);
  for (int k = 0; k < 4; k++) ob[3 + k] = sc * ((R)-0.5 * q[k]);
  /* static friction */
  R qi[4], rr[3], r1[3], r2[3], p1bar[3], p2bar[3];
  quat_inv(a->rot, qi);
  for (int k = 0; k < 3; k++) rr[k] = cpos[k] - a->pos[k];
  rotate(rr, qi, r1);
  quat_inv(b->rot, qi);
  for (int k = 0; k < 3; k++) rr[k] = cpos[k] - b->pos[k];
  rotate(rr, qi, r2);
  rotate(r1, ao->rot, p1bar);
  rotate(r2, bo->rot, p2bar);
  R dp[3];
  for (int k = 0; k < 3; k++) {
    p1bar[k] += ao->pos[k];
    p2bar[k] += bo->pos[k];
    dp[k] = (cpos[k] - p1bar[k]) - (cpos[k] - p2bar[k]);
  }
  R dpn = dot3(dp, n);
  R dt_[3];
  for (int k = 0; k < 3; k++) dt_[k] = dp[k] - dpn * n[k];
  for (int k = 0; k < 3; k++) { pp[k] = cpos[k] - a->pos[k]; pc[k] = cpos[k] - b->pos[k]; }
  R c2 = safe_norm3(dt_);
  R n2[3];
  for (int k = 0; k < 3; k++) n2[k] = dt_[k] / (c2 + (R)1e-6);
  cross3(pp, n2, cr1);
  cross3(pc, n2, cr2);
  w1 = (R)1 / ma + quad_I(Ia, cr1);
  w2 = (R)1 / mb + quad_I(Ib, cr2);
  R dlt = -c2 / (w1 + w2);
  R sm = fabs((double)dlt) < fabs((double)dl) ? (R)1 : (R)0;
  for (int k = 0; k < 3; k++) pv[k] = dlt * n2[k] * sm * cm;
  cross3(pp, pv, t);
  for (int k = 0; k < 3; k++) u[k] = Ia[k] * t[k];
  vec_quat_mul(u, a->rot, q);
  for (int k = 0; k < 3; k++) oa[k] = oa[k] + sc * (pv[k] / ma);
  for (int k = 0; k < 4; k++) oa[3 + k] = oa[3 + k] + sc * ((R)0.5 * q[k]);
  R mp[3] = {-pv[0], -pv[1], -pv[2]};
  cross3(pc, mp, t);
  for (int k = 0; k < 3; k++) u[k] = Ib[k] * t[k];
  vec_quat_mul(u, b->rot, q);
  for (int k = 0; k < 3; k++) ob[k] = ob[k] + sc * (-pv[k] / mb);
  for (int k = 0; k < 4; k++) ob[3 + k] = ob[3 + k] + sc * ((R)0.5 * q[k]);
  return dl;
}

/* One/TwoWay._velocity_contact (colliders.py:379-442, :584-658).
 * qo = qp_right_before (the `qp_prev` argument of velocity_apply). */
static void velocity_contact(const sysc* s, int r, const body_t* qp, const body_t* qo,
                             const R* cpos, const R* n, R cpen, R dlam, R* oa, R* ob) {
  const bx_desc* d = s->d;
  int g = d->row_group[r];
  int ia = d->row_body_a[r], ib = d->row_body_b[r];
  const body_t* a = &qp[ia];
  const body_t* b = &qp[ib];
  const body_t* ao = &qo[ia];
  const body_t* bo = &qo[ib];
  const R* Ia = s->I + 3 * ia;
  const R* Ib = s->I + 3 * ib;
  R ma = s->mass[ia], mb = s->mass[ib];
  R fr = s->rfric[r], el = s->relas[r];
  R h = s->h;
  int one = d->col_oneway[g];
  for (int k = 0; k < 6; k++) { oa[k] = 0; ob[k] = 0; }
  R ra[3], rb[3], ca[3], cb[3], rv[3];
  for (int k = 0; k < 3; k++) { ra[k] = cpos[k] - a->pos[k]; rb[k] = cpos[k] - b->pos[k]; }
  cross3(a->ang, ra, ca);
  cross3(b->ang, rb, cb);
  for (int k = 0; k < 3; k++)
    rv[k] = one ? a->vel[k] + ca[k] : (a->vel[k] + ca[k]) - (b->vel[k] + cb[k]);
  R vn = dot3(rv, n);
  R vt[3];
  for (int k = 0; k < 3; k++) vt[k] = rv[k] - n[k] * vn;
  R vtn = safe_norm3(vt);
  R vtd[3];
  for (int k = 0; k < 3; k++) vtd[k] = vt[k] / ((R)1e-6 + vtn);
  R lim = fr * (R)fabs((double)dlam) / ((R)2 * h);
  R mag = lim < vtn ? lim : vtn; /* jp.amin over [lim, vtn] */
  R dvel[3];
  for (int k = 0; k < 3; k++) dvel[k] = -vtd[k] * mag;
  R pdyn[3];
  if (one) {
    R aw[3];
    cross3(ra, vtd, aw);
    R w = (R)1 / ma + dot3(aw, aw);
    for (int k = 0; k < 3; k++) pdyn[k] = dvel[k] / (w + (R)1e-6);
  } else {
    R a1[3], a2[3];
    cross3(ra, vtd, a1);
    cross3(rb, vtd, a2);
    R w1 = (R)1 / ma + quad_I(Ia, a1);
    R w2 = (R)1 / mb + quad_I(Ib, a2);
    for (int k = 0; k < 3; k++) pdyn[k] = dvel[k] / (w1 + w2 + (R)1e-6);
  }
  /* restitution */
  R rao[3], rbo[3], cao[3], cbo[3], rvo[3];
  for (int k = 0; k < 3; k++) { rao[k] = cpos[k] - ao->pos[k]; rbo[k] = cpos[k] - bo->pos[k]; }
  cross3(ao->ang, rao, cao);
  cross3(bo->ang, rbo, cbo);
  for (int k = 0; k < 3; k++)
    rvo[k] = one ? ao->vel[k] + cao[k] : (ao->vel[k] + cao[k]) - (bo->vel[k] + cbo[k]);
  R vno = dot3(rvo, n);
  R ev = el * vno;
  R mn = ev < 0 ? ev : (R)0;
  R dvr[3];
  for (int k = 0; k < 3; k++) dvr[k] = n[k] * (-vn - mn);
  R pp[3], pc[3];
  for (int k = 0; k < 3; k++) {
    pp[k] = cpos[k] - a->pos[k];
    pc[k] = (cpos[k] + n[k] * cpen) - b->pos[k];
  }
  R c = safe_norm3(dvr);
  R n2[3];
  for (int k = 0; k < 3; k++) n2[k] = dvr[k] / (c + (R)1e-6);
  R cr1[3], cr2[3];
  cross3(pp, n2, cr1);
  R w1 = (R)1 / ma + quad_I(Ia, cr1);
  R dlr;
  if (one) {
    dlr = c / (w1 + (R)1e-6);
  } else {
    cross3(pc, n2, cr2);
    R w2 = (R)1 / mb + quad_I(Ib, cr2);
    dlr = c / (w1 + w2 + (R)1e-6);
  }
  R sm = cpen > 0 ? (R)1 : (R)0;
  R sink = one ? (vno <= -s->gthr[g] ? (R)1 : (R)0) : (vno <= 0 ? (R)1 : (R)0);
  R pv[3];
  for (int k = 0; k < 3; k++) pv[k] = (dlr * n2[k] * sink + pdyn[k]) * sm;
  R t[3];
  for (int k = 0; k < 3; k++) { oa[k] = pv[k] / ma; t[k] = Ia[k] * ra[k]; }
  cross3(t, pv, oa + 3);
  if (!one) {
    R mp[3] = {-pv[0], -pv[1], -pv[2]};
    for (int k = 0; k < 3; k++) { ob[k] = -pv[k] / mb; t[k] = Ib[k] * rb[k]; }
    cross3(t, mp, ob + 3);
  }
}

/* One/TwoWay._contact (colliders.py:267-304, :449-493): impulse model used by
 * System.info at reset. oa/ob: (vel3, ang3). */
static void impulse_contact(const sysc* s, int r, const body_t* qp, const R* cpos,
                            const R* cvel, const R* n, R cpen, R* oa, R* ob) {
  const bx_desc* d = s->d;
  int g = d->row_group[r];
  int ia = d->row_body_a[r], ib = d->row_body_b[r];
  const body_t* a = &qp[ia];
  const body_t* b = &qp[ib];
  const R* Ia = s->I + 3 * ia;
  const R* Ib = s->I + 3 * ib;
  R ma = s->mass[ia], mb = s->mass[ib];
  R fr = s->rfric[r], el = s->relas[r];
  int one = d->col_oneway[g];
  R rpa[3], rpb[3];
  for (int k = 0; k < 3; k++) { rpa[k] = cpos[k] - a->pos[k]; rpb[k] = cpos[k] - b->pos[k]; }
  R bv = s->gerp[g] * cpen;
  R nv = dot3(n, cvel);
  R c1[3], t1[3], x1[3];
  cross3(rpa, n, c1);
  for (int k = 0; k < 3; k++) t1[k] = Ia[k] * c1[k];
  cross3(t1, rpa, x1);
  R ang;
  R denom;
  if (one) {
    ang = dot3(n, x1);
    denom = (R)1 / ma + ang;
  } else {
    R c2[3], t2[3], x2[3], sx[3];
    cross3(rpb, n, c2);
    for (int k = 0; k < 3; k++) t2[k] = Ib[k] * c2[k];
    cross3(t2, rpb, x2);
    for (int k = 0; k < 3; k++) sx[k] = x1[k] + x2[k];
    ang = dot3(n, sx);
    denom = (R)1 / ma + (R)1 / mb + ang;
  }
  R imp = ((R)-1 * ((R)1 + el) * nv + bv) / denom;
  R vd[3];
  for (int k = 0; k < 3; k++) vd[k] = cvel[k] - nv * n[k];
  R vdn = safe_norm3(vd);
  R impd = vdn / denom;
  R fi = fr * imp;
  impd = impd < fi ? impd : fi;
  R dird[3];
  for (int k = 0; k < 3; k++) dird[k] = vd[k] / ((R)1e-6 + vdn);
  R an = (cpen > 0 && nv < 0 && imp > 0) ? (R)1 : (R)0;
  R ad = an * (vdn > (R)0.01 ? (R)1 : (R)0);
  /* Body.impulse (bodies.py:46-59): dvel = J/m, dang = I * cross(pos - qp.pos, J) */
  R J[3], Jd[3], cx[3], cxd[3];
  for (int k = 0; k < 3; k++) { J[k] = imp * n[k]; Jd[k] = -impd * dird[k]; }
  cross3(rpa, J, cx);
  cross3(rpa, Jd, cxd);
  for (int k = 0; k < 3; k++) {
    oa[k] = (J[k] / ma) * an + (Jd[k] / ma) * ad;
    oa[3 + k] = (Ia[k] * cx[k]) * an + (Ia[k] * cxd[k]) * ad;
  }
  if (!one) {
    for (int k = 0; k < 3; k++) { J[k] = -imp * n[k]; Jd[k] = impd * dird[k]; }
    cross3(rpb, J, cx);
    cross3(rpb, Jd, cxd);
    for (int k = 0; k < 3; k++) {
      ob[k] = (J[k] / mb) * an + (Jd[k] / mb) * ad;
      ob[3 + k] = (Ib[k] * cx[k]) * an + (Ib[k] * cxd[k]) * ad;
    }
  } else {
    for (int k = 0; k < 6; k++) ob[k] = 0;
  }
}

/* segment-sum rows of one collider group into w->g*, with the any()-count and
 * the (eps + count) normalisation (colliders.py:141-153, :179-196, :221-240).
 * width 7 -> (pos, rot) targets; width 6 -> (vel, ang). */
static void group_reduce(const sysc* s, work_t* w, int g, int width, R eps,
                         const R* rows_a, const R* rows_b, R* out_lin, R* out_rot) {
  const bx_desc* d = s->d;
  int N = s->N, Rn = s->Rn;
  int rw = width == 7 ? 4 : 3;
  memset(w->cnt, 0, sizeof(R) * N);
  memset(w->gpos, 0, sizeof(R) * 3 * N);
  memset(w->grot, 0, sizeof(R) * 4 * N);
  for (int side = 0; side < 2; side++) {
    if (side == 1 && d->col_oneway[g]) break;
    const R* rows = side == 0 ? rows_a : rows_b;
    for (int r = 0; r < Rn; r++) {
      if (d->row_group[r] != g) continue;
      int b = side == 0 ? d->row_body_a[r] : d->row_body_b[r];
      const R* v = rows + width * r;
      int any = v[0] != 0 || v[1] != 0 || v[2] != 0;
      w->cnt[b] += any ? (R)1 : (R)0;
      for (int k = 0; k < 3; k++) w->gpos[3 * b + k] += v[k];
      for (int k = 0; k < rw; k++) w->grot[4 * b + k] += v[3 + k];
    }
  }
  for (int b = 0; b < N; b++) {
    R c = eps + w->cnt[b];
    for (int k = 0; k < 3; k++) out_lin[3 * b + k] += w->gpos[3 * b + k] / c;
    for (int k = 0; k < rw; k++) out_rot[rw * b + k] += w->grot[4 * b + k] / c;
  }
}

/* ------------------------------------------------------- culling -------- */

/* NearNeighbors.update (colliders.py:71-85): for each culled group, the
 * `cutoff` allowed cells whose candidate centres (body pos + rotate(offset))
 * are nearest get ranks 0.. in top_k order; ties to the lower flat index
 * (= row order), as jax.lax.top_k. Pairs rows are always active (rank 0). */
static void nn_select(const sysc* s, work_t* w) {
  const bx_desc* d = s->d;
  for (int r = 0; r < s->Rn; r++) w->ract[r] = d->col_cutoff[d->row_group[r]] ? -1 : 0;
  for (int g = 0; g < s->G; g++) {
    int cut = d->col_cutoff[g];
    if (!cut) continue;
    for (int k = 0; k < cut; k++) {
      int best = -1;
      R bd = 0;
      for (int r = 0; r < s->Rn; r++) {
        if (d->row_group[r] != g || w->ract[r] >= 0) continue;
        const body_t* a = &w->qp[d->row_body_a[r]];
        const body_t* b = &w->qp[d->row_body_b[r]];
        R pa[3], pb[3], da[3];
        rotate(s->ra_pos + 3 * r, a->rot, pa);
        rotate(s->rb_pos + 3 * r, b->rot, pb);
        for (int i = 0; i < 3; i++) da[i] = (b->pos[i] + pb[i]) - (a->pos[i] + pa[i]);
        R dist = (R)sqrt(da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
        /* a masked cell (more cutoff than allowed cells): sim = -inf, after
         * every finite cell, ties to the lower flat index (colliders.py:78-85) */
        if (d->row_nn_masked && d->row_nn_masked[r]) dist = (R)INFINITY;
        if (best < 0 || dist < bd) { best = r; bd = dist; }
      }
      w->ract[best] = k;
    }
  }
}

/* Info contact index of row r (system.py:36-43), -1 when culled */
static int row_info(const sysc* s, const work_t* w, int r) {
  const bx_desc* d = s->d;
  int g = d->row_group[r], base = 0, r0 = -1;
  for (int x = 0; x < s->Rn; x++)
    if (d->row_group[x] == g) { r0 = x; break; }
  for (int h = 0; h < g; h++) {
    if (d->col_cutoff[h]) { base += d->col_cutoff[h]; continue; }
    for (int x = 0; x < s->Rn; x++) base += d->row_group[x] == h;
  }
  if (!d->col_cutoff[g]) return base + r - r0;
  return w->ract[r] < 0 ? -1 : base + w->ract[r];
}

static int info_rows(const sysc* s) {
  int n = 0;
  for (int g = 0; g < s->G; g++) {
    if (s->d->col_cutoff[g]) { n += s->d->col_cutoff[g]; continue; }
    for (int x = 0; x < s->Rn; x++) n += s->d->row_group[x] == g;
  }
  return n;
}

/* --------------------------------------------------------------- step ---- */

static void one_substep(const sysc* s, work_t* w, const R* act) {
  actuators_apply(s, w, act);
  joints_damp(s, w);
  update_acc(s, w, act);
  kinetic(s, w);
  joints_apply(s, w);
  update_pos(s, w);
}

/* System._pbd_step (system.py:254-325) for one env */
static void pbd_step_env(const sysc* s, work_t* w, const R* act, R* rows_a, R* rows_b) {
  int N = s->N, Rn = s->Rn;
  memset(w->info_c, 0, sizeof(R) * 6 * N);
  memset(w->info_a, 0, sizeof(R) * 6 * N);
  nn_select(s, w);  /* cull.update, once per step (system.py:320-321) */
  for (int it = 0; it < s->d->substeps / 2; it++) {
    memcpy(w->qprev, w->qp, sizeof(body_t) * N);
    one_substep(s, w, act);
    velocity_projection(s, w, w->qprev);
    memcpy(w->qprev, w->qp, sizeof(body_t) * N);
    one_substep(s, w, act);
    /* Collider.position_apply (colliders.py:198-240) */
    for (int r = 0; r < Rn; r++)
      if (w->ract[r] >= 0)
        contact_row(s, r, w->qp, w->c_pos + 3 * r, w->c_vel + 3 * r, w->c_norm + 3 * r, &w->c_pen[r]);
    for (int r = 0; r < Rn; r++) {
      if (w->ract[r] < 0) {  /* culled this step: no update, not counted */
        memset(rows_a + 7 * r, 0, 7 * sizeof(R));
        memset(rows_b + 7 * r, 0, 7 * sizeof(R));
        continue;
      }
      w->dlam[r] = position_contact(s, r, w->qp, w->qprev, w->c_pos + 3 * r, w->c_norm + 3 * r,
                                    w->c_pen[r], rows_a + 7 * r, rows_b + 7 * r);
    }
    memset(w->dq_pos, 0, sizeof(R) * 3 * N);
    memset(w->dq_rot, 0, sizeof(R) * 4 * N);
    for (int g = 0; g < s->G; g++) group_reduce(s, w, g, 7, (R)1e-6, rows_a, rows_b, w->dq_pos, w->dq_rot);
    update_pos(s, w);
    memcpy(w->qrb, w->qp, sizeof(body_t) * N);
    velocity_projection(s, w, w->qprev);
    /* Collider.velocity_apply (colliders.py:155-196); rows at stride 6 */
    for (int r = 0; r < Rn; r++) {
      if (w->ract[r] < 0) {
        memset(rows_a + 6 * r, 0, 6 * sizeof(R));
        memset(rows_b + 6 * r, 0, 6 * sizeof(R));
        continue;
      }
      velocity_contact(s, r, w->qp, w->qrb, w->c_pos + 3 * r, w->c_norm + 3 * r, w->c_pen[r],
                       w->dlam[r], rows_a + 6 * r, rows_b + 6 * r);
    }
    memset(w->dp_vel, 0, sizeof(R) * 3 * N);
    memset(w->dp_ang, 0, sizeof(R) * 3 * N);
    for (int g = 0; g < s->G; g++) group_reduce(s, w, g, 6, (R)1e-6, rows_a, rows_b, w->dp_vel, w->dp_ang);
    update_vel(s, w);
    for (int b = 0; b < N; b++)
      for (int k = 0; k < 3; k++) {
        w->info_c[6 * b + k] += w->dp_vel[3 * b + k];
        w->info_c[6 * b + 3 + k] += w->dp_ang[3 * b + k];
        w->info_a[6 * b + 3 + k] += w->dp_a[3 * b + k];
      }
  }
}

/* -------------------------------------------------- legacy_spring ------- */

/* spring Revolute/Universal/Spherical.apply_reduced (spring_joints.py:122-155,
 * 170-204, 262-287) for joint j: dP of parent and child, (vel3, ang3) each */
static void spring_joint_one(const sysc* s, int j, const body_t* qp, R* op, R* oc) {
  int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
  const body_t* p = &qp[bp];
  const body_t* c = &qp[bc];
  const R* Ip = s->I + 3 * bp;
  const R* Ic = s->I + 3 * bc;
  R stiff = s->jstiff[j], sdamp = s->jsdamp[j], lstr = s->jlstr[j];
  /* QP.to_world (base.py:110-124) */
  R offp[3], offc[3], wp[3], wc[3], pos_p[3], pos_c[3], vel_p[3], vel_c[3];
  rotate(s->joff_p + 3 * j, p->rot, offp);
  rotate(s->joff_c + 3 * j, c->rot, offc);
  cross3(p->ang, offp, wp);
  cross3(c->ang, offc, wc);
  for (int k = 0; k < 3; k++) {
    pos_p[k] = p->pos[k] + offp[k]; vel_p[k] = p->vel[k] + wp[k];
    pos_c[k] = c->pos[k] + offc[k]; vel_c[k] = c->vel[k] + wc[k];
  }
  R imp[3], nimp[3], rp[3], rc[3], cp[3], cc[3];
  for (int k = 0; k < 3; k++) {
    imp[k] = (pos_p[k] - pos_c[k]) * stiff + sdamp * (vel_p[k] - vel_c[k]);
    nimp[k] = -imp[k];
    rp[k] = pos_p[k] - p->pos[k];
    rc[k] = pos_c[k] - c->pos[k];
  }
  /* Body.impulse (bodies.py:46-59) */
  cross3(rp, nimp, cp);
  cross3(rc, imp, cc);
  for (int k = 0; k < 3; k++) {
    op[k] = nimp[k] / s->mass[bp];
    op[3 + k] = Ip[k] * cp[k];
    oc[k] = imp[k] / s->mass[bc];
    oc[3 + k] = Ic[k] * cc[k];
  }
  R axes[3][3], ang[3], dang[3] = {0, 0, 0};
  int dof = axis_angle(s, j, p, c, axes, ang);
  const R* lim = s->jlim + 6 * j;
  for (int l = 0; l < dof; l++) {
    R dd = ang[l] < lim[2 * l] ? lim[2 * l] - ang[l] : (R)0;
    dang[l] = ang[l] > lim[2 * l + 1] ? lim[2 * l + 1] - ang[l] : dd;
  }
  R tq[3];
  int type = s->d->joint_type[j];
  if (type == BX_JOINT_REVOLUTE) {
    R axc[3];
    rotate(s->jax_c + 9 * j, c->rot, axc);
    cross3(axes[0], axc, tq);
    for (int k = 0; k < 3; k++) tq[k] = stiff * tq[k] - (lstr * axes[0][k]) * dang[0];
  } else if (type == BX_JOINT_UNIVERSAL) {
    R d21 = dot3(axes[1], axes[0]), proj[3];
    for (int k = 0; k < 3; k++) proj[k] = axes[1][k] - d21 * axes[0][k];
    R pn = safe_norm3(proj);
    for (int k = 0; k < 3; k++) proj[k] /= pn;
    cross3(proj, axes[1], tq);
    for (int k = 0; k < 3; k++)
      tq[k] = (lstr / (R)5) * tq[k] - lstr * (axes[0][k] * dang[0] + axes[1][k] * dang[1]);
  } else {
    for (int k = 0; k < 3; k++)
      tq[k] = -lstr * ((axes[0][k] * dang[0] + axes[1][k] * dang[1]) + axes[2][k] * dang[2]);
  }
  for (int k = 0; k < 3; k++) {
    tq[k] -= s->jdamp[j] * (p->ang[k] - c->ang[k]);
    op[3 + k] += Ip[k] * tq[k];
    oc[3 + k] += -Ic[k] * tq[k];
  }
}

/* spring Joint.apply (spring_joints.py:89-113), segment-summed per group over
 * concat(parents, children), groups added in order: w->sj_v, w->sj_a */
static void spring_joints_apply(const sysc* s, work_t* w) {
  int N = s->N, J = s->J;
  memset(w->sj_v, 0, sizeof(R) * 3 * N);
  memset(w->sj_a, 0, sizeof(R) * 3 * N);
  int j0 = 0;
  while (j0 < J) {
    int g = s->d->joint_group[j0], j1 = j0;
    while (j1 < J && s->d->joint_group[j1] == g) j1++;
    memset(w->gvel, 0, sizeof(R) * 3 * N);
    memset(w->gang, 0, sizeof(R) * 3 * N);
    R (*op)[6] = calloc(j1 - j0, sizeof(R[6]));
    R (*oc)[6] = calloc(j1 - j0, sizeof(R[6]));
    for (int j = j0; j < j1; j++) spring_joint_one(s, j, w->qp, op[j - j0], oc[j - j0]);
    for (int side = 0; side < 2; side++)
      for (int j = j0; j < j1; j++) {
        int b = side == 0 ? s->d->joint_body_p[j] : s->d->joint_body_c[j];
        const R* v = side == 0 ? op[j - j0] : oc[j - j0];
        for (int k = 0; k < 3; k++) { w->gvel[3 * b + k] += v[k]; w->gang[3 * b + k] += v[3 + k]; }
      }
    for (int i = 0; i < 3 * N; i++) { w->sj_v[i] += w->gvel[i]; w->sj_a[i] += w->gang[i]; }
    free(op); free(oc);
    j0 = j1;
  }
}

/* System._spring_step (system.py:342-375) for one env */
static void spring_step_env(const sysc* s, work_t* w, const R* act, R* rows_a, R* rows_b) {
  int N = s->N, Rn = s->Rn;
  memset(w->info_c, 0, sizeof(R) * 6 * N);
  memset(w->info_a, 0, sizeof(R) * 6 * N);
  memset(w->info_j, 0, sizeof(R) * 6 * N);
  nn_select(s, w);  /* cull.update, once per step (system.py:371-372) */
  for (int sub = 0; sub < s->d->substeps; sub++) {
    kinetic(s, w);
    spring_joints_apply(s, w);
    actuators_apply(s, w, act);
    /* Euler.update(acc_p = dp_j + dp_a + dp_f) (integrators.py:85-93) */
    for (int b = 0; b < N; b++) {
      body_t* q = &w->qp[b];
      R fv[3], fa[3];
      body_forces(s, b, act, fv, fa);
      for (int k = 0; k < 3; k++) {
        R dv = (w->sj_v[3 * b + k] + (R)0) + fv[k];
        R da = (w->sj_a[3 * b + k] + w->dp_a[3 * b + k]) + fa[k];
        R v = s->vdamp_exp * q->vel[k];
        v += (dv + s->g[k]) * s->h;
        v *= s->pos_mask[3 * b + k];
        R a = s->adamp_exp * q->ang[k];
        a += da * s->h;
        a *= s->rot_mask[3 * b + k];
        q->vel[k] = v;
        q->ang[k] = a;
      }
    }
    /* Collider.apply (colliders.py:116-153), then Euler.update(vel_p = dp_c) */
    for (int r = 0; r < Rn; r++) {
      if (w->ract[r] < 0) {
        memset(rows_a + 6 * r, 0, 6 * sizeof(R));
        memset(rows_b + 6 * r, 0, 6 * sizeof(R));
        continue;
      }
      contact_row(s, r, w->qp, w->c_pos + 3 * r, w->c_vel + 3 * r, w->c_norm + 3 * r, &w->c_pen[r]);
      impulse_contact(s, r, w->qp, w->c_pos + 3 * r, w->c_vel + 3 * r, w->c_norm + 3 * r,
                      w->c_pen[r], rows_a + 6 * r, rows_b + 6 * r);
    }
    memset(w->dp_vel, 0, sizeof(R) * 3 * N);
    memset(w->dp_ang, 0, sizeof(R) * 3 * N);
    for (int g = 0; g < s->G; g++) group_reduce(s, w, g, 6, (R)1e-8, rows_a, rows_b, w->dp_vel, w->dp_ang);
    update_vel(s, w);
    for (int b = 0; b < N; b++)
      for (int k = 0; k < 3; k++) {
        w->info_c[6 * b + k] += w->dp_vel[3 * b + k];
        w->info_c[6 * b + 3 + k] += w->dp_ang[3 * b + k];
        w->info_j[6 * b + k] += w->sj_v[3 * b + k];
        w->info_j[6 * b + 3 + k] += w->sj_a[3 * b + k];
        w->info_a[6 * b + 3 + k] += w->dp_a[3 * b + k];
      }
  }
}

/* System.step (system.py:244-247): the config's dynamics mode */
static void step_env(const sysc* s, work_t* w, const R* act, R* rows_a, R* rows_b) {
  if (s->spring) {
    spring_step_env(s, w, act, rows_a, rows_b);
  } else {
    pbd_step_env(s, w, act, rows_a, rows_b);
    memset(w->info_j, 0, sizeof(R) * 6 * s->N);
  }
}

int FN(oracle_system_step)(const bx_desc* d, int64_t B, const R* qp_in, const R* act,
                           R* qp_out, R* info_contact, R* info_actuator, R* cpos,
                           R* cnorm, R* cpen, R* info_joint) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, Rn = s.Rn, A = s.aw, IR = info_rows(&s);
#pragma omp parallel
  {
    work_t w;
    work_alloc(&w, N, Rn);
    R* ra = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
    R* rb = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      load_qp(w.qp, qp_in + e * 13 * N, N);
      step_env(&s, &w, act + e * A, ra, rb);
      store_qp(w.qp, qp_out + e * 13 * N, N);
      if (info_contact) memcpy(info_contact + e * 6 * N, w.info_c, sizeof(R) * 6 * N);
      if (info_joint) memcpy(info_joint + e * 6 * N, w.info_j, sizeof(R) * 6 * N);
      if (info_actuator) memcpy(info_actuator + e * 6 * N, w.info_a, sizeof(R) * 6 * N);
      for (int r = 0; r < Rn; r++) {
        int x = row_info(&s, &w, r);
        if (x < 0) continue;
        if (cpos) memcpy(cpos + (e * IR + x) * 3, w.c_pos + 3 * r, sizeof(R) * 3);
        if (cnorm) memcpy(cnorm + (e * IR + x) * 3, w.c_norm + 3 * r, sizeof(R) * 3);
        if (cpen) cpen[e * IR + x] = w.c_pen[r];
      }
    }
    free(ra); free(rb);
    work_free(&w);
  }
  sys_free(&s);
  return 0;
}

/* System._pbd_info contact part (system.py:327-340; Collider.apply
 * colliders.py:116-153) for one env: info_c (N,6) */
static void pbd_info_env(const sysc* s, work_t* w, R* rows_a, R* rows_b) {
  int N = s->N, Rn = s->Rn;
  nn_select(s, w);  /* culled groups: the cells nearest in this qp */
  for (int r = 0; r < Rn; r++) {
    if (w->ract[r] < 0) {
      memset(rows_a + 6 * r, 0, 6 * sizeof(R));
      memset(rows_b + 6 * r, 0, 6 * sizeof(R));
      continue;
    }
    contact_row(s, r, w->qp, w->c_pos + 3 * r, w->c_vel + 3 * r, w->c_norm + 3 * r, &w->c_pen[r]);
    impulse_contact(s, r, w->qp, w->c_pos + 3 * r, w->c_vel + 3 * r, w->c_norm + 3 * r,
                    w->c_pen[r], rows_a + 6 * r, rows_b + 6 * r);
  }
  memset(w->dp_vel, 0, sizeof(R) * 3 * N);
  memset(w->dp_ang, 0, sizeof(R) * 3 * N);
  for (int g = 0; g < s->G; g++) group_reduce(s, w, g, 6, (R)1e-8, rows_a, rows_b, w->dp_vel, w->dp_ang);
  for (int b = 0; b < N; b++)
    for (int k = 0; k < 3; k++) {
      w->info_c[6 * b + k] = w->dp_vel[3 * b + k];
      w->info_c[6 * b + 3 + k] = w->dp_ang[3 * b + k];
    }
}

int FN(oracle_system_info)(const bx_desc* d, int64_t B, const R* qp, R* info_contact) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, Rn = s.Rn;
#pragma omp parallel
  {
    work_t w;
    work_alloc(&w, N, Rn);
    R* ra = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
    R* rb = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      load_qp(w.qp, qp + e * 13 * N, N);
      pbd_info_env(&s, &w, ra, rb);
      memcpy(info_contact + e * 6 * N, w.info_c, sizeof(R) * 6 * N);
    }
    free(ra); free(rb);
    work_free(&w);
  }
  sys_free(&s);
  return 0;
}

/* ---------------------------------------------------------------- env ---- */

/* Joint.angle_vel (joints.py:197-226) for all joints, free-dof gathered.
 * Returns the count written to angles/vels. */
static int angle_vel(const sysc* s, const body_t* qp, R* angles, R* vels) {
  int n = 0;
  for (int j = 0; j < s->J; j++) {
    int bp = s->d->joint_body_p[j], bc = s->d->joint_body_c[j];
    R axes[3][3], ang[3];
    int dof = axis_angle(s, j, &qp[bp], &qp[bc], axes, ang);
    int fd = s->d->joint_free_dofs[j];
    int use = fd >= 0 ? fd : dof;
    for (int l = 0; l < use; l++) {
      R dv[3];
      for (int k = 0; k < 3; k++) dv[k] = qp[bp].ang[k] - qp[bc].ang[k];
      angles[n] = ang[l];
      vels[n] = dot3(dv, axes[l]);
      n++;
    }
  }
  return n;
}

/* Every joint's limited angles (`axis_angle`: the angles joint_apply_one and
 * the spring limit clip against joint_limit), (B, J, 3), zero past the
 * joint's dof: the goldens' joint-limit census (tests/test_golden_coverage.py) */
int FN(oracle_joint_angles)(const bx_desc* d, int64_t B, const R* qp, R* angles) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, J = s.J;
  body_t* q = calloc(N > 0 ? N : 1, sizeof(body_t));
  for (int64_t e = 0; e < B; e++) {
    load_qp(q, qp + e * 13 * N, N);
    for (int j = 0; j < J; j++) {
      R axes[3][3], ang[3] = {0, 0, 0};
      int dof = axis_angle(&s, j, &q[d->joint_body_p[j]], &q[d->joint_body_c[j]], axes, ang);
      for (int l = 0; l < 3; l++) angles[(e * J + j) * 3 + l] = l < dof ? ang[l] : (R)0;
    }
  }
  free(q);
  sys_free(&s);
  return J;
}

static R clip1(R x) { return clip(x, -1, 1); }

/* Ant._get_obs (ant.py:257-282), use_contact_forces=True -> 87 */
static int obs_ant(const sysc* s, const body_t* qp, const R* info_c, R* obs, int xy) {
  int n = 0, N = s->N;
  R ang[64], vel[64];
  int nd = angle_vel(s, qp, ang, vel);
  /* exclude_current_positions_from_observation=False: qp.pos[0] whole (ant.py:262-265) */
  if (xy) { obs[n++] = qp[0].pos[0]; obs[n++] = qp[0].pos[1]; }
  obs[n++] = qp[0].pos[2];
  for (int k = 0; k < 4; k++) obs[n++] = qp[0].rot[k];
  for (int i = 0; i < nd; i++) obs[n++] = ang[i];
  for (int k = 0; k < 3; k++) obs[n++] = qp[0].vel[k];
  for (int k = 0; k < 3; k++) obs[n++] = qp[0].ang[k];
  for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  for (int b = 0; b < N; b++)
    for (int k = 0; k < 3; k++) obs[n++] = clip1(info_c[6 * b + k]);
  for (int b = 0; b < N; b++)
    for (int k = 0; k < 3; k++) obs[n++] = clip1(info_c[6 * b + 3 + k]);
  return n;
}

/* Halfcheetah._get_obs (half_cheetah.py:200-214) -> 18 */
static int obs_halfcheetah(const sysc* s, const body_t* qp, R* obs, int xy) {
  int n = 0;
  R ang[64], vel[64];
  int nd = angle_vel(s, qp, ang, vel);
  /* qp.pos[0, (0, 2)] when positions are included (half_cheetah.py:206-209) */
  if (xy) obs[n++] = qp[0].pos[0];
  obs[n++] = qp[0].pos[2];
  obs[n++] = qp[0].rot[0];
  obs[n++] = qp[0].rot[2];
  for (int i = 0; i < nd; i++) obs[n++] = ang[i];
  obs[n++] = qp[0].vel[0];
  obs[n++] = qp[0].vel[2];
  obs[n++] = qp[0].ang[1];
  for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  return n;
}

/* math.quat_to_euler(q)[1] (math.py:80-91) */
static R euler_y(const R* q) {
  R v = (R)2 * q[1] * q[3] + (R)2 * q[0] * q[2];
  v = v < (R)-1 ? (R)-1 : (v > (R)1 ? (R)1 : v);
  return (R)asin((double)v);
}

/* Hopper / Walker2d._get_obs (hopper.py:231-246, walker2d.py:240-253) */
static int obs_loco2d(const sysc* s, const body_t* qp, R* obs, int xy) {
  int n = 0;
  R ang[64], vel[64];
  int nd = angle_vel(s, qp, ang, vel);
  if (xy) obs[n++] = qp[0].pos[0];
  obs[n++] = qp[0].pos[2];
  obs[n++] = euler_y(qp[0].rot);
  for (int i = 0; i < nd; i++) obs[n++] = ang[i];
  obs[n++] = qp[0].vel[0];
  obs[n++] = qp[0].vel[2];
  obs[n++] = qp[0].ang[1];
  for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  return n;
}

/* InvertedPendulum / InvertedDoublePendulum / Acrobot._get_obs
 * (inverted_pendulum.py:152-160, inverted_double_pendulum.py:166-178,
 * acrobot.py:90-95) */
static int obs_pendulums(const sysc* s, int kind, const body_t* qp, R* obs, R* ang, R* vel) {
  int n = 0;
  int nd = angle_vel(s, qp, ang, vel);
  if (kind != BX_ENV_ACROBOT) obs[n++] = qp[0].pos[0];
  if (kind == BX_ENV_INVERTED_DOUBLE_PENDULUM) {
    for (int i = 0; i < nd; i++) obs[n++] = (R)sin((double)ang[i]);
    for (int i = 0; i < nd; i++) obs[n++] = (R)cos((double)ang[i]);
  } else {
    for (int i = 0; i < nd; i++) obs[n++] = ang[i];
  }
  if (kind != BX_ENV_ACROBOT) obs[n++] = qp[0].vel[0];
  for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  return n;
}

/* math.quat_to_euler(q)[2] (math.py:80-91) */
static R euler_z(const R* q) {
  R y = (R)-2 * q[1] * q[2] + (R)2 * q[0] * q[3];
  R x = q[1] * q[1] + q[0] * q[0] - q[3] * q[3] - q[2] * q[2];
  return (R)atan2((double)y, (double)x);
}

/* the reachers' arm tip: body arm's (.11, 0, 0) via QP.to_world (base.py:112-126) */
static void arm_tip(const body_t* qp, int arm, R* tp, R* tv) {
  const R off0[3] = {(R)0.11, 0, 0};
  R off[3], w[3];
  rotate(off0, qp[arm].rot, off);
  cross3(qp[arm].ang, off, w);
  for (int k = 0; k < 3; k++) { tp[k] = qp[arm].pos[k] + off[k]; tv[k] = qp[arm].vel[k] + w[k]; }
}

/* Reacher(Angle) / Swimmer / Pusher._get_obs (reacher.py:205-224,
 * swimmer.py:257-272, pusher.py:232-242); coef = bx_env_params.coef */
static int obs_task(const sysc* s, int kind, const body_t* qp, const double* coef, R* obs, int xy) {
  int n = 0;
  R ang[64], vel[64];
  int nd = angle_vel(s, qp, ang, vel);
  if (kind == BX_ENV_REACHER || kind == BX_ENV_REACHERANGLE) {
    int tg = (int)coef[0], arm = (int)coef[1];
    for (int i = 0; i < nd; i++) obs[n++] = (R)cos((double)ang[i]);
    for (int i = 0; i < nd; i++) obs[n++] = (R)sin((double)ang[i]);
    obs[n++] = qp[tg].pos[0];
    obs[n++] = qp[tg].pos[1];
    R tp[3], tv[3];
    arm_tip(qp, arm, tp, tv);
    obs[n++] = tv[0];
    obs[n++] = tv[1];
    for (int k = 0; k < 3; k++) obs[n++] = tp[k] - qp[tg].pos[k];
  } else if (kind == BX_ENV_SWIMMER) {
    if (xy) { obs[n++] = qp[0].pos[0]; obs[n++] = qp[0].pos[1]; }
    obs[n++] = euler_z(qp[0].rot);
    for (int i = 0; i < nd; i++) obs[n++] = ang[i];
    obs[n++] = qp[0].vel[0];
    obs[n++] = qp[0].vel[1];
    obs[n++] = qp[0].ang[2];
    for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  } else if (kind == BX_ENV_PUSHER) {
    for (int i = 0; i < nd; i++) obs[n++] = ang[i];
    for (int i = 0; i < nd; i++) obs[n++] = vel[i];
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) obs[n++] = qp[(int)coef[j]].pos[k];
  }
  return n;
}

/* Ur5e / Fetch._get_obs (ur5e.py:115-135, fetch.py:101-121): egocentric in
 * the torso's frame; info_c = Info contact (vel 3, ang 3) per body */
static int obs_ego(const sysc* s, const body_t* qp, const R* info_c, const double* coef, R* obs) {
  int n = 0, N = s->N, t = (int)coef[0], g = (int)coef[1];
  const R e1[3] = {1, 0, 0}, e3[3] = {0, 0, 1};
  const R ti[4] = {qp[t].rot[0], -qp[t].rot[1], -qp[t].rot[2], -qp[t].rot[3]};
  R v[3], d[3];
  rotate(e1, qp[t].rot, v);
  for (int k = 0; k < 3; k++) obs[n++] = v[k];
  rotate(e3, qp[t].rot, v);
  for (int k = 0; k < 3; k++) obs[n++] = v[k];
  for (int k = 0; k < 3; k++) d[k] = qp[g].pos[k] - qp[t].pos[k];
  rotate(d, ti, v);
  R mag = norm3(v);
  obs[n++] = mag;
  for (int k = 0; k < 3; k++) obs[n++] = v[k] / ((R)1e-6 + mag);
  for (int b = 0; b < N; b++) {
    for (int k = 0; k < 3; k++) d[k] = qp[b].pos[k] - qp[t].pos[k];
    rotate(d, ti, v);
    for (int k = 0; k < 3; k++) obs[n++] = v[k];
  }
  for (int b = 0; b < N; b++) {
    rotate(qp[b].vel, ti, v);
    for (int k = 0; k < 3; k++) obs[n++] = v[k];
  }
  for (int b = 0; b < N; b++) {
    const R* c = info_c + 6 * b;
    obs[n++] = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] > (R)0.00001 ? (R)1 : (R)0;
  }
  return n;
}

/* Grasp._get_obs (grasp.py:132-175), in the palm's frame; coef = palm,
 * object, target, hand bodies */
static int obs_grasp(const sysc* s, const body_t* qp, const R* info_c, const double* coef, R* obs) {
  int n = 0, N = s->N, p = (int)coef[0], ob = (int)coef[1], tg = (int)coef[2], hd = (int)coef[3];
  const R ri[4] = {qp[p].rot[0], -qp[p].rot[1], -qp[p].rot[2], -qp[p].rot[3]};
  R d[3], v[3];
  for (int w = 0; w < 2; w++) {
    int b = w == 0 ? ob : tg;
    for (int k = 0; k < 3; k++) d[k] = qp[b].pos[k] - qp[p].pos[k];
    rotate(d, ri, v);
    R mag = norm3(v);
    obs[n++] = mag;
    for (int k = 0; k < 3; k++) obs[n++] = v[k] / ((R)1e-6 + mag);
  }
  for (int b = 0; b < N; b++) {
    for (int k = 0; k < 3; k++) d[k] = qp[b].pos[k] - qp[p].pos[k];
    rotate(d, ri, v);
    for (int k = 0; k < 3; k++) obs[n++] = v[k];
  }
  for (int b = 0; b < N; b++) {
    rotate(qp[b].vel, ri, v);
    for (int k = 0; k < 3; k++) obs[n++] = v[k];
  }
  R h2o[3], hdir[3], o2t[3], odir[3];
  for (int k = 0; k < 3; k++) h2o[k] = qp[ob].pos[k] - qp[p].pos[k];
  for (int k = 0; k < 3; k++) obs[n++] = h2o[k];
  for (int k = 0; k < 3; k++) obs[n++] = qp[hd].vel[k];
  R hm = norm3(h2o);
  for (int k = 0; k < 3; k++) hdir[k] = h2o[k] / ((R)1e-6 + hm);
  obs[n++] = dot3(hdir, qp[hd].vel);
  for (int k = 0; k < 3; k++) o2t[k] = qp[tg].pos[k] - qp[ob].pos[k];
  R om = norm3(o2t);
  obs[n++] = om;
  for (int k = 0; k < 3; k++) { odir[k] = o2t[k] / ((R)1e-6 + om); obs[n++] = odir[k]; }
  obs[n++] = dot3(odir, qp[ob].vel);
  for (int b = 0; b < N; b++) {
    const R* c = info_c + 6 * b;
    obs[n++] = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] > (R)0.00001 ? (R)1 : (R)0;
  }
  return n;
}

/* Humanoid._center_of_mass (humanoid.py:336-338): bodies [:-1] */
static void humanoid_com(const sysc* s, const body_t* qp, R* com) {
  R m = 0;
  R acc[3] = {0, 0, 0};
  for (int b = 0; b < s->N - 1; b++) {
    for (int k = 0; k < 3; k++) acc[k] += s->mass[b] * qp[b].pos[k];
    m += s->mass[b];
  }
  for (int k = 0; k < 3; k++) com[k] = acc[k] / m;
}

/* Humanoid._get_obs (humanoid.py:282-334) -> 240 */
static int obs_humanoid(const sysc* s, const body_t* qp, const R* act, R* obs, int xy) {
  int n = 0, N = s->N;
  R ang[64], vel[64];
  int nd = angle_vel(s, qp, ang, vel);
  /* qp.pos[0] whole when positions are included (humanoid.py:289-292) */
  if (xy) { obs[n++] = qp[0].pos[0]; obs[n++] = qp[0].pos[1]; }
  obs[n++] = qp[0].pos[2];
  for (int k = 0; k < 4; k++) obs[n++] = qp[0].rot[k];
  for (int i = 0; i < nd; i++) obs[n++] = ang[i];
  for (int k = 0; k < 3; k++) obs[n++] = qp[0].vel[k];
  for (int k = 0; k < 3; k++) obs[n++] = qp[0].ang[k];
  for (int i = 0; i < nd; i++) obs[n++] = vel[i];
  R com[3];
  humanoid_com(s, qp, com);
  R msum = 0;
  for (int b = 0; b < N - 1; b++) msum += s->mass[b];
  /* cinert: (N-1) x 3x3 */
  for (int b = 0; b < N - 1; b++) {
    R dd[3];
    for (int k = 0; k < 3; k++) dd[k] = qp[b].pos[k] - com[k];
    R nn = norm3(dd);
    R n2 = nn * nn;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        R v = s->mass[b] * (R)(r == c) * n2;
        v += (r == c ? s->I[3 * b + r] : (R)0) - dd[r] * dd[c];
        obs[n++] = v;
      }
  }
  /* cvel: com_vel (N-1)x3 then com_ang (N-1)x3 */
  for (int b = 0; b < N - 1; b++)
    for (int k = 0; k < 3; k++) obs[n++] = s->mass[b] * qp[b].vel[k] / msum;
  for (int b = 0; b < N - 1; b++) {
    R dd[3], cr[3];
    for (int k = 0; k < 3; k++) dd[k] = qp[b].pos[k] - com[k];
    cross3(dd, qp[b].vel, cr);
    R nn = norm3(dd);
    for (int k = 0; k < 3; k++) obs[n++] = cr[k] / ((R)1e-7 + nn * nn);
  }
  /* qfrc_actuator: take(action, act_index) unmasked (-1 -> clip -> 0) */
  for (int a = 0; a < s->K; a++) {
    int j = s->d->act_joint[a];
    int dof = s->d->joint_dof[j];
    for (int l = 0; l < dof; l++) {
      int ai = take_idx(s->d->act_index[3 * a + l], s->aw);
      obs[n++] = act[ai] * s->astr[a];
    }
  }
  return n;
}

int FN(oracle_env_obs)(const bx_desc* d, int kind, int64_t B, const R* qp, const R* info_c,
                       const R* act, R* obs, int obs_size, const double* coef) {
  sysc s;
  sys_init(&s, d);
  if ((kind & 0xFF) >= BX_ENV_REACHER && (kind & 0xFF) <= BX_ENV_GRASP && !coef) {
    sys_free(&s);
    return -2;
  }
  int N = s.N;
  int rc = 0;
  const int xy = (kind >> 8) & BX_OBS_XY; /* kind | obs_flags << 8 */
  kind &= 0xFF;
#pragma omp parallel
  {
    body_t* q = calloc(N, sizeof(body_t));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      load_qp(q, qp + e * 13 * N, N);
      int n = 0;
      if (kind == BX_ENV_ANT) n = obs_ant(&s, q, info_c + e * 6 * N, obs + e * obs_size, xy);
      else if (kind == BX_ENV_HALFCHEETAH) n = obs_halfcheetah(&s, q, obs + e * obs_size, xy);
      else if (kind == BX_ENV_HOPPER || kind == BX_ENV_WALKER2D)
        n = obs_loco2d(&s, q, obs + e * obs_size, xy);
      else if (kind >= BX_ENV_INVERTED_PENDULUM && kind <= BX_ENV_ACROBOT) {
        R ang[64], vel[64];
        n = obs_pendulums(&s, kind, q, obs + e * obs_size, ang, vel);
      } else if (kind >= BX_ENV_REACHER && kind <= BX_ENV_PUSHER)
        n = obs_task(&s, kind, q, coef, obs + e * obs_size, xy);
      else if (kind == BX_ENV_UR5E || kind == BX_ENV_FETCH)
        n = obs_ego(&s, q, info_c + e * 6 * N, coef, obs + e * obs_size);
      else if (kind == BX_ENV_GRASP)
        n = obs_grasp(&s, q, info_c + e * 6 * N, coef, obs + e * obs_size);
      else if (kind == BX_ENV_HUMANOID || kind == BX_ENV_HUMANOID_STANDUP)
        n = obs_humanoid(&s, q, act + e * s.aw, obs + e * obs_size, xy);
      if (n != obs_size) rc = -1;
    }
    free(q);
  }
  sys_free(&s);
  return rc;
}

/* Env.step of the unwrapped env (ant.py:222-255, humanoid.py:246-280,
 * half_cheetah.py:178-197). done_io is read (HalfCheetah keeps it) and written. */
int FN(oracle_env_step)(const bx_desc* d, int kind, int64_t B, const R* qp_in, const R* act,
                        R* qp_out, R* obs, int obs_size, R* reward, R* done_io,
                        R* metrics, int n_metrics, const double* coef) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, Rn = s.Rn, A = s.aw;
  int rc = 0;
  const int xy = (kind >> 8) & BX_OBS_XY; /* kind | obs_flags << 8 */
  kind &= 0xFF;
  if (kind >= BX_ENV_REACHER && kind <= BX_ENV_GRASP && !coef) {
    sys_free(&s);
    return -2;
  }
  /* Swimmer appends its drag forces to the action (swimmer.py:218-220): the
   * System.step reads A + 9 values, clipped at that width */
  if (kind == BX_ENV_SWIMMER) s.aw = A + 9;
#pragma omp parallel
  {
    work_t w;
    work_alloc(&w, N, Rn);
    R* ra = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
    R* rb = calloc(7 * (Rn > 0 ? Rn : 1), sizeof(R));
    body_t* q0 = calloc(N, sizeof(body_t));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      const R* a = act + e * A;
      load_qp(w.qp, qp_in + e * 13 * N, N);
      memcpy(q0, w.qp, sizeof(body_t) * N);
      /* the action System.step reads */
      R xa[64];
      const R* sa = a;
      if (kind == BX_ENV_REACHERANGLE) {
        /* reacherangle.py:79: min + range * (a + 1) / 2 */
        for (int i = 0; i < A; i++) xa[i] = (R)coef[2 + i] + (R)coef[4 + i] * ((a[i] + 1) / 2);
        sa = xa;
      } else if (kind == BX_ENV_SWIMMER) {
        /* swimmer.py:246-255, jp.diag keeping D00, D11, D22 for every segment */
        R D[3];
        for (int b = 0; b < 3; b++) {
          const R qi[4] = {q0[b].rot[0], -q0[b].rot[1], -q0[b].rot[2], -q0[b].rot[3]};
          R lv[3];
          rotate(q0[b].vel, qi, lv);
          D[b] = (R)coef[3 + b] * (R)fabs((double)lv[b]) * lv[b];
        }
        for (int i = 0; i < A; i++) xa[i] = a[i];
        for (int b = 0; b < 3; b++) {
          R f[3], fw[3];
          for (int k = 0; k < 3; k++) f[k] = q0[b].vel[k] * (R)coef[2] - D[k];
          rotate(f, q0[b].rot, fw);
          for (int k = 0; k < 3; k++)
            xa[A + 3 * b + k] = fw[k] < (R)-5 ? (R)-5 : (fw[k] > (R)5 ? (R)5 : fw[k]);
        }
        sa = xa;
      } else if (kind == BX_ENV_GRASP) {
        /* grasp.py:63-77: the mapped action; the palm moves 15 % toward the
         * last three (at most 2 units) before the physics */
        for (int i = 0; i < A; i++)
          xa[i] = (R)g_act_map[i] + (R)g_act_map[64 + i] * ((a[i] + 1) / 2);
        int p = (int)coef[0];
        R d[3];
        for (int k = 0; k < 3; k++) d[k] = xa[A - 3 + k] - w.qp[p].pos[k];
        R nrm = norm3(d);
        R scl = nrm > (R)2 ? (R)2 / nrm : (R)1;
        for (int k = 0; k < 3; k++) w.qp[p].pos[k] = w.qp[p].pos[k] + scl * d[k] * (R)0.15;
        sa = xa;
      }
      step_env(&s, &w, sa, ra, rb);
      store_qp(w.qp, qp_out + e * 13 * N, N);
      R* o = obs + e * obs_size;
      R* m = metrics + e * n_metrics;
      R dt = (R)d->dt;
      R sq = 0;
      for (int i = 0; i < A; i++) sq += a[i] * a[i];
      int n = 0;
      if (kind == BX_ENV_ANT) {
        n = obs_ant(&s, w.qp, w.info_c, o, xy);
        R vel[3];
        for (int k = 0; k < 3; k++) vel[k] = (w.qp[0].pos[k] - q0[0].pos[k]) / dt;
        R fwd = vel[0];
        R z = w.qp[0].pos[2];
        R healthy = z < (R)0.2 ? (R)0 : (R)1;
        healthy = z > (R)1.0 ? (R)0 : healthy;
        R ctrl = (R)0.5 * sq;
        R csum = 0;
        for (int b = 0; b < N; b++)
          for (int k = 0; k < 3; k++) { R c = clip1(w.info_c[6 * b + k]); csum += c * c; }
        R ccost = (R)5e-4 * csum;
        reward[e] = fwd + (R)1 - ctrl - ccost;
        done_io[e] = (R)1 - healthy;
        /* metric keys sorted: distance_from_origin, forward_reward,
         * reward_contact, reward_ctrl, reward_forward, reward_survive,
         * x_position, x_velocity, y_position, y_velocity */
        m[0] = norm3(w.qp[0].pos); m[1] = fwd; m[2] = -ccost; m[3] = -ctrl;
        m[4] = fwd; m[5] = 1; m[6] = w.qp[0].pos[0]; m[7] = vel[0];
        m[8] = w.qp[0].pos[1]; m[9] = vel[1];
      } else if (kind == BX_ENV_HALFCHEETAH) {
        n = obs_halfcheetah(&s, w.qp, o, xy);
        R v0 = (w.qp[0].pos[0] - q0[0].pos[0]) / dt;
        R fwd = (R)1.0 * v0;
        R ctrl = (R)0.1 * sq;
        reward[e] = fwd - ctrl;
        /* done unchanged; metrics sorted: reward_ctrl, reward_run, x_position, x_velocity */
        m[0] = -ctrl; m[1] = fwd; m[2] = w.qp[0].pos[0]; m[3] = v0;
      } else if (kind == BX_ENV_HUMANOID) {
        n = obs_humanoid(&s, w.qp, a, o, xy);
        R cb[3], ca[3], v[3];
        humanoid_com(&s, q0, cb);
        humanoid_com(&s, w.qp, ca);
        for (int k = 0; k < 3; k++) v[k] = (ca[k] - cb[k]) / dt;
        R fwd = (R)1.25 * v[0];
        R z = w.qp[0].pos[2];
        R healthy = z < (R)0.8 ? (R)0 : (R)1;
        healthy = z > (R)2.1 ? (R)0 : healthy;
        R ctrl = (R)0.1 * sq;
        reward[e] = fwd + (R)5.0 - ctrl;
        done_io[e] = (R)1 - healthy;
        /* sorted: distance_from_origin, forward_reward, reward_alive,
         * reward_linvel, reward_quadctrl, x_position, x_velocity,
         * y_position, y_velocity */
        m[0] = norm3(ca); m[1] = fwd; m[2] = 5; m[3] = fwd; m[4] = -ctrl;
        m[5] = ca[0]; m[6] = v[0]; m[7] = ca[1]; m[8] = v[1];
      } else if (kind == BX_ENV_HOPPER || kind == BX_ENV_WALKER2D) {
        /* hopper.py:204-229 with the constructor defaults (hopper.py:146-158,
         * walker2d.py:153-163); sorted metrics: reward_ctrl, reward_forward,
         * reward_healthy, x_position, x_velocity */
        n = obs_loco2d(&s, w.qp, o, xy);
        const int hop = kind == BX_ENV_HOPPER;
        const R zmin = (R)0.7, zmax = hop ? (R)INFINITY : (R)2.0;
        const R amin = hop ? (R)-0.2 : (R)-1.0, amax = hop ? (R)0.2 : (R)1.0;
        R xv = (w.qp[0].pos[0] - q0[0].pos[0]) / dt;
        R fwd = (R)1.0 * xv;
        R ay = euler_y(w.qp[0].rot);
        R z = w.qp[0].pos[2];
        R healthy = z < zmin ? (R)0 : (R)1;
        healthy = z > zmax ? (R)0 : healthy;
        healthy = ay > amax ? (R)0 : healthy;
        healthy = ay < amin ? (R)0 : healthy;
        R hr = (R)1.0;
        R ctrl = (R)1e-3 * sq;
        reward[e] = fwd + hr - ctrl;
        done_io[e] = (R)1 - healthy;
        m[0] = -ctrl; m[1] = fwd; m[2] = hr; m[3] = w.qp[0].pos[0]; m[4] = xv;
      } else if (kind >= BX_ENV_INVERTED_PENDULUM && kind <= BX_ENV_ACROBOT) {
        R ang[64], vel[64];
        n = obs_pendulums(&s, kind, w.qp, o, ang, vel);
        if (kind == BX_ENV_INVERTED_PENDULUM) {
          reward[e] = 1;
          done_io[e] = fabs((double)o[1]) > 0.2 ? (R)1 : (R)0;
        } else if (kind == BX_ENV_INVERTED_DOUBLE_PENDULUM) {
          /* jp.take(qp, 2).to_world([0, 0, .3]) */
          const R off[3] = {0, 0, (R)0.3};
          R tip[3];
          rotate(off, w.qp[2].rot, tip);
          R x = w.qp[2].pos[0] + tip[0], y = w.qp[2].pos[2] + tip[2];
          R dist = (R)0.01 * (x * x) + (y - 2) * (y - 2);
          R velp = (R)1e-3 * (vel[0] * vel[0]) + (R)5e-3 * (vel[1] * vel[1]);
          reward[e] = (R)10 - dist - velp;
          done_io[e] = y <= 1 ? (R)1 : (R)0;
        } else {
          R dist = ang[0] * ang[0] + ang[1] * ang[1];
          R velp = (R)1e-3 * (vel[0] * vel[0] + vel[1] * vel[1]);
          R r = (R)10 - dist - velp;
          reward[e] = r;
          done_io[e] = 0;
          /* sorted: alive_bonus, dist_penalty, r_tot, vel_penalty */
          m[0] = 0; m[1] = dist; m[2] = r; m[3] = velp;
        }
      } else if (kind == BX_ENV_REACHER || kind == BX_ENV_REACHERANGLE) {
        n = obs_task(&s, kind, w.qp, coef, o, xy);
        R rd = -norm3(o + n - 3);  /* obs[-3:] = tip - target */
        if (kind == BX_ENV_REACHER) {
          R rc2 = -sq;
          reward[e] = rd + rc2;
          m[0] = rc2; m[1] = rd;  /* sorted: reward_ctrl, reward_dist */
        } else {
          reward[e] = rd;
          m[0] = 0; m[1] = rd;    /* sorted: rewardCtrl, rewardDist */
        }
      } else if (kind == BX_ENV_SWIMMER) {
        n = obs_task(&s, kind, w.qp, coef, o, xy);
        R cb[3], ca[3], v[3];
        humanoid_com(&s, q0, cb);
        humanoid_com(&s, w.qp, ca);
        for (int k = 0; k < 3; k++) v[k] = (ca[k] - cb[k]) / dt;
        R fwd = (R)coef[0] * v[0];
        R ctrl = (R)coef[1] * sq;
        reward[e] = fwd - ctrl;
        /* done unchanged; sorted: distance_from_origin, forward_reward,
         * reward_ctrl, reward_fwd, x_position, x_velocity, y_position, y_velocity */
        m[0] = norm3(w.qp[0].pos); m[1] = fwd; m[2] = -ctrl; m[3] = fwd;
        m[4] = ca[0]; m[5] = v[0]; m[6] = ca[1]; m[7] = v[1];
      } else if (kind == BX_ENV_UR5E || kind == BX_ENV_FETCH) {
        /* ur5e.py:82-101, fetch.py:58-99 (the hit target's teleport draws
         * from JAX's key: not restated; done unchanged) */
        n = obs_ego(&s, w.qp, w.info_c, coef, o);
        int t = (int)coef[0], g = (int)coef[1];
        R delta[3], rel[3], dir[3];
        for (int k = 0; k < 3; k++) {
          delta[k] = w.qp[t].pos[k] - q0[t].pos[k];
          rel[k] = w.qp[g].pos[k] - w.qp[t].pos[k];
        }
        R dist = norm3(rel);
        for (int k = 0; k < 3; k++) dir[k] = rel[k] / ((R)1e-6 + dist);
        R moving = (R)0.1 * dot3(delta, dir);
        R hit = dist < (R)coef[2] ? (R)1 : (R)0;
        if (kind == BX_ENV_UR5E) {
          reward[e] = moving + hit;
          m[0] = hit; m[1] = moving; m[2] = hit;
        } else {
          const R e1[3] = {1, 0, 0}, e3[3] = {0, 0, 1};
          R up[3], fw[3];
          rotate(e3, w.qp[t].rot, up);
          rotate(e1, w.qp[t].rot, fw);
          R is_up = (R)0.1 * dt * dot3(up, e3);
          R height = (R)0.1 * dt * w.qp[0].pos[2];
          R whit = hit * dot3(dir, fw);
          reward[e] = height + moving + is_up + whit;
          m[0] = hit; m[1] = moving; m[2] = height; m[3] = is_up; m[4] = whit;
        }
      } else if (kind == BX_ENV_GRASP) {
        /* grasp.py:80-126 (teleport not restated; done unchanged) */
        n = obs_grasp(&s, w.qp, w.info_c, coef, o);
        int p = (int)coef[0], ob = (int)coef[1], tg = (int)coef[2], hd = (int)coef[3];
        R rel[3], odir[3], trel[3], tdir[3];
        for (int k = 0; k < 3; k++) rel[k] = w.qp[ob].pos[k] - w.qp[p].pos[k];
        R od = norm3(rel);
        const R pl[3] = {rel[0], rel[1], 0};
        R planar = norm3(pl);
        for (int k = 0; k < 3; k++) odir[k] = rel[k] / ((R)1e-6 + od);
        R mto = (R)0.1 * dt * dot3(w.qp[hd].vel, odir);
        R close = (R)0.1 * dt * (R)1 / ((R)1 + planar);
        for (int k = 0; k < 3; k++) trel[k] = w.qp[tg].pos[k] - w.qp[ob].pos[k];
        R td = norm3(trel);
        for (int k = 0; k < 3; k++) tdir[k] = trel[k] / ((R)1e-6 + td);
        R mtt = (R)1.5 * dt * dot3(w.qp[ob].vel, tdir);
        const int tb[4] = {3, 9, 12, 15};
        R touch = 0;
        for (int k = 0; k < 4; k++) {
          const R* c = w.info_c + 6 * tb[k];
          touch += c[0] * c[0] + c[1] * c[1] + c[2] * c[2] > (R)0.00001 ? (R)1 : (R)0;
        }
        touch = (R)0.2 * dt * touch;
        R hit = td < (R)coef[4] ? (R)1 : (R)0;
        reward[e] = mto + close + touch + (R)5 * hit + mtt;
        m[0] = close; m[1] = hit; m[2] = mtt; m[3] = mto; m[4] = touch;
      } else if (kind == BX_ENV_PUSHER) {
        n = obs_task(&s, kind, w.qp, coef, o, xy);
        R v1[3], v2[3];
        int tip = (int)coef[0], obj = (int)coef[1], goal = (int)coef[2];
        for (int k = 0; k < 3; k++) {
          v1[k] = q0[obj].pos[k] - q0[tip].pos[k];
          v2[k] = q0[obj].pos[k] - q0[goal].pos[k];
        }
        R near = -norm3(v1), dist = -norm3(v2), rc2 = -sq;
        reward[e] = dist + (R)0.1 * rc2 + (R)0.5 * near;
        m[0] = rc2; m[1] = dist; m[2] = near;  /* sorted: ctrl, dist, near */
      } else if (kind == BX_ENV_HUMANOID_STANDUP) {
        /* humanoid_standup.py:232-247; done unchanged; sorted metrics:
         * reward_linup, reward_quadctrl */
        n = obs_humanoid(&s, w.qp, a, o, 0);
        R uph = (w.qp[0].pos[2] - (R)0) / dt;
        R ctrl = (R)0.01 * sq;
        reward[e] = uph + (R)1 - ctrl;
        m[0] = uph; m[1] = -ctrl;
      }
      if (n != obs_size) rc = -1;
    }
    free(q0); free(ra); free(rb);
    work_free(&w);
  }
  sys_free(&s);
  return rc;
}

/* single phases over B envs (the standalone phase kernels' checker) */
int FN(oracle_phase)(const bx_desc* d, int which, int64_t B, const R* qp, const R* aux, R* out) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, Rn = s.Rn;
#pragma omp parallel
  {
    work_t w;
    work_alloc(&w, N, Rn);
    body_t* prev = calloc(N, sizeof(body_t));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      load_qp(w.qp, qp + e * 13 * N, N);
      if (which == 0) {
        kinetic(&s, &w);
      } else if (which == 1) {
        /* aux (B,N,6): dp vel, dp ang (integrators.py:85-93) */
        for (int b = 0; b < N; b++) {
          body_t* q = &w.qp[b];
          const R* dp = aux + (e * N + b) * 6;
          for (int k = 0; k < 3; k++) {
            R v = s.vdamp_exp * q->vel[k];
            v += (dp[k] + s.g[k]) * s.h;
            q->vel[k] = v * s.pos_mask[3 * b + k];
            R a = s.adamp_exp * q->ang[k];
            a += dp[3 + k] * s.h;
            q->ang[k] = a * s.rot_mask[3 * b + k];
          }
        }
      } else if (which == 2) {
        load_qp(prev, aux + e * 13 * N, N);
        velocity_projection(&s, &w, prev);
      }
      store_qp(w.qp, out + e * 13 * N, N);
    }
    free(prev);
    work_free(&w);
  }
  sys_free(&s);
  return 0;
}

/* capsule_plane contacts of every capsule-plane row: out (B,R,10) =
 * pos, vel, normal, penetration (rows of other kinds left untouched) */
int FN(oracle_phase_capsule_plane)(const bx_desc* d, int64_t B, const R* qp, R* out) {
  sysc s;
  sys_init(&s, d);
  int N = s.N, Rn = s.Rn;
#pragma omp parallel
  {
    body_t* q = calloc(N, sizeof(body_t));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      load_qp(q, qp + e * 13 * N, N);
      for (int r = 0; r < Rn; r++) {
        if (d->col_fn[d->row_group[r]] != BX_COL_CAPSULE_PLANE) continue;
        R* o = out + (e * Rn + r) * 10;
        contact_row(&s, r, q, o, o + 3, o + 6, o + 9);
      }
    }
    free(q);
  }
  sys_free(&s);
  return 0;
}

/* geometry.closest_segment_to_segment_points (geometry.py:394-461), exported
 * for the reference's known-answer cases (geometry_test.py:217-272) */
void FN(oracle_closest_segments)(int64_t n, const R* seg, R* a_best, R* b_best) {
  for (int64_t i = 0; i < n; i++) {
    const R* s = seg + 12 * i;
    R a0[3], a1[3], b0[3], b1[3];
    for (int k = 0; k < 3; k++) { a0[k] = s[k]; a1[k] = s[3 + k]; b0[k] = s[6 + k]; b1[k] = s[9 + k]; }
    R da[3], db[3];
    for (int k = 0; k < 3; k++) { da[k] = a1[k] - a0[k]; db[k] = b1[k] - b0[k]; }
    R la = safe_norm3(da);
    la += (R)1e-6 * (R)(la == 0);
    for (int k = 0; k < 3; k++) da[k] /= la;
    R hla = la * (R)0.5;
    R lb = safe_norm3(db);
    lb += (R)1e-6 * (R)(lb == 0);
    for (int k = 0; k < 3; k++) db[k] /= lb;
    R hlb = lb * (R)0.5;
    R am[3], bm[3], tr[3];
    for (int k = 0; k < 3; k++) { am[k] = a0[k] + da[k] * hla; bm[k] = b0[k] + db[k] * hlb; tr[k] = am[k] - bm[k]; }
    R dadb = dot3(da, db), datr = dot3(da, tr), dbtr = dot3(db, tr);
    R den = 1 - dadb * dadb;
    R ota = (-datr + dadb * dbtr) / (den + (R)1e-6);
    R otb = dbtr + ota * dadb;
    R ta = clip(ota, -hla, hla), tb = clip(otb, -hlb, hlb);
    R ba[3], bb[3];
    for (int k = 0; k < 3; k++) { ba[k] = am[k] + da[k] * ta; bb[k] = bm[k] + db[k] * tb; }
    R na[3], nb[3], d1, d2, ab[3], t[3], v[3], tt;
    for (int k = 0; k < 3; k++) { ab[k] = a1[k] - a0[k]; t[k] = bb[k] - a0[k]; }
    tt = clip(dot3(t, ab) / (dot3(ab, ab) + (R)1e-6), 0, 1);
    for (int k = 0; k < 3; k++) { na[k] = a0[k] + tt * ab[k]; v[k] = bb[k] - na[k]; }
    d1 = dot3(v, v);
    for (int k = 0; k < 3; k++) { ab[k] = b1[k] - b0[k]; t[k] = ba[k] - b0[k]; }
    tt = clip(dot3(t, ab) / (dot3(ab, ab) + (R)1e-6), 0, 1);
    for (int k = 0; k < 3; k++) { nb[k] = b0[k] + tt * ab[k]; v[k] = ba[k] - nb[k]; }
    d2 = dot3(v, v);
    if (d1 < d2) memcpy(ba, na, sizeof(na)); else memcpy(bb, nb, sizeof(nb));
    memcpy(a_best + 3 * i, ba, sizeof(ba));
    memcpy(b_best + 3 * i, bb, sizeof(bb));
  }
}

/* -------------------------------------------------------------- reset ---- */

/* System.default_qp (system.py:112-242) for B envs from explicit joint angles
 * and velocities (B, num_joint_dof). */
int FN(oracle_default_qp)(const bx_desc* d, const bx_reset_desc* rd, int64_t B,
                          const R* angles, const R* vels, R* qp_out) {
  int N = d->n_bodies, D = d->num_joint_dof;
#pragma omp parallel
  {
    body_t* q = calloc(N > 0 ? N : 1, sizeof(body_t));
    R* zmin = malloc(sizeof(R) * (rd->n_root_groups > 0 ? rd->n_root_groups : 1));
#pragma omp for schedule(static)
    for (int64_t e = 0; e < B; e++) {
      const R* ja = angles + e * D;
      const R* jv = vels + e * D;
      for (int b = 0; b < N; b++) {
        const double* s = rd->base_qp + 13 * b;
        for (int k = 0; k < 3; k++) { q[b].pos[k] = (R)s[k]; q[b].vel[k] = (R)s[7 + k]; q[b].ang[k] = (R)s[10 + k]; }
        for (int k = 0; k < 4; k++) q[b].rot[k] = (R)s[3 + k];
      }
      for (int f = 0; f < rd->n_fk; f++) {
        R ang3[3], vel3[3];
        for (int l = 0; l < 3; l++) {
          int ix = rd->fk_dof_index[3 * f + l];
          ang3[l] = ix >= 0 ? ja[ix] : (R)0;
          vel3[l] = ix >= 0 ? jv[ix] : (R)0;
        }
        R jr[4], ref[4];
        for (int k = 0; k < 4; k++) { jr[k] = (R)rd->fk_rot[4 * f + k]; ref[k] = (R)rd->fk_ref[4 * f + k]; }
        /* local_rot_ang (system.py:178-188) */
        R axes[3][3];
        for (int l = 0; l < 3; l++) {
          R e3[3] = {0, 0, 0};
          e3[l] = 1;
          rotate(e3, jr, axes[l]);
        }
        R lang[3];
        for (int k = 0; k < 3; k++) lang[k] = axes[0][k] * vel3[0] + axes[1][k] * vel3[1] + axes[2][k] * vel3[2];
        R rot[4];
        memcpy(rot, ref, sizeof(rot));
        for (int l = 0; l < 3; l++) {
          R ax[3], nr[4], t[4];
          rotate(axes[l], rot, ax);
          quat_rot_axis(ax, ang3[l], nr);
          quat_mul(nr, rot, t);
          memcpy(rot, t, sizeof(rot));
        }
        /* set_qp (system.py:197-209) */
        int bp = rd->fk_body_p[f], bc = rd->fk_body_c[f];
        R wr[4], oc[3], lp[3], wp[3], wa[3], offp[3], offc[3];
        for (int k = 0; k < 3; k++) { offp[k] = (R)rd->fk_off_p[3 * f + k]; offc[k] = (R)rd->fk_off_c[3 * f + k]; }
        quat_mul(q[bp].rot, rot, wr);
        rotate(offc, rot, oc);
        for (int k = 0; k < 3; k++) lp[k] = offp[k] - oc[k];
        rotate(lp, q[bp].rot, wp);
        rotate(lang, q[bp].rot, wa);
        for (int k = 0; k < 3; k++) { q[bc].pos[k] = q[bp].pos[k] + wp[k]; q[bc].ang[k] = wa[k]; }
        memcpy(q[bc].rot, wr, sizeof(wr));
      }
      /* bodies.min_z per root group, then lift (system.py:213-240) */
      for (int gi = 0; gi < rd->n_root_groups; gi++) zmin[gi] = (R)INFINITY;
      for (int b = 0; b < N; b++) {
        int gi = rd->body_root_group[b];
        if (gi < 0) continue;
        R bz = (R)INFINITY;
        for (int p = 0; p < rd->n_zpts; p++) {
          if (rd->zpt_body[p] != b) continue;
          R loc[3], wz[3];
          for (int k = 0; k < 3; k++) loc[k] = (R)rd->zpt_local[3 * p + k];
          rotate(loc, q[b].rot, wz);
          R z = q[b].pos[2] + wz[2] - (R)rd->zpt_radius[p];
          bz = z < bz ? z : bz;
        }
        if (rd->body_zero_cand[b]) bz = bz < 0 ? bz : (R)0;
        zmin[gi] = bz < zmin[gi] ? bz : zmin[gi];
      }
      for (int b = 0; b < N; b++) {
        int gi = rd->body_root_group[b];
        if (gi < 0) continue;
        q[b].pos[2] = q[b].pos[2] - zmin[gi] * (R)1;
        q[b].pos[0] = q[b].pos[0] - zmin[gi] * (R)0;
        q[b].pos[1] = q[b].pos[1] - zmin[gi] * (R)0;
      }
      store_qp(q, qp_out + e * 13 * N, N);
    }
    free(q); free(zmin);
  }
  return 0;
}
