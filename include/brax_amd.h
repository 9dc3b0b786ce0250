/*
 * brax_amd — C ABI of the MI355X-native PBD rigid-body stepper.
 *
 * This is the drop-in boundary for the reference's hot path:
 * what `brax.System.step`, `brax.System.default_qp/info` and the
 * `Env.step/reset` + Episode/AutoReset wrapper stack compute under `jax.jit`
 * is exported here as stream-ordered C calls on caller-owned device buffers.
 *
 *   reference interface                                  replaced by
 *   brax.System(config)          system.py:53-84         bx_system_create
 *   System.step(qp, act)         system.py:244-325       bx_system_step
 *   System.default_qp(a, v)      system.py:112-242       bx_system_default_qp
 *   System.info(qp)              system.py:249-252,327-340  bx_system_info
 *   Env.step + EpisodeWrapper + AutoResetWrapper
 *     ant.py:222-255, wrappers.py:105-148                bx_env_step
 *   Env.reset (+ EpisodeWrapper/AutoResetWrapper.reset counters)
 *     ant.py:198-220, humanoid.py:223-244,
 *     half_cheetah.py:164-180, wrappers.py:94-97,128-133 bx_env_reset
 *   Joint.angle_vel              joints.py:197-226       bx_system_joint_angles
 *
 * Conventions
 *   - Every array argument is a raw device pointer (HBM) owned by the caller.
 *     Sizes are explicit (n_envs, strides in elements); no torch types.
 *   - fp32 throughout on the device (what jit computes; `config.proto` floats
 *     are fp32). The descriptor is float64/int32 host memory, copied at create.
 *   - All calls enqueue on `stream` (a hipStream_t; NULL = default stream) and
 *     return immediately. Not re-entrant per handle.
 *   - Return 0 on success, non-zero on error; `bx_last_error()` returns a
 *     thread-local message. Descriptor errors surface at create time.
 */
#ifndef BRAX_AMD_H_
#define BRAX_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BX_ABI_VERSION 14

/* joint kinds, actuator kinds, contact functions (descriptor enums) */
enum { BX_JOINT_REVOLUTE = 1, BX_JOINT_UNIVERSAL = 2, BX_JOINT_SPHERICAL = 3 };
/* dynamics modes (config.proto dynamics_mode; system.py:244-247) */
enum { BX_DYN_PBD = 0, BX_DYN_LEGACY_SPRING = 1 };
enum { BX_ACT_TORQUE = 0, BX_ACT_ANGLE = 1 };
enum { BX_COL_CAPSULE_PLANE = 0, BX_COL_CAPSULE_CAPSULE = 1,
       /* box corner vs height map (colliders.py:699-739), capsule end vs
        * clipped plane (:762-802), capsule vs one triangle of a box / mesh
        * (:822-848) */
       BX_COL_HEIGHTMAP = 2, BX_COL_CLIPPED_PLANE = 3, BX_COL_CAPSULE_MESH = 4,
       /* box vs box by the separating axis test (:851-888), 4 rows a pair */
       BX_COL_HULL_HULL = 5 };
enum { BX_FORCE_THRUSTER = 0, BX_FORCE_TWISTER = 1 };
/* env layer kinds (obs / reward programs) */
enum { BX_ENV_NONE = 0, BX_ENV_ANT = 1, BX_ENV_HUMANOID = 2, BX_ENV_HALFCHEETAH = 3,
       BX_ENV_HUMANOID_STANDUP = 4,
       /* the planar walkers (hopper.py:183-246, walker2d.py:194-253): one
        * program, their own constructor defaults */
       BX_ENV_HOPPER = 5, BX_ENV_WALKER2D = 6,
       /* inverted_pendulum.py:133-164, inverted_double_pendulum.py:140-184,
        * acrobot.py:56-95 */
       BX_ENV_INVERTED_PENDULUM = 7, BX_ENV_INVERTED_DOUBLE_PENDULUM = 8, BX_ENV_ACROBOT = 9,
       /* reacher.py:172-236, reacherangle.py:60-106, swimmer.py:216-283,
        * pusher.py:211-242 */
       BX_ENV_REACHER = 10, BX_ENV_REACHERANGLE = 11, BX_ENV_SWIMMER = 12, BX_ENV_PUSHER = 13,
       /* egocentric target envs (ur5e.py:59-135, fetch.py:58-134) */
       BX_ENV_UR5E = 14, BX_ENV_FETCH = 15,
       /* a hand grasping an object (grasp.py:29-190) */
       BX_ENV_GRASP = 16 };
/* observation options. BX_OBS_XY: exclude_current_positions_from_observation
 * = False, the torso's x (and y) precede its z (ant.py:262-265,
 * humanoid.py:289-292: x, y; half_cheetah.py:206-209: x) */
enum { BX_OBS_XY = 1 };

/*
 * System descriptor: the compiled constant arrays of `brax.System`
 * (bodies.py:38-44, joints.py:36-77, actuators.py:28-35, colliders.py:95-114,
 * geometry.py:78-99,242-288, integrators.py:32-48). Built on the host by
 * brax_amd/compiler.py. Shapes in brackets; row-major; J = n_joints etc.
 */
typedef struct bx_desc {
  int32_t n_bodies, n_joints, n_actuators, n_rows, n_groups;
  int32_t substeps, action_size, num_joint_dof;
  double dt, h;
  double gravity[3];
  double velocity_damping, angular_damping;
  /* bodies */
  const double* body_mass;         /* [N] */
  const double* body_inv_inertia;  /* [N,3]  (inverse, body-frame diagonal) */
  const double* pos_mask;          /* [N,3] */
  const double* rot_mask;          /* [N,3] */
  const double* quat_mask;         /* [N,4] */
  /* joints, in application order (grouped by dof like joints.get) */
  const int32_t* joint_type;       /* [J] BX_JOINT_* */
  const int32_t* joint_dof;        /* [J] 1..3 (limit rows in use) */
  const int32_t* joint_free_dofs;  /* [J] -1 for revolute groups */
  const int32_t* joint_body_p;     /* [J] */
  const int32_t* joint_body_c;     /* [J] */
  const int32_t* joint_group;      /* [J] */
  const double* joint_off_p;       /* [J,3] */
  const double* joint_off_c;       /* [J,3] */
  const double* joint_axis_p;      /* [J,3,3] */
  const double* joint_axis_c;      /* [J,3,3] */
  const double* joint_limit;       /* [J,3,2] radians */
  const double* joint_damping;     /* [J] */
  const double* joint_scale_pos;   /* [J] */
  const double* joint_scale_ang;   /* [J] */
  /* actuators, in application order (sorted by type, dof) */
  const int32_t* act_type;         /* [K] BX_ACT_* */
  const int32_t* act_joint;        /* [K] index into joints */
  const int32_t* act_index;        /* [K,3] action index, -1 = masked */
  const int32_t* act_group;        /* [K] */
  const double* act_strength;      /* [K] */
  /* collider groups and flattened contact rows */
  const int32_t* col_oneway;       /* [G] 1 = OneWayCollider */
  const int32_t* col_fn;           /* [G] BX_COL_* */
  const double* col_scale;         /* [G] solver_scale_collide */
  const double* col_velocity_threshold; /* [G] */
  const double* col_baumgarte_erp; /* [G] */
  const int32_t* row_group;        /* [R] */
  const int32_t* row_body_a;       /* [R] */
  const int32_t* row_body_b;       /* [R] */
  const double* row_a_pos;         /* [R,3] collidable offset of a */
  const double* row_a_end;         /* [R,3] capsule end (plane: end point in body a) */
  const double* row_a_radius;      /* [R] */
  const double* row_b_pos;         /* [R,3] */
  const double* row_b_end;         /* [R,3] */
  const double* row_b_radius;      /* [R] */
  const double* row_friction;      /* [R] friction_a * friction_b */
  const double* row_elasticity;    /* [R] */
  /* forces (forces.py:27-138), in application order: Thrusters, then
   * Twisters, each in config order; action indices assigned in config order
   * after the actuators' (post-sphericalisation) dofs */
  int32_t n_forces;
  const int32_t* force_type;       /* [NF] BX_FORCE_* */
  const int32_t* force_body;       /* [NF] */
  const int32_t* force_index;      /* [NF,3] action index (clipped like jp.take) */
  const double* force_strength;    /* [NF] */
  /* NearNeighbors culling (colliders.py:55-89): per group the number of rows
   * kept each step (0 = Pairs, every row active); per row its cell i*U+j in
   * the candidate matrix (-1 for Pairs rows). A culled group's rows are its
   * allowed cells in flat order; Info carries `cutoff` rows for it, nearest
   * first (top_k order). */
  const int32_t* col_cutoff;       /* [G] */
  const int32_t* row_flat;         /* [R] */
  /* legacy_spring dynamics (system.py:342-390, spring_joints.py): joints are
   * springy Revolute / Universal / Spherical groups by dof (no
   * sphericalisation), constrained at the acceleration level; contacts use
   * the impulse model with Baumgarte stabilisation every substep. The three
   * arrays may be NULL for pbd systems. */
  int32_t dynamics_mode;           /* BX_DYN_* */
  const double* joint_stiffness;       /* [J] */
  const double* joint_spring_damping;  /* [J] (default: 0.5 or 2 x sqrt(stiffness)) */
  const double* joint_limit_strength;  /* [J] (default: stiffness) */
  /* extended contact functions: per-row constants (may be NULL when no row
   * uses them)
   *   HEIGHTMAP:     ext[0] cell size; row_hm (offset into hm_data, mesh size)
   *   CLIPPED_PLANE: ext normal 0..2, x 3..5, y 6..8, position 9..11,
   *                  half sizes 12, 13 (b's body frame)
   *   CAPSULE_MESH:  ext triangle p0 0..2, p1 3..5, p2 6..8, normal 9..11
   *                  (b's body frame, winding fixed as geometry.py:138-154) */
  const double* row_ext;           /* [R,16] */
  const int32_t* row_hm;           /* [R,2] */
  int32_t n_hm;
  const double* hm_data;           /* [n_hm] row-major square grids */
  /* HULL_HULL rows: ext (hull a, hull b, contact e) into these box hulls
   * (geometry.py:201-206), body frame */
  int32_t n_hull;
  const double* hull_vert;         /* [H,8,3] corners */
  const double* hull_face;         /* [H,6,4,3] quads, winding fixed */
  const double* hull_norm;         /* [H,6,3] face normals */
  /* NearNeighbors with more `cutoff` than allowed cells: top_k of the
   * masked (-inf) cells picks the lowest flat indices (jax.lax.top_k keeps
   * ties in index order), so those cells are rows too, flagged 1 here; they
   * rank after every allowed cell, in flat order (colliders.py:78-85).
   * NULL = no masked rows. */
  const int32_t* row_nn_masked;    /* [R] */
} bx_desc;

/*
 * Reset descriptor (`System.default_qp`, system.py:112-242; bodies.min_z
 * bodies.py:62-98): joint-tree forward kinematics in depth order, then lift
 * every free root tree so its lowest collider touches z = 0.
 */
typedef struct bx_reset_desc {
  int32_t n_fk;                    /* joints in depth order */
  const int32_t* fk_body_p;        /* [n_fk] */
  const int32_t* fk_body_c;        /* [n_fk] */
  const int32_t* fk_dof_index;     /* [n_fk,3] index into joint angle vector, -1 = 0 */
  const double* fk_rot;            /* [n_fk,4] euler_to_quat(rotation) */
  const double* fk_ref;            /* [n_fk,4] euler_to_quat(reference_rotation) */
  const double* fk_off_p;          /* [n_fk,3] */
  const double* fk_off_c;          /* [n_fk,3] */
  const double* base_qp;           /* [N,13] config default qps (else identity) */
  int32_t n_zpts;                  /* min_z candidate points */
  const int32_t* zpt_body;         /* [n_zpts] */
  const double* zpt_local;         /* [n_zpts,3] point in body frame */
  const double* zpt_radius;        /* [n_zpts] */
  const int32_t* body_zero_cand;   /* [N] 1: min_z also sees 0.0 (plane/none) */
  const int32_t* body_root_group;  /* [N] lift group, -1 = not lifted */
  int32_t n_root_groups;
  /* System.default_angle (system.py:86-110) of this default: the joint-angle
   * vector that bx_env_reset adds its noise to */
  const double* default_angle;     /* [num_joint_dof] */
} bx_reset_desc;

/* A strided view of one fp32 QP field: element (env e, body b, k) lives at
 * ptr[e*env_stride + b*body_stride + k]. Lets the caller pass the reference's
 * (B,N,3)/(B,N,4) arrays or the packed (B,N,16) layout without copies. */
typedef struct bx_field {
  float* ptr;
  int64_t env_stride;
  int64_t body_stride;
} bx_field;

typedef struct bx_qp {
  bx_field pos, rot, vel, ang;     /* rot is wxyz */
} bx_qp;

/* Optional Info outputs of System.step (base.py:136-153); NULL ptr = skip. */
typedef struct bx_info {
  bx_field contact_vel, contact_ang;     /* (B,N,3) accumulated contact P */
  bx_field actuator_vel, actuator_ang;  /* (B,N,3) */
  float* contact_pos;                   /* (B,R,3) contiguous */
  float* contact_normal;                /* (B,R,3) */
  float* contact_penetration;           /* (B,R)   */
  bx_field joint_vel, joint_ang;        /* (B,N,3) accumulated joint P
                                           (legacy_spring; zero under pbd) */
  /* (B,R) contiguous, bx_system_step only (ABI 9): the NearNeighbors cell
   * i * U + j behind each Info contact row, i.e. the `idx` of
   * `jp.top_k(sim.ravel(), cutoff)` in colliders.py:84 for a culled group's
   * rows (nearest first), -1 for Pairs rows */
  int32_t* contact_cell;
} bx_info;

/* Env-layer state of one batch (ant.py:198-255, wrappers.py:83-148).
 * obs (B,O), reward/done/steps/truncation (B,), metrics (B,M); contiguous. */
typedef struct bx_env_state {
  bx_qp qp;
  float* obs;
  float* reward;
  float* done;
  float* metrics;
  float* steps;
  float* truncation;
  /* per-env random stream of the target envs (UR5E, FETCH: the teleported
   * target, ur5e.py:107-113); read from the input state, advanced in the
   * output; NULL for the other kinds */
  uint32_t* rng;
} bx_env_state;

typedef struct bx_env_params {
  int32_t kind;             /* BX_ENV_* */
  int32_t obs_size;
  int32_t n_metrics;
  int32_t episode_length;   /* <= 0: no EpisodeWrapper */
  int32_t action_repeat;    /* EpisodeWrapper action_repeat (>= 1) */
  int32_t auto_reset;       /* AutoResetWrapper present */
  int32_t obs_flags;        /* BX_OBS_* */
  /* env constructor arguments (ant.py:173-183, humanoid.py:196-212,
   * half_cheetah.py:147-158):
   *   ANT:         forward_w(unused=1), ctrl_cost_weight, contact_cost_weight,
   *                healthy_reward, healthy_z_min, healthy_z_max,
   *                terminate_when_unhealthy, use_contact_forces
   *   HUMANOID:    forward_reward_weight, ctrl_cost_weight, 0, healthy_reward,
   *                healthy_z_min, healthy_z_max, terminate_when_unhealthy, 0
   *   HALFCHEETAH: forward_reward_weight, ctrl_cost_weight, 0...
   *   HOPPER / WALKER2D: forward_reward_weight, ctrl_cost_weight,
   *                healthy_reward, healthy_z_min, healthy_z_max (+inf: pass
   *                FLT_MAX), healthy_angle_min, healthy_angle_max,
   *                terminate_when_unhealthy
   *   INVERTED_PENDULUM, INVERTED_DOUBLE_PENDULUM, ACROBOT: none (the
   *                reference envs take no reward arguments)
   *   REACHER:     target body, arm body (indices as floats)
   *   REACHERANGLE: target body, arm body, then per action i (<= 2) the
   *                angle-limit min (coef[2 + i]) and range (coef[4 + i]) the
   *                [-1, 1] action maps onto
   *   SWIMMER:     forward_reward_weight, ctrl_cost_weight, spherical drag,
   *                capsule drag corrections x, y, z (swimmer.py:177-193)
   *   PUSHER:      tip body, object body, goal body
   *   UR5E / FETCH: torso body, target body, target radius, target
   *                distance, target height (a hit target moves to a fresh
   *                random spot on the ring [radius, radius + distance))
   *   GRASP:       palm body, object body, target body, hand body (thumb
   *                proximal), target radius, distance, height */
  float coef[8];
  /* AutoReset targets (first_qp / first_obs); required when auto_reset */
  bx_qp first_qp;
  const float* first_obs;
  /* GRASP: device array [2, A] of per-action (min, range); System.step reads
   * min + range * (a + 1) / 2 (grasp.py:42-52,65); NULL for the other kinds */
  const float* act_map;
} bx_env_params;

typedef struct bx_system bx_system;

int bx_abi_version(void);
const char* bx_last_error(void);
int bx_device_count(int* count);

int bx_system_create(const bx_desc* desc, const bx_reset_desc* reset,
                     int device, bx_system** out);
int bx_system_destroy(bx_system* sys);

/* Threads that own one env in this system's step kernels: 16/32/64 lanes of
 * one wavefront, or a whole 128/256-thread workgroup for large scenes. */
int bx_system_lanes(bx_system* sys);

/* Threads per env of this system's Env.step / rollout kernels (bx_env_step,
 * bx_env_rollout_*): the step kernels' lanes. (ABI 12's opt-in 32-lane
 * spherical joint halves measured slower and were removed in ABI 13.) */
int bx_system_env_lanes(bx_system* sys);

/* The host half of bx_system_create, without a device: the kernel plan the
 * descriptor compiles to -- mode (1 SINGLE: register-hoisted, one env per
 * 16/32/64 lanes; 3 MULTI: one env per 256-thread workgroup; 0 item loops),
 * threads per env, and the System.step kernel's LDS bytes per workgroup
 * (160 KB per CU / that = envs a CU holds at once). */
int bx_system_plan(const bx_desc* desc, const bx_reset_desc* reset, int32_t* mode,
                   int32_t* lanes, int32_t* lds_bytes);

/* The same host half with its product: the blob bx_system_create would copy
 * to the device (n_words 32-bit words, the BlobHdr first) and the whole plan,
 * plan = {mode, lanes, lds_bytes, feat, gw, fold, jb, cb}. words may be NULL
 * to ask only for n_words and the plan; a capacity (in words) below n_words is
 * an error. No device. */
int bx_system_blob(const bx_desc* desc, const bx_reset_desc* reset, uint32_t* words,
                   int64_t capacity, int64_t* n_words, int32_t plan[8]);

/* LDS bytes per workgroup of this system's System.step kernel (the current
 * variant): with 160 KB per CU it sets how many envs a CU holds at once (the
 * large-scene kernel runs one env per 256-thread workgroup). A diagnostic
 * query; 0 for a null handle. */
int bx_system_lds_bytes(bx_system* sys);

/* Select the register-hoisted kernel variant (default when the system fits:
 * every lane owns <= 1 body/joint/actuator/contact row) or the generic
 * item-loop variant (on = 0). For testing both paths on one system. */
int bx_system_set_single(bx_system* sys, int on);

/* Kernel variant: threads per env (16/32/64/128/256) and constant placement
 * (0: read from HBM in the loops, 1: hoisted to registers, needs <= 1 item per
 * lane, 2: staged in LDS once per workgroup, 3: MULTI, the large-scene pbd
 * kernel at 256 threads: items and <= 4 contact rows per lane hoisted to
 * registers, per-body contact sums through gather tasks). */
int bx_system_set_variant(bx_system* sys, int lanes, int mode);

/* Threads per workgroup of the step kernels: a multiple of the lanes per env,
 * at most 64 (default 64, i.e. 64 / lanes envs per wavefront). Fewer envs per
 * wave means more waves for the same batch (32: two waves per SIMD at 4096
 * Ant envs). Results are identical bit for bit. */
int bx_system_set_block(bx_system* sys, int threads);

/* Physics only: B independent System.step calls (system.py:244-325).
 * act: (B, act_width) with row stride act_stride (0 broadcasts one row).
 * Action indices are clipped to [0, act_width) like the reference's
 * `jp.take(act, index)` (jumpy.py:146-151); act_width >= 1 unless the system
 * reads no action. qp_in and qp_out may not alias. info may be NULL.
 * A MULTI system's overflow buffer (the penetrating contacts past the first
 * 128 of a pass) is scratch, written before it is read within a step, and
 * every allocation of it lives as long as the System, so a graph captured at
 * one batch stays valid after later steps at larger ones. Stepping one System
 * concurrently on two streams is unsupported: both calls would use the same
 * per-env slices of that buffer. */
int bx_system_step(bx_system* sys, int64_t n_envs, const bx_qp* qp_in,
                   const float* act, int64_t act_stride, int64_t act_width,
                   const bx_qp* qp_out, const bx_info* info, void* stream);

/* Env layer fused with physics: for each env, EpisodeWrapper-repeat
 * action_repeat times (System.step + obs/reward/done/metrics), then the
 * episode counters and the AutoReset select. in/out may not alias. */
int bx_env_step(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                const bx_env_state* in, const float* act, int64_t act_stride,
                int64_t act_width, const bx_env_state* out, void* stream);

/* bx_env_step on the packed layout, every pointer plain: the input state is
 * qp_in (B,N,16) (pos 0:3, rot 3:7, vel 7:10, ang 10:13), done_in (B,),
 * steps_in (B,) or NULL, rng_in (B,) or NULL; the output is ONE buffer
 * `out` holding qp (B,N,16) | obs (B,O) | reward | done | steps |
 * truncation (B each) | metrics (B,M), and rng_out (B,) or NULL. Same
 * semantics and errors as bx_env_step; the host-side fast path of
 * Env.step. */
int bx_env_step_packed(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                       const float* qp_in, const float* done_in, const float* steps_in,
                       const uint32_t* rng_in, const float* act, int64_t act_stride,
                       int64_t act_width, float* out, uint32_t* rng_out, void* stream);

/* n_steps consecutive bx_env_step_packed calls in ONE launch: an open-loop
 * rollout (the reference's `jax.lax.scan` of `env.step`, e.g.
 * training/acting.py:53-77 generate_unroll, with the actions known up front:
 * random-action rollouts). Step t reads its action rows at act + t *
 * act_step_stride (row stride act_stride) and writes its whole output - qp
 * (B,N,16) | obs (B,O) | reward | done | steps | truncation (B each) |
 * metrics (B,M) - as block t of `out` (block = B * (N*16 + O + 4 + M)
 * floats), its rng stream (target envs) at rng_out + t * B; its input state
 * is step t - 1's output (step 0: qp_in, done_in, steps_in, rng_in). Every
 * step's outputs are bit-identical to the chained single-step calls; the
 * state stays on chip between steps (ABI 9). */
int bx_env_rollout_packed(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                          int32_t n_steps, const float* qp_in, const float* done_in,
                          const float* steps_in, const uint32_t* rng_in, const float* act,
                          int64_t act_stride, int64_t act_step_stride, int64_t act_width,
                          float* out, uint32_t* rng_out, void* stream);

/* bx_env_rollout_packed with the actions drawn on the device inside the same
 * launch: the reference's random-action rollout, a `lax.scan` of `env.step`
 * on `jax.random.uniform` actions (notebooks/environments.ipynb:386-423, the
 * published benchmark loop; the scan of training/acting.py:53-77). Step t's
 * action a of env e is uniform_at(seed, offset + t * step_stride +
 * e * act_width + a) in [lo, hi): the same bits bx_uniform_slabs(act, B * A,
 * K, seed, offset, step_stride, NULL, 0, lo, hi) writes, so this equals that
 * draw followed by bx_env_rollout_packed on its slabs. act_out (optional,
 * (K, n_envs, act_width) contiguous) records the drawn actions. The whole
 * action row is staged on chip: act_width must not exceed the widest row the
 * system reads (every env's own action size fits). Env kinds whose program
 * reads the raw row itself (ReacherAngle, Swimmer, Grasp, Humanoid,
 * HumanoidStandup) are refused: draw with bx_uniform_slabs. n_steps = 0
 * only checks the arguments (ABI 10). */
int bx_env_rollout_random(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                          int32_t n_steps, const float* qp_in, const float* done_in,
                          const float* steps_in, const uint32_t* rng_in, uint64_t seed,
                          uint64_t offset, uint64_t step_stride, float lo, float hi,
                          int64_t act_width, float* act_out, float* out, uint32_t* rng_out,
                          void* stream);

/* An MLP policy with a NormalTanh head (the reference's networks.MLP,
 * distribution.NormalTanhDistribution and ppo/networks.make_inference_fn) as
 * a plain descriptor; every buffer is the caller's, on the system's device,
 * and is read at launch time, so parameters updated in place (or a replayed
 * graph) take effect without a new descriptor.
 *   params: layer l's kernel W (width[l-1], width[l]) row-major (flax's
 *     layout; width[-1] = obs_size), then its bias (width[l]), layer after
 *     layer, float32, 16-byte aligned;
 *   the last layer's width is 2 A (loc | scale parameter), or A with
 *     deterministic set; hidden layers apply `activation`;
 *   obs_mean / obs_std (obs_size each, both or neither): x = (obs - mean) / std;
 *   scale = softplus(s) + min_std; raw = loc + scale * eps (loc when
 *     deterministic); action = tanh(raw).
 * Limits (beyond them the call fails, nothing is launched): 1..8 layers,
 * widths 1..128, obs_size <= 512, and the workgroup's LDS (the system's
 * bx_system_lds_bytes plus, per env of the workgroup, 4 * (obs_size + 2 *
 * max(obs_size, widths, 2 A)) bytes rounded up to 16-byte records) within
 * 160 KiB. The parameters are staged in LDS when that total plus 4 * n_params
 * stays within 40 KiB (four workgroups co-resident per compute unit), else
 * they are read from global memory through the cache (ABI 14). */
#define BX_POLICY_MAX_LAYERS 8
#define BX_POLICY_MAX_WIDTH 128
#define BX_POLICY_MAX_OBS 512
#define BX_POLICY_SWISH 0
#define BX_POLICY_RELU 1
#define BX_POLICY_TANH 2
typedef struct bx_policy {
  const float* params;
  int32_t n_layers;
  int32_t width[BX_POLICY_MAX_LAYERS];
  int32_t activation; /* BX_POLICY_* */
  const float* obs_mean;
  const float* obs_std;
  float min_std;
  int32_t deterministic;
  int32_t action_size; /* A: the env's action row (the system stages all of it) */
} bx_policy;

/* bx_env_rollout_packed with step t's actions computed inside the launch by
 * `policy` from the env's current observation: step 0 reads obs_in (n_envs,
 * obs_size), step t > 0 the observation step t - 1 wrote to its output block
 * (after an AutoReset select: first_obs); the row stays on chip. The noise of
 * step t, env e, action a is N(seed, i) = sqrt(-2 ln(1 - U(seed, i))) *
 * cos(2 pi U(seed, i + 1)) with i = offset + t * step_stride + (e * A + a) * 2
 * and U the [0, 1) draw of bx_uniform: the bits bx_normal_slabs(eps, B * A, K,
 * seed, offset, step_stride, NULL, 0) writes. Optional outputs: act_out and
 * raw_out (K, n_envs, A), logp_out (K, n_envs): log_prob of raw under the
 * head's Normal minus the tanh log-det, summed over the actions
 * (deterministic: evaluated at the mode, eps = 0). The env kinds
 * bx_env_rollout_random refuses are refused here too, as are systems not in
 * SINGLE mode. n_steps = 0 only checks the arguments (ABI 14). */
int bx_env_rollout_policy(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                          int32_t n_steps, const float* qp_in, const float* obs_in,
                          const float* done_in, const float* steps_in, const uint32_t* rng_in,
                          const bx_policy* policy, uint64_t seed, uint64_t offset,
                          uint64_t step_stride, float* act_out, float* raw_out, float* logp_out,
                          float* out, uint32_t* rng_out, void* stream);

/* Whole evaluation episodes in one launch (the reference's acting.Evaluator
 * over EvalWrapper, training/acting.py:77-139, envs/wrappers.py:169-203): the
 * K steps of bx_env_rollout_policy (bx_env_eval_policy) or of
 * bx_env_rollout_packed (bx_env_eval_packed, step t's actions at act + t *
 * act_step_stride), with EvalWrapper.step applied per env after every step,
 * in float32 and in the wrapper's order:
 *   episode_steps = active != 0 ? steps : episode_steps
 *   sum[k] += metric[k] * active   (the env's M metrics, then the step's reward)
 *   active *= 1 - done
 * steps and done being the values the step writes to its block. The sums stay
 * on chip for the whole launch and no per-step output is written:
 *   out      ONE block, n_envs * (N*16 + O + 4 + M) floats: the K-th step's
 *            qp | obs | reward, done, steps, truncation | metrics;
 *   eval_in, eval_out  (M + 3, n_envs) float32: rows 0..M-1 the metric sums in
 *            the env's metric order, row M the reward sum, row M + 1
 *            active_episodes, row M + 2 episode_steps. They may be the same
 *            buffer; a null eval_in starts a fresh evaluation (zero sums,
 *            active 1, steps 0), so an evaluation continues across launches;
 *   rng_out  (n_envs), the target envs' streams after the K-th step.
 * bx_env_eval_policy refuses what bx_env_rollout_policy refuses;
 * bx_env_eval_packed takes every env kind. Both need a SINGLE-mode system and
 * add 16-byte-rounded 4 * (2 M + 3) bytes per env of the workgroup to its LDS
 * (within 160 KiB). n_steps = 0 only checks the arguments. */
int bx_env_eval_policy(bx_system* sys, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                       const float* qp_in, const float* obs_in, const float* done_in,
                       const float* steps_in, const uint32_t* rng_in, const bx_policy* policy,
                       uint64_t seed, uint64_t offset, uint64_t step_stride, const float* eval_in,
                       float* out, float* eval_out, uint32_t* rng_out, void* stream);
int bx_env_eval_packed(bx_system* sys, const bx_env_params* env, int64_t n_envs, int32_t n_steps,
                       const float* qp_in, const float* done_in, const float* steps_in,
                       const uint32_t* rng_in, const float* act, int64_t act_stride,
                       int64_t act_step_stride, int64_t act_width, const float* eval_in, float* out,
                       float* eval_out, uint32_t* rng_out, void* stream);

/* One episode per perturbed policy in one launch: the env-side half of the
 * reference's evolution agents (ES training/agents/es/train.py:136-164, ARS
 * training/agents/ars/train.py:106-130, run_episode). bx_env_eval_policy with
 * `policy` as the shape shared by every member and, from `pop`:
 *   param_stride  env e evaluates the parameter row at policy->params + e *
 *            param_stride floats (>= n_params, a multiple of 4; rows in
 *            bx_policy's layout). 0: every env shares the one row;
 *   head     BX_HEAD_NORMAL_TANH: bx_policy's head, bit for bit.
 *            BX_HEAD_IDENTITY: action = raw = loc (ARS's obs @ W; a zero bias
 *            row expresses a bias-free matrix): the last layer is A wide, no
 *            noise is drawn and `deterministic` / `min_std` are not read;
 *   reward_shift  the reward sum becomes sum += (reward - reward_shift) *
 *            active (0: bx_env_eval_policy's line exactly);
 *   mom_in, mom_out  (n_envs, 2 O + 1) float32 per env S1 (O) | S2 (O) | count,
 *            the weighted observation sums of running_statistics.update
 *            (acme/running_statistics.py:156-173) centred on the policy's
 *            obs_mean m (0 without one). Before each step's policy
 *            evaluation, with a the env's active flag before the step and o
 *            the row the policy is about to read: d = o[i] - m[i], q = d * d,
 *            S1[i] += a * d, S2[i] += a * q, count += a, one float32 rounding
 *            each. They may be the same buffer; a null mom_in starts from
 *            zeros; a null mom_out keeps no moments (and none of their LDS);
 *   flags    BX_POP_NO_STAGE: read the rows from global memory whatever the
 *            LDS budget (the same bits; an A/B switch).
 * Written back on success, n_steps = 0 included: `staged` (1: each env's lanes
 * copy its row into LDS once per launch; 0: the rows, or the shared row, are
 * read as bx_env_eval_policy reads its parameters) and `lds_bytes`, the
 * workgroup's dynamic LDS. Rows are staged when param_stride != 0 and
 * bx_env_eval_policy's LDS without a staged copy, plus per env of the workgroup
 * the 16-byte-rounded moments and row, stays within 40 KiB. A non-finite row
 * or observation poisons its own env alone. Refuses what bx_env_rollout_policy
 * refuses, a param_stride that is non-zero and below n_params or not a
 * multiple of 4, an unknown head, and a workgroup LDS beyond 160 KiB.
 * n_steps = 0 only checks the arguments. (Additive: no ABI bump.) */
#define BX_HEAD_NORMAL_TANH 0
#define BX_HEAD_IDENTITY 1
#define BX_POP_NO_STAGE 1
typedef struct bx_population {
  int64_t param_stride;
  int32_t head; /* BX_HEAD_* */
  float reward_shift;
  const float* mom_in;
  float* mom_out;
  int32_t flags;     /* BX_POP_* */
  int32_t staged;    /* out */
  int32_t lds_bytes; /* out */
} bx_population;
int bx_env_eval_population(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                           int32_t n_steps, const float* qp_in, const float* obs_in,
                           const float* done_in, const float* steps_in, const uint32_t* rng_in,
                           const bx_policy* policy, uint64_t seed, uint64_t offset,
                           uint64_t step_stride, const float* eval_in, float* out, float* eval_out,
                           uint32_t* rng_out, bx_population* pop, void* stream);

/* Batched System.default_qp from per-env joint angles/velocities
 * (B, num_joint_dof) contiguous (system.py:112-242). */
int bx_system_default_qp(bx_system* sys, int64_t n_envs,
                         const float* joint_angle, const float* joint_velocity,
                         const bx_qp* qp_out, void* stream);

/* Batched reset-time Info (`_pbd_info`, system.py:327-340: Collider.apply). */
int bx_system_info(bx_system* sys, int64_t n_envs, const bx_qp* qp,
                   const bx_info* info, void* stream);

/* Observation and metric widths the env layer writes for `env` on this
 * system (obs_size / n_metrics in bx_env_params must equal them). */
int bx_env_sizes(bx_system* sys, const bx_env_params* env, int32_t* obs_size,
                 int32_t* n_metrics);

/* Env.reset of every env kind, batched, in two launches (ant.py:198-220,
 * humanoid.py:223-244, half_cheetah.py:164-180, humanoid_standup.py:216-230,
 * reacher.py:156-174, reacherangle.py:44-60, pusher.py:178-209,
 * ur5e.py:41-58, fetch.py:41-57, grasp.py:54-70). For env e (global id
 * g = env_offset + e), with D = num_joint_dof and W draws per env, the k-th
 * draw is the counter RNG at (seed, g * W + k):
 *   default kinds (W = 2D, s = noise_scale):
 *     qpos = default_angle + U[-s, s) (k = dof), qvel = U[-s, s) (k = D + dof)
 *   REACHER, REACHERANGLE (W = 2D + 2): the same with U[-.1, .1) and
 *     U[-.005, .005); the target (coef[0]) at (d cos a, d sin a, .01) with
 *     d = .2 u (ReacherAngle .2 sqrt(u)) at k = 2D, a = 2 pi u at k = 2D + 1
 *   PUSHER (W = D - 2): default angles, qvel U[-.005, .005) on the first
 *     D - 4 dofs (k = dof); the object (coef[1]) at U[-.3, 0) x U[-.2, .2)
 *     (k = D - 4, D - 3) scaled into a .17 disc, z = .05; the goal (coef[2])
 *     at (.45, .05, .05); the table (coef[3]) at the origin
 *   UR5E, FETCH (W = 2): the default pose at rest; the target (coef[1]) at
 *     radius coef[2] + coef[3] u (k = 0), angle 2 pi u (k = 1), z = coef[4]
 *   GRASP: the default pose at rest
 *   qp   = System.default_qp(qpos, qvel) (system.py:112-242), then the
 *          placed bodies' positions
 *   obs  = _get_obs(qp, System.info(qp), 0)    (system.py:327-340)
 *   reward = done = metrics = 0; steps = truncation = 0 when given;
 *   UR5E, FETCH, GRASP: out->rng (required) = the env's stream, a hash of
 *   (seed, g).
 * noise_scale is read by the default kinds only (the others' ranges are
 * fixed by the reference envs). Keying by global env id makes the states
 * independent of how a batch is sharded over GPUs. env_seeds
 * (device, n_envs uint64, may be NULL) gives every env its own key instead,
 * as `VmapWrapper.reset` over a (B, 2) key batch (wrappers.py:79-80): env e
 * then draws from (env_seeds[e], k) and hashes (env_seeds[e], 0) for its
 * stream. The JAX threefry stream itself is parity-unpinned.
 * The params' first_qp / first_obs are not read. */
int bx_env_reset(bx_system* sys, const bx_env_params* env, int64_t n_envs, uint64_t seed,
                 int64_t env_offset, const uint64_t* env_seeds, float noise_scale,
                 const bx_env_state* out, void* stream);

/* Env observation of a state (Env._get_obs with the reset-time Info). */
int bx_env_observe(bx_system* sys, const bx_env_params* env, int64_t n_envs,
                   const bx_qp* qp, const float* act, int64_t act_stride,
                   int64_t act_width, float* obs, void* stream);

/* Joint angles and angular velocities of every joint dof (Joint.angle_vel,
 * joints.py:197-226,311-319,388-415; Spherical: line-of-nodes x-y'-z''
 * angles), in joint order: angle and vel are (B, num_joint_dof) contiguous
 * (num_joint_dof counted after sphericalisation). */
int bx_system_joint_angles(bx_system* sys, int64_t n_envs, const bx_qp* qp, float* angle,
                           float* vel, void* stream);

/* Counter-based uniform [lo,hi) fill: out[i] = U(seed, offset + i), a
 * splitmix64 hash of (seed, global index); the same stream bx_env_reset draws
 * its noise from. Used for synthetic actions (offset = global env id x width,
 * so shards reproduce one big batch) and reset noise (the JAX threefry stream
 * is parity unpinned). */
int bx_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset,
               float lo, float hi, void* stream);

/* bx_uniform with the offset read on the device: out[i] = U(seed, offset +
 * (*epoch) * epoch_stride + i), `epoch` a device int64 the caller advances
 * in stream order. A hipGraph-captured rollout (brax_amd.envs.graph) replays
 * the same launch and still draws a fresh slab per replay, exactly the slab
 * bx_uniform would draw at offset + epoch * epoch_stride (ABI 8). */
int bx_uniform_epoch(float* out, int64_t n, uint64_t seed, uint64_t offset,
                     const int64_t* epoch, uint64_t epoch_stride,
                     float lo, float hi, void* stream);

/* n_slabs slabs of slab_n elements in one launch, each slab at its own
 * offset: out[s * slab_n + j] = U(seed, offset + (*epoch) * epoch_stride +
 * s * slab_stride + j), epoch NULL reading as 0. A graph-captured rollout of K
 * steps draws its K action slabs with one launch (slab_stride = the job's
 * per-step stride world x B x A, so every slab is bit-identical to the
 * bx_uniform draw of that step; ABI 9). The bx_uniform* calls launch on the
 * device that owns `stream` (the current device for NULL). */
int bx_uniform_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                     uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                     uint64_t epoch_stride, float lo, float hi, void* stream);

/* Standard normals over the same slabs: out[s * slab_n + j] = N(seed, offset +
 * (*epoch) * epoch_stride + s * slab_stride + 2 j), N as bx_env_rollout_policy
 * defines it (each sample takes two counters; ABI 14). */
int bx_normal_slabs(float* out, int64_t slab_n, int64_t n_slabs, uint64_t seed,
                    uint64_t offset, uint64_t slab_stride, const int64_t* epoch,
                    uint64_t epoch_stride, void* stream);

/* A strided view of one fp32 (T, B) sequence array: element (step t, env e)
 * lives at ptr[t * time_stride + e * env_stride] (strides in elements). The
 * time-major (K, B) rows of bx_env_rollout_policy's blocks and the reference's
 * [B, T] arrays both pass without a copy. */
typedef struct bx_seq {
  float* ptr;
  int64_t time_stride;
  int64_t env_stride;
} bx_seq;

/* Generalised advantage estimation of a whole (T, B) unroll in one launch:
 * the reference's `compute_gae` (training/agents/ppo/losses.py:37-93) with the
 * reward scaling and the termination product of `compute_ppo_loss` (:142-144)
 * in front of it. `done` stands for 1 - discount_t, so termination = done *
 * (1 - truncation). One lane per env runs the reverse scan; for t = T-1 .. 0,
 * with v_next = t == T-1 ? bootstrap[e] : values[t+1], vs_next likewise (the
 * previous iteration's vs[t]) and acc starting at 0:
 *   r     = reward[t] * reward_scaling
 *   term  = done[t] * (1 - truncation[t])
 *   mask  = 1 - truncation[t]
 *   g     = discount * (1 - term)
 *   delta = ((r + g * v_next) - values[t]) * mask
 *   acc   = delta + ((g * mask) * lambda) * acc
 *   vs[t] = acc + values[t]
 *   advantages[t] = ((r + g * vs_next) - values[t]) * mask
 * in float32, every operation rounded on its own (no fused multiply-add), in
 * that order: bit for bit what the same lines give as separate elementwise
 * float32 operations. NaN and Inf propagate as IEEE has them (NaN * 0 is
 * NaN); a non-finite input of env e reaches no other env's outputs.
 * bootstrap is (B,) contiguous. The outputs may have any layout but must not
 * overlap the inputs or each other. n_steps < 1, n_envs < 0, a null pointer
 * or a zero stride on an output fail; n_envs = 0 launches nothing. No system
 * handle: the launch goes to the device that owns `stream` (the current
 * device for NULL). (Additive: no ABI bump.) */
int bx_compute_gae(int64_t n_steps, int64_t n_envs, const bx_seq* reward, const bx_seq* done,
                   const bx_seq* truncation, const bx_seq* values, const float* bootstrap,
                   const bx_seq* vs, const bx_seq* advantages, float reward_scaling,
                   float discount, float lambda, void* stream);

/* The optimiser side of the evolution agents (ES, ARS), the parameter noise
 * regenerated from the counter RNG instead of stored: direction p's noise for
 * parameter j is eps[p, j] = N(seed, offset + 2 (p * n_params + j)), exactly
 * the sample bx_normal_slabs(out, P * n_params, 1, seed, offset, ...) writes
 * at out[p * n_params + j]. No system handle: the launches go to the device
 * that owns `stream` (the current device for NULL). (Additive: no ABI bump.)
 *
 * bx_population_perturb writes the population's rows in one launch:
 *   rows[p * stride + j]                  = (float)((double)theta[j] + sigma * (double)eps[p, j])
 *   rows[(n_directions + p) * stride + j] = (float)((double)theta[j] - sigma * (double)eps[p, j])
 * (the second only when `antithetic`), p < n_directions, j < n_params; the
 * float64 product and the sum are each rounded on their own (no fused
 * multiply-add). The words j >= n_params of a row (stride padding) are not
 * written. `frozen` (NULL: none) is n_params device bytes: where frozen[j] is
 * not 0 every row gets theta[j] itself; the counters of a frozen j are
 * skipped, not reused. Rows whose base and stride are 16-byte aligned are
 * written with 16-byte stores. A null `rows` or `theta`, n_directions < 1,
 * n_params < 1, stride < n_params, more than 2^40 samples, or rows that
 * overlap theta fail. */
int bx_population_perturb(float* rows, const float* theta, int64_t n_directions, int64_t n_params,
                          int64_t stride, double sigma, uint64_t seed, uint64_t offset,
                          int antithetic, const uint8_t* frozen, void* stream);

/* out[j] = (float) sum_{p < n_directions} (double)weights[p] * (double)eps[p, j],
 * `weights` (n_directions,) float32 on the device, the same eps. The sum is
 * float64 in a fixed order that depends on (n_directions, n_params) alone, so
 * it is the same bit for bit from run to run (no floating-point atomics): the
 * directions are split into chunks of BX_POPULATION_DELTA_CHUNK, one
 * workgroup row per chunk, each chunk summed in ascending p, and the chunk
 * partials are summed in ascending chunk order. A direction whose weight is
 * +-0 is skipped (eps is finite, so its term is an exact zero); a NaN or Inf
 * weight makes every non-frozen out[j] non-finite. frozen[j] != 0 gives
 * out[j] = 0.
 *
 * The partials live in the caller's `workspace` (device memory, 8-byte
 * aligned) of *workspace_bytes bytes; the library keeps no scratch of its
 * own. With workspace == NULL the call launches nothing and writes the size
 * it needs to *workspace_bytes: 8 * n_params * ceil(n_directions /
 * BX_POPULATION_DELTA_CHUNK). With a workspace, *workspace_bytes below that
 * size or a misaligned workspace fails. A null `workspace_bytes`, a null
 * `out` or `weights` with a workspace, n_directions < 1, n_params < 1 or more
 * than 2^40 samples fail. */
#define BX_POPULATION_DELTA_CHUNK 64
int bx_population_delta(float* out, const float* weights, int64_t n_directions, int64_t n_params,
                        uint64_t seed, uint64_t offset, const uint8_t* frozen, void* workspace,
                        int64_t* workspace_bytes, void* stream);

/* A batch of rows held as up to BX_FIELDS_MAX separate fp32 arrays: row r of
 * the batch is the concatenation, in field order, of the width[f] floats at
 * ptr[f] + r * row_stride[f] (strides in floats; a field may be a column
 * slice of a wider buffer, row_stride[f] > width[f]). The widths sum to the
 * row's length in words. */
#define BX_FIELDS_MAX 8
typedef struct bx_fields {
  int32_t n_fields;
  float* ptr[BX_FIELDS_MAX];
  int64_t width[BX_FIELDS_MAX];
  int64_t row_stride[BX_FIELDS_MAX];
} bx_fields;

/* The replay queue of the off-policy learner (the reference's
 * `UniformSamplingQueue`, training/replay_buffers.py:92-131, :200-215): a ring
 * `data` of `capacity` rows of `row_words` fp32 words, contiguous. The ring's
 * control numbers (`position`, the next row to write, 0 <= position <
 * capacity, and `size`, the live rows) are the caller's and pass by value. No
 * system handle: the launches go to the device that owns `stream` (the current
 * device for NULL). Both kernels only copy 32-bit words, so NaN payloads and
 * any other bit pattern arrive unchanged. (Additive: no ABI bump.)
 *
 * bx_replay_insert writes batch row r of `src` to ring row (position + r) mod
 * capacity, r < n_rows, in one launch: the ring wraps inside the batch and is
 * never rolled. The caller then advances position by n_rows mod capacity and
 * size to min(size + n_rows, capacity). A null `data` or `src` or field
 * pointer with n_rows > 0, n_fields above BX_FIELDS_MAX, a negative width,
 * widths that do not sum to row_words, a position outside [0, capacity) or
 * n_rows > capacity fail; n_rows = 0 launches nothing. `src` must not overlap
 * `data`. */
int bx_replay_insert(float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t n_rows, const bx_fields* src, void* stream);

/* bx_replay_sample draws n_samples rows uniformly with replacement from the
 * `size` live rows, the oldest of which is ring row (position - size) mod
 * capacity, and scatters sample j into row j of `dst`'s fields, in one launch:
 *   z   = mix(seed, offset + j)            (uint64 arithmetic, wrapping)
 *   k   = (z * size) >> 64                 (the high half of the 128-bit product)
 *   row = (position - size + k) mod capacity
 * with mix the counter RNG's 64-bit splitmix64 finaliser (bx_uniform's bits
 * before their top 24 are taken):
 *   z = seed * 0x9E3779B97F4A7C15 + i + 0x632BE59BD9B4E019
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   z = z ^ (z >> 31)
 * so the rows are a pure function of (seed, offset, position, size,
 * capacity). idx_out (NULL: not wanted) receives the n_samples ring rows as
 * int64. The failures of bx_replay_insert (with `dst` for `src`, n_samples for
 * n_rows, without the n_rows bound), and size < 1 or size > capacity, fail;
 * n_samples = 0 launches nothing. `dst` must not overlap `data`. */
int bx_replay_sample(const float* data, int64_t capacity, int64_t row_words, int64_t position,
                     int64_t size, int64_t n_samples, uint64_t seed, uint64_t offset,
                     const bx_fields* dst, int64_t* idx_out, void* stream);

/* The learners' MLPs (the reference's `networks.MLP`): y = layer_{L-1}(...
 * act(layer_0(x))), layer_l(a) = a . w[l] + b[l], the activation (BX_POLICY_SWISH
 * / RELU / TANH) after every layer but the last. float32; w[l] is (in[l],
 * out[l]) row-major and b[l] is (out[l],), separate device arrays that the
 * kernels only read (an optimiser updates them in place between calls);
 * n_layers 1 .. BX_MLP_MAX_LAYERS, every out[l] 1 .. BX_MLP_MAX_WIDTH, in[0]
 * 1 .. BX_MLP_MAX_IN, in[l] = out[l - 1]. Every product is an f32 MFMA, a
 * k-ordered fmaf chain; NaN and Inf propagate as IEEE has them and a
 * non-finite input row reaches no other row's y or dx. No system handle: the
 * launches go to the device that owns `stream` (the current device for NULL).
 * (Additive: no ABI bump.) */
#define BX_MLP_MAX_LAYERS 8
#define BX_MLP_MAX_WIDTH 256
#define BX_MLP_MAX_IN 1024
typedef struct bx_mlp {
  int32_t n_layers;
  int32_t activation;
  int32_t in[BX_MLP_MAX_LAYERS];
  int32_t out[BX_MLP_MAX_LAYERS];
  const float* w[BX_MLP_MAX_LAYERS];
  const float* b[BX_MLP_MAX_LAYERS];
} bx_mlp;

/* Where bx_mlp_backward writes layer l's gradients, shaped as w[l] and b[l];
 * a null entry switches that gradient off. */
typedef struct bx_mlp_grads {
  float* dw[BX_MLP_MAX_LAYERS];
  float* db[BX_MLP_MAX_LAYERS];
} bx_mlp_grads;

/* sizeof(bx_mlp) and sizeof(bx_mlp_grads) as the library was compiled */
int bx_mlp_sizes(int32_t* mlp_bytes, int32_t* grads_bytes);

/* The whole network in ONE launch, a workgroup per 32 rows, the tile's
 * activations in LDS between layers. x is (rows, in[0]) with row pitch
 * x_stride >= in[0] floats (a column slice of a wider buffer passes as it
 * is); y is (rows, out[n_layers - 1]) contiguous. `saved` (NULL: not wanted)
 * is (rows, H) contiguous, H the sum of the hidden layers' widths out[0 ..
 * n_layers - 2]: every hidden layer's pre-activation, layer l's at column
 * out[0] + .. + out[l - 1], which bx_mlp_backward reads. A null net, x or y
 * (or weight or bias), n_layers, a width or an activation outside the limits
 * above, in[l] != out[l - 1], x_stride < in[0] or rows < 0 fail before any
 * device call; rows = 0 launches nothing. */
int bx_mlp_forward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride, float* y,
                   float* saved, void* stream);

/* The gradients of sum(y * dy) in at most TWO launches. dy is (rows,
 * out[n_layers - 1]) contiguous, x and saved as bx_mlp_forward took and wrote
 * them. Launch (i) runs the reverse chain per 32-row tile: dx (rows, in[0])
 * contiguous when not NULL, and the hidden layers' pre-activation gradients
 * dz into the workspace, (rows, H) as `saved`. Launch (ii) writes every layer's
 * dW = a^T . dz and db = the column sums of dz that `grads` names (NULL: none),
 * one workgroup per (layer, 32 x 64 tile of dW), a recomputed from saved (or x)
 * as it is read. Launch (i) is left out when neither dx nor a hidden layer's
 * gradient is wanted, launch (ii) when no gradient is. No floating-point
 * atomics: each workgroup's 8 waves sum contiguous eighths of the rows in
 * ascending order and the 8 partials are added in wave order, so the bits
 * depend on (rows, shapes, inputs) alone.
 *
 * The workspace is the caller's (device memory, 16-byte aligned) of
 * *workspace_bytes bytes; with workspace == NULL the call launches nothing
 * and writes the size it needs to *workspace_bytes: max(16, 4 * rows * H).
 * The failures of bx_mlp_forward, a null dy or workspace_bytes, a null saved
 * with n_layers > 1, a workspace that is too small or misaligned fail before
 * any device call; rows = 0 launches nothing. */
int bx_mlp_backward(const bx_mlp* net, int64_t rows, const float* x, int64_t x_stride,
                    const float* saved, const float* dy, float* dx, const bx_mlp_grads* grads,
                    void* workspace, int64_t* workspace_bytes, void* stream);

/* The PPO loss head: everything of `compute_ppo_loss` (training/agents/ppo/
 * losses.py:96-182) between the two networks' outputs and the scalar loss,
 * and the loss's gradients in `logits` and `baseline`, in TWO launches.
 * float32. The (T, B) arrays are bx_seq views as bx_compute_gae takes them; a
 * (T, B, W) array is a bx_seq whose element (t, e) is the row of W floats at
 * ptr + t * time_stride + e * env_stride, the row itself with UNIT stride
 * (logits and dlogits: W = 2 A, the A locations then the A scale parameters;
 * raw_action and eps: W = A). bootstrap is (B,) contiguous. With N = T * B:
 *   scale      = softplus(s) + min_std      (softplus(x) = x above 20, else
 *                                            log1p(exp(x)))
 *   det(x)     = 2 (log 2 - x - softplus(-2 x))
 *   lp[t, e]   = sum_a -0.5 z^2 - 0.5 log 2 pi - log scale - det(raw),
 *                z = (raw - loc) / scale
 *   vs, adv    = bx_compute_gae(reward, done, truncation, values = baseline,
 *                bootstrap, reward_scaling, discount, lambda), bit for bit
 *   A^         = normalize_advantage ? (adv - mean) / (std + 1e-8) : adv, the
 *                mean and the population standard deviation over all N
 *   rho        = exp(lp - log_prob)
 *   losses[1]  = -1/N sum min(rho A^, clamp(rho, 1 - clipping_epsilon,
 *                1 + clipping_epsilon) A^)                    (policy)
 *   losses[2]  = 0.25/N sum (vs - baseline)^2                 (v)
 *   losses[3]  = -entropy_cost/N sum sum_a [0.5 + 0.5 log 2 pi + log scale +
 *                det(loc + scale eps)]                        (entropy)
 *   losses[0]  = losses[1] + losses[2] + losses[3]            (total)
 * dlogits (T, B, 2 A) and dbaseline (T, B) are d losses[0] / d logits and
 * / d baseline with vs and adv held constant (the reference stops their
 * gradient, so bootstrap has none): dbaseline = -0.5 (vs - baseline) / N; in
 * rho the surrogate's derivative is A^ times what autograd's minimum and clamp
 * give (1 on the closed clip interval and where the unclipped product is the
 * strictly smaller one, a half where the two products tie outside it, else 0).
 * vs and advantages (NULL, or a null ptr: not wanted) receive the GAE outputs
 * before normalisation. clipping_epsilon is a double so that the interval's
 * ends are (float)(1 -+ clipping_epsilon) as a float32 tensor's clamp has them.
 *
 * Launch 1: a workgroup per 256 envs runs the scan, one lane per env, and
 * writes dbaseline; a workgroup per 256 (t, e) rows sums lp and the entropy
 * over the actions, one lane per row. Launch 2: a workgroup per 256 rows writes
 * dlogits and one more sums the losses. No floating-point atomics: every sum
 * across rows is float64, lane-strided in ascending order and then added over
 * lanes and waves in a fixed tree, workgroup partials in workgroup order, so
 * the bits depend on (T, B, A) and the inputs alone. The standard deviation
 * comes from per-workgroup (count, mean, centred square sum) triples combined
 * pairwise, not from a sum of squares. NaN and Inf propagate as IEEE has
 * them; a non-finite input of env e reaches no other env's dbaseline, vs or
 * advantages (through the mean it reaches every dlogits when normalising).
 *
 * The workspace is the caller's (device memory, 16-byte aligned) of
 * *workspace_bytes bytes; with workspace == NULL the call launches nothing
 * and writes the size it needs to *workspace_bytes: 8 (4 ceil(B / 256) +
 * ceil(N / 256)) + 8 N, rounded up to 16. The outputs may have any layout (but
 * unit stride along a row) and must not overlap the inputs, the workspace or
 * each other. A null workspace_bytes, n_steps < 1, n_actions < 1, n_envs < 0,
 * more than 2^31 rows or 2^20 actions, a null pointer, a zero stride on an
 * output, a workspace that is too small or misaligned fail before any device
 * call; n_envs = 0 launches nothing. No system handle: the launches go to the
 * device that owns `stream` (the current device for NULL). (Additive: no ABI
 * bump.) */
int bx_ppo_head(int64_t n_steps, int64_t n_envs, int64_t n_actions, const bx_seq* logits,
                const bx_seq* baseline, const float* bootstrap, const bx_seq* raw_action,
                const bx_seq* eps, const bx_seq* log_prob, const bx_seq* reward,
                const bx_seq* done, const bx_seq* truncation, float reward_scaling,
                float discount, float lambda, double clipping_epsilon, float entropy_cost,
                float min_std, int normalize_advantage, float* losses, const bx_seq* dlogits,
                const bx_seq* dbaseline, const bx_seq* vs, const bx_seq* advantages,
                void* workspace, int64_t* workspace_bytes, void* stream);

/*
 * The fused optimiser step: torch.optim.Adam's update (its default path: no
 * weight decay, no amsgrad, not maximising) of up to BX_OPT_MAX_TENSORS
 * float32 tensors, and the soft update of a target copy of those that have
 * one, in ONE launch on `stream`. Tensor k is n contiguous floats at each of
 * p (the parameter), g (its gradient, read only), m and v (the first and
 * second moments); the arrays of the table must not overlap.
 *
 * `step` >= 1 is the step count AFTER this step, as torch has it. The betas
 * are doubles because 1 - beta is formed from them: 1 - (float)0.999 is off
 * 0.001 by 1.3e-5 of it, a hundred float32 ulps of every v. The host forms, in
 * double, narrowed to float32 once:
 *   w1      = (float)(1 - beta1)         w2 = (float)(1 - beta2)
 *   b2      = (float)beta2
 *   c2      = (float)sqrt(1 - beta2^step)
 *   s_k     = (float)(lr_k / (1 - beta1^step))
 *   u_k     = (float)(1 - tau_k)
 * and the kernel does, per element, every operation rounded to float32 on its
 * own (no contraction, no pow, IEEE division and square root):
 *   m      = m + (g - m) * w1
 *   v      = v * b2 + (g * g) * w2
 *   denom  = sqrt(v) / c2 + eps
 *   p      = p - s_k * (m / denom)
 * and then, where target != NULL, in the same lane on the same element
 *   target = target * u_k + p * tau_k        (p the value just written)
 * which are the bits of `t * (1 - tau) + q * tau` as three float32 tensor
 * operations. NaN and Inf propagate as IEEE has them; the step is elementwise,
 * so a non-finite gradient element reaches no other element.
 *
 * A workgroup of 256 lanes owns 1024 consecutive elements of one tensor; the
 * table and the prefix sums of the tensors' workgroup counts travel in the
 * kernel's arguments, so a call allocates nothing, copies nothing, does not
 * synchronise, may be captured into a graph, and may name other gradient
 * pointers on every call. (`step` is a host value: a captured call replays
 * that step's bias corrections.) A tensor whose p, g, m, v and target are all
 * 16-byte aligned moves in 16-byte accesses, any other a float at a time with
 * the same results; no lane touches an element at or past n.
 *
 * A null table, n_tensors outside 1..BX_OPT_MAX_TENSORS, step < 1, a negative
 * n, a null p, g, m or v on a tensor with n > 0, a beta outside [0, 1) (NaN
 * included), eps < 0 (or NaN), or more than 2^31 - 1 workgroups fail before
 * any device call. Tensors with n = 0 are skipped and a table of only such
 * tensors launches nothing. No system handle: the launch goes to the device
 * that owns `stream` (the current device for NULL). bx_opt_sizes writes
 * sizeof(bx_opt_tensor) as compiled. (Additive: no ABI bump.) */
#define BX_OPT_MAX_TENSORS 32
typedef struct bx_opt_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;      /* n floats each */
  float* target; /* NULL: no target update */
  int64_t n;
  float lr;
  float tau;
} bx_opt_tensor;
int bx_opt_sizes(int32_t* tensor_bytes);
int bx_adam_step(const bx_opt_tensor* t, int32_t n_tensors, int64_t step, double beta1,
                 double beta2, float eps, void* stream);

/*
 * The SAC loss heads: what a SAC gradient step computes between its network
 * evaluations (brax_amd/training/sac_losses.py), in FOUR launches on `stream`,
 * one per entry point, called in this order around the networks. B rows, O
 * observations, A actions, C critics; everything float32; a `pitch` is a
 * row's stride in elements (the row itself has unit stride).
 *
 * bx_sac_head_prep writes the critics' three inputs (B, O + A) at one pitch:
 *   x_cur  = [n(obs) | action]     x_next = [n(next_obs) | .]
 *   x_pi   = [n(obs) | .]          n(o) = (o - mean) / std, two float32
 *                                  operations; mean = std = NULL: n(o) = o
 * The action columns of x_next and x_pi are not written (bx_sac_head_sample
 * fills them). mean and std are (O,).
 *
 * bx_sac_head_sample runs n_jobs (1..BX_SAC_MAX_JOBS) samples in one launch.
 * Per job, logits (B, 2 A) = [loc | s], eps (B, A):
 *   scale      = softplus(s) + min_std     (softplus(x) = x above 20, else
 *                                           log1p(exp(x)))
 *   raw        = loc + scale eps
 *   action     = tanh(raw)                 (B, A); NULL: not wanted
 *   log_prob   = sum_a -0.5 z^2 - 0.5 log 2 pi - log scale - det(raw),
 *                z = (raw - loc) / scale, det(x) = 2 (log 2 - x - softplus(-2 x))
 *
 * bx_sac_head_losses reads the three jobs' log-probs (B,) and the critics'
 * outputs, C separate contiguous (B,) arrays each (bx_sac_q): q_old =
 * Q(x_cur), next_q = Qtarget(x_next), q_pi = Q(x_pi); reward, discount and
 * truncation (B,) with an element stride; log_alpha on the device. With alpha
 * = exp(*log_alpha):
 *   y_b        = reward_b reward_scaling + discount_b discounting
 *                (min_c next_q_cb - alpha lp_next_b)
 *   e_bc       = (q_old_cb - y_b) (1 - truncation_b)
 *   dq_old_cb  = e_bc (1 - truncation_b) / (B C)
 *   dq_pi_cb   = -1/B at the minimal q_pi_cb (the lowest c of a tie), else 0
 *   g_lp_b     = alpha / B
 * and leaves each workgroup's sums of e^2, of alpha lp_pi - min_c q_pi and of
 * alpha (-lp_alpha - target_entropy) in the workspace as doubles.
 *
 * bx_sac_head_sample_backward is the actor sample's backward pass, with g =
 * g_lp and da = the sum over c, in the order of c, of the C arrays da->ptr[c]
 * (B, A) (the action columns of each critic's input gradient):
 *   u = g 2 tanh(raw) + da (1 - tanh(raw)^2)
 *   dlogits = [u | (u eps - g / scale) sigmoid(s)]            (B, 2 A)
 * One more workgroup sums the workspace's partials (the SAME workspace the
 * losses call of this step wrote) into
 *   losses[0] = 0.5/(B C) sum e^2                              (critic)
 *   losses[1] = 1/B sum (alpha lp_pi - min_c q_pi)             (actor)
 *   losses[2] = 1/B sum alpha (-lp_alpha - target_entropy)     (alpha)
 * and *dlog_alpha = losses[2], the alpha loss's derivative in log_alpha.
 *
 * No floating-point atomics: every sum across rows is float64, added over the
 * lanes and waves of a workgroup in a fixed tree and over the workgroups'
 * partials lane-strided in ascending order, so the bits depend on (B, A, C)
 * and the inputs alone. alpha is never read on the host, so a step can be
 * captured. NaN and Inf propagate as IEEE has them; a non-finite input of row
 * b reaches no other row's outputs (and the losses it is summed into).
 *
 * The workspace is the caller's (device memory, 16-byte aligned) of
 * *workspace_bytes bytes; with workspace == NULL the call launches nothing
 * and writes the size it needs to *workspace_bytes: 24 ceil(B / 256), rounded
 * up to 16. Outputs must not overlap the inputs, the workspace or each other.
 * A null workspace_bytes, n_rows < 0 or above 2^31, n_obs < 1, n_actions < 1
 * or above 2^20, n_jobs outside 1..BX_SAC_MAX_JOBS, n_critics outside
 * 1..BX_SAC_MAX_CRITICS, a null required pointer, one of mean and std alone, a
 * pitch below its row's width, a workspace that is too small or misaligned
 * fail before any device call; n_rows = 0 launches nothing. No system handle:
 * the launches go to the device that owns `stream` (the current device for
 * NULL). (Additive: no ABI bump.) */
#define BX_SAC_MAX_CRITICS 4
#define BX_SAC_MAX_JOBS 3
typedef struct bx_sac_sample_job {
  const float* logits;
  int64_t logits_pitch;
  const float* eps;
  int64_t eps_pitch;
  float* action; /* NULL: not wanted */
  int64_t action_pitch;
  float* log_prob;
} bx_sac_sample_job;
typedef struct bx_sac_q {
  const float* q_old[BX_SAC_MAX_CRITICS];
  const float* next_q[BX_SAC_MAX_CRITICS];
  const float* q_pi[BX_SAC_MAX_CRITICS];
  float* dq_old[BX_SAC_MAX_CRITICS];
  float* dq_pi[BX_SAC_MAX_CRITICS];
} bx_sac_q;
typedef struct bx_sac_daction {
  const float* ptr[BX_SAC_MAX_CRITICS];
  int64_t pitch[BX_SAC_MAX_CRITICS];
} bx_sac_daction;
int bx_sac_head_prep(int64_t n_rows, int64_t n_obs, int64_t n_actions, const float* obs,
                     int64_t obs_pitch, const float* next_obs, int64_t next_obs_pitch,
                     const float* action, int64_t action_pitch, const float* mean,
                     const float* std, float* x_cur, float* x_next, float* x_pi, int64_t x_pitch,
                     void* stream);
int bx_sac_head_sample(int64_t n_rows, int64_t n_actions, const bx_sac_sample_job* jobs,
                       int32_t n_jobs, float min_std, void* stream);
int bx_sac_head_losses(int64_t n_rows, int32_t n_critics, const float* lp_alpha,
                       const float* lp_next, const float* lp_pi, const bx_sac_q* q,
                       const float* reward, int64_t reward_stride, const float* discount,
                       int64_t discount_stride, const float* truncation,
                       int64_t truncation_stride, const float* log_alpha, float reward_scaling,
                       float discounting, float target_entropy, float* g_lp, void* workspace,
                       int64_t* workspace_bytes, void* stream);
int bx_sac_head_sample_backward(int64_t n_rows, int64_t n_actions, int32_t n_critics,
                                const float* logits, int64_t logits_pitch, const float* eps,
                                int64_t eps_pitch, const float* g_lp, const bx_sac_daction* da,
                                float min_std, float* dlogits, int64_t dlogits_pitch,
                                float* losses, float* dlog_alpha, void* workspace,
                                int64_t* workspace_bytes, void* stream);

/*
 * Standalone HBM-streaming phase kernels over a structure-of-arrays batch
 * (the integrator and collider phases benchmarked in isolation).
 * SoA: field plane k, body b, env e at base[k*plane + b*n_envs + e]; the 13
 * state planes are pos xyz, rot wxyz, vel xyz, ang xyz. n_envs % 4 == 0,
 * planes 16-byte aligned.
 *   which 0: Euler.kinetic              (integrators.py:50-68)   in -> out pos, rot
 *   which 1: Euler.update(acc_p=aux)    (integrators.py:85-93)   aux = dp vel 3 + ang 3 planes
 *   which 2: Euler.velocity_projection  (integrators.py:122-146) aux = previous state planes
 */
int bx_phase(bx_system* sys, int which, int64_t n_envs, int64_t plane, const float* in,
             float* out, const float* aux, int64_t aux_plane, void* stream);

/* capsule_plane contacts (colliders.py:744-759) of every capsule-plane row:
 * out planes pos xyz, vel xyz, normal xyz, penetration, each (R, n_envs). */
int bx_phase_capsule_plane(bx_system* sys, int64_t n_envs, int64_t plane, const float* in,
                           float* out, int64_t out_plane, void* stream);

/* Diagnostic builds only (-DBX_STAMPS): per-phase s_memtime cycle sums of the
 * single-mode step, [0..9] phases, [15] samples; with reset bit 1 set, the
 * MULTI-mode step's (-DBX_MSTAMPS), [0..10]; with bit 2 set (single-mode),
 * the per-workgroup sums, 4096 x 16 entries. Fails on product builds. */
int bx_debug_stamps(unsigned long long* out16, int reset);

/* The revolute joint halves' partner exchange on its own (diagnostic): one
 * wavefront writes out64[l] = the value lane l receives from its partner lane
 * (l ^ 8 within each env of `lanes` = 16 threads) when every lane offers its
 * own index. */
int bx_debug_partner(float* out64, int lanes, void* stream);

/* Multi-rank episodic exchange is done over RCCL by the host (torch.distributed);
 * no collective lives in this library. */

#ifdef __cplusplus
}
#endif
#endif /* BRAX_AMD_H_ */
