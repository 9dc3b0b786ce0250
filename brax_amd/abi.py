"""ctypes mirror of `include/brax_amd.h` (structs only, no library loading).

`make_desc` / `make_reset_desc` turn the compiler's numpy descriptor into the
C structs; the returned keep-alive list must outlive every call that reads the
struct (create copies it to the device, so only the create call needs it).
"""
import ctypes as C

import numpy as np

i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)
f32p = C.POINTER(C.c_float)

ABI_VERSION = 14  # include/brax_amd.h BX_ABI_VERSION

_DESC_FIELDS = [
    ('n_bodies', C.c_int32), ('n_joints', C.c_int32), ('n_actuators', C.c_int32),
    ('n_rows', C.c_int32), ('n_groups', C.c_int32),
    ('substeps', C.c_int32), ('action_size', C.c_int32), ('num_joint_dof', C.c_int32),
    ('dt', C.c_double), ('h', C.c_double), ('gravity', C.c_double * 3),
    ('velocity_damping', C.c_double), ('angular_damping', C.c_double),
    ('body_mass', f64p), ('body_inv_inertia', f64p), ('pos_mask', f64p),
    ('rot_mask', f64p), ('quat_mask', f64p),
    ('joint_type', i32p), ('joint_dof', i32p), ('joint_free_dofs', i32p),
    ('joint_body_p', i32p), ('joint_body_c', i32p), ('joint_group', i32p),
    ('joint_off_p', f64p), ('joint_off_c', f64p), ('joint_axis_p', f64p),
    ('joint_axis_c', f64p), ('joint_limit', f64p), ('joint_damping', f64p),
    ('joint_scale_pos', f64p), ('joint_scale_ang', f64p),
    ('act_type', i32p), ('act_joint', i32p), ('act_index', i32p),
    ('act_group', i32p), ('act_strength', f64p),
    ('col_oneway', i32p), ('col_fn', i32p), ('col_scale', f64p),
    ('col_velocity_threshold', f64p), ('col_baumgarte_erp', f64p),
    ('row_group', i32p), ('row_body_a', i32p), ('row_body_b', i32p),
    ('row_a_pos', f64p), ('row_a_end', f64p), ('row_a_radius', f64p),
    ('row_b_pos', f64p), ('row_b_end', f64p), ('row_b_radius', f64p),
    ('row_friction', f64p), ('row_elasticity', f64p),
    ('n_forces', C.c_int32), ('force_type', i32p), ('force_body', i32p),
    ('force_index', i32p), ('force_strength', f64p),
    ('col_cutoff', i32p), ('row_flat', i32p),
    ('dynamics_mode', C.c_int32), ('joint_stiffness', f64p),
    ('joint_spring_damping', f64p), ('joint_limit_strength', f64p),
    ('row_ext', f64p), ('row_hm', i32p), ('n_hm', C.c_int32), ('hm_data', f64p),
    ('n_hull', C.c_int32), ('hull_vert', f64p), ('hull_face', f64p), ('hull_norm', f64p),
    ('row_nn_masked', i32p),
]

DYN_PBD, DYN_LEGACY_SPRING = 0, 1
OBS_XY = 1  # BX_OBS_XY: exclude_current_positions_from_observation=False
_SPRING_FIELDS = ('joint_stiffness', 'joint_spring_damping', 'joint_limit_strength')


class BxDesc(C.Structure):
  _fields_ = _DESC_FIELDS


class BxResetDesc(C.Structure):
  _fields_ = [
      ('n_fk', C.c_int32), ('fk_body_p', i32p), ('fk_body_c', i32p),
      ('fk_dof_index', i32p), ('fk_rot', f64p), ('fk_ref', f64p),
      ('fk_off_p', f64p), ('fk_off_c', f64p), ('base_qp', f64p),
      ('n_zpts', C.c_int32), ('zpt_body', i32p), ('zpt_local', f64p),
      ('zpt_radius', f64p), ('body_zero_cand', i32p), ('body_root_group', i32p),
      ('n_root_groups', C.c_int32), ('default_angle', f64p),
  ]


class BxField(C.Structure):
  _fields_ = [('ptr', C.c_void_p), ('env_stride', C.c_int64),
              ('body_stride', C.c_int64)]


class BxQP(C.Structure):
  _fields_ = [('pos', BxField), ('rot', BxField), ('vel', BxField),
              ('ang', BxField)]


class BxInfo(C.Structure):
  _fields_ = [('contact_vel', BxField), ('contact_ang', BxField),
              ('actuator_vel', BxField), ('actuator_ang', BxField),
              ('contact_pos', C.c_void_p), ('contact_normal', C.c_void_p),
              ('contact_penetration', C.c_void_p),
              ('joint_vel', BxField), ('joint_ang', BxField),
              ('contact_cell', C.c_void_p)]


class BxEnvState(C.Structure):
  _fields_ = [('qp', BxQP), ('obs', C.c_void_p), ('reward', C.c_void_p),
              ('done', C.c_void_p), ('metrics', C.c_void_p),
              ('steps', C.c_void_p), ('truncation', C.c_void_p), ('rng', C.c_void_p)]


class BxEnvParams(C.Structure):
  _fields_ = [('kind', C.c_int32), ('obs_size', C.c_int32),
              ('n_metrics', C.c_int32), ('episode_length', C.c_int32),
              ('action_repeat', C.c_int32), ('auto_reset', C.c_int32),
              ('obs_flags', C.c_int32), ('coef', C.c_float * 8),
              ('first_qp', BxQP), ('first_obs', C.c_void_p), ('act_map', C.c_void_p)]


POLICY_MAX_LAYERS, POLICY_MAX_WIDTH, POLICY_MAX_OBS = 8, 128, 512  # BX_POLICY_MAX_*
POLICY_ACTIVATIONS = {'swish': 0, 'relu': 1, 'tanh': 2}  # BX_POLICY_SWISH / RELU / TANH


class BxPolicy(C.Structure):
  _fields_ = [('params', C.c_void_p), ('n_layers', C.c_int32),
              ('width', C.c_int32 * POLICY_MAX_LAYERS), ('activation', C.c_int32),
              ('obs_mean', C.c_void_p), ('obs_std', C.c_void_p), ('min_std', C.c_float),
              ('deterministic', C.c_int32), ('action_size', C.c_int32)]


# The evaluation entry points, argument by argument in the header's order
# (name, ctypes type); `eval_in` / `eval_out` are (M + 3, B) float32: the M
# metric sums in the env's metric order, the reward sum, active_episodes,
# episode_steps.
_vp = C.c_void_p
EVAL_POLICY_ARGS = (
    ('sys', _vp), ('env', C.POINTER(BxEnvParams)), ('n_envs', C.c_int64), ('n_steps', C.c_int32),
    ('qp_in', _vp), ('obs_in', _vp), ('done_in', _vp), ('steps_in', _vp), ('rng_in', _vp),
    ('policy', C.POINTER(BxPolicy)), ('seed', C.c_uint64), ('offset', C.c_uint64),
    ('step_stride', C.c_uint64), ('eval_in', _vp), ('out', _vp), ('eval_out', _vp),
    ('rng_out', _vp), ('stream', _vp))
EVAL_PACKED_ARGS = (
    ('sys', _vp), ('env', C.POINTER(BxEnvParams)), ('n_envs', C.c_int64), ('n_steps', C.c_int32),
    ('qp_in', _vp), ('done_in', _vp), ('steps_in', _vp), ('rng_in', _vp), ('act', _vp),
    ('act_stride', C.c_int64), ('act_step_stride', C.c_int64), ('act_width', C.c_int64),
    ('eval_in', _vp), ('out', _vp), ('eval_out', _vp), ('rng_out', _vp), ('stream', _vp))

HEADS = {'normal_tanh': 0, 'identity': 1}  # BX_HEAD_NORMAL_TANH / BX_HEAD_IDENTITY
POP_NO_STAGE = 1  # BX_POP_NO_STAGE


class BxPopulation(C.Structure):
  _fields_ = [('param_stride', C.c_int64), ('head', C.c_int32), ('reward_shift', C.c_float),
              ('mom_in', C.c_void_p), ('mom_out', C.c_void_p), ('flags', C.c_int32),
              ('staged', C.c_int32), ('lds_bytes', C.c_int32)]


# bx_env_eval_population: bx_env_eval_policy's arguments, then the population
# struct before the stream
EVAL_POPULATION_ARGS = EVAL_POLICY_ARGS[:-1] + (('pop', C.POINTER(BxPopulation)), ('stream', _vp))


class BxSeq(C.Structure):
  """One float32 (T, B) array: element (t, e) at ptr[t * time_stride + e *
  env_stride], strides in elements."""
  _fields_ = [('ptr', C.c_void_p), ('time_stride', C.c_int64), ('env_stride', C.c_int64)]


_seq = C.POINTER(BxSeq)
COMPUTE_GAE_ARGS = (
    ('n_steps', C.c_int64), ('n_envs', C.c_int64), ('reward', _seq), ('done', _seq),
    ('truncation', _seq), ('values', _seq), ('bootstrap', _vp), ('vs', _seq),
    ('advantages', _seq), ('reward_scaling', C.c_float), ('discount', C.c_float),
    ('lambda', C.c_float), ('stream', _vp))
POPULATION_DELTA_CHUNK = 64  # BX_POPULATION_DELTA_CHUNK
POPULATION_PERTURB_ARGS = (
    ('rows', _vp), ('theta', _vp), ('n_directions', C.c_int64), ('n_params', C.c_int64),
    ('stride', C.c_int64), ('sigma', C.c_double), ('seed', C.c_uint64), ('offset', C.c_uint64),
    ('antithetic', C.c_int), ('frozen', _vp), ('stream', _vp))
POPULATION_DELTA_ARGS = (
    ('out', _vp), ('weights', _vp), ('n_directions', C.c_int64), ('n_params', C.c_int64),
    ('seed', C.c_uint64), ('offset', C.c_uint64), ('frozen', _vp), ('workspace', _vp),
    ('workspace_bytes', C.POINTER(C.c_int64)), ('stream', _vp))
FIELDS_MAX = 8  # BX_FIELDS_MAX


class BxFields(C.Structure):
  """A batch of rows held as up to FIELDS_MAX float32 arrays: row r is the
  concatenation of the width[f] floats at ptr[f] + r * row_stride[f]."""
  _fields_ = [('n_fields', C.c_int32), ('ptr', C.c_void_p * FIELDS_MAX),
              ('width', C.c_int64 * FIELDS_MAX), ('row_stride', C.c_int64 * FIELDS_MAX)]


_fields = C.POINTER(BxFields)
REPLAY_INSERT_ARGS = (
    ('data', _vp), ('capacity', C.c_int64), ('row_words', C.c_int64), ('position', C.c_int64),
    ('n_rows', C.c_int64), ('src', _fields), ('stream', _vp))
REPLAY_SAMPLE_ARGS = (
    ('data', _vp), ('capacity', C.c_int64), ('row_words', C.c_int64), ('position', C.c_int64),
    ('size', C.c_int64), ('n_samples', C.c_int64), ('seed', C.c_uint64), ('offset', C.c_uint64),
    ('dst', _fields), ('idx_out', _vp), ('stream', _vp))
MLP_MAX_LAYERS, MLP_MAX_WIDTH, MLP_MAX_IN = 8, 256, 1024  # BX_MLP_MAX_*


class BxMlp(C.Structure):
  """One MLP for bx_mlp_forward / bx_mlp_backward: w[l] is (in[l], out[l])
  row-major float32, b[l] is (out[l],); the activation is a
  POLICY_ACTIVATIONS code."""
  _fields_ = [('n_layers', C.c_int32), ('activation', C.c_int32),
              ('in', C.c_int32 * MLP_MAX_LAYERS), ('out', C.c_int32 * MLP_MAX_LAYERS),
              ('w', C.c_void_p * MLP_MAX_LAYERS), ('b', C.c_void_p * MLP_MAX_LAYERS)]


class BxMlpGrads(C.Structure):
  """Where bx_mlp_backward writes each layer's gradients; None switches one off."""
  _fields_ = [('dw', C.c_void_p * MLP_MAX_LAYERS), ('db', C.c_void_p * MLP_MAX_LAYERS)]


_mlp = C.POINTER(BxMlp)
MLP_SIZES_ARGS = (('mlp_bytes', C.POINTER(C.c_int32)), ('grads_bytes', C.POINTER(C.c_int32)))
MLP_FORWARD_ARGS = (
    ('net', _mlp), ('rows', C.c_int64), ('x', _vp), ('x_stride', C.c_int64), ('y', _vp),
    ('saved', _vp), ('stream', _vp))
MLP_BACKWARD_ARGS = (
    ('net', _mlp), ('rows', C.c_int64), ('x', _vp), ('x_stride', C.c_int64), ('saved', _vp),
    ('dy', _vp), ('dx', _vp), ('grads', C.POINTER(BxMlpGrads)), ('workspace', _vp),
    ('workspace_bytes', C.POINTER(C.c_int64)), ('stream', _vp))
# bx_ppo_head: the (T, B, W) arrays are BxSeq with unit stride along a row
PPO_HEAD_BLOCK = 256  # envs of a scan workgroup, rows of a row workgroup
PPO_HEAD_ARGS = (
    ('n_steps', C.c_int64), ('n_envs', C.c_int64), ('n_actions', C.c_int64), ('logits', _seq),
    ('baseline', _seq), ('bootstrap', _vp), ('raw_action', _seq), ('eps', _seq),
    ('log_prob', _seq), ('reward', _seq), ('done', _seq), ('truncation', _seq),
    ('reward_scaling', C.c_float), ('discount', C.c_float), ('lambda', C.c_float),
    ('clipping_epsilon', C.c_double), ('entropy_cost', C.c_float), ('min_std', C.c_float),
    ('normalize_advantage', C.c_int), ('losses', _vp), ('dlogits', _seq), ('dbaseline', _seq),
    ('vs', _seq), ('advantages', _seq), ('workspace', _vp),
    ('workspace_bytes', C.POINTER(C.c_int64)), ('stream', _vp))
# bx_sac_head_*: the SAC loss heads, one entry point per launch
SAC_MAX_CRITICS, SAC_MAX_JOBS = 4, 3  # BX_SAC_MAX_CRITICS / BX_SAC_MAX_JOBS
SAC_HEAD_BLOCK = 256  # rows of a workgroup
SAC_HEAD_PART = 3  # doubles a workgroup of the losses launch leaves


class BxSacSampleJob(C.Structure):
  """One sample of bx_sac_head_sample: logits (B, 2A) and eps (B, A) in, action
  (B, A) (None: not wanted) and log_prob (B,) out; pitches in elements."""
  _fields_ = [('logits', C.c_void_p), ('logits_pitch', C.c_int64), ('eps', C.c_void_p),
              ('eps_pitch', C.c_int64), ('action', C.c_void_p), ('action_pitch', C.c_int64),
              ('log_prob', C.c_void_p)]


class BxSacQ(C.Structure):
  """The critics' outputs and their gradients for bx_sac_head_losses: C
  contiguous (B,) arrays each."""
  _fields_ = [(n, C.c_void_p * SAC_MAX_CRITICS)
              for n in ('q_old', 'next_q', 'q_pi', 'dq_old', 'dq_pi')]


class BxSacDaction(C.Structure):
  """The action columns of each critic's input gradient, (B, A) at a pitch."""
  _fields_ = [('ptr', C.c_void_p * SAC_MAX_CRITICS), ('pitch', C.c_int64 * SAC_MAX_CRITICS)]


SAC_HEAD_PREP_ARGS = (
    ('n_rows', C.c_int64), ('n_obs', C.c_int64), ('n_actions', C.c_int64), ('obs', _vp),
    ('obs_pitch', C.c_int64), ('next_obs', _vp), ('next_obs_pitch', C.c_int64), ('action', _vp),
    ('action_pitch', C.c_int64), ('mean', _vp), ('std', _vp), ('x_cur', _vp), ('x_next', _vp),
    ('x_pi', _vp), ('x_pitch', C.c_int64), ('stream', _vp))
SAC_HEAD_SAMPLE_ARGS = (
    ('n_rows', C.c_int64), ('n_actions', C.c_int64), ('jobs', C.POINTER(BxSacSampleJob)),
    ('n_jobs', C.c_int32), ('min_std', C.c_float), ('stream', _vp))
SAC_HEAD_LOSSES_ARGS = (
    ('n_rows', C.c_int64), ('n_critics', C.c_int32), ('lp_alpha', _vp), ('lp_next', _vp),
    ('lp_pi', _vp), ('q', C.POINTER(BxSacQ)), ('reward', _vp), ('reward_stride', C.c_int64),
    ('discount', _vp), ('discount_stride', C.c_int64), ('truncation', _vp),
    ('truncation_stride', C.c_int64), ('log_alpha', _vp), ('reward_scaling', C.c_float),
    ('discounting', C.c_float), ('target_entropy', C.c_float), ('g_lp', _vp), ('workspace', _vp),
    ('workspace_bytes', C.POINTER(C.c_int64)), ('stream', _vp))
SAC_HEAD_SAMPLE_BACKWARD_ARGS = (
    ('n_rows', C.c_int64), ('n_actions', C.c_int64), ('n_critics', C.c_int32), ('logits', _vp),
    ('logits_pitch', C.c_int64), ('eps', _vp), ('eps_pitch', C.c_int64), ('g_lp', _vp),
    ('da', C.POINTER(BxSacDaction)), ('min_std', C.c_float), ('dlogits', _vp),
    ('dlogits_pitch', C.c_int64), ('losses', _vp), ('dlog_alpha', _vp), ('workspace', _vp),
    ('workspace_bytes', C.POINTER(C.c_int64)), ('stream', _vp))
OPT_MAX_TENSORS = 32  # BX_OPT_MAX_TENSORS
OPT_CHUNK = 1024  # elements of one tensor that one workgroup of bx_adam_step owns


class BxOptTensor(C.Structure):
  """One tensor of bx_adam_step's table: n contiguous float32 at each of p, g,
  m, v (and target, None for no target update)."""
  _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p),
              ('target', C.c_void_p), ('n', C.c_int64), ('lr', C.c_float), ('tau', C.c_float)]


OPT_SIZES_ARGS = (('tensor_bytes', C.POINTER(C.c_int32)),)
ADAM_STEP_ARGS = (
    ('t', C.POINTER(BxOptTensor)), ('n_tensors', C.c_int32), ('step', C.c_int64),
    ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_float), ('stream', _vp))
PLAN_FIELDS = ('mode', 'lanes', 'lds_bytes', 'feat', 'gw', 'fold', 'jb', 'cb')  # bx_system_blob
SYSTEM_BLOB_ARGS = (
    ('desc', _vp), ('reset', _vp), ('words', C.POINTER(C.c_uint32)), ('capacity', C.c_int64),
    ('n_words', C.POINTER(C.c_int64)), ('plan', C.POINTER(C.c_int32)))
ARGS = {'bx_system_blob': SYSTEM_BLOB_ARGS,
        'bx_env_eval_policy': EVAL_POLICY_ARGS, 'bx_env_eval_packed': EVAL_PACKED_ARGS,
        'bx_env_eval_population': EVAL_POPULATION_ARGS, 'bx_compute_gae': COMPUTE_GAE_ARGS,
        'bx_population_perturb': POPULATION_PERTURB_ARGS,
        'bx_population_delta': POPULATION_DELTA_ARGS,
        'bx_replay_insert': REPLAY_INSERT_ARGS, 'bx_replay_sample': REPLAY_SAMPLE_ARGS,
        'bx_mlp_sizes': MLP_SIZES_ARGS, 'bx_mlp_forward': MLP_FORWARD_ARGS,
        'bx_mlp_backward': MLP_BACKWARD_ARGS, 'bx_ppo_head': PPO_HEAD_ARGS,
        'bx_sac_head_prep': SAC_HEAD_PREP_ARGS, 'bx_sac_head_sample': SAC_HEAD_SAMPLE_ARGS,
        'bx_sac_head_losses': SAC_HEAD_LOSSES_ARGS,
        'bx_sac_head_sample_backward': SAC_HEAD_SAMPLE_BACKWARD_ARGS,
        'bx_opt_sizes': OPT_SIZES_ARGS, 'bx_adam_step': ADAM_STEP_ARGS}
SIGNATURES = {name: ([t for _, t in args], C.c_int) for name, args in ARGS.items()}


def _arr(x, dtype):
  a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
  if a.size == 0:
    a = np.zeros(1, dtype)
  return a


def make_desc(d):
  """numpy descriptor dict -> (BxDesc, keepalive)."""
  keep = []
  s = BxDesc()
  s.n_bodies = int(d['n_bodies'])
  s.n_joints = len(d['joint_type'])
  s.n_actuators = len(d['act_type'])
  s.n_rows = len(d['row_group'])
  s.n_groups = len(d['col_oneway'])
  s.n_forces = len(d.get('force_type', ()))
  s.substeps = int(d['substeps'])
  s.action_size = int(d.get('action_size', 0))
  s.num_joint_dof = int(d.get('num_joint_dof', 0))
  s.dt = float(d['dt'])
  s.h = float(d['h'])
  for k in range(3):
    s.gravity[k] = float(d['gravity'][k])
  s.velocity_damping = float(d['velocity_damping'])
  s.angular_damping = float(d['angular_damping'])
  s.dynamics_mode = int(d.get('dynamics_mode', DYN_PBD))
  s.n_hm = len(d.get('hm_data', ()))
  s.n_hull = len(d.get('hull_vert', ()))
  for name, ctype in _DESC_FIELDS:
    if ctype is i32p or ctype is f64p:
      if name in d:
        v = d[name]
      elif name == 'col_cutoff':
        v = np.zeros(len(d['col_oneway']))
      elif name == 'row_flat':
        v = -np.ones(len(d['row_group']))
      elif name == 'row_nn_masked':
        v = np.zeros(len(d['row_group']))
      elif name.startswith('force_'):
        v = np.zeros(0)
      elif name in _SPRING_FIELDS:
        v = np.zeros(len(d['joint_type']))
      elif name == 'row_ext':
        v = np.zeros((len(d['row_group']), 16))
      elif name == 'row_hm':
        v = np.tile([-1, 0], (len(d['row_group']), 1))
      elif name in ('hm_data', 'hull_vert', 'hull_face', 'hull_norm'):
        v = np.zeros(0)
      else:
        raise KeyError(name)
      a = _arr(v, np.int32 if ctype is i32p else np.float64)
      keep.append(a)
      setattr(s, name, a.ctypes.data_as(ctype))
  return s, keep


def info_rows(d):
  """Contact rows of `Info` (`_get_contact_info`, system.py:36-43): every row
  of a Pairs group, `cutoff` rows of a NearNeighbors group."""
  groups = np.asarray(d['row_group'])
  cut = np.asarray(d.get('col_cutoff', np.zeros(len(d['col_oneway']))))
  return int(sum(int(c) if c else int((groups == g).sum()) for g, c in enumerate(cut)))


def make_reset_desc(r, num_joint_dof=None):
  """Reset descriptor -> (BxResetDesc, keepalive). default_angle is padded
  with zeros to num_joint_dof (the kernels' joint-angle stride)."""
  keep = []
  r = dict(r)
  da = np.asarray(r.get('default_angle', np.zeros(0)), np.float64)
  n = len(da) if num_joint_dof is None else int(num_joint_dof)
  r['default_angle'] = np.pad(da, (0, max(n - len(da), 0)))[:max(n, len(da))]
  s = BxResetDesc()
  s.n_fk = len(r['fk_body_p'])
  s.n_zpts = len(r['zpt_body'])
  s.n_root_groups = int(r['n_root_groups'])
  for name, ctype in BxResetDesc._fields_:
    if ctype is i32p or ctype is f64p:
      a = _arr(r[name], np.int32 if ctype is i32p else np.float64)
      keep.append(a)
      setattr(s, name, a.ctypes.data_as(ctype))
  return s, keep
