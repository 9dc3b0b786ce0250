"""ctypes mirror of `include/brax_amd.h`: its structs, its constants and every
entry point's signature (`ARGS`); no library loading.

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


HEADS = {'normal_tanh': 0, 'identity': 1}  # BX_HEAD_NORMAL_TANH / BX_HEAD_IDENTITY
POP_NO_STAGE = 1  # BX_POP_NO_STAGE


class BxPopulation(C.Structure):
  _fields_ = [('param_stride', C.c_int64), ('head', C.c_int32), ('reward_shift', C.c_float),
              ('mom_in', C.c_void_p), ('mom_out', C.c_void_p), ('flags', C.c_int32),
              ('staged', C.c_int32), ('lds_bytes', C.c_int32)]


class BxSeq(C.Structure):
  """One float32 (T, B) array: element (t, e) at ptr[t * time_stride + e *
  env_stride], strides in elements."""
  _fields_ = [('ptr', C.c_void_p), ('time_stride', C.c_int64), ('env_stride', C.c_int64)]


POPULATION_DELTA_CHUNK = 64  # BX_POPULATION_DELTA_CHUNK
FIELDS_MAX = 8  # BX_FIELDS_MAX


class BxFields(C.Structure):
  """A batch of rows held as up to FIELDS_MAX float32 arrays: row r is the
  concatenation of the width[f] floats at ptr[f] + r * row_stride[f]."""
  _fields_ = [('n_fields', C.c_int32), ('ptr', C.c_void_p * FIELDS_MAX),
              ('width', C.c_int64 * FIELDS_MAX), ('row_stride', C.c_int64 * FIELDS_MAX)]


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


PPO_HEAD_BLOCK = 256  # bx_ppo_head: envs of a scan workgroup, rows of a row workgroup
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


OPT_MAX_TENSORS = 32  # BX_OPT_MAX_TENSORS
OPT_CHUNK = 1024  # elements of one tensor that one workgroup of bx_adam_step owns


class BxOptTensor(C.Structure):
  """One tensor of bx_adam_step's table: n contiguous float32 at each of p, g,
  m, v (and target, None for no target update)."""
  _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p),
              ('target', C.c_void_p), ('n', C.c_int64), ('lr', C.c_float), ('tau', C.c_float)]


PLAN_FIELDS = ('mode', 'lanes', 'lds_bytes', 'feat', 'gw', 'fold', 'jb', 'cb')  # bx_system_blob


def _sig(*args):
  """One entry point's (name, ctype) pairs; a bare name is a `c_void_p`: a
  device array, the system handle or the stream."""
  return tuple((a, C.c_void_p) if isinstance(a, str) else a for a in args)


_ptr = C.POINTER
_int, _i32, _i64, _u64, _f32, _f64 = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
_seq, _qp, _state, _fields = _ptr(BxSeq), _ptr(BxQP), _ptr(BxEnvState), _ptr(BxFields)
_bytes = ('workspace', ('workspace_bytes', _ptr(_i64)))
_host = (('desc', _ptr(BxDesc)), ('reset', _ptr(BxResetDesc)))
_env = ('sys', ('env', _ptr(BxEnvParams)), ('n_envs', _i64))
_act = ('act', ('act_stride', _i64))
# what every K-step launch starts with (the closed-loop ones read obs_in too)
# and how each kind names its actions: given, drawn, or the policy's
_open = _env + (('n_steps', _i32), 'qp_in', 'done_in', 'steps_in', 'rng_in')
_closed = _env + (('n_steps', _i32), 'qp_in', 'obs_in', 'done_in', 'steps_in', 'rng_in')
_given = _act + (('act_step_stride', _i64), ('act_width', _i64))
_draw = (('seed', _u64), ('offset', _u64), ('step_stride', _u64))
_policy = (('policy', _ptr(BxPolicy)),) + _draw
# `eval_in` / `eval_out` are (M + 3, B) float32: the M metric sums in the env's
# metric order, the reward sum, active_episodes, episode_steps
_eval = ('eval_in', 'out', 'eval_out', 'rng_out')
_slabs = ('out', ('slab_n', _i64), ('n_slabs', _i64), ('seed', _u64), ('offset', _u64),
          ('slab_stride', _u64), 'epoch', ('epoch_stride', _u64))
_gae = (('reward', _seq), ('done', _seq), ('truncation', _seq))
_scales = (('reward_scaling', _f32), ('discount', _f32), ('lambda', _f32))
_ring = ('data', ('capacity', _i64), ('row_words', _i64), ('position', _i64))
_mlp = (('net', _ptr(BxMlp)), ('rows', _i64), 'x', ('x_stride', _i64))

# Every entry point of the header, argument by argument in its order: the one
# table the loader, `_native.args` and tests/test_abi.py read. (The learner
# heads' (T, B, W) arrays are BxSeq with unit stride along a row.)
ARGS = {
    'bx_abi_version': (), 'bx_last_error': (), 'bx_device_count': _sig(('count', _ptr(_int))),
    'bx_system_create': _sig(*_host, ('device', _int), ('out', _ptr(C.c_void_p))),
    'bx_system_destroy': _sig('sys'), 'bx_system_lanes': _sig('sys'),
    'bx_system_env_lanes': _sig('sys'),
    'bx_system_plan': _sig(*_host, ('mode', _ptr(_i32)), ('lanes', _ptr(_i32)),
                           ('lds_bytes', _ptr(_i32))),
    'bx_system_blob': _sig(*_host, ('words', _ptr(C.c_uint32)), ('capacity', _i64),
                           ('n_words', _ptr(_i64)), ('plan', _ptr(_i32))),
    'bx_system_lds_bytes': _sig('sys'), 'bx_system_set_single': _sig('sys', ('on', _int)),
    'bx_system_set_variant': _sig('sys', ('lanes', _int), ('mode', _int)),
    'bx_system_set_block': _sig('sys', ('threads', _int)),
    'bx_system_step': _sig('sys', ('n_envs', _i64), ('qp_in', _qp), *_act, ('act_width', _i64),
                           ('qp_out', _qp), ('info', _ptr(BxInfo)), 'stream'),
    'bx_env_step': _sig(*_env, ('in', _state), *_act, ('act_width', _i64), ('out', _state),
                        'stream'),
    'bx_env_step_packed': _sig(*_env, 'qp_in', 'done_in', 'steps_in', 'rng_in', *_act,
                               ('act_width', _i64), 'out', 'rng_out', 'stream'),
    'bx_env_rollout_packed': _sig(*_open, *_given, 'out', 'rng_out', 'stream'),
    'bx_env_rollout_random': _sig(*_open, *_draw, ('lo', _f32), ('hi', _f32), ('act_width', _i64),
                                  'act_out', 'out', 'rng_out', 'stream'),
    'bx_env_rollout_policy': _sig(*_closed, *_policy, 'act_out', 'raw_out', 'logp_out', 'out',
                                  'rng_out', 'stream'),
    'bx_env_eval_policy': _sig(*_closed, *_policy, *_eval, 'stream'),
    'bx_env_eval_packed': _sig(*_open, *_given, *_eval, 'stream'),
    # bx_env_eval_policy's arguments, then the population struct before the stream
    'bx_env_eval_population': _sig(*_closed, *_policy, *_eval, ('pop', _ptr(BxPopulation)),
                                   'stream'),
    'bx_system_default_qp': _sig('sys', ('n_envs', _i64), 'joint_angle', 'joint_velocity',
                                 ('qp_out', _qp), 'stream'),
    'bx_system_info': _sig('sys', ('n_envs', _i64), ('qp', _qp), ('info', _ptr(BxInfo)), 'stream'),
    'bx_env_sizes': _sig(*_env[:2], ('obs_size', _ptr(_i32)), ('n_metrics', _ptr(_i32))),
    'bx_env_reset': _sig(*_env, ('seed', _u64), ('env_offset', _i64), 'env_seeds',
                         ('noise_scale', _f32), ('out', _state), 'stream'),
    'bx_env_observe': _sig(*_env, ('qp', _qp), *_act, ('act_width', _i64), 'obs', 'stream'),
    'bx_system_joint_angles': _sig('sys', ('n_envs', _i64), ('qp', _qp), 'angle', 'vel', 'stream'),
    'bx_uniform': _sig('out', ('n', _i64), ('seed', _u64), ('offset', _u64), ('lo', _f32),
                       ('hi', _f32), 'stream'),
    'bx_uniform_epoch': _sig('out', ('n', _i64), ('seed', _u64), ('offset', _u64), 'epoch',
                             ('epoch_stride', _u64), ('lo', _f32), ('hi', _f32), 'stream'),
    'bx_uniform_slabs': _sig(*_slabs, ('lo', _f32), ('hi', _f32), 'stream'),
    'bx_normal_slabs': _sig(*_slabs, 'stream'),
    'bx_compute_gae': _sig(('n_steps', _i64), ('n_envs', _i64), *_gae, ('values', _seq),
                           'bootstrap', ('vs', _seq), ('advantages', _seq), *_scales, 'stream'),
    'bx_population_perturb': _sig('rows', 'theta', ('n_directions', _i64), ('n_params', _i64),
                                  ('stride', _i64), ('sigma', _f64), ('seed', _u64),
                                  ('offset', _u64), ('antithetic', _int), 'frozen', 'stream'),
    'bx_population_delta': _sig('out', 'weights', ('n_directions', _i64), ('n_params', _i64),
                                ('seed', _u64), ('offset', _u64), 'frozen', *_bytes, 'stream'),
    'bx_replay_insert': _sig(*_ring, ('n_rows', _i64), ('src', _fields), 'stream'),
    'bx_replay_sample': _sig(*_ring, ('size', _i64), ('n_samples', _i64), ('seed', _u64),
                             ('offset', _u64), ('dst', _fields), 'idx_out', 'stream'),
    'bx_mlp_sizes': _sig(('mlp_bytes', _ptr(_i32)), ('grads_bytes', _ptr(_i32))),
    'bx_mlp_forward': _sig(*_mlp, 'y', 'saved', 'stream'),
    'bx_mlp_backward': _sig(*_mlp, 'saved', 'dy', 'dx', ('grads', _ptr(BxMlpGrads)), *_bytes,
                            'stream'),
    'bx_ppo_head': _sig(
        ('n_steps', _i64), ('n_envs', _i64), ('n_actions', _i64), ('logits', _seq),
        ('baseline', _seq), 'bootstrap', ('raw_action', _seq), ('eps', _seq), ('log_prob', _seq),
        *_gae, *_scales, ('clipping_epsilon', _f64), ('entropy_cost', _f32), ('min_std', _f32),
        ('normalize_advantage', _int), 'losses', ('dlogits', _seq), ('dbaseline', _seq),
        ('vs', _seq), ('advantages', _seq), *_bytes, 'stream'),
    'bx_opt_sizes': _sig(('tensor_bytes', _ptr(_i32))),
    'bx_adam_step': _sig(('t', _ptr(BxOptTensor)), ('n_tensors', _i32), ('step', _i64),
                         ('beta1', _f64), ('beta2', _f64), ('eps', _f32), 'stream'),
    'bx_sac_head_prep': _sig(
        ('n_rows', _i64), ('n_obs', _i64), ('n_actions', _i64), 'obs', ('obs_pitch', _i64),
        'next_obs', ('next_obs_pitch', _i64), 'action', ('action_pitch', _i64), 'mean', 'std',
        'x_cur', 'x_next', 'x_pi', ('x_pitch', _i64), 'stream'),
    'bx_sac_head_sample': _sig(('n_rows', _i64), ('n_actions', _i64),
                               ('jobs', _ptr(BxSacSampleJob)), ('n_jobs', _i32),
                               ('min_std', _f32), 'stream'),
    'bx_sac_head_losses': _sig(
        ('n_rows', _i64), ('n_critics', _i32), 'lp_alpha', 'lp_next', 'lp_pi', ('q', _ptr(BxSacQ)),
        'reward', ('reward_stride', _i64), 'discount', ('discount_stride', _i64), 'truncation',
        ('truncation_stride', _i64), 'log_alpha', ('reward_scaling', _f32), ('discounting', _f32),
        ('target_entropy', _f32), 'g_lp', *_bytes, 'stream'),
    'bx_sac_head_sample_backward': _sig(
        ('n_rows', _i64), ('n_actions', _i64), ('n_critics', _i32), 'logits',
        ('logits_pitch', _i64), 'eps', ('eps_pitch', _i64), 'g_lp', ('da', _ptr(BxSacDaction)),
        ('min_std', _f32), 'dlogits', ('dlogits_pitch', _i64), 'losses', 'dlog_alpha', *_bytes,
        'stream'),
    'bx_phase': _sig('sys', ('which', _int), ('n_envs', _i64), ('plane', _i64), 'in', 'out', 'aux',
                     ('aux_plane', _i64), 'stream'),
    'bx_phase_capsule_plane': _sig('sys', ('n_envs', _i64), ('plane', _i64), 'in', 'out',
                                   ('out_plane', _i64), 'stream'),
    'bx_debug_stamps': _sig(('out16', _ptr(C.c_ulonglong)), ('reset', _int)),
    'bx_debug_partner': _sig('out64', ('lanes', _int), 'stream'),
}
# name -> (argtypes, restype): 0 on success everywhere but the message itself
SIGNATURES = {name: ([t for _, t in args], C.c_char_p if name == 'bx_last_error' else C.c_int)
              for name, args in ARGS.items()}


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
