"""Shared test helpers: systems by name and the parity gate."""
import os
import re

import numpy as np

from brax_amd import compiler
from brax_amd import config as cfgmod
from brax_amd.envs import configs
from brax_amd.envs import robots
from brax_amd.envs.mountain import ant_mountain_config

ENV_CONFIG = {
    'humanoidstandup': robots.HUMANOID_STANDUP_CONFIG,
    'ant': configs.ANT_CONFIG,
    'humanoid': configs.HUMANOID_CONFIG,
    'halfcheetah': configs.HALFCHEETAH_CONFIG,
}


# the other registered envs' pbd systems (physics goldens, oracle/gen_golden.py)
ROBOTS = ['inverted_pendulum', 'inverted_double_pendulum', 'swimmer', 'hopper', 'walker2d',
          'reacher', 'reacherangle', 'acrobot', 'ur5e', 'pusher', 'grasp', 'fetch']


# the CapsuleTest scene (reference `brax/tests/physics_test.py:292-328`) as
# test input data; variants 'ground', 'capsule', 'cull' as in its three tests
CAPSULE_TEST_CONFIG = """
dt: 20.0 substeps: 10000 friction: 0.6 gravity { z: -9.8 }
bodies { name: "Capsule1" mass: 1 colliders { capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule2" mass: 1 colliders { rotation { y: 90 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule3" mass: 1 colliders { rotation { y: 45 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule4" mass: 1 colliders { rotation { x: 45 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Ground" frozen { all: true } colliders { plane {} } }
defaults { qps { name: "Capsule1" pos { z: 1 } } qps { name: "Capsule2" pos { x: 1 z: 1 } } qps { name: "Capsule3" pos { x: 3 z: 1 } } qps { name: "Capsule4" pos { x: 5 z: 1 } } }
defaults { qps { name: "Capsule1" pos { z: 1 } } qps { name: "Capsule2" pos { z: 2 } } qps { name: "Capsule3" pos { x: 3 z: 1 } } qps { name: "Capsule4" pos { x: 5 z: 1 } } }
"""
CAPSULES = ['capsule_ground', 'capsule_capsule', 'capsule_cull']
# short-horizon twins of the long physics-test scenes (dt 0.05, 10 substeps,
# from a state falling into contact; oracle/gen_golden.py _short_scenes):
# the golden trajectory gates run on these, the long scenes stay KATs
SHORT_SCENES = ['capsule_ground_s', 'capsule_capsule_s', 'capsule_cull_s', 'box_ground_s',
                'box_slide_s']
# NearNeighbors with more cutoff than allowed cells: top_k also returns
# masked cells (oracle/scenes.py TWIN_CULL_CONFIG; golden generated under
# jax.lax.top_k's tie order)
NN_MASKED = ['twin_cull']
# legacy_spring systems (`_SYSTEM_CONFIG_SPRING`, system.py:342-390): envs with
# the kernel env layer, and physics rollouts of the other registered envs
SPRING_ENVS = ['ant_spring', 'humanoid_spring', 'halfcheetah_spring', 'humanoidstandup_spring']
SPRING_ROBOTS = [m + '_spring' for m in (
    'inverted_pendulum', 'inverted_double_pendulum', 'swimmer', 'hopper', 'walker2d', 'reacher',
    'reacherangle', 'acrobot', 'ur5e', 'grasp', 'fetch')]
_SPRING_MOD = {'halfcheetah': 'HALF_CHEETAH', 'humanoidstandup': 'HUMANOID_STANDUP'}


# exclude_current_positions_from_observation=False rollouts (traj_<env>_xy)
XY_ENVS = ['ant_xy', 'humanoid_xy', 'halfcheetah_xy']


# kernel env kinds whose reference rollouts are the envtraj_* goldens (the
# env-layer rollouts of oracle/gen_golden.py) rather than traj_*
ENVTRAJ_KERNEL = ['hopper', 'walker2d', 'inverted_pendulum', 'inverted_double_pendulum', 'acrobot',
                  'reacher', 'reacherangle', 'swimmer', 'pusher', 'ur5e', 'fetch', 'grasp']
# bodies a kernel env's reset places after default_qp (reacher.py:177-179,
# pusher.py:196-201): name -> body names


def reset_bodies(name):
  return {'reacher': ['target'], 'reacherangle': ['target'], 'ur5e': ['Target'],
          'fetch': ['Target'], 'pusher': ['goal', 'object', 'table']}.get(name, [])


def env_coef(name):
  """bx_env_params.coef of a kernel env with its constructor defaults, built
  on the CPU (None: the oracle's built-in defaults apply)."""
  from brax_amd.envs import tasks
  if name in ('reacher', 'reacherangle'):
    cfg = config_for(name)
    return tasks.reacher_coef(cfg, compiled(name)[3]['body_index'], angle=name == 'reacherangle')
  if name == 'swimmer':
    return tasks.swimmer_coef()
  if name == 'pusher':
    return tasks.pusher_coef(compiled(name)[3]['body_index'])
  if name == 'grasp':
    return tasks.grasp_coef(compiled(name)[3]['body_index'])
  if name in ('ur5e', 'fetch'):
    cls = tasks.Ur5e if name == 'ur5e' else tasks.Fetch
    return tasks.target_coef(compiled(name)[3]['body_index'], cls.torso, *cls.ring)
  return None


def prep_oracle(o, name):
  """Per-env oracle state: Grasp's action map."""
  name = env_kind(name) if name else name
  if name == 'grasp':
    from brax_amd.envs import tasks
    o.set_act_map(tasks.grasp_act_map(config_for(name)))
  return o


def golden_reset_qp(name, o, T):
  """The oracle's default_qp of the golden reset angles, with the bodies the
  env's reset places copied from the golden's reset state."""
  qp0 = o.default_qp(T['reset_qpos'], T['reset_qvel'])
  idx = [compiled(name)[3]['body_index'][b] for b in reset_bodies(name)]
  for b in idx:
    qp0[:, b, 0:3] = T['qp'][0][:, b, 0:3]
  return qp0


# mid-episode fixtures (oracle/gen_golden.py MID): env-layer rollouts of 2
# steps from states the float64 oracle reached by seeded burn-in (Pusher: by a
# seeded search over `object` placements), chosen so that the contact rows
# `row_target` penetrate; one file serves the system and the env gates
MID = ['mid_pusher', 'mid_halfcheetah', 'mid_hopper', 'mid_walker2d', 'mid_humanoidstandup']
# Grasp's env step moves the palm and maps the action before System.step
# (grasp.py:73-87), so its env-layer fixture's actions are not System.step's:
# the env gate takes the file as it is, the system gate takes what
# oracle/mid_states.py `pre_step` makes of its states and actions (the action
# map and the palm move in float64 on the host). 16 envs, not 8
MID_ENV = ['mid_grasp']

# the target envs' steps teleport a hit target to a random spot AFTER the
# observation, the reward and the metrics are taken (ur5e.py:83-89,
# fetch.py:90-96, grasp.py:130-136): only that body's pos is replaced, its
# rot / vel / ang stay the physics'. The reference draws the spot from a JAX
# key, the HIP env from its own counter stream, and the C oracle does not
# restate it (parity-unpinned), so on a sample whose recorded
# `hits` metric is 1 the recorded next state's target pos is compared with
# nothing: env kind -> the body
TELEPORTS = {'ur5e': 'Target', 'fetch': 'Target', 'grasp': 'Target'}


def teleported(name, T):
  """Of an env-layer golden `T` of the golden name `name`: (the teleported
  body's index, (steps, B) bool: the recorded `hits` metric is 1, the target
  of that sample's step was teleported), or (None, None) for an env kind
  whose step teleports nothing."""
  body = TELEPORTS.get(env_kind(name))
  if body is None:
    return None, None
  hits = T['metrics'][..., [str(k) for k in T['metric_keys']].index('hits')]
  assert np.isin(hits, (0.0, 1.0)).all()
  return compiled(name)[3]['body_index'][body], hits == 1.0


def without_teleported(qp, body, hit):
  """A copy of the states `qp` (B, N, 13) with the pos of `body` taken out
  (zeroed: it then adds nothing to a normwise error or its scale) on the
  envs `hit` (B,) bool; the body's rot / vel / ang and every other sample
  stay. `body` None: `qp` itself."""
  if body is None:
    return qp
  qp = np.array(qp, copy=True)
  qp[hit, body, 0:3] = 0
  return qp


def env_golden(name):
  """Golden file of a kernel env's reference rollout."""
  if name.startswith('mid_'):
    return name
  return ('envtraj_' if name in ENVTRAJ_KERNEL else 'traj_') + name


def sys_golden(name):
  """Golden file of a system's reference System.step rollout."""
  return name if name.startswith('mid_') else 'traj_' + name


def env_kind(name):
  """Env-layer kind of a golden name ('ant_spring', 'ant_xy', 'mid_ant' ->
  'ant')."""
  if name.startswith('mid_'):
    name = name[len('mid_'):]
  for suf in ('_spring', '_xy'):
    if name.endswith(suf):
      return name[:-len(suf)]
  return name


def obs_flags(name):
  """BX_OBS_* of a golden name (abi.OBS_XY for the *_xy rollouts)."""
  return 1 if name.endswith('_xy') else 0


# point-plane scenes: BoxTest (box corners) and an inline-mesh MeshTest
# (mesh vertices), oracle/scenes.py
POINTS = ['box_ground', 'box_slide', 'mesh_ground', 'mesh_tilt']
# the extended contact functions' scenes (oracle/scenes.py): box corners on a
# height map, spheres on a clipped plane, capsules against box / mesh triangles
XCOL = ['heightmap', 'clipped', 'box_capsule', 'mesh_capsule', 'box_box', 'box_capsule_hull']


def config_for(name):
  if name.startswith('mid_'):
    name = name[len('mid_'):]
  if name in SHORT_SCENES:
    base = name[:-2]
    cfg = config_for('box_ground' if base.startswith('box') else base)
    cfg.dt, cfg.substeps = 0.05, 10
    return cfg
  if name.endswith('_xy'):
    name = name[:-len('_xy')]
  if name.endswith('_spring'):
    base = name[:-len('_spring')]
    return cfgmod.parse(getattr(robots, _SPRING_MOD.get(base, base.upper()) + '_SPRING_CONFIG'))
  if name in CAPSULES:
    cfg = cfgmod.parse(CAPSULE_TEST_CONFIG)
    if name != 'capsule_ground':
      cfg.dt = 2.0
      cfg.substeps = 400
    if name == 'capsule_cull':
      cfg.collider_cutoff = 1
    return cfg
  if name in XCOL:
    from oracle import scenes
    return cfgmod.parse({'heightmap': lambda: scenes.heightmap_config(0.05, 10),
                         'clipped': lambda: scenes.clipped_plane_config(0.05, 10),
                         'box_capsule': lambda: scenes.BOX_CAPSULE_NO_HULL_CONFIG,
                         'mesh_capsule': scenes.mesh_capsule_config,
                         'box_box': lambda: scenes.box_box_config(0.05, 20),
                         'box_capsule_hull': lambda: scenes.BOX_CAPSULE_TEST_CONFIG}[name]())
  if name in POINTS:
    from oracle import scenes
    return cfgmod.parse(scenes.BOX_TEST_CONFIG if name.startswith('box')
                        else scenes.mesh_test_config())
  if name == 'twin_cull':
    from oracle import scenes
    return cfgmod.parse(scenes.TWIN_CULL_CONFIG)
  if name in ('mountain1nn', 'mountain2nn', 'mountain4nn'):
    n = int(name[len('mountain')])
    cfg = ant_mountain_config(n)
    cfg.collider_cutoff = 9 * n
    return cfg
  if name in ROBOTS:
    return cfgmod.parse(getattr(robots, name.upper() + '_CONFIG'))
  if name.startswith('mountain'):
    return ant_mountain_config(int(name[len('mountain'):]))
  return cfgmod.parse(ENV_CONFIG[name])


def compiled(name):
  vc, d, meta = compiler.compile_system(config_for(name))
  rd = compiler.compile_reset(vc, meta['body_index'])
  return vc, d, rd, meta


def set_variant(sys_, variant):
  """Put a System on one large-scene kernel: 'multi' (the MULTI kernel at its
  own width: 128 threads per env where the scene fits, else 256), 'multi256'
  (the MULTI kernel at 256 threads per env), 'itemloop' / 'items' (the item
  loops at 256 threads per env). Returns bx_system_set_variant's status."""
  from brax_amd import _native
  lib = _native.lib()
  if variant == 'multi':
    rc = lib.bx_system_set_variant(sys_._h, 128, 3)
    return rc if rc == 0 else lib.bx_system_set_variant(sys_._h, 256, 3)
  if variant == 'multi256':
    return lib.bx_system_set_variant(sys_._h, 256, 3)
  return lib.bx_system_set_variant(sys_._h, 256, 0)


def piled_mountain4(cutoff, substeps):
  """Ant Mountain(4) with its four ants piled onto one spot: (cfg, qp0), the
  config with `collider_cutoff` / `substeps` set and a start state (N, 13)
  pos|rot|vel|ang rounded to fp32. From the float64 oracle's default_qp with
  zero joint angles and velocities, every body of cloned ant i (the bodies
  named `*_i`, i in 0..2) is translated so that its torso sits 2 cm from ant
  0's: at torso0 + 0.02 (cos 2.1 k, sin 2.1 k, 0.6 k), k = i + 1. Rotations
  and velocities stay. Its first collision pass lists more penetrating rows
  than the MULTI kernel's LDS contact buffer holds (pbd_layout.h MCBUF), all
  finite (tests/test_gpu_multi_overflow.py; the counts are pinned on the CPU
  there)."""
  from oracle import oracle
  cfg = config_for('mountain4')
  cfg.collider_cutoff = cutoff
  cfg.substeps = substeps
  vc, d, meta = compiler.compile_system(cfg)
  o = oracle.Oracle(d, compiler.compile_reset(vc, meta['body_index']), np.float64)
  z = np.zeros((1, meta['num_joint_dof']))
  qp = o.default_qp(z, z)[0]
  bi = meta['body_index']
  torso0 = qp[bi['$ Torso'], 0:3].copy()
  for i in range(3):
    k = i + 1
    shift = (torso0 + 0.02 * np.array([np.cos(2.1 * k), np.sin(2.1 * k), 0.6 * k])
             - qp[bi[f'$ Torso_{i}'], 0:3])
    for name, b in bi.items():
      if name.endswith(f'_{i}'):
        qp[b, 0:3] += shift
  return cfg, qp.astype(np.float32)


def piled_actions(B, steps):
  """The piled scene's actions: env e's action at step t is row e of the t-th
  (B, 32) draw of default_rng(5).uniform(-1, 1), rounded to fp32."""
  rng = np.random.default_rng(5)
  return [rng.uniform(-1, 1, (B, 32)).astype(np.float32) for _ in range(steps)]


def normwise(a, b):
  """Per-env normwise error max|a-b| / max(1, max|b|) over trailing axes."""
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  axes = tuple(range(1, a.ndim))
  err = np.abs(a - b).max(axis=axes) if axes else np.abs(a - b)
  scale = np.maximum(1.0, np.abs(b).max(axis=axes) if axes else np.abs(b))
  return err / scale


WIDE = 1e-2  # a sample whose own bound 2 x E32 exceeds this is ill-conditioned
NEAR_TOL = 1e-3  # the ill-conditioned envs: floor of the nearest-realisation bound
# fp32-ulp perturbed copies per oracle build in the envelope:
# 2 builds x (1 exact + 32 perturbed) = 66 realisations per env, so a
# per-env E32_i is not a noisy maximum of a handful of runs
N_PERTURB = int(os.environ.get('BX_ENVELOPE_N', '32'))

QP_FIELDS = {'pos': slice(0, 3), 'rot': slice(3, 7), 'vel': slice(7, 10), 'ang': slice(10, 13)}


# ---------------------------------------------------------------------------
# the counter RNG restated on the host (include/brax_amd.h): plain
# numpy from the formulas, no call into the library
# ---------------------------------------------------------------------------
_U64 = (1 << 64) - 1


def _u64(x):
  """Python ints (any sign or size) or arrays as wrapping uint64."""
  if isinstance(x, (int, np.integer)):
    return np.uint64(int(x) & _U64)
  x = np.asarray(x)
  if x.dtype == np.uint64:
    return x
  if x.dtype == object:
    return np.array([int(v) & _U64 for v in x.ravel()], np.uint64).reshape(x.shape)
  return x.astype(np.uint64)


def counters(offset, n, step=1):
  """The n counters offset + step * j, j = 0..n-1, wrapping in uint64."""
  with np.errstate(over='ignore'):
    return _u64(offset) + _u64(step) * np.arange(n, dtype=np.uint64)


def splitmix_bits(seed, idx):
  """The 24 bits behind a draw: splitmix64 of seed * 0x9E3779B97F4A7C15 + idx +
  0x632BE59BD9B4E019 in wrapping uint64, its top 24 bits (z >> 40)."""
  with np.errstate(over='ignore'):
    z = _u64(seed) * np.uint64(0x9E3779B97F4A7C15) + _u64(idx) + np.uint64(0x632BE59BD9B4E019)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
  return z >> np.uint64(40)


def uniform01_ref(seed, idx):
  """U(seed, idx) in [0, 1) as float64: (z >> 40) / 2^24, a 24-bit value, so
  its float32 cast is exact."""
  return splitmix_bits(seed, idx).astype(np.float64) / 16777216.0


def normal_ref(seed, idx, dtype=np.float64):
  """N(seed, idx): Box-Muller's cosine branch on counters idx and idx + 1,
  sqrt(-2 ln(1 - U_idx)) cos(2 pi U_{idx+1}), every operation in `dtype`."""
  dt = np.dtype(dtype).type
  idx = _u64(idx)
  with np.errstate(over='ignore'):
    nxt = idx + np.uint64(1)
  u0 = uniform01_ref(seed, idx).astype(dt)
  u1 = uniform01_ref(seed, nxt).astype(dt)
  r = np.sqrt(dt(-2.0) * np.log(dt(1.0) - u0))
  c = np.cos(dt(2.0 * np.pi) * u1)
  out = r * c
  assert out.dtype == np.dtype(dtype)
  return out


# ---------------------------------------------------------------------------
# include/brax_amd.h as data: the one parser of the header (tests/test_abi.py)
# ---------------------------------------------------------------------------
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           'include', 'brax_amd.h')


def _declarator(text):
  """'const float* w[BX_MLP_MAX_LAYERS]' -> ('const float*', 'w', 'BX_MLP_MAX_LAYERS')."""
  ctype, name, dim = re.fullmatch(r'(.*?)(\w+)\s*(?:\[(\w+)\])?', text.strip()).groups()
  return re.sub(r'\s*\*', '*', ' '.join(ctype.split())), name, dim


class Header:
  """The declarations of the header, comments removed:
    functions  {name: (return type, [(C type, parameter, array length or None)])}
    structs    {name: [(C type, field, array length or None)]}, a declaration
               with several declarators (`bx_field pos, rot;`) one field each
    constants  {name: int} of the `#define BX_* <integer>` macros and the
               enumerators
  all in the header's order."""

  def __init__(self, path=HEADER_PATH):
    with open(path) as f:
      self.text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', f.read(), flags=re.S)
    self.functions = {}
    for res, name, params in re.findall(r'^([\w ]+?\*?)\s*\b(bx_\w+)\s*\(([^)]*)\)\s*;', self.text,
                                        re.M):
      params = [] if params.strip() == 'void' else params.split(',')
      self.functions[name] = (' '.join(res.split()), [_declarator(p) for p in params])
    self.structs = {}
    for name, body in re.findall(r'typedef\s+struct\s+(bx_\w+)\s*\{(.*?)\}\s*\1\s*;', self.text,
                                 re.S):
      fields = self.structs[name] = []
      for decl in filter(None, (d.strip() for d in body.split(';'))):
        first, *rest = decl.split(',')
        ctype, field, dim = _declarator(first)
        fields.append((ctype, field, dim))
        for more in rest:  # the header never mixes `T a, *b`
          assert '*' not in more and not ctype.endswith('*'), decl
          fields.append((ctype,) + _declarator(more)[1:])
    self.constants = {n: int(v, 0) for n, v in re.findall(
        r'^#define\s+(BX_\w+)\s+(-?\w+)\s*$', self.text, re.M) if re.fullmatch(r'-?\d\w*', v)}
    for body in re.findall(r'\benum\s*\{(.*?)\}', self.text, re.S):
      self.constants.update({n: int(v, 0) for n, v in re.findall(r'(BX_\w+)\s*=\s*(-?\w+)', body)})


class Envelope:
  """Brax's algorithm in fp32 on the exact inputs and on ulp-perturbed
  copies, in two oracle builds: plain float32 and float32 with a*b+c
  contracted to fused multiply-adds (XLA's jit contracts them, as hipcc does);
  the envelope is the max normwise error over every run."""

  def __init__(self, oracle_lib, name, n_perturb=None, desc=None):
    d, rd = desc if desc is not None else compiled(name)[1:3]
    self.os = [prep_oracle(oracle_lib.Oracle(d, rd, np.float32, safe_guard=True, fma=f), name)
               for f in (False, True)]
    self.n = N_PERTURB if n_perturb is None else n_perturb

  def _inputs(self, qp):
    yield qp.astype(np.float32)
    rng = np.random.default_rng(1234)
    for _ in range(self.n):
      noise = 1 + rng.uniform(-6e-8, 6e-8, qp.shape)
      yield (qp * noise).astype(np.float32)

  def system(self, qp, act):
    return [o.system_step(q, act.astype(np.float32)) for o in self.os for q in self._inputs(qp)]

  def env(self, name, qp, act, O, M, flags=0, coef=None):
    return [o.env_step(name, q, act.astype(np.float32), O, M, obs_flags=flags, coef=coef)
            for o in self.os for q in self._inputs(qp)]
