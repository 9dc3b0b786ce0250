"""The frozen plane side of the Ant env kernels' contact rows, held in
registers over a launch (CBH: pbd_features.h cbh_feat, pbd_kernels.hip
FrozenB / load_frozen, read after the state is in LDS and again after a step
in which the env took AutoReset's first state).

(A) Six Ant envs (one full wave of four plus a half-empty one),
`episode_length = 2`, one 5-step rollout launch: every env resets twice
inside the launch. The launch equals five chained `env.step`s bit for bit and
every step passes tests/test_gpu_parity.py's per-env `_gate` against the
float64 oracle stepped from the device's own fp32 input.

(B) The same on a tilted ground: the Ant config with the Ground body's
default pose rotated (`defaults { qps { name: "Ground" rot ... } }`), so a
normal left at (0, 0, 1) fails, and once more with the start state's Ground
at another tilt than first_qp's (the host takes any state: nothing on it
checks a frozen body's pose), so a normal kept over the reset fails. Each
step is also held against the all-kinds kernel (BX_NO_JB, the kernel
ineligible Ant-kind systems take) stepped from the same input: both are fp32
realisations of one algorithm, so their distance is held to the same per-env
bound, max(1e-5, 2 x E32_i).

(C) Eligibility: `contact_on_body` of the five pinned plans is unchanged, and
the tilted system is eligible (it runs the kernels under test).

The preconditions are asserted on the float64 oracle: a foot penetrates
(`pen > 0`) in the first collision pass of step 0 and of the step after the
reset (the same system at `substeps = 2`, `dt / 5`, whose only pass it is, as
tests/test_gpu_contact_body.py reads a first pass).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from brax_amd.envs import configs
from tests.helpers import QP_FIELDS
from tests.test_plan_contact_body import _flags

_ANT = configs.ANT_CONFIG  # as shipped (the tests below patch configs.ANT_CONFIG)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, EPISODE = 6, 5, 2
FEET = [1, 2, 3, 4]  # the rows (Ant: torso, then the four feet)
TILT = ' defaults { qps { name: "Ground" rot { x: 7 y: -4 } } }'
START_TILT = (-5.0, 6.0, 0.0)  # the start state's Ground in (B), second run (euler degrees)


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _text(tilted):
  assert 'defaults' not in _ANT
  return _ANT + (TILT if tilted else '')


def _config(tilted, first_pass=False):
  from brax_amd import config as cfgmod
  cfg = cfgmod.parse(_text(tilted))
  if first_pass:
    cfg.dt /= cfg.substeps / 2
    cfg.substeps = 2
  return cfg


@functools.lru_cache(maxsize=None)
def _oracles(oracle_lib, tilted):
  """(descriptors, float64 oracle, float64 first-pass oracle, Ground's index)."""
  from brax_amd import compiler
  vc, d, meta = compiler.compile_system(_config(tilted))
  rd = compiler.compile_reset(vc, meta['body_index'])
  vc1, d1, meta1 = compiler.compile_system(_config(tilted, first_pass=True))
  o1 = oracle_lib.Oracle(d1, compiler.compile_reset(vc1, meta1['body_index']), np.float64,
                         safe_guard=True)
  return (d, rd), oracle_lib.Oracle(d, rd, np.float64, safe_guard=True), o1, meta['body_index']['Ground']


def _actions():
  return np.random.default_rng(23).uniform(-1, 1, (K, B, 8)).astype(np.float32)


def _make_env(dev, monkeypatch, tilted, fallback=False):
  from brax_amd import envs
  from brax_amd.envs import configs
  monkeypatch.setattr(configs, 'ANT_CONFIG', _text(tilted))
  if fallback:
    monkeypatch.setenv('BX_NO_JB', '1')
  else:
    monkeypatch.delenv('BX_NO_JB', raising=False)
  return envs.create('ant', batch_size=B, episode_length=EPISODE, auto_reset=True, device=dev)


def _np(t):
  return t.detach().cpu().numpy()


def _start(env, dev, oracle_lib, tilted, start_tilt):
  """The reset state, and the state the run starts from: the reset pose with
  whole ants moved in z so that envs 1 and 4 stand 5 mm deep (flat ground; on
  the tilted one the low-side feet are deep as they are), in (B)'s second run
  with the Ground at another tilt than first_qp's."""
  from brax_amd.base import qp_from_numpy
  from brax_amd.compiler import euler_to_quat
  ground = _oracles(oracle_lib, tilted)[3]
  st = env.reset(np.array([4, 2], np.uint32))
  q = st.info['first_qp'].numpy().astype(np.float32).copy()
  if not tilted:
    moving = [b for b in range(q.shape[1]) if b != ground]
    dz = np.array([0.05, -0.005, 0.02, 0.2, -0.006, 0.0], np.float32)
    q[:, moving, 2] += dz[:, None]
  if start_tilt is not None:
    q[:, ground, 3:7] = euler_to_quat(np.array(start_tilt)).astype(np.float32)
  return st, st.replace(qp=qp_from_numpy(q, dev)), q


def _first_pass_feet(o1, qp, act):
  return o1.system_step(qp, act)[1]['contact_penetration'][:, FEET]


def _run(dev, oracle_lib, monkeypatch, tilted, start_tilt):
  from tests.test_gpu_parity import Envelope, _env_err, _gate
  from tests.test_gpu_rollout import _check
  desc, o64, o1, ground = _oracles(oracle_lib, tilted)
  env = _make_env(dev, monkeypatch, tilted)
  fb = _make_env(dev, monkeypatch, tilted, fallback=True) if tilted else None
  u = env.unwrapped
  O, M = u.obs_size, len(u.metric_keys)
  env32 = Envelope(oracle_lib, None, desc=desc)
  act = _actions()
  acts = torch.as_tensor(act, device=dev)
  st_reset, st0, qp0 = _start(env, dev, oracle_lib, tilted, start_tilt)
  first_qp, first_obs = st_reset.info['first_qp'].numpy(), _np(st_reset.info['first_obs'])
  if tilted:
    n0 = first_qp[0, ground, 3:7]
    assert abs(n0[0]) < 0.999, n0  # the plane's normal is not (0, 0, 1)
    if start_tilt is not None:
      assert not np.allclose(qp0[:, ground, 3:7], first_qp[:, ground, 3:7], atol=1e-2)
  # the launch against the chained steps, bit for bit
  tr = _check(env, st0, acts)
  done_t = _np(tr.done)
  assert (done_t.sum(0) >= 2).all(), done_t  # every env reset twice inside the launch
  # preconditions: a foot in contact in the first pass of step 0 and of the
  # step after the first reset (which starts from first_qp)
  p0 = _first_pass_feet(o1, qp0, act[0])
  p1 = _first_pass_feet(o1, first_qp.astype(np.float32), act[EPISODE])
  print('first pass, step 0', np.round(p0, 5), 'first pass after the reset', np.round(p1, 5), sep='\n')
  assert (p0 > 0).any() and (p1 > 0).any()
  # every step against the oracle (and, tilted, the all-kinds kernel)
  st = st0
  steps = np.zeros(B)
  for t in range(K):
    qin = st.qp.numpy().astype(np.float32)
    steps = np.where(_np(st.done) != 0, 0, steps)
    prev, st = st, env.step(st, acts[t])
    ref, robs, rrew, rdone, _ = o64.env_step('ant', qin, act[t], O, M, coef=u.coef)
    outs = env32.env('ant', qin, act[t], O, M, 0, u.coef)
    steps = steps + 1
    done = np.where(steps >= EPISODE, 1.0, rdone)
    got, obs = st.qp.numpy(), _np(st.obs)
    assert np.array_equal(_np(st.done), done), (t, _np(st.done), done)
    sel = done != 0
    assert np.array_equal(got[sel], first_qp[sel]) and np.array_equal(obs[sel], first_obs[sel]), t
    k = ~sel
    other = fb.step(prev, acts[t]) if fb is not None else None
    if other is not None:
      assert torch.equal(other.done, st.done), t
    if k.any():
      e_rew = _env_err([o[2][k][:, None] for o in outs], rrew[k][:, None])
      _gate(_np(st.reward)[k][:, None], rrew[k][:, None], e_rew, 'reward')
      e_obs = _env_err([o[1][k] for o in outs], robs[k])
      _gate(obs[k], robs[k], e_obs, 'obs')
      for f, sl in QP_FIELDS.items():
        e32 = _env_err([o[0][k][..., sl] for o in outs], ref[k][..., sl])
        _gate(got[k][..., sl], ref[k][..., sl], e32, f)
        if other is not None:
          _gate(got[k][..., sl], other.qp.numpy()[k][..., sl].astype(np.float64), e32, f + ':all_kinds')
      if other is not None:
        _gate(obs[k], _np(other.obs)[k].astype(np.float64), e_obs, 'obs:all_kinds')


@gpu
def test_ragged_wave_with_resets_inside_the_launch(dev, oracle_lib, monkeypatch):
  _run(dev, oracle_lib, monkeypatch, False, None)


@gpu
@pytest.mark.parametrize('start_tilt', [None, START_TILT], ids=['tilted', 'start_tilt_differs'])
def test_tilted_ground(dev, oracle_lib, monkeypatch, start_tilt):
  _run(dev, oracle_lib, monkeypatch, True, start_tilt)


# ---- (C) eligibility (CPU) -------------------------------------------------

@pytest.mark.parametrize('name,want', [('ant', 1), ('ant_two_rows', 0), ('halfcheetah', 0),
                                       ('humanoid', 0)])
def test_contact_on_body_unchanged(name, want):
  assert _flags(('ant', 'ant_two_rows', 'halfcheetah', 'humanoid'), False)[name] == want


def test_contact_on_body_needs_body_copies():
  assert _flags(('ant',), True)['ant'] == 0


_CHILD = r"""
import sys
from brax_amd import config as cfgmod
from brax_amd.system import System
from tests.test_gpu_frozen_side import _text
System.plan(cfgmod.parse(_text(True)))
"""


def test_tilted_ground_is_eligible():
  """The tilted system takes the body-lane kernels: (B) runs the code under
  test, not the fallback."""
  env = dict(os.environ, BX_PLAN_DEBUG='1', PYTHONPATH=ROOT)
  env.pop('BX_NO_JB', None)
  r = subprocess.run([sys.executable, '-c', _CHILD], env=env, cwd=ROOT, text=True,
                     capture_output=True, timeout=120)
  assert r.returncode == 0, r.stderr[-2000:]
  assert re.findall(r'contact_on_body=(\d)', r.stderr) == ['1'], r.stderr[-2000:]


def test_preconditions_on_the_oracle(oracle_lib):
  """The scenes' contacts on the CPU: the flat start state has feet 5-6 mm
  deep in envs 1 and 4, and the tilted ground's low-side feet are deep from
  the reset pose on."""
  from brax_amd import compiler
  act = _actions()
  for tilted in (False, True):
    (d, rd), o64, o1, ground = _oracles(oracle_lib, tilted)
    ang = np.asarray(rd['default_angle'], np.float64)[None]
    q = np.repeat(o64.default_qp(ang, np.zeros_like(ang)), B, axis=0).astype(np.float32)
    p = _first_pass_feet(o1, q, act[EPISODE])
    print('tilted' if tilted else 'flat', np.round(p, 5))
    assert np.isfinite(p).all()
    assert (p > 0).any(), p
    if tilted:
      assert not np.allclose(q[0, ground, 3:7], [1, 0, 0, 0])
