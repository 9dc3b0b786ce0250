"""The Ant env kernels' contact passes on the body lanes (CB: pbd_kernels.hip
pbd_step_single, pbd_features.h cb_feat) at the smallest ragged shape.

B = 6 Ant envs: one full wave of four envs plus a half-empty one, so the
four-envs-per-wave lane mapping and the invalid envs' lanes both run.
`episode_length = 5` over 12 steps with per-env actions, so AutoReset fires
inside the run. The start states are the default pose with whole ants
translated in z (`START_DZ`), chosen so that the float64 oracle shows:

  (a) envs 0, 3: the torso's row penetrates (the path of the torso's four
      body copies, lanes 0-3);
  (b) envs 1, 4: all four feet penetrate and the torso is clear (their first
      action is zero: a full-size one lifts a foot within the step);
  (c) envs 2, 5: no row penetrates.

(b) and (c) are step 0's Info (its last collision pass), as the precondition
test asserts. (a) cannot show there from a z translation alone: the feet's
capsules end 0.263 below the torso's, so a touching torso means feet 0.26 deep,
and their correction throws the ant clear of the ground within the step
(measured on the oracle: every row of step 0's Info is < -0.1 for shifts of
-0.26 .. -0.5). (a) is therefore asserted on the Info of step 0's FIRST
collision pass: the same system at `substeps = 2`, `dt / 5` (the same h), whose
only pass it is (tests/test_gpu_multi_overflow.py `_two_pass` reads a first
pass the same way).

Every state gate is tests/test_gpu_parity.py's per-env `_gate` against the
float64 oracle stepped from the device's own fp32 input. The same gate runs
on the Ant variant with two rows on one foot
(tests/test_plan_contact_body.py), which takes the all-kinds kernel.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import QP_FIELDS
from tests.test_plan_contact_body import two_row_ant_config

gpu = pytest.mark.gpu

B, K, EPISODE = 6, 12, 5
START_DZ = np.array([-0.30, -0.005, 0.05, -0.28, -0.006, 0.2])
TORSO, FEET = 0, [1, 2, 3, 4]  # the rows (Ant: torso, then the four feet)
AMBIGUOUS = 1e-5


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _config(two_rows, first_pass=False):
  from brax_amd import config as cfgmod
  from brax_amd.envs import configs
  cfg = cfgmod.parse(two_row_ant_config() if two_rows else configs.ANT_CONFIG)
  if first_pass:
    cfg.dt /= cfg.substeps / 2
    cfg.substeps = 2
  return cfg


@functools.lru_cache(maxsize=None)
def _scene(oracle_lib, two_rows):
  """(descriptors, float64 oracle, start state (B, N, 13) fp32, actions
  (K, B, A) fp32) of the Ant system or its two-rows-on-a-foot variant."""
  from brax_amd import compiler
  vc, d, meta = compiler.compile_system(_config(two_rows))
  rd = compiler.compile_reset(vc, meta['body_index'])
  o64 = oracle_lib.Oracle(d, rd, np.float64, safe_guard=True)
  ang = np.asarray(rd['default_angle'], np.float64)[None]
  q = np.repeat(o64.default_qp(ang, np.zeros_like(ang)), B, axis=0)
  ground = meta['body_index']['Ground']
  moving = [b for b in range(q.shape[1]) if b != ground]
  q[:, moving, 2] += START_DZ[:, None]
  act = np.random.default_rng(17).uniform(-1, 1, (K, B, ang.shape[1])).astype(np.float32)
  act[0, [1, 4]] = 0  # (b): a full-size first action lifts a foot within the step
  return (d, rd), o64, q.astype(np.float32), act


def test_start_states_show_the_three_contact_cases(oracle_lib):
  """The scene's own precondition, on the CPU (float64 oracle, step 0)."""
  from brax_amd import compiler
  (d, rd), o64, qp0, act = _scene(oracle_lib, False)
  assert list(d['row_body_a']) == [0, 2, 4, 6, 8]
  last = o64.system_step(qp0, act[0])[1]['contact_penetration']
  vc, d1, meta = compiler.compile_system(_config(False, first_pass=True))
  o1 = oracle_lib.Oracle(d1, compiler.compile_reset(vc, meta['body_index']), np.float64,
                         safe_guard=True)
  first = o1.system_step(qp0, act[0])[1]['contact_penetration']
  print('first pass', np.round(first, 5), 'last pass', np.round(last, 5), sep='\n')
  assert np.isfinite(first).all() and np.isfinite(last).all()
  assert (np.abs(first) > AMBIGUOUS).all() and (np.abs(last) > AMBIGUOUS).all()
  for e in (0, 3):  # (a)
    assert first[e, TORSO] > 0, (e, first[e])
  for e in (1, 4):  # (b)
    assert (last[e, FEET] > 0).all() and last[e, TORSO] < 0, (e, last[e])
  for e in (2, 5):  # (c)
    assert (last[e] < 0).all(), (e, last[e])


def _make_env(dev, monkeypatch, two_rows):
  from brax_amd import envs
  from brax_amd.envs import configs
  if two_rows:
    monkeypatch.setattr(configs, 'ANT_CONFIG', two_row_ant_config())
  return envs.create('ant', batch_size=B, episode_length=EPISODE, auto_reset=True, device=dev)


def _start(env, qp0, dev):
  """The reset state (its first_qp / first_obs are AutoReset's target) with
  the scene's start state put in."""
  from brax_amd.base import qp_from_numpy
  st = env.reset(np.array([4, 2], np.uint32))
  return st.replace(qp=qp_from_numpy(qp0, dev))


def _np(t):
  return t.detach().cpu().numpy()


@gpu
@pytest.mark.parametrize('two_rows', [False, True], ids=['ant', 'two_rows_on_a_foot'])
def test_every_step_against_the_oracle(dev, oracle_lib, monkeypatch, two_rows):
  """Each of the 12 chained `env.step`s: pos, rot, vel, ang, obs and reward
  pass the per-env gate against the float64 oracle stepped from the same
  input, done is exact, and a done env comes out at AutoReset's first state
  bit for bit."""
  from tests.test_gpu_parity import Envelope, _env_err, _gate
  desc, o64, qp0, act = _scene(oracle_lib, two_rows)
  env = _make_env(dev, monkeypatch, two_rows)
  u = env.unwrapped
  O, M = u.obs_size, len(u.metric_keys)
  env32 = Envelope(oracle_lib, None, desc=desc)
  st = _start(env, qp0, dev)
  first_qp, first_obs = st.info['first_qp'].numpy(), _np(st.info['first_obs'])
  steps = np.zeros(B)
  n_done = 0
  for t in range(K):
    qin = st.qp.numpy().astype(np.float32)
    steps = np.where(_np(st.done) != 0, 0, steps)
    st = env.step(st, torch.as_tensor(act[t], device=dev))
    ref, robs, rrew, rdone, _ = o64.env_step('ant', qin, act[t], O, M, coef=u.coef)
    outs = env32.env('ant', qin, act[t], O, M, 0, u.coef)
    steps = steps + 1
    done = np.where(steps >= EPISODE, 1.0, rdone)
    got, obs = st.qp.numpy(), _np(st.obs)
    assert np.array_equal(_np(st.done), done), (t, _np(st.done), done)
    assert np.array_equal(_np(st.info['steps']), steps), t
    _gate(_np(st.reward)[:, None], rrew[:, None], _env_err([o[2][:, None] for o in outs], rrew[:, None]),
          'reward')
    sel = done != 0
    n_done += int(sel.sum())
    assert np.array_equal(got[sel], first_qp[sel]) and np.array_equal(obs[sel], first_obs[sel]), t
    if (~sel).any():
      k = ~sel
      for f, sl in QP_FIELDS.items():
        _gate(got[k][..., sl], ref[k][..., sl],
              _env_err([o[0][k][..., sl] for o in outs], ref[k][..., sl]), f)
      _gate(obs[k], robs[k], _env_err([o[1][k] for o in outs], robs[k]), 'obs')
  assert n_done >= B  # every env ended an episode inside the run


def _trajectory(env, st0, acts):
  """K chained `env.step`s: per step (qp, obs, reward, done, steps)."""
  out, st = [], st0
  for t in range(acts.shape[0]):
    st = env.step(st, acts[t])
    out.append([torch.cat([st.qp.pos, st.qp.rot, st.qp.vel, st.qp.ang], -1), st.obs, st.reward,
                st.done, st.info['steps']])
  return [torch.stack(x) for x in zip(*out)]


@gpu
def test_rollout_launches_equal_chained_steps(dev, oracle_lib, monkeypatch):
  """The 12 steps as one `bx_env_rollout_packed` launch equal the chained
  steps bit for bit (tests/test_gpu_rollout.py `_check`: state, obs, reward,
  done, counters, metrics), a second chained run equals the first, and a
  start state given as four separate tensors (the unpacked `bx_env_step`
  kernel) gives the same bits."""
  import brax_amd
  from tests.test_gpu_rollout import _check
  _, _, qp0, act = _scene(oracle_lib, False)
  env = _make_env(dev, monkeypatch, False)
  st0 = _start(env, qp0, dev)
  acts = torch.as_tensor(act, device=dev)
  tr = _check(env, st0, acts)
  assert float(tr.done.sum()) >= B
  a, b = _trajectory(env, st0, acts), _trajectory(env, st0, acts)
  for x, y in zip(a, b):
    assert torch.equal(x, y)
  q = st0.qp
  loose = st0.replace(qp=brax_amd.QP(pos=q.pos.contiguous(), rot=q.rot.contiguous(),
                                     vel=q.vel.contiguous(), ang=q.ang.contiguous()))
  for x, y in zip(a, _trajectory(env, loose, acts)):
    assert torch.equal(x, y)


@gpu
def test_random_rollout_launch_equals_chained_steps(dev, oracle_lib, monkeypatch):
  """One `bx_env_rollout_random` launch (the actions drawn in the kernel)
  equals `env.step` chained over the same draws (`bx_uniform_slabs`)."""
  import ctypes as C
  from brax_amd import _native
  from brax_amd.envs.rollout import RolloutRunner
  _, _, qp0, _ = _scene(oracle_lib, False)
  env = _make_env(dev, monkeypatch, False)
  st0 = _start(env, qp0, dev)
  A = env.action_size
  seed, off, stride = 9, 500, 2 * B * A
  runner = RolloutRunner(env, st0, K, seed=seed, offset=off, step_stride=stride)
  assert runner.draw
  runner.run()
  got = runner.trajectory()
  acts = torch.empty((K, B, A), dtype=torch.float32, device=dev)
  _native.check(_native.lib().bx_uniform_slabs(
      C.c_void_p(acts.data_ptr()), B * A, K, seed, off, stride, None, 0, -1.0, 1.0,
      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
  qp, obs, reward, done, steps = _trajectory(env, st0, acts)
  torch.cuda.synchronize()
  assert torch.equal(runner.actions(), acts)
  assert torch.equal(got.qp[..., :13], qp) and torch.equal(got.obs, obs)
  assert torch.equal(got.reward, reward) and torch.equal(got.done, done)
  assert torch.equal(got.steps, steps)
  assert float(done.sum()) >= B
