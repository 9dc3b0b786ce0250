"""Closed-loop rollouts (`brax_amd.envs.policy.policy_rollout`, one
`bx_env_rollout_policy` launch for K steps of policy + env).

A chaotic simulator diverges under rounding, so nothing here compares a fused
trajectory with a chained one step for step; the checks are teacher-forced on
the kernel's own recorded outputs:

* policy evaluation: `MLPPolicy.forward` in float64 on the observations the
  kernel read (state.obs, then traj.obs[t - 1]) with the noise of
  `bx_normal_slabs` must give the recorded raw action, action and log_prob.
  The tolerance is measured, not fixed: the yardstick is torch's float32 CPU
  `forward` on the same inputs against the float64 one (largest absolute
  error over the batch); the kernel may be within 8 x that plus 1e-6 (another
  summation order, fast exp / rcp). Each figure is printed before it is
  asserted.
* recorded action == tanh(recorded raw) to 2 float32 ulp (tanh in float64).
* physics unchanged: the open-loop `rollout` on the recorded actions
  reproduces the fused trajectory bit for bit.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _weights(sizes, seed):
  """lecun-uniform kernels (U(+-sqrt(3 / fan_in))) and small biases from a
  seeded CPU generator."""
  g = torch.Generator(device='cpu').manual_seed(seed)
  out = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    lim = math.sqrt(3.0 / i)
    out.append(((torch.rand((i, o), generator=g) * 2 - 1) * lim,
                (torch.rand((o,), generator=g) * 2 - 1) * 0.1))
  return out


def _policy(env, dev, hidden=(32,) * 4, activation='swish', norm=False, seed=11,
            deterministic=False):
  from brax_amd.envs.policy import MLPPolicy
  O, A = env.observation_size, env.action_size
  kw = {}
  if norm:
    g = torch.Generator(device='cpu').manual_seed(seed + 1)
    kw = dict(obs_mean=torch.rand((O,), generator=g) - 0.5,
              obs_std=torch.rand((O,), generator=g) + 0.5)
  return MLPPolicy(_weights((O,) + tuple(hidden) + (2 * A,), seed), activation=activation,
                   deterministic=deterministic, device=dev, **kw)


def _make(dev, name, B, ep, ar, reset_seed=(2, 9)):
  from brax_amd import envs
  env = envs.create(name, batch_size=B, episode_length=ep, action_repeat=ar, auto_reset=True,
                    device=dev)
  return env, env.reset(np.array(reset_seed, np.uint32))


def _eps(dev, K, B, A, seed, offset, stride=None):
  from brax_amd.envs.policy import normal_slabs
  eps = torch.empty((K, B, A), dtype=torch.float32, device=dev)
  normal_slabs(eps, B * A, K, seed, offset, 2 * B * A if stride is None else stride)
  return eps


def _check_policy(policy, st0, tr, ex, eps, label):
  """The teacher-forced policy check; returns the worst kernel / yardstick
  ratio."""
  obs_prev = torch.cat([st0.obs[None], tr.obs[:-1]]).cpu()
  e = eps.cpu()
  a64, r64, l64, _ = policy.forward(obs_prev.double(), e.double())
  a32, r32, l32, _ = policy.forward(obs_prev, e)
  worst = 0.0
  for nm, got, f32, f64 in (('raw', ex.raw_action, r32, r64), ('action', ex.action, a32, a64),
                            ('log_prob', ex.log_prob, l32, l64)):
    err = float((got.cpu().double() - f64).abs().max())
    yard = float((f32.double() - f64).abs().max())
    print(f'{label} {nm}: kernel err {err:.3e}  float32 yardstick {yard:.3e}  '
          f'ratio {err / max(yard, 1e-30):.2f}')
    worst = max(worst, err / max(yard, 1e-30))
    assert err <= 8 * yard + 1e-6, (label, nm, err, yard)
  # action = tanh(raw) to 2 ulp of the float32 result
  raw = ex.raw_action.cpu()
  t64 = torch.tanh(raw.double())
  ulp = torch.from_numpy(np.spacing(np.abs(t64.float().numpy()).astype(np.float32))).double()
  off = ((ex.action.cpu().double() - t64).abs() / ulp).max()
  print(f'{label} action vs tanh(raw): {float(off):.2f} ulp')
  assert float(off) <= 2.0, (label, float(off))
  return worst


def _check_physics(env, st0, tr, ex):
  """The open-loop kernel on the recorded actions: the same bits."""
  from brax_amd.envs.rollout import rollout
  _, ref = rollout(env, st0, ex.action)
  # (words 13..15 of a packed qp record are padding no kernel writes)
  assert torch.equal(tr.qp[..., :13], ref.qp[..., :13]), 'qp'
  for f in ('obs', 'reward', 'done', 'steps', 'truncation', 'metrics'):
    assert torch.equal(getattr(tr, f), getattr(ref, f)), f
  assert (tr.rng is None) == (ref.rng is None)
  if tr.rng is not None:
    assert torch.equal(tr.rng, ref.rng)


@pytest.mark.parametrize('name,B,K,ep,ar,hidden,activation,norm', [
    ('ant', 64, 9, 4, 1, (32,) * 4, 'swish', True),
    # B not a multiple of 4, widths not a multiple of 16: the env and lane tails
    ('ant', 61, 7, 3, 2, (24, 40), 'relu', False),
    ('halfcheetah', 64, 8, 3, 1, (32,) * 4, 'swish', False),
    ('hopper', 64, 8, 4, 1, (32,) * 4, 'swish', False),  # an EK_ANY variant
])
def test_fused_policy_rollout(dev, name, B, K, ep, ar, hidden, activation, norm):
  from brax_amd.envs.policy import policy_rollout
  env, st0 = _make(dev, name, B, ep, ar)
  policy = _policy(env, dev, hidden, activation, norm)
  seed, offset = 5, 1000
  final, tr, ex = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, fused=True)
  torch.cuda.synchronize()
  # the episodes ended inside the launch: the policy read a post-reset
  # observation (first_obs) there
  assert float(tr.done.sum()) > 0
  assert tuple(ex.action.shape) == (K, B, env.action_size) and tuple(ex.log_prob.shape) == (K, B)
  assert torch.isfinite(ex.action).all() and torch.isfinite(ex.log_prob).all()
  eps = _eps(dev, K, B, env.action_size, seed, offset)
  _check_policy(policy, st0, tr, ex, eps, f'{name}/{B}')
  _check_physics(env, st0, tr, ex)
  assert torch.equal(final.obs, tr.obs[-1]) and torch.equal(final.done, tr.done[-1])


def test_fused_policy_rollout_full_batch_ant(dev):
  """4,096 Ant envs, 20 steps, the default PPO policy, in one launch."""
  from brax_amd import envs
  from brax_amd.envs.policy import policy_rollout
  env = envs.create('ant', batch_size=4096, episode_length=1000, auto_reset=True, device=dev)
  st0 = env.reset(np.array([0, 0x5EED], np.uint32))
  policy = _policy(env, dev, norm=True)
  _, tr, ex = policy_rollout(env, st0, policy, 20, seed=3, fused=True)
  eps = _eps(dev, 20, 4096, 8, 3, 0)
  _check_policy(policy, st0, tr, ex, eps, 'ant/4096')
  _check_physics(env, st0, tr, ex)


def test_deterministic_mode(dev):
  """raw = loc, action = tanh(loc), the seed unused; log_prob is the mode's
  (eps = 0), as `forward` computes it."""
  from brax_amd.envs.policy import policy_rollout
  env, st0 = _make(dev, 'ant', 64, 4, 1)
  policy = _policy(env, dev, norm=True, deterministic=True)
  _, tr, ex = policy_rollout(env, st0, policy, 6, seed=1, fused=True)
  _, tr2, ex2 = policy_rollout(env, st0, policy, 6, seed=77, offset=12345, fused=True)
  for a, b in ((ex.action, ex2.action), (ex.raw_action, ex2.raw_action),
               (ex.log_prob, ex2.log_prob), (tr.qp[..., :13], tr2.qp[..., :13]), (tr.obs, tr2.obs)):
    assert torch.equal(a, b)
  zeros = torch.zeros_like(ex.action)
  _check_policy(policy, st0, tr, ex, zeros, 'ant/deterministic')
  _check_physics(env, st0, tr, ex)


def test_normal_slabs(dev):
  from brax_amd.envs.policy import normal_slabs
  n = 1 << 20
  x = normal_slabs(torch.empty((n,), dtype=torch.float32, device=dev), n, 1, 7, 3, 0)
  y = normal_slabs(torch.empty((n,), dtype=torch.float32, device=dev), n, 1, 7, 3, 0)
  assert torch.equal(x, y)
  assert torch.isfinite(x).all()
  mean, std = float(x.double().mean()), float(x.double().std())
  print(f'normal_slabs n={n}: mean {mean:.3e} std {std:.5f}')
  assert abs(mean) <= 5e-3 and abs(std - 1.0) <= 5e-3
  assert not torch.equal(x, normal_slabs(torch.empty_like(x), n, 1, 8, 3, 0))
  # shard independence: a 128-env batch's noise as two 64-env calls with the
  # offset advanced by 64 * A * 2
  A, K = 8, 3
  stride = 2 * 128 * A
  whole = _eps(dev, K, 128, A, 9, 40, stride)
  lo = _eps(dev, K, 64, A, 9, 40, stride)
  hi = _eps(dev, K, 64, A, 9, 40 + 64 * A * 2, stride)
  assert torch.equal(whole[:, :64], lo) and torch.equal(whole[:, 64:], hi)


def test_nan_observation(dev):
  """A non-finite observation gives that env a non-finite action (as jnp
  does) and touches no other env."""
  from brax_amd.envs.policy import policy_rollout
  env, st0 = _make(dev, 'ant', 64, 4, 1)
  policy = _policy(env, dev, norm=True)
  _, tr, ex = policy_rollout(env, st0, policy, 6, seed=2, fused=True)
  obs = st0.obs.clone()
  obs[5, 3] = float('nan')
  _, trn, exn = policy_rollout(env, st0.replace(obs=obs), policy, 6, seed=2, fused=True)
  assert not torch.isfinite(exn.action[0, 5]).any()
  keep = torch.arange(64, device=dev) != 5
  for a, b in ((tr.qp[..., :13], trn.qp[..., :13]), (tr.obs, trn.obs), (tr.reward, trn.reward), (tr.done, trn.done),
               (ex.action, exn.action), (ex.raw_action, exn.raw_action),
               (ex.log_prob, exn.log_prob)):
    assert torch.equal(a[:, keep], b[:, keep])


def test_refusals_and_fallback(dev):
  from brax_amd import envs
  from brax_amd.envs.policy import MLPPolicy, fused_supported, policy_rollout
  env = envs.create('humanoid', batch_size=32, episode_length=1000, auto_reset=True, device=dev)
  st0 = env.reset(np.array([1, 2], np.uint32))
  policy = _policy(env, dev, (32, 32))
  with pytest.raises(NotImplementedError):
    policy_rollout(env, st0, policy, 3, fused=True)
  # the chained path: bx_normal_slabs, policy.forward, env.step per step
  final, tr, ex = policy_rollout(env, st0, policy, 3, seed=4)
  assert tuple(tr.obs.shape) == (3, 32, env.observation_size)
  assert tuple(tr.qp.shape)[:2] == (3, 32) and tuple(tr.reward.shape) == (3, 32)
  assert tuple(ex.action.shape) == (3, 32, env.action_size) and tuple(ex.log_prob.shape) == (3, 32)
  for t in (tr.obs, tr.reward, ex.action, ex.raw_action, ex.log_prob, final.obs):
    assert torch.isfinite(t).all()
  eps = _eps(dev, 3, 32, env.action_size, 4, 0)
  a, _, _, _ = policy.forward(st0.obs, eps[0])
  assert torch.equal(ex.action[0], a)
  # past the documented limits (8 layers, widths <= 128): refused, no launch
  ant, sa = _make(dev, 'ant', 64, 4, 1)
  wide = _policy(ant, dev, (129,))
  deep = _policy(ant, dev, (16,) * 8)
  for p in (wide, deep):
    assert fused_supported(ant, p) is not None
    with pytest.raises(NotImplementedError):
      policy_rollout(ant, sa, p, 2, fused=True)
  # a head that is not 2 x action_size wide
  with pytest.raises((ValueError, NotImplementedError)):
    policy_rollout(ant, sa, MLPPolicy(_weights((ant.observation_size, 16, 7), 0), device=dev), 2,
                   fused=True)
  # fused=False: the chained path on a fusable env too
  _, trc, exc = policy_rollout(ant, sa, _policy(ant, dev), 2, seed=4, fused=False)
  assert tuple(trc.obs.shape) == (2, 64, ant.observation_size) and torch.isfinite(exc.log_prob).all()
  torch.cuda.synchronize()


def test_graph_capture_and_in_place_weights(dev):
  """One fused call captured on a single stream replays the eager call's
  bits, and sees weights loaded in place."""
  from brax_amd.envs.policy import PolicyExtras, policy_rollout
  env, st0 = _make(dev, 'ant', 64, 4, 1)
  policy = _policy(env, dev, norm=True, seed=11)
  K, B, A = 5, 64, env.action_size
  _, tr_e, ex_e = policy_rollout(env, st0, policy, K, seed=6, fused=True)
  block = B * (tr_e.qp.shape[2] * 16 + tr_e.obs.shape[2] + 4 + tr_e.metrics.shape[2])
  out = torch.empty((K * block,), dtype=torch.float32, device=dev)
  ex = PolicyExtras(action=torch.empty((K, B, A), device=dev),
                    raw_action=torch.empty((K, B, A), device=dev),
                    log_prob=torch.empty((K, B), device=dev))
  with torch.cuda.device(dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      policy_rollout(env, st0, policy, K, seed=6, fused=True, out=out, extras=ex)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
      _, tr_g, ex_g = policy_rollout(env, st0, policy, K, seed=6, fused=True, out=out, extras=ex)
    torch.cuda.current_stream(dev).synchronize()
  out.zero_()
  ex.action.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert ex_g.action is ex.action
  for a, b in ((ex_g.action, ex_e.action), (ex_g.raw_action, ex_e.raw_action),
               (ex_g.log_prob, ex_e.log_prob), (tr_g.qp[..., :13], tr_e.qp[..., :13]), (tr_g.obs, tr_e.obs),
               (tr_g.reward, tr_e.reward), (tr_g.done, tr_e.done)):
    assert torch.equal(a, b)
  # new weights in place, at the same address: the replay reads them
  old = ex_g.action.clone()
  ptr = policy.params.data_ptr()
  policy.load_(_weights((env.observation_size, 32, 32, 32, 32, 2 * A), 99))
  assert policy.params.data_ptr() == ptr
  graph.replay()
  torch.cuda.synchronize()
  assert not torch.equal(ex_g.action, old)
  got = (ex_g.action.clone(), ex_g.log_prob.clone(), tr_g.qp.clone())
  _, tr_n, ex_n = policy_rollout(env, st0, policy, K, seed=6, fused=True)
  assert torch.equal(got[0], ex_n.action) and torch.equal(got[1], ex_n.log_prob)
  assert torch.equal(got[2][..., :13], tr_n.qp[..., :13])


@pytest.mark.parametrize('name', ['pusher', 'halfcheetah'])
def test_fused_policy_rollout_from_contact_states(dev, oracle_lib, name):
  """The fused policy kernel from the mid-episode fixtures' start states
  (contact rows at work, tests/golden/mid_<name>.npz) with one small MLP:
  the teacher-forced policy check, the open-loop kernel's bits on the
  recorded actions, and the target rows penetrate inside the trajectory."""
  from brax_amd.envs.policy import policy_rollout
  from tests.test_gpu_rollout import contact_start, target_rows_penetrate
  env, st0, acts, T = contact_start(name, dev)
  B, K = acts.shape[1], 3
  st0 = st0.replace(obs=env.observe(st0.qp, torch.zeros((B, env.action_size), device=dev)))
  policy = _policy(env, dev, (32, 32))
  seed, offset = 5, 1000
  final, tr, ex = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, fused=True)
  torch.cuda.synchronize()
  assert torch.isfinite(ex.action).all() and torch.isfinite(tr.obs).all()
  eps = _eps(dev, K, B, env.action_size, seed, offset)
  _check_policy(policy, st0, tr, ex, eps, f'{name}/mid')
  _check_physics(env, st0, tr, ex)
  # the policy's actions are not the fixture's, so the set of rows may differ
  # from the recorded one: at least half of the fixture's active target rows
  # penetrate in the closed-loop trajectory (HalfCheetah: its one row, on at
  # least 4 envs)
  from tests.test_gpu_rollout import fixture_rows
  rows, envs = target_rows_penetrate(oracle_lib, name, T, st0, tr, ex.action)
  assert 2 * len(rows & fixture_rows(T)) >= len(fixture_rows(T)), (rows, fixture_rows(T))
  assert name != 'halfcheetah' or envs[0] >= 4, envs
