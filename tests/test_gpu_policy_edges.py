"""The closed-loop rollout's paths that tests/test_gpu_policy_rollout.py does
not launch: the other env kinds (the Pusher kernel, the per-env rng stream,
A = 1), policy shapes at and between the limits (one layer, 8 x 128, width 1,
widths off the 4-word and 16-lane grids, tanh, min_std, the loc-only head),
batches below one workgroup, K = 1, a saturated head and the scale floor, the
chained path at every step, and the argument checks.

Every launch gets the checks of that module, unchanged: the teacher-forced
float64 `MLPPolicy.forward` on the observations the kernel read (raw, action,
log_prob within 8 x the float32 yardstick plus 1e-6), action = tanh(raw) to
2 ulp, and the open-loop `rollout` on the recorded actions bit for bit.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_policy_rollout import (_check_physics, _check_policy, _eps, _make, _policy,
                                           _weights)

pytestmark = pytest.mark.gpu

# the registry, split as DESIGN.md's closed-loop section lists it
FUSABLE = {'acrobot', 'ant', 'fetch', 'halfcheetah', 'hopper', 'inverted_pendulum',
           'inverted_double_pendulum', 'pusher', 'reacher', 'ur5e', 'walker2d'}
REFUSED = {'reacherangle', 'swimmer', 'grasp', 'humanoid', 'humanoidstandup',  # read the action row
           'fast'}  # no kernel env at all


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _mlp(env, dev, hidden, seed=11, loc_only=False, **kw):
  from brax_amd.envs.policy import MLPPolicy
  O, A = env.observation_size, env.action_size
  return MLPPolicy(_weights((O,) + tuple(hidden) + (A if loc_only else 2 * A,), seed), device=dev,
                   **kw)


def _launch(env, st0, policy, K, seed=5, offset=1000, **kw):
  from brax_amd.envs.policy import policy_rollout
  out = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, fused=True, **kw)
  torch.cuda.synchronize()
  return out


def _checks(dev, env, st0, policy, K, label, final, tr, ex, seed=5, offset=1000, expect_done=True):
  """The full check of one fused launch; returns the worst ratio."""
  B, A = st0.obs.shape[0], env.action_size
  if expect_done:
    assert float(tr.done.sum()) > 0
  assert tuple(ex.action.shape) == (K, B, A) and tuple(ex.raw_action.shape) == (K, B, A)
  assert tuple(ex.log_prob.shape) == (K, B)
  assert torch.isfinite(ex.action).all() and torch.isfinite(ex.log_prob).all()
  eps = (torch.zeros((K, B, A), device=dev) if policy.deterministic
         else _eps(dev, K, B, A, seed, offset))
  worst = _check_policy(policy, st0, tr, ex, eps, label)
  _check_physics(env, st0, tr, ex)
  assert torch.equal(final.obs, tr.obs[-1]) and torch.equal(final.done, tr.done[-1])
  print(f'{label}: worst ratio {worst:.2f}')
  return worst


def _run(dev, env, st0, policy, K, label, expect_done=True, **kw):
  """One fused launch and the full check; returns (tr, ex, worst ratio)."""
  final, tr, ex = _launch(env, st0, policy, K, **kw)
  return tr, ex, _checks(dev, env, st0, policy, K, label, final, tr, ex, expect_done=expect_done)


# --------------------------------------------------------------- D1: env kinds
@pytest.mark.parametrize('name,B,K,ep,ar', [
    ('pusher', 21, 8, 3, 1),
    ('reacher', 21, 8, 3, 1),
    ('fetch', 21, 8, 3, 1),
    ('ur5e', 21, 8, 3, 1),
    ('ur5e', 21, 6, 4, 2),
    ('walker2d', 21, 8, 3, 1),
    ('inverted_pendulum', 21, 8, 3, 1),  # A = 1
    ('inverted_double_pendulum', 21, 8, 3, 1),
    ('acrobot', 21, 8, 3, 1),
])
def test_env_kinds(dev, name, B, K, ep, ar):
  from brax_amd.envs.rollout import chain_options
  env, st0 = _make(dev, name, B, ep, ar)
  u, _ = chain_options(env)
  print(f'{name}: lanes per env {u.sys.lanes}, obs {u.obs_size}, actions {u.action_size}, '
        f'per-env rng stream {bool(getattr(u, "needs_rng", False))}')
  policy = _policy(env, dev)
  tr, _, _ = _run(dev, env, st0, policy, K, f'{name}/{B}/ar{ar}')
  if name in ('fetch', 'ur5e'):
    # the target envs' stream: one draw per env step, action repeats included
    assert tr.rng is not None and tuple(tr.rng.shape) == (K, B)
    rng0 = st0.info['rng']
    assert rng0 is not None
    prev = torch.cat([rng0[None], tr.rng[:-1]]).long()
    assert torch.equal((prev + ar) & 0xFFFFFFFF, tr.rng.long() & 0xFFFFFFFF)
  else:
    # (Reacher places its target at reset only: it carries no stream)
    assert not getattr(u, 'needs_rng', False) and tr.rng is None


# -------------------------------------------------- D2: registry completeness
def test_registry_is_classified():
  from brax_amd import envs
  assert set(envs._envs) == FUSABLE | REFUSED and not FUSABLE & REFUSED  # pylint: disable=protected-access


@pytest.mark.parametrize('name', sorted(FUSABLE | REFUSED))
def test_registry_fused_or_chained(dev, name):
  """`fused_supported` is None exactly for the fusable kinds; fused=None runs
  every env (the others through the chained path)."""
  from brax_amd import envs
  from brax_amd.envs.policy import fused_supported, policy_rollout
  env = envs.create(name, batch_size=8, episode_length=1000, auto_reset=True, device=dev)
  st0 = env.reset(np.array([1, 2], np.uint32))
  policy = _policy(env, dev, (16,))
  why = fused_supported(env, policy)
  print(f'{name}: {why!r}')
  if name in FUSABLE:
    assert why is None, why
  else:
    assert isinstance(why, str) and why.strip()
    with pytest.raises(NotImplementedError):
      policy_rollout(env, st0, policy, 2, seed=3, fused=True)
  B = st0.obs.shape[0]
  final, tr, ex = policy_rollout(env, st0, policy, 2, seed=3)
  torch.cuda.synchronize()
  assert tuple(tr.obs.shape) == (2, B, env.observation_size)
  assert tuple(ex.action.shape) == (2, B, env.action_size) and tuple(ex.log_prob.shape) == (2, B)
  for t in (tr.obs, tr.reward, tr.done, ex.action, ex.raw_action, ex.log_prob, final.obs):
    assert torch.isfinite(t).all()


# ------------------------------------------------------- D3: policy shapes
@pytest.mark.parametrize('hidden,kw', [
    ((), {}),                             # one dense layer, obs to head
    ((128,) * 7, {}),                     # 8 layers at the width limit, weights in global memory
    ((1,), {}),
    ((33, 7, 127), {}),                   # scalar tail in n_in, ragged n_out over the 16 lanes
    ((17,), {'activation': 'tanh'}),
    ((32, 32), {'min_std': 0.5}),
    ((32, 32), {'deterministic': True, 'loc_only': True}),
], ids=['none', '128x7', '1', '33-7-127', '17-tanh', 'min_std', 'loc_only'])
def test_policy_shapes(dev, hidden, kw):
  from brax_amd.envs.policy import fused_supported
  env, st0 = _make(dev, 'ant', 20, 3, 1)
  policy = _mlp(env, dev, hidden, **kw)
  assert fused_supported(env, policy) is None
  assert len(policy.sizes) == len(hidden) + 1
  if kw.get('loc_only'):
    assert policy.sizes[-1][1] == env.action_size
  _run(dev, env, st0, policy, 6, f'ant/hidden {hidden} {kw}')


# ------------------------------------------------ D4: batch and step edges
@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('B', [1, 3])
def test_small_batch_writes_nothing_past_it(dev, B, K):
  """Fewer envs than a workgroup holds: the absent envs' lanes write nothing.
  `out` and the extras carry a guard row of sentinels past the exact-size
  views the call gets."""
  from brax_amd.envs.policy import PolicyExtras
  from brax_amd.envs.rollout import chain_options
  ep = 3
  env, st0 = _make(dev, 'ant', B, ep, 1)
  u, _ = chain_options(env)
  A = env.action_size
  block = B * (u.sys.num_bodies * 16 + u.obs_size + 4 + len(u.metric_keys))
  S = -777.0
  out = torch.full((K * block + block,), S, dtype=torch.float32, device=dev)
  act = torch.full((K + 1, B, A), S, dtype=torch.float32, device=dev)
  raw = torch.full((K + 1, B, A), S, dtype=torch.float32, device=dev)
  lp = torch.full((K + 1, B), S, dtype=torch.float32, device=dev)
  ex_in = PolicyExtras(action=act[:K], raw_action=raw[:K], log_prob=lp[:K])
  policy = _policy(env, dev)
  tr, ex, _ = _run(dev, env, st0, policy, K, f'ant/B{B}/K{K}', expect_done=K >= ep,
                   out=out[:K * block], extras=ex_in)
  assert ex.action.data_ptr() == act.data_ptr() and tr.qp.data_ptr() == out.data_ptr()
  for nm, guard in (('out', out[K * block:]), ('action', act[K]), ('raw_action', raw[K]),
                    ('log_prob', lp[K])):
    assert bool((guard == S).all()), nm
  # and every word of the views was written
  for nm, t in (('action', act[:K]), ('raw_action', raw[:K]), ('log_prob', lp[:K]),
                ('obs', tr.obs), ('reward', tr.reward), ('done', tr.done)):
    assert not bool((t == S).any()), nm


# ----------------------------------------------------- D5: saturated head
def _forward64(policy, st0, tr, eps):
  obs_prev = torch.cat([st0.obs[None], tr.obs[:-1]]).cpu().double()
  return policy.forward(obs_prev, eps.cpu().double())


def test_saturated_head(dev):
  """The loc half of the last layer scaled until most |raw| pass 9, where
  float32 tanh is +-1 and the log-det is 2 ln 2 - 2 |raw|."""
  from brax_amd.envs.policy import MLPPolicy
  env, st0 = _make(dev, 'ant', 20, 3, 1)
  O, A, K, B = env.observation_size, env.action_size, 6, 20
  layers = _weights((O, 32, 32, 32, 32, 2 * A), 11)
  # the factor from the reset observations alone: the median |loc| to 40
  base = MLPPolicy(layers, device='cpu')
  _, _, _, lg = base.forward(st0.obs.cpu().double())
  factor = 40.0 / float(lg[:, :A].abs().median())
  w, b = layers[-1]
  w, b = w.clone(), b.clone()
  w[:, :A] *= factor
  b[:A] *= factor
  policy = MLPPolicy(layers[:-1] + [(w, b)], device=dev)
  final, tr, ex = _launch(env, st0, policy, K)
  eps = _eps(dev, K, B, A, 5, 1000)
  _, r64, _, _ = _forward64(policy, st0, tr, eps)
  share = float((r64.abs() > 9.0).double().mean())
  print(f'saturated head: factor {factor:.1f}, share of |raw| > 9 {share:.3f}, '
        f'max |raw| {float(r64.abs().max()):.1f}')
  assert share >= 0.5  # a condition on the input, before the kernel's outputs are read
  _checks(dev, env, st0, policy, K, 'ant/saturated', final, tr, ex)
  t = torch.tanh(ex.raw_action.cpu().double()).float()
  one = t.abs() == 1.0
  # (float32 tanh is 1 past 13 ln 2 = 9.011; the recorded raw is within the
  # check's bound of r64, far below the 0.09 to spare)
  assert bool(one[r64.abs() > 9.1].all()) and float(one.double().mean()) > 0
  assert torch.equal(ex.action.cpu()[one], t[one])
  assert torch.isfinite(ex.log_prob).all()


def test_scale_floor(dev):
  """The scale half's biases at -30 under min_std = 1e-3: softplus underflows
  to 1e-13 and the scale is the floor."""
  from brax_amd.envs.policy import MLPPolicy
  env, st0 = _make(dev, 'ant', 20, 3, 1)
  O, A, K, B = env.observation_size, env.action_size, 6, 20
  layers = _weights((O, 32, 32, 32, 32, 2 * A), 11)
  w, b = layers[-1]
  b = b.clone()
  b[A:] = -30.0
  policy = MLPPolicy(layers[:-1] + [(w, b)], min_std=1e-3, device=dev)
  final, tr, ex = _launch(env, st0, policy, K)
  eps = _eps(dev, K, B, A, 5, 1000)
  _, _, _, lg = _forward64(policy, st0, tr, eps)
  scale = torch.nn.functional.softplus(lg[..., A:]) + 1e-3
  gap = float((scale - 1e-3).abs().max())
  print(f'scale floor: max |scale - min_std| {gap:.3e}')
  assert gap <= 1e-12  # a condition on the input
  _checks(dev, env, st0, policy, K, 'ant/scale floor', final, tr, ex)


# ------------------------------------------ D6: chained path, teacher-forced
@pytest.mark.parametrize('name,fused', [('humanoid', None), ('ant', False)])
def test_chained_path_every_step(dev, name, fused):
  from brax_amd.envs.policy import policy_rollout
  B, K = 32, 4
  env, st0 = _make(dev, name, B, 3, 1)
  A = env.action_size
  policy = _policy(env, dev, (32, 32))
  seed, offset = 4, 77
  final, tr, ex = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, fused=fused)
  torch.cuda.synchronize()
  assert float(tr.done.sum()) > 0
  eps = _eps(dev, K, B, A, seed, offset)
  for t in range(K):
    obs = st0.obs if t == 0 else tr.obs[t - 1]
    a, r, lp, _ = policy.forward(obs, eps[t])
    assert torch.equal(ex.action[t], a), t
    assert torch.equal(ex.raw_action[t], r), t
    assert torch.equal(ex.log_prob[t], lp), t
  _check_physics(env, st0, tr, ex)
  assert torch.equal(final.obs, tr.obs[-1])


# ------------------------------------- D7: argument checks before any launch
def test_argument_checks(dev):
  from brax_amd.envs.policy import PolicyExtras, fused_supported, policy_rollout
  from brax_amd.envs.rollout import chain_options
  B, K = 8, 3
  env, st0 = _make(dev, 'ant', B, 1000, 1)
  u, _ = chain_options(env)
  A = env.action_size
  policy = _policy(env, dev)
  block = B * (u.sys.num_bodies * 16 + u.obs_size + 4 + len(u.metric_keys))

  def extras(lp):
    return PolicyExtras(action=torch.empty((K, B, A), device=dev),
                        raw_action=torch.empty((K, B, A), device=dev), log_prob=lp)
  with pytest.raises(ValueError):
    policy_rollout(env, st0, policy, K, fused=True,
                   out=torch.empty((K * block - 1,), dtype=torch.float32, device=dev))
  with pytest.raises(ValueError):
    policy_rollout(env, st0, policy, K, fused=True, extras=extras(torch.empty((K, B + 1), device=dev)))
  with pytest.raises(ValueError):
    policy_rollout(env, st0, policy, K, fused=True, extras=extras(torch.empty((B, K), device=dev)))
  with pytest.raises(ValueError):  # the right shape, not contiguous
    policy_rollout(env, st0, policy, K, fused=True, extras=extras(torch.empty((B, K), device=dev).t()))
  for fused in (None, True, False):
    with pytest.raises(ValueError):
      policy_rollout(env, st0, policy, 0, fused=fused)
  # the exact size passes
  policy_rollout(env, st0, policy, K, fused=True,
                 out=torch.empty((K * block,), dtype=torch.float32, device=dev),
                 extras=extras(torch.empty((K, B), device=dev)))
  torch.cuda.synchronize()
  why = fused_supported(env, _policy(env, torch.device('cpu')))
  assert isinstance(why, str) and 'cpu' in why
  from brax_amd.envs.policy import MLPPolicy
  other = MLPPolicy(_weights((env.observation_size + 1, 16, 2 * A), 0), device=dev)
  why = fused_supported(env, other)
  assert isinstance(why, str) and str(env.observation_size + 1) in why
  with pytest.raises(NotImplementedError):
    policy_rollout(env, st0, other, K, fused=True)
