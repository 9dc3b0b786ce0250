"""`brax_amd.training` on the GPU.

Every GAE comparison is bit for bit against the chained form (`fused=False`)
on the same device tensors: `torch.equal` on the finite values plus equal NaN
masks. The kernel loads its inputs in chunks of 8 time steps (`GAE_CHUNK`,
`brax_amd/csrc/train_launch.h`): T = 1, 2 and 7 run the tail path alone, 8 and
16 whole chunks alone, 33 four chunks and a tail of one.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAE_CHUNK = 8


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _same(got, want, what=''):
  assert got.shape == want.shape and got.dtype == want.dtype, what
  nan = want.isnan()
  assert torch.equal(got.isnan(), nan), f'{what}: NaN masks differ'
  zero = torch.zeros_like(want)
  assert torch.equal(torch.where(nan, zero, got), torch.where(nan, zero, want)), what


def _inputs(T, B, dev, seed=0):
  """Random float32 rewards / values, random 0 / 1 flags with truncation <=
  done; env 0 is done at t = 0, env 1 at t = T - 1, env 2 truncated at T - 1."""
  g = torch.Generator().manual_seed(seed * 1000 + T * 131 + B)
  done = (torch.rand((T, B), generator=g) < 0.3).float()
  trunc = done * (torch.rand((T, B), generator=g) < 0.5).float()
  done[0, 0] = 1
  if B > 1:
    done[T - 1, 1] = 1
    trunc[T - 1, 1] = 0
  if B > 2:
    done[T - 1, 2] = trunc[T - 1, 2] = 1
  reward = torch.randn((T, B), generator=g) * 3
  values = torch.randn((T, B), generator=g) * 10
  boot = torch.randn((B,), generator=g) * 10
  return [x.to(dev) for x in (trunc, done, reward, values, boot)]


def _both(args, **kw):
  from brax_amd.training import compute_gae
  got = compute_gae(*args, fused=True, **kw)
  want = compute_gae(*args, fused=False, **kw)
  return got, want


@pytest.mark.parametrize('T', [1, 2, 7, GAE_CHUNK, 2 * GAE_CHUNK, 33])
def test_gae_equals_the_chained_form(dev, T):
  for B in (1, 63, 65, 130):  # a ragged wave, a second workgroup
    args = _inputs(T, B, dev)
    for lam in (0.0, 0.95, 1.0):
      got, want = _both(args, lambda_=lam, discount=0.97, reward_scaling=0.1)
      for g_, w_, nm in zip(got, want, ('vs', 'advantages')):
        assert torch.isfinite(w_).all()
        _same(g_, w_, f'T={T} B={B} lambda={lam} {nm}')
        assert not g_.requires_grad
  # the defaults (lambda 1, discount 0.99, no scaling), values carrying a graph
  args = _inputs(T, 65, dev, seed=1)
  args[3].requires_grad_()
  got, want = _both(args)
  _same(got[0], want[0]), _same(got[1], want[1])


def test_gae_strides(dev):
  from brax_amd.training import compute_gae
  T, B, pad = 11, 70, 3
  args = _inputs(T, B, dev, seed=2)
  kw = dict(lambda_=0.95, discount=0.97, reward_scaling=0.1)
  want = compute_gae(*args, fused=False, **kw)
  # [B, T] views of the inputs, time-major outputs
  bt = [a.t().contiguous().t() for a in args[:4]]
  assert bt[0].stride() == (1, T)
  got = compute_gae(*bt, args[4], fused=True, **kw)
  _same(got[0], want[0], 'bt vs'), _same(got[1], want[1], 'bt adv')
  # mixed input layouts, and outputs laid out [B, T]
  out = (torch.empty((B, T), device=dev).t(), torch.empty((B, T), device=dev).t())
  got = compute_gae(bt[0], args[1], bt[2], args[3], args[4], fused=True, out=out, **kw)
  assert got[0].data_ptr() == out[0].data_ptr() and got[0].stride() == (1, T)
  _same(got[0], want[0], 'out bt vs'), _same(got[1], want[1], 'out bt adv')
  # everything a column and row slice of wider buffers, sentinels all round
  wide = [torch.full((T + 2, B + 2 * pad), -7.25, device=dev) for _ in range(6)]
  view = [w[1:T + 1, pad:pad + B] for w in wide]
  for v, a in zip(view[:4], args[:4]):
    v.copy_(a)
  got = compute_gae(*view[:4], args[4], fused=True, out=(view[4], view[5]), **kw)
  _same(got[0], want[0], 'slice vs'), _same(got[1], want[1], 'slice adv')
  for w in wide[4:]:
    frame = w.clone()
    frame[1:T + 1, pad:pad + B] = -7.25
    assert torch.equal(frame, torch.full_like(frame, -7.25)), 'a sentinel was written'
  for w, a in zip(wide[:4], args[:4]):  # the inputs are only read
    assert torch.equal(w[1:T + 1, pad:pad + B], a)
  # a broadcast (zero-stride) input
  zeros = torch.zeros((1, 1), device=dev).expand(T, B)
  got = compute_gae(zeros, zeros, args[2], args[3], args[4], fused=True, **kw)
  want0 = compute_gae(zeros, zeros, args[2], args[3], args[4], fused=False, **kw)
  _same(got[0], want0[0]), _same(got[1], want0[1])


def test_gae_non_finite_inputs_stay_in_their_env(dev):
  T, B = 9, 67
  clean = _inputs(T, B, dev, seed=3)
  clean[0][:, 40:] = 0  # envs 40.. : no flags, the poison travels the whole sequence
  clean[1][:, 40:] = 0
  dirty = [a.clone() for a in clean]
  e_nan, e_inf, e_boot, e_masked = 41, 50, 66, 5
  dirty[2][2, e_nan] = float('nan')
  dirty[3][0, e_inf] = float('inf')
  dirty[4][e_boot] = float('nan')
  # a NaN reward on a truncated step: NaN * 0 stays NaN
  dirty[0][4, e_masked] = dirty[1][4, e_masked] = 1
  clean[0][4, e_masked] = clean[1][4, e_masked] = 1
  dirty[2][4, e_masked] = float('nan')
  kw = dict(lambda_=0.95, discount=0.97, reward_scaling=0.1)
  got, want = _both(dirty, **kw)
  base, _ = _both(clean, **kw)
  poisoned = [e_nan, e_inf, e_boot, e_masked]
  others = [e for e in range(B) if e not in poisoned]
  for g_, w_, b_, nm in zip(got, want, base, ('vs', 'advantages')):
    _same(g_, w_, nm)
    assert torch.equal(g_[:, others], b_[:, others]), f'{nm}: another env changed'
    assert torch.isfinite(b_).all()
  assert got[0][:3, e_nan].isnan().all() and torch.isfinite(got[0][3:, e_nan]).all()
  assert got[0][:, e_boot].isnan().all() and got[1][:, e_boot].isnan().all()
  assert got[1][4, e_masked].isnan() and got[0][4, e_masked].isnan()
  assert not torch.isfinite(got[0][0, e_inf]) and torch.isfinite(got[0][1:, e_inf]).all()


def test_gae_empty_batch_and_refusals(dev):
  from brax_amd.training import compute_gae
  T = 4
  e = [torch.empty((T, 0), device=dev) for _ in range(4)]
  out = (torch.empty((T, 0), device=dev), torch.empty((T, 0), device=dev))
  vs, adv = compute_gae(*e, torch.empty((0,), device=dev), fused=True, out=out)
  torch.cuda.synchronize()
  assert vs is out[0] and adv is out[1] and vs.shape == (T, 0)
  args = _inputs(T, 8, dev)
  with pytest.raises(NotImplementedError):
    compute_gae(*[a.double() for a in args], fused=True)
  with pytest.raises(NotImplementedError):
    compute_gae(args[0].cpu(), *args[1:], fused=True)
  # float64 on the device takes the chained form by default
  vs64, _ = compute_gae(*[a.double() for a in args])
  assert vs64.dtype == torch.float64
  with pytest.raises(Exception, match='stride'):  # an output that overlaps itself
    compute_gae(*args, fused=True,
                out=(torch.empty((1, 8), device=dev).expand(T, 8), torch.empty((T, 8), device=dev)))


def test_ppo_loss_fused_equals_chained_bit_for_bit(dev):
  from brax_amd.training import Transition, make_ppo_networks, ppo_loss
  T, B, O, A = 5, 64, 87, 8  # Ant's observation and action sizes
  g = torch.Generator().manual_seed(5)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  done = (torch.rand((B, T), generator=g) < 0.2).float()
  trunc = done * (torch.rand((B, T), generator=g) < 0.5).float()
  data = Transition(observation=r(B, T, O), action=torch.tanh(r(B, T, A)), reward=r(B, T),
                    discount=(1 - done).to(dev), next_observation=r(B, T, O),
                    truncation=trunc.to(dev), raw_action=r(B, T, A), log_prob=r(B, T) * 0.3 - 8)
  normalizer = (r(O) * 0.1, (torch.rand((O,), generator=g) + 0.5).to(dev))
  eps = r(B, T, A)
  policy, value = make_ppo_networks(O, A, seed=2, device=dev)
  params = [t for layers in (policy, value) for wb in layers for t in wb]
  res = {}
  for fused in (True, False):
    loss, metrics = ppo_loss(policy, value, normalizer, data, eps, fused=fused)
    res[fused] = (loss.detach(), {k: v.detach() for k, v in metrics.items()},
                  torch.autograd.grad(loss, params))
  assert torch.isfinite(res[True][0])
  assert torch.equal(res[True][0], res[False][0])
  for k in res[True][1]:
    assert torch.equal(res[True][1][k], res[False][1][k]), k
  for a, b in zip(res[True][2], res[False][2]):
    assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_trajectory_plumbing(dev):
  """Ant, episode_length 4, K = 6: truncation and AutoReset fall inside the
  unroll."""
  from brax_amd import envs
  from brax_amd.envs.policy import MLPPolicy, PolicyExtras, policy_rollout
  from brax_amd.training import make_ppo_networks, mlp, transitions
  from brax_amd.training.losses import head_scale, normal_tanh_log_prob, normalize
  from tests.test_gpu_policy_rollout import _check_policy, _eps
  B, K = 16, 6
  env = envs.create('ant', batch_size=B, episode_length=4, action_repeat=1, device=dev)
  st0 = env.reset(np.array([3, 4], np.uint32))
  layers, _ = make_ppo_networks(env.observation_size, env.action_size, seed=7, device=dev)
  g = torch.Generator().manual_seed(1)
  mean = (torch.rand((env.observation_size,), generator=g) - 0.5).to(dev)
  std = (torch.rand((env.observation_size,), generator=g) + 0.5).to(dev)
  policy = MLPPolicy([(w.detach(), b.detach()) for w, b in layers], obs_mean=mean, obs_std=std,
                     device=dev)
  seed, offset = 9, 64
  final, traj, ex = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, fused=True)
  d = transitions(st0.obs, traj, ex)
  assert float(traj.truncation.sum()) > 0 and float(traj.done.sum()) > 0
  assert tuple(d.observation.shape) == (B, K, env.observation_size) and tuple(d.reward.shape) == (B, K)
  assert torch.equal(d.observation[:, 0], st0.obs)
  assert torch.equal(d.observation[:, 1:], d.next_observation[:, :-1])
  assert torch.equal(d.next_observation[:, -1], final.obs)
  assert torch.equal(d.discount, 1 - traj.done.t())
  assert torch.equal(d.truncation, traj.truncation.t()) and torch.equal(d.reward, traj.reward.t())
  assert torch.equal(d.raw_action, ex.raw_action.transpose(0, 1))
  assert torch.equal(d.log_prob, ex.log_prob.t())
  # under AutoReset the obs after a done step is the reset obs
  first = st0.info['first_obs']
  ended = traj.done.t() != 0
  assert torch.equal(d.next_observation[ended], first[:, None].expand(-1, K, -1)[ended])
  # the learner's log-prob of the recorded raw action under the acting
  # weights, held to the bound tests/test_gpu_policy_rollout.py holds the
  # kernel's to (that module's check, with the learner's figure in the
  # kernel's place)
  logits = mlp(layers, normalize(d.observation, (mean, std)))
  loc, s = torch.chunk(logits, 2, dim=-1)
  learner_lp = normal_tanh_log_prob(loc, head_scale(s, policy.min_std), d.raw_action).sum(-1)
  eps = _eps(dev, K, B, env.action_size, seed, offset)
  _check_policy(policy, st0, traj, ex, eps, 'kernel')
  mine = PolicyExtras(action=ex.action, raw_action=ex.raw_action,
                      log_prob=learner_lp.detach().t().contiguous())
  _check_policy(policy, st0, traj, mine, eps, 'learner')


def test_train_end_to_end(dev, monkeypatch):
  from brax_amd.training import ppo
  seen, calls = [], []
  real = ppo.policy_rollout

  def spy(env, state, policy, k, **kw):
    seen.append((policy.params.data_ptr(), policy.params.clone(), policy.obs_mean.clone()))
    return real(env, state, policy, k, **kw)
  monkeypatch.setattr(ppo, 'policy_rollout', spy)
  cfg = dict(num_envs=64, unroll_length=5, batch_size=32, num_minibatches=4,
             num_updates_per_batch=2, num_evals=2, normalize_observations=True)
  acct = ppo.step_accounting(1900, cfg['num_evals'], cfg['batch_size'], cfg['unroll_length'],
                             cfg['num_minibatches'], 1, cfg['num_envs'])
  assert acct.num_training_steps_per_epoch == 3
  make_policy, params, metrics = ppo.train(
      'inverted_pendulum', num_timesteps=1900, episode_length=50, num_eval_envs=32, seed=1,
      device=dev, progress_fn=lambda step, m: calls.append((step, dict(m))), **cfg)
  torch.cuda.synchronize()
  # the evaluation schedule and the step accounting
  assert [c[0] for c in calls] == [0, 3 * acct.env_step_per_training_step] == [0, 1920]
  for _, m in calls:
    assert 'eval/episode_reward' in m and np.isfinite(float(m['eval/episode_reward']))
  assert 'training/sps' in metrics and metrics['training/walltime'] > 0
  assert {'training/total_loss', 'training/policy_loss', 'training/v_loss',
          'training/entropy_loss'} <= set(metrics)
  assert metrics is not calls[0][1] and float(metrics['eval/episode_reward']) == float(
      calls[1][1]['eval/episode_reward'])
  # 3 training steps x 2 unrolls, all through one buffer whose contents moved
  assert len(seen) == 6 and len({p for p, _, _ in seen}) == 1
  assert torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1])
  assert not torch.equal(seen[2][1], seen[4][1])
  assert not torch.equal(seen[0][2], seen[2][2])  # the acting normaliser moved too
  normalizer, policy_layers, value_layers = params
  assert normalizer.count == 3 * 128 * 5  # every observation of every unroll
  for w, b in policy_layers + value_layers:
    assert torch.isfinite(w).all() and torch.isfinite(b).all()
  assert np.isfinite(normalizer.mean).all() and np.isfinite(normalizer.std).all()
  p = make_policy(params, deterministic=True)
  assert p.deterministic and p.params.data_ptr() != seen[0][0]
  flat = torch.cat([torch.cat([w.detach().reshape(-1), b.detach()]) for w, b in policy_layers])
  assert torch.equal(p.params, flat)
  assert torch.equal(p.obs_mean, torch.as_tensor(normalizer.mean, dtype=torch.float32).to(dev))


def test_train_humanoid_takes_the_chained_rollout(dev):
  """The policy kernel refuses Humanoid (tests/test_gpu_policy_rollout.py
  asserts it); `train` completes through `policy_rollout`'s chained path."""
  from brax_amd import envs
  from brax_amd.envs.policy import fused_supported
  from brax_amd.training import ppo
  calls = []
  make_policy, params, metrics = ppo.train(
      'humanoid', num_timesteps=16, episode_length=4, num_envs=8, num_eval_envs=8,
      unroll_length=2, batch_size=4, num_minibatches=2, num_updates_per_batch=1, num_evals=1,
      device=dev, progress_fn=lambda step, m: calls.append(step))
  assert calls == [16]
  env = envs.create('humanoid', batch_size=8, episode_length=4, device=dev)
  assert fused_supported(env, make_policy(params)) is not None
  assert params[0] is None  # normalize_observations defaults to False
  for w, b in params[1] + params[2]:
    assert torch.isfinite(w).all() and torch.isfinite(b).all()
  assert np.isfinite(float(metrics['eval/episode_reward']))
