"""The evaluation entry points without a GPU: the `(M + 3, B)` packing,
`Evaluator` on the torch-only `fast` env (the chained fallback) and the
argument checks that need no device (the ABI mirror: tests/test_abi.py)."""
import numpy as np
import pytest
import torch

from brax_amd import _native
from brax_amd import abi


def test_library_exports_the_entry_points():
  lib = _native.lib()
  assert hasattr(lib, 'bx_env_eval_policy') and hasattr(lib, 'bx_env_eval_packed')
  # a null system fails with a message, no GPU touched
  rc = lib.bx_env_eval_packed(None, None, 0, 0, None, None, None, None, None, 0, 0, 0, None, None,
                              None, None, None)
  assert rc != 0 and b'null' in lib.bx_last_error()


def test_eval_metrics_packing_round_trips():
  from brax_amd.envs.evaluator import eval_keys, pack_eval_metrics, unpack_eval_metrics
  from brax_amd.envs.wrappers import EvalMetrics
  keys = ('b_metric', 'a_metric', 'z')
  assert eval_keys(keys) == keys + ('reward',)
  B = 5
  g = torch.Generator().manual_seed(3)
  em = EvalMetrics(episode_metrics={k: torch.rand((B,), generator=g) for k in sorted(keys + ('reward',))},
                   active_episodes=torch.tensor([1., 0., 1., 1., 0.]),
                   episode_steps=torch.arange(B, dtype=torch.float32))
  buf = pack_eval_metrics(em, keys)
  assert tuple(buf.shape) == (len(keys) + 3, B) and buf.dtype == torch.float32
  # rows: metric_keys order, then reward, active_episodes, episode_steps
  for i, k in enumerate(keys + ('reward',)):
    assert torch.equal(buf[i], em.episode_metrics[k]), k
  assert torch.equal(buf[4], em.active_episodes) and torch.equal(buf[5], em.episode_steps)
  back = unpack_eval_metrics(buf, keys)
  assert list(back.episode_metrics) == list(keys + ('reward',))
  for k in em.episode_metrics:
    assert torch.equal(back.episode_metrics[k], em.episode_metrics[k])
  assert torch.equal(back.active_episodes, em.active_episodes)
  assert torch.equal(back.episode_steps, em.episode_steps)
  # views of the buffer, not copies
  assert back.episode_steps.data_ptr() == buf[5].data_ptr()
  with pytest.raises(ValueError):
    pack_eval_metrics(em, ('a_metric',))
  with pytest.raises(ValueError):
    unpack_eval_metrics(buf[:4], keys)
  with pytest.raises(ValueError):
    pack_eval_metrics({'reward': 1}, keys)


def _fast_eval_env(B, ep):
  from brax_amd.envs import wrappers
  from brax_amd.envs.fast import Fast
  return wrappers.EvalWrapper(wrappers.AutoResetWrapper(
      wrappers.EpisodeWrapper(Fast(batch_size=B, device='cpu'), ep, 1)))


def _fast_policy(bias=1.0):
  from brax_amd.envs.policy import MLPPolicy
  return MLPPolicy([([[0.0, 0.0], [0.0, 0.0]], [bias, 0.0])], deterministic=True)


def test_evaluator_on_the_torch_only_env():
  """Fast has no kernel form: `Evaluator` takes the chained path and gives
  the `EvalWrapper` recurrences' values under the reference's key names."""
  from brax_amd.envs import Evaluator, eval_supported
  B, ep = 3, 4
  env = _fast_eval_env(B, ep)
  policy = _fast_policy()  # action tanh(1) > 0: the point accelerates
  assert eval_supported(env, policy)
  ev = Evaluator(env, policy, num_eval_envs=B, episode_length=ep, seed=7)
  tm = {'training/sps': 1.0, 'eval/walltime': -1.0}
  out = ev.run_evaluation(tm)
  assert set(out) == {'eval/episode_reward', 'eval/avg_episode_length', 'eval/epoch_eval_time',
                      'eval/sps', 'eval/walltime', 'training/sps'}
  # the recurrences by hand: vel += dt, pos += vel dt, reward = pos, summed
  # while the first episode is active (all ep steps)
  dt, pos, vel, want = 0.02, 0.0, 0.0, 0.0
  for _ in range(ep):
    vel = np.float32(vel + np.float32(dt))
    pos = np.float32(pos + np.float32(vel * np.float32(dt)))
    want = np.float32(want + pos)
  assert float(out['eval/episode_reward']) == pytest.approx(float(want), rel=1e-6)
  assert float(out['eval/avg_episode_length']) == ep
  assert out['training/sps'] == 1.0 and out['eval/walltime'] == -1.0  # training_metrics win, as the reference's merge
  assert out['eval/sps'] == pytest.approx(ep * B / out['eval/epoch_eval_time'])
  em = ev.state.info['eval_metrics']
  assert em.active_episodes.tolist() == [0.0] * B and em.episode_steps.tolist() == [float(ep)] * B
  assert 'reward' in ev.state.metrics
  per_env = ev.run_evaluation(aggregate_episodes=False)
  assert tuple(per_env['eval/episode_reward'].shape) == (B,)
  assert per_env['eval/walltime'] == pytest.approx(out['eval/epoch_eval_time'] + per_env['eval/epoch_eval_time'])
  # new weights in place are seen by the next run: a non-positive action
  # leaves the point at rest
  policy.load_([([[0.0, 0.0], [0.0, 0.0]], [-1.0, 0.0])])
  assert float(ev.run_evaluation()['eval/episode_reward']) == 0.0


def test_eval_rollout_chained_equals_env_step():
  from brax_amd.envs import eval_rollout
  B, ep, K = 3, 2, 5
  env = _fast_eval_env(B, ep)
  policy = _fast_policy()
  st0 = env.reset(np.array([1, 2], np.uint32))
  got = eval_rollout(env, st0, k=K, policy=policy)
  acts = torch.full((K, B, 1), 0.5)
  got_a = eval_rollout(env, st0, actions=acts)
  ref = st0
  for t in range(K):
    ref = env.step(ref, acts[t])
  for g in (got, got_a):
    ge, re_ = g.info['eval_metrics'], ref.info['eval_metrics']
    assert torch.equal(ge.episode_metrics['reward'], re_.episode_metrics['reward'])
    assert torch.equal(ge.active_episodes, re_.active_episodes)
    assert torch.equal(ge.episode_steps, re_.episode_steps)
    assert torch.equal(g.obs, ref.obs) and torch.equal(g.done, ref.done)
  # the first episode ended at step ep: the sums stopped there
  assert ref.info['eval_metrics'].active_episodes.tolist() == [0.0] * B
  assert ref.info['eval_metrics'].episode_steps.tolist() == [float(ep)] * B
  with pytest.raises(NotImplementedError):
    eval_rollout(env, st0, k=K, policy=policy, fused=True)


def test_argument_checks():
  from brax_amd.envs import eval_rollout, eval_supported, wrappers
  env = _fast_eval_env(2, 3)
  policy = _fast_policy()
  st0 = env.reset(np.array([0, 1], np.uint32))
  acts = torch.zeros((2, 2, 1))
  with pytest.raises(ValueError):
    eval_rollout(env, st0, k=2, policy=policy, actions=acts)
  with pytest.raises(ValueError):
    eval_rollout(env, st0, k=2)
  with pytest.raises(ValueError):
    eval_rollout(env, st0, k=3, actions=acts)  # k against the actions' K
  with pytest.raises(ValueError):
    eval_rollout(env, st0, policy=policy)  # a policy needs k
  with pytest.raises(ValueError):
    eval_rollout(env.env, st0, k=2, policy=policy)  # EvalWrapper is not outermost
  with pytest.raises(ValueError):
    eval_supported(env.env, policy)
  assert isinstance(env, wrappers.EvalWrapper)
  info = {k: v for k, v in st0.info.items() if k != 'eval_metrics'}
  with pytest.raises(ValueError):
    eval_rollout(env, st0.replace(info=info), k=2, policy=policy)
