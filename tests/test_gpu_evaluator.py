"""Whole evaluation episodes in one launch (`brax_amd.envs.evaluator`:
`bx_env_eval_policy` / `bx_env_eval_packed`). Needs an MI355X.

The fused sums are the same float32 operations, in the same order, on the same
per-step values as `EvalWrapper.step`'s, so every comparison here is bit for
bit:

* the open-loop form against K chained `env.step` calls on the eval env (that
  path is held to the reference by `tests/test_gpu_eval.py`);
* the policy form against `policy_rollout(fused=True)` on the unwrapped env
  followed by the `EvalWrapper` recurrences applied step by step in torch
  float32 to its trajectory (a chained closed loop would diverge under the
  policy's rounding; the trajectory kernel is pinned by
  `tests/test_gpu_policy_rollout.py`).
"""
import math

import numpy as np
import pytest
import torch

from tests.conftest import golden
from tests.helpers import set_variant

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _weights(sizes, seed):
  g = torch.Generator(device='cpu').manual_seed(seed)
  out = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    lim = math.sqrt(3.0 / i)
    out.append(((torch.rand((i, o), generator=g) * 2 - 1) * lim,
                (torch.rand((o,), generator=g) * 2 - 1) * 0.1))
  return out


def _policy(env, dev, hidden=(32, 32), seed=11, deterministic=False):
  from brax_amd.envs.policy import MLPPolicy
  O, A = env.observation_size, env.action_size
  return MLPPolicy(_weights((O,) + tuple(hidden) + (2 * A,), seed), deterministic=deterministic,
                   device=dev)


def _make(dev, name, B, ep=3, ar=1, lift=None, key=(2, 9)):
  """The eval env (Episode, Vector, AutoReset, Eval) and its reset state;
  `lift`: that env's bodies raised out of a healthy z range."""
  from brax_amd import envs
  from brax_amd.base import PackedQP
  from brax_amd.envs.policy import _packed
  env = envs.create(name, batch_size=B, episode_length=ep, action_repeat=ar, auto_reset=True,
                    eval_metrics=True, device=dev)
  st = env.reset(np.array(key, np.uint32))
  if lift is not None:
    buf = _packed(st, dev).clone()
    buf[lift, :, 2] += 3.0
    st = st.replace(qp=PackedQP(buf))
  return env, st


def _tensors(st):
  """Every tensor of an eval env's state, by name (a packed qp's words
  13..15 are padding no kernel writes)."""
  from brax_amd.envs.policy import _packed
  em = st.info['eval_metrics']
  out = {'qp': _packed(st, st.obs.device)[..., :13], 'obs': st.obs, 'reward': st.reward,
         'done': st.done, 'steps': st.info['steps'], 'truncation': st.info['truncation'],
         'active_episodes': em.active_episodes, 'episode_steps': em.episode_steps}
  for k, v in st.metrics.items():
    out['metric/' + k] = v
  for k, v in em.episode_metrics.items():
    out['episode/' + k] = v
  if st.info.get('rng') is not None:
    out['rng'] = st.info['rng']
  return out


def _assert_same(got, want, rows=None):
  a, b = _tensors(got), _tensors(want)
  assert sorted(a) == sorted(b)
  for k in a:
    x, y = a[k], b[k]
    if rows is not None:
      x, y = x[rows], y[rows]
    # bit for bit (a NaN equals the same NaN)
    assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), k


def _chain(env, st, acts):
  for t in range(acts.shape[0]):
    st = env.step(st, acts[t])
  return st


def _golden_env(dev):
  from brax_amd import envs
  from brax_amd.base import qp_from_numpy
  from brax_amd.envs.env import State
  from brax_amd.envs.wrappers import EvalMetrics
  T = golden('eval_ant')
  B = T['qp0'].shape[0]
  keys = [str(k) for k in T['metric_keys']]
  env = envs.create('ant', episode_length=int(T['episode_length']), batch_size=B,
                    eval_metrics=True, device=dev)
  f32 = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev)  # noqa: E731
  rm = T['reset_metrics']
  em = EvalMetrics(episode_metrics={k: torch.zeros(B, device=dev) for k in keys},
                   active_episodes=torch.ones(B, device=dev),
                   episode_steps=torch.zeros(B, device=dev))
  st = State(qp=qp_from_numpy(T['qp0'], dev), obs=f32(T['obs0']),
             reward=torch.zeros(B, device=dev), done=torch.zeros(B, device=dev),
             metrics={k: f32(rm[:, i]) for i, k in enumerate(keys) if k != 'reward'},
             info={'first_qp': qp_from_numpy(T['first_qp'], dev), 'first_obs': f32(T['first_obs']),
                   'steps': torch.zeros(B, device=dev), 'truncation': torch.zeros(B, device=dev),
                   'eval_metrics': em})
  return T, env, st, f32(T['action'])


@pytest.fixture(scope='module')
def golden_run(dev):
  """The golden scene, its recorded actions, and the eval env's own chain."""
  T, env, st, acts = _golden_env(dev)
  return T, env, st, acts, _chain(env, st, acts)


def test_open_loop_vs_golden_and_chain(dev, golden_run):
  from brax_amd.envs import eval_rollout
  T, env, st, acts, ref = golden_run
  assert acts.shape[0] == 7 and st.obs.shape[0] == 8 and int(T['episode_length']) == 3
  # the golden's last step: an inactive env, an episode cut short, full ones
  assert (T['active_episodes'][-1] == 0).any()
  assert (T['episode_steps'][-1] < 3).any() and (T['episode_steps'][-1] == 3).any()
  got = eval_rollout(env, st, actions=acts, fused=True)
  em = got.info['eval_metrics']
  assert np.array_equal(em.active_episodes.cpu().numpy(), T['active_episodes'][-1])
  assert np.array_equal(em.episode_steps.cpu().numpy(), T['episode_steps'][-1])
  assert np.array_equal(got.done.cpu().numpy(), T['done'][-1])
  assert np.array_equal(got.info['steps'].cpu().numpy(), T['steps'][-1])
  rem = ref.info['eval_metrics']
  assert sorted(em.episode_metrics) == sorted(rem.episode_metrics)
  for k in rem.episode_metrics:
    assert torch.equal(em.episode_metrics[k], rem.episode_metrics[k]), k
  assert 'reward' in got.metrics
  _assert_same(got, ref)


def test_continuation(dev, golden_run):
  """K = 3 then K = 4, the first call's state fed to the second: the single
  K = 7 launch in every returned tensor."""
  from brax_amd.envs import eval_rollout
  _, env, st, acts, _ = golden_run
  whole = eval_rollout(env, st, actions=acts, fused=True)
  mid = eval_rollout(env, st, actions=acts[:3], fused=True)
  assert float(mid.info['eval_metrics'].active_episodes.min()) == 0.0
  two = eval_rollout(env, mid, actions=acts[3:], fused=True)
  _assert_same(two, whole)


def _expected(env, st0, policy, K, seed, offset, stride):
  """policy_rollout on the unwrapped env, then EvalWrapper.step's recurrences
  on its trajectory: (final state, sums (M + 1, B), active, episode_steps,
  whether an env was inactive before the last step)."""
  from brax_amd.envs.policy import policy_rollout
  final, tr, _ = policy_rollout(env.env, st0, policy, K, seed=seed, offset=offset,
                                step_stride=stride, fused=True)
  B, M = tr.reward.shape[1], tr.metrics.shape[2]
  dev = tr.reward.device
  sums = [torch.zeros(B, device=dev) for _ in range(M + 1)]
  active = torch.ones(B, device=dev)
  ep_steps = torch.zeros(B, device=dev)
  early = False
  for t in range(K):
    if t == K - 1:
      early = bool((active == 0).any())
    ep_steps = torch.where(active != 0, tr.steps[t], ep_steps)
    per_step = [tr.metrics[t, :, k] for k in range(M)] + [tr.reward[t]]
    sums = [s + m * active for s, m in zip(sums, per_step)]
    active = active * (1 - tr.done[t])
  return final, tr, sums, active, ep_steps, early


def _check_policy_case(dev, name, B, ar, det, K=8, ep=3, lift=None, hidden=(32, 32)):
  from brax_amd.envs import eval_rollout
  from brax_amd.envs.policy import _packed
  env, st0 = _make(dev, name, B, ep, ar, lift)
  policy = _policy(env, dev, hidden, deterministic=det)
  seed, offset, stride = 5, 1000, 2 * B * env.action_size + 6
  final, tr, sums, active, ep_steps, early = _expected(env, st0, policy, K, seed, offset, stride)
  got = eval_rollout(env, st0, k=K, policy=policy, seed=seed, offset=offset, step_stride=stride,
                     fused=True)
  torch.cuda.synchronize()
  em = got.info['eval_metrics']
  keys = tuple(env.unwrapped.metric_keys) + ('reward',)
  assert list(em.episode_metrics) == list(keys)
  for k, want in zip(keys, sums):
    assert torch.equal(em.episode_metrics[k], want), (name, k)
  assert torch.equal(em.active_episodes, active) and torch.equal(em.episode_steps, ep_steps)
  assert torch.equal(_packed(got, dev)[..., :13], tr.qp[K - 1][..., :13])
  for f, want in (('obs', tr.obs[K - 1]), ('reward', tr.reward[K - 1]), ('done', tr.done[K - 1])):
    assert torch.equal(getattr(got, f), want), (name, f)
  assert torch.equal(got.info['steps'], tr.steps[K - 1])
  assert torch.equal(got.info['truncation'], tr.truncation[K - 1])
  for i, k in enumerate(keys[:-1]):
    assert torch.equal(got.metrics[k], tr.metrics[K - 1, :, i]), (name, k)
  assert torch.equal(got.metrics['reward'], tr.reward[K - 1])
  assert (tr.rng is None) == (got.info.get('rng') is None)
  if tr.rng is not None:
    assert torch.equal(got.info['rng'], tr.rng[K - 1])
  assert torch.equal(got.obs, final.obs)
  return tr, early


@pytest.mark.parametrize('name,B,ar,det,lift', [
    ('ant', 6, 1, False, 2),  # a ragged wave, EK_ANT
    ('ant', 6, 1, True, 2),
    ('ant', 21, 1, False, 3),
    ('ant', 21, 1, True, 3),
    ('halfcheetah', 21, 1, False, None),
    ('pusher', 21, 1, False, None),
    ('hopper', 21, 1, False, 3),  # EK_ANY
    ('fetch', 21, 1, False, None),  # the target envs' rng stream
    ('ur5e', 21, 2, False, None),
    ('inverted_pendulum', 21, 1, False, None),  # A = 1, no metrics
])
def test_policy_form_vs_trajectory(dev, name, B, ar, det, lift):
  tr, early = _check_policy_case(dev, name, B, ar, det, lift=lift)
  # episodes ended inside the launch: AutoReset fired, `active` dropped
  assert early, name
  assert float(tr.done.sum()) > 0
  if name == 'ant':  # the lifted env terminated on its first step
    assert float(tr.done[0, lift]) == 1.0 and float(tr.steps[0, lift]) == 1.0


def test_policy_form_wide_kernel(dev):
  """Past one wave per SIMD the Ant launch takes the register-capped kernel
  (the selection of `launch_env_policy_single`: more workgroups than 4 per
  compute unit)."""
  B = 4160
  assert (B + 3) // 4 > 4 * torch.cuda.get_device_properties(dev).multi_processor_count
  _check_policy_case(dev, 'ant', B, 1, False, K=3, ep=2, lift=7)


@pytest.mark.parametrize('name', ['humanoid', 'swimmer'])
def test_open_loop_on_action_reading_kinds(dev, name):
  """The env kinds the policy form refuses (their programs read the action
  row): given actions, against the eval env's own chain."""
  from brax_amd.envs import eval_rollout, eval_supported
  B, K = 5, 4
  env, st0 = _make(dev, name, B, 3, 1)
  assert eval_supported(env) is None
  g = torch.Generator(device='cpu').manual_seed(4)
  acts = (torch.rand((K, B, env.action_size), generator=g) * 2 - 1).to(dev)
  got = eval_rollout(env, st0, actions=acts, fused=True)
  ref = _chain(env, st0, acts)
  assert float(ref.info['eval_metrics'].active_episodes.max()) == 0.0
  _assert_same(got, ref)


@pytest.mark.parametrize('B', [8, 1])
@pytest.mark.parametrize('form', ['policy', 'actions'])
def test_no_stores_outside_the_documented_buffers(dev, B, form):
  """`out` is one block and `eval_out` (M + 3, B), whatever K is: sentinels
  on both sides of both stay intact after a K = 8 launch."""
  from brax_amd.envs import eval_rollout
  K, pad = 8, 4096
  env, st0 = _make(dev, 'ant', B, 3, 1)
  u = env.unwrapped
  N, O, M = u.sys.num_bodies, u.obs_size, len(u.metric_keys)
  block, nev = B * (N * 16 + O + 4 + M), (M + 3) * B
  big = torch.full((pad + block + pad,), SENTINEL, device=dev)
  bev = torch.full((pad + nev + pad,), SENTINEL, device=dev)
  kw = dict(out=big[pad:pad + block], eval_out=bev[pad:pad + nev].view(M + 3, B), fused=True)
  if form == 'policy':
    got = eval_rollout(env, st0, k=K, policy=_policy(env, dev), seed=3, **kw)
    ref = eval_rollout(env, st0, k=K, policy=_policy(env, dev), seed=3, fused=True)
  else:
    g = torch.Generator(device='cpu').manual_seed(8)
    acts = (torch.rand((K, B, env.action_size), generator=g) * 2 - 1).to(dev)
    got = eval_rollout(env, st0, actions=acts, **kw)
    ref = eval_rollout(env, st0, actions=acts, fused=True)
  torch.cuda.synchronize()
  for buf, n in ((big, block), (bev, nev)):
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())
  assert got.info['eval_metrics'].episode_steps.data_ptr() == bev[pad + (M + 2) * B:].data_ptr()
  # every word of eval_out and every word of the block but the qp records'
  # padding was written
  assert not bool((bev[pad:pad + nev] == SENTINEL).any())
  q = big[pad:pad + B * N * 16].view(B, N, 16)
  assert not bool((q[..., :13] == SENTINEL).any())
  assert not bool((big[pad + B * N * 16:pad + block] == SENTINEL).any())
  _assert_same(got, ref)


def test_nan_isolation(dev):
  from brax_amd.envs import eval_rollout
  B, K = 8, 8
  env, st0 = _make(dev, 'ant', B, 3, 1)
  policy = _policy(env, dev)
  clean = eval_rollout(env, st0, k=K, policy=policy, seed=2, fused=True)
  obs = st0.obs.clone()
  obs[5, 3] = float('nan')
  dirty = eval_rollout(env, st0.replace(obs=obs), k=K, policy=policy, seed=2, fused=True)
  torch.cuda.synchronize()
  assert not bool(torch.isfinite(dirty.info['eval_metrics'].episode_metrics['reward'][5]))
  assert bool(torch.isfinite(clean.info['eval_metrics'].episode_metrics['reward']).all())
  keep = torch.arange(B, device=dev) != 5
  _assert_same(dirty, clean, rows=keep)


class _MountainAnt:
  """An Ant-kind env over the four-ant mountain scene: a MULTI-mode system."""

  @staticmethod
  def make(dev, B):
    from brax_amd.envs import wrappers
    from brax_amd.envs.ant import Ant
    from brax_amd.envs.env import PhysicsEnv
    from brax_amd.envs.mountain import ant_mountain_config

    class MountainAnt(PhysicsEnv):
      kind = Ant.kind
      metric_keys = Ant.metric_keys

      def __init__(self, **kwargs):
        super().__init__(ant_mountain_config(4), **kwargs)
        self.coef = np.array([1.0, 0.5, 5e-4, 1.0, 0.2, 1.0, 1.0, 1.0], np.float32)
        self._set_sizes()

    inner = MountainAnt(device=dev)
    env = wrappers.EvalWrapper(wrappers.AutoResetWrapper(wrappers.VectorWrapper(
        wrappers.EpisodeWrapper(inner, 3, 1), B)))
    return env, inner


def _blank_state(env, B, dev):
  """A state that carries only what the refusal paths read."""
  from brax_amd.envs.env import State
  from brax_amd.envs.wrappers import EvalMetrics
  keys = tuple(env.unwrapped.metric_keys) + ('reward',)
  z = torch.zeros(B, device=dev)
  em = EvalMetrics(episode_metrics={k: z.clone() for k in keys}, active_episodes=z + 1,
                   episode_steps=z.clone())
  return State(qp=None, obs=torch.zeros((B, env.observation_size), device=dev), reward=z, done=z,
               info={'eval_metrics': em})


def test_refusals_and_fallback(dev):
  from brax_amd import envs
  from brax_amd.envs import eval_rollout, eval_supported
  from brax_amd.envs.policy import normal_slabs
  # Humanoid's program reads the action row: no policy form
  B, K = 5, 3
  env, st0 = _make(dev, 'humanoid', B, 3, 1)
  policy = _policy(env, dev)
  why = eval_supported(env, policy)
  assert why and 'reads the action row' in why
  with pytest.raises(NotImplementedError, match='reads the action row'):
    eval_rollout(env, st0, k=K, policy=policy, fused=True)
  # fused=None: the chained path, policy.forward then env.step per step
  got = eval_rollout(env, st0, k=K, policy=policy, seed=4, offset=10)
  A = env.action_size
  ref = st0
  for t in range(K):
    eps = torch.empty((B, A), device=dev)
    normal_slabs(eps, B * A, 1, 4, 10 + t * 2 * B * A, 0)
    ref = env.step(ref, policy.forward(ref.obs.to(torch.float32), eps)[0])
  _assert_same(got, ref)
  # a 129-wide layer
  ant, sa = _make(dev, 'ant', 8, 3, 1)
  wide = _policy(ant, dev, (129,))
  why = eval_supported(ant, wide)
  assert why and 'layer widths' in why
  with pytest.raises(NotImplementedError, match='layer widths'):
    eval_rollout(ant, sa, k=2, policy=wide, fused=True)
  # a MULTI-mode system (and the item loops): both forms refused
  menv, inner = _MountainAnt.make(dev, 2)
  assert set_variant(inner.sys, 'multi') == 0
  ms = _blank_state(menv, 2, dev)
  mpol = _policy(menv, dev)
  why = eval_supported(menv)
  assert why and 'SINGLE-mode' in why
  assert eval_supported(menv, mpol)
  macts = torch.zeros((2, 2, menv.action_size), device=dev)
  with pytest.raises(NotImplementedError, match='SINGLE-mode'):
    eval_rollout(menv, ms, actions=macts, fused=True)
  with pytest.raises(NotImplementedError):
    eval_rollout(menv, ms, k=2, policy=mpol, fused=True)
  assert set_variant(inner.sys, 'itemloop') == 0
  assert 'SINGLE-mode' in eval_supported(menv)
  # argument checks
  plain = envs.create('ant', batch_size=8, episode_length=3, device=dev)
  with pytest.raises(ValueError):
    eval_rollout(plain, sa, k=2, policy=_policy(ant, dev))
  acts = torch.zeros((2, 8, ant.action_size), device=dev)
  with pytest.raises(ValueError):
    eval_rollout(ant, sa, k=2, policy=_policy(ant, dev), actions=acts)
  with pytest.raises(ValueError):
    eval_rollout(ant, sa, k=2)
  torch.cuda.synchronize()


def test_evaluator(dev):
  from brax_amd.envs import Evaluator, eval_rollout
  from brax_amd.envs.ant import Ant
  from brax_amd import envs
  B, ep = 16, 6
  probe = envs.create('ant', batch_size=B, episode_length=ep, eval_metrics=True, device=dev)
  policy = _policy(probe, dev, seed=21, deterministic=True)
  ev = Evaluator('ant', policy, num_eval_envs=B, episode_length=ep, seed=5, device=dev)
  m1 = ev.run_evaluation({'training/x': 2.0})
  names = tuple(Ant.metric_keys) + ('reward',)
  assert set(m1) == ({f'eval/episode_{k}' for k in names} |
                     {'eval/avg_episode_length', 'eval/epoch_eval_time', 'eval/sps',
                      'eval/walltime', 'training/x'})
  em = ev.state.info['eval_metrics']
  assert float(m1['eval/avg_episode_length']) == float(em.episode_steps.mean())
  assert float(m1['eval/episode_reward']) == float(em.episode_metrics['reward'].mean())
  assert float(em.active_episodes.abs().max()) == 0.0
  assert 1.0 <= float(em.episode_steps.min()) and float(em.episode_steps.max()) <= ep
  first1 = ev.first_state.obs.clone()
  m2 = ev.run_evaluation(aggregate_episodes=False)
  for k in names:
    assert tuple(m2[f'eval/episode_{k}'].shape) == (B,), k
  assert float(ev.state.info['eval_metrics'].active_episodes.abs().max()) == 0.0
  # a fresh reset key per run
  assert not torch.equal(ev.first_state.obs, first1)
  assert m2['eval/walltime'] == pytest.approx(m1['eval/epoch_eval_time'] + m2['eval/epoch_eval_time'])
  # weights loaded in place are seen by the next run: it equals a rollout of
  # the new weights from its reset state, and differs from the old weights'
  old = _policy(probe, dev, seed=21, deterministic=True)
  policy.load_(_weights((probe.observation_size, 32, 32, 2 * probe.action_size), 99))
  m3 = ev.run_evaluation(aggregate_episodes=False)
  want = eval_rollout(ev.env, ev.first_state, k=ep, policy=policy, fused=True)
  was = eval_rollout(ev.env, ev.first_state, k=ep, policy=old, fused=True)
  r_new = want.info['eval_metrics'].episode_metrics['reward']
  assert torch.equal(m3['eval/episode_reward'], r_new)
  assert not torch.equal(r_new, was.info['eval_metrics'].episode_metrics['reward'])
