"""Whole evaluation episodes in ONE launch, the episode sums kept on chip.

The reference wraps `generate_unroll` in `acting.Evaluator`
(`brax/training/acting.py:77-139`): `EvalWrapper` around the env, a reset of
`num_eval_envs` envs, `episode_length // action_repeat` policy steps, and then
only `state.info['eval_metrics']` is read. `eval_rollout` is that unroll
through `bx_env_eval_policy` (an `MLPPolicy` acting inside the launch) or
`bx_env_eval_packed` (given actions): `EvalWrapper.step`'s recurrences run per
env inside the K-step kernel, in float32 and in the wrapper's order, and the
launch writes one state block and `M + 3` floats per env, whatever K is. The
result is the state K chained `env.step` calls on the eval env return
(`tests/test_gpu_evaluator.py`, bit for bit).

`Evaluator` is the reference's class over it.
"""
import ctypes as C
import time
from typing import Optional

import numpy as np
import torch

from brax_amd import abi
from brax_amd.base import pack_qp
from brax_amd.envs import packed, wrappers
from brax_amd.envs.env import State
from brax_amd.envs.policy import MLPPolicy, fused_supported, step_noise
from brax_amd.envs.rollout import chain_options
from brax_amd.fused import use_kernel


def eval_keys(metric_keys):
  """The rows of the `(M + 3, B)` evaluation buffer that are episode sums:
  the env's `metric_keys`, then 'reward' (then active_episodes and
  episode_steps)."""
  return tuple(metric_keys) + ('reward',)


def pack_eval_metrics(em, metric_keys, device=None):
  """An `EvalMetrics` as the `(M + 3, B)` float32 buffer of the evaluation
  kernels: the sums in `eval_keys` order, active_episodes, episode_steps."""
  if not isinstance(em, wrappers.EvalMetrics):
    raise ValueError(f'Incorrect type for state_metrics: {type(em)}')
  keys = eval_keys(metric_keys)
  if sorted(em.episode_metrics) != sorted(keys):
    raise ValueError(f'eval_metrics holds {sorted(em.episode_metrics)}, the env sums {sorted(keys)}')
  dev = torch.device(em.active_episodes.device if device is None else device)
  rows = [em.episode_metrics[k] for k in keys] + [em.active_episodes, em.episode_steps]
  return torch.stack([torch.as_tensor(r, dtype=torch.float32, device=dev).reshape(-1) for r in rows])


def unpack_eval_metrics(buf, metric_keys):
  """The `EvalMetrics` over views of an `(M + 3, B)` evaluation buffer."""
  keys = eval_keys(metric_keys)
  if buf.dim() != 2 or buf.shape[0] != len(keys) + 2:
    raise ValueError(f'evaluation buffer {tuple(buf.shape)} != ({len(keys) + 2}, B)')
  return wrappers.EvalMetrics(episode_metrics={k: buf[i] for i, k in enumerate(keys)},
                              active_episodes=buf[len(keys)], episode_steps=buf[len(keys) + 1])


def _peel(env):
  if not isinstance(env, wrappers.EvalWrapper):
    raise ValueError(f'eval_rollout needs EvalWrapper outermost, got {type(env).__name__}')
  return env.env


def eval_supported(env, policy=None) -> Optional[str]:
  """None when the one-launch evaluation takes this eval env (and policy;
  None: given actions), else the library's reason (a zero-step call: argument
  checks only, no launch)."""
  inner = _peel(env)
  if policy is not None:
    # (an identity head goes to the population kernel, one shared row)
    why = fused_supported(inner, policy, trajectory=policy.head == 'normal_tanh')
    if why is not None:
      return why
  try:
    u, opts = chain_options(inner)
  except NotImplementedError as e:
    return str(e)
  if policy is None:
    return packed.refusal(u, opts, 'bx_env_eval_packed', act_width=u.action_size)
  desc = policy.descriptor(u.action_size)
  if policy.head != 'normal_tanh':
    pop = abi.BxPopulation(head=abi.HEADS[policy.head])
    return packed.refusal(u, opts, 'bx_env_eval_population', policy=C.byref(desc),
                          pop=C.byref(pop))
  return packed.refusal(u, opts, 'bx_env_eval_policy', policy=C.byref(desc))


def eval_rollout(env, state: State, k: Optional[int] = None, policy: Optional[MLPPolicy] = None,
                 actions=None, seed: int = 0, offset: int = 0, step_stride: Optional[int] = None,
                 fused: Optional[bool] = None, out: Optional[torch.Tensor] = None,
                 eval_out: Optional[torch.Tensor] = None) -> State:
  """K `env.step`s of an eval env (EvalWrapper outermost) in one launch.

  Exactly one of `policy` (closed loop: action_t = policy(obs_t, eps_t), the
  noise as `policy_rollout`'s) and `actions` (K, B, A) is given; `k` is
  needed with a policy and defaults to K with actions.

  Args:
    state: carries `info['eval_metrics']` (from `env.reset` or an earlier
      call: an evaluation continues across calls).
    fused: None takes the one-launch kernel where the library allows it, else
      the chained path (`policy.forward` or the given action, then
      `env.step`, per step); True raises NotImplementedError where the kernel
      refuses; False forces the chained path.
    out, eval_out: optional buffers for the fused launch to write: a flat
      contiguous float32 of one block (`packed.Layout.block` floats) and a
      contiguous float32 (M + 3, B); the returned state's tensors are views of
      them.
  Returns:
    The state `EvalWrapper.step` returns after the K-th step: `metrics`
    includes 'reward', `info['eval_metrics']` is an `EvalMetrics` over views
    of the launch's `(M + 3, B)` output.
  """
  inner = _peel(env)
  if (policy is None) == (actions is None):
    raise ValueError('eval_rollout takes exactly one of policy and actions')
  if actions is not None:
    if getattr(actions, 'ndim', None) != 3:
      raise ValueError('actions must be (K, B, A)')
    if k is not None and int(k) != actions.shape[0]:
      raise ValueError(f'k = {k} but actions hold {actions.shape[0]} steps')
    k = actions.shape[0]
  if k is None or int(k) < 1:
    raise ValueError(f'k must be >= 1, got {k}')
  K = int(k)
  em_in = state.info.get('eval_metrics')
  if not isinstance(em_in, wrappers.EvalMetrics):
    raise ValueError(f'Incorrect type for state_metrics: {type(em_in)}')
  if not use_kernel(fused, 'evaluation', lambda: eval_supported(env, policy)):
    return _chained(env, state, policy, actions, K, seed, offset, step_stride)
  u, opts = chain_options(inner)
  dev = u.sys.device
  qbuf = pack_qp(state.qp, dev)
  B, A = qbuf.shape[0], u.action_size
  inputs = packed.step_inputs(u, opts, state, B)
  keys = tuple(u.metric_keys)
  M = len(keys)
  ev = pack_eval_metrics(em_in, keys, dev)
  if tuple(ev.shape) != (M + 3, B):
    raise ValueError(f'eval_metrics holds {ev.shape[1]} envs, the state {B}')
  lay = packed.layout(u, B)
  out = lay.out_buffer(out, 1, dev)
  if eval_out is not None:
    ev = packed.output_buffer('eval_out', eval_out, (M + 3, B), dev).copy_(ev)
  if policy is not None:
    stride = 2 * B * A if step_stride is None else int(step_stride)
    entry = 'bx_env_eval_policy'
    own = dict(obs_in=packed.obs_input(u, state, B), policy=C.byref(policy.descriptor(A)),
               seed=seed, offset=offset, step_stride=stride)
    if policy.head != 'normal_tanh':
      # ARS's policy: the population kernel with one shared row, no moments
      entry = 'bx_env_eval_population'
      own['pop'] = C.byref(abi.BxPopulation(head=abi.HEADS[policy.head]))
  else:
    act = packed.actions_input(actions, B, A, dev)
    entry, own = 'bx_env_eval_packed', dict(act=act, act_stride=act.stride(1),
                                            act_step_stride=act.stride(0), act_width=A)
  rng_out = packed.launch(u, entry, inputs, qbuf, K, out, False, eval_in=ev, eval_out=ev, **own)
  return packed.final_state(u, inputs[0], state, lay.step_views(out[:lay.block]), rng_out,
                            eval_metrics=unpack_eval_metrics(ev, keys))


def _chained(env, state, policy, actions, K, seed, offset, step_stride):
  """The same loop through the eval env's own `step`: any env, any chain."""
  dev = torch.device(state.obs.device)
  B, A = state.obs.shape[0], env.action_size
  if policy is None:
    for t in range(K):
      state = env.step(state, torch.as_tensor(actions[t], dtype=torch.float32, device=dev))
    return state
  policy.for_actions(A)
  stride = 2 * B * A if step_stride is None else int(step_stride)
  for eps in step_noise(policy, K, B, A, seed, offset, stride, dev):
    state = env.step(state, policy.forward(state.obs.to(torch.float32), eps)[0])
  return state


class Evaluator:
  """`acting.Evaluator` (`training/acting.py:77-139`): one evaluation epoch is
  a reset of `num_eval_envs` envs and ONE `eval_rollout` of `episode_length
  // action_repeat` steps.

  Args:
    env: an env name (created with Episode / Vector / AutoReset / Eval
      wrappers at `num_eval_envs`) or a batched env (wrapped in `EvalWrapper`
      unless it already is).
    policy: an `MLPPolicy`; the kernel reads its buffer at launch, so
      `policy.load_` between runs is seen by the next run.
    seed: the key the per-run reset keys are split from.
  """

  def __init__(self, env, policy: MLPPolicy, num_eval_envs: int = 128, episode_length: int = 1000,
               action_repeat: int = 1, seed: int = 0, device=None, fused: Optional[bool] = None):
    if isinstance(env, str):
      from brax_amd import envs  # pylint: disable=import-outside-toplevel
      kw = {} if device is None else {'device': device}
      env = envs.create(env, episode_length=episode_length, action_repeat=action_repeat,
                        batch_size=num_eval_envs, eval_metrics=True, **kw)
    elif not isinstance(env, wrappers.EvalWrapper):
      env = wrappers.EvalWrapper(env)
    self.env, self.policy, self.fused = env, policy, fused
    self.num_eval_envs = int(num_eval_envs)
    self.unroll_length = int(episode_length) // int(action_repeat)
    self.seed = int(seed)
    self._key = np.array([0, self.seed], np.uint32)  # jax.random.PRNGKey(seed) layout
    self._runs = 0
    self._eval_walltime = 0.
    self._steps_per_unroll = int(episode_length) * self.num_eval_envs
    self.first_state = self.state = None  # the last run's reset and final states

  def run_evaluation(self, training_metrics=None, aggregate_episodes: bool = True):
    """One epoch of evaluation: the reference's metric dict (`eval/episode_*`
    means over the envs, or the per-env tensors), merged over
    `training_metrics`."""
    self._key, reset_key = wrappers.split_key(self._key)
    t = time.time()
    first = self.first_state = self.env.reset(reset_key)
    B, A = first.obs.shape[0], self.env.action_size
    # each run's noise continues the counter stream where the last one ended
    stride = 2 * B * A
    self.state = eval_rollout(self.env, first, k=self.unroll_length, policy=self.policy,
                              seed=self.seed, offset=self._runs * self.unroll_length * stride,
                              step_stride=stride, fused=self.fused)
    self._runs += 1
    em = self.state.info['eval_metrics']
    if em.active_episodes.is_cuda:
      torch.cuda.synchronize(em.active_episodes.device)
    epoch_eval_time = time.time() - t
    metrics = {f'eval/episode_{name}': value.mean() if aggregate_episodes else value
               for name, value in em.episode_metrics.items()}
    metrics['eval/avg_episode_length'] = em.episode_steps.mean()
    metrics['eval/epoch_eval_time'] = epoch_eval_time
    metrics['eval/sps'] = self._steps_per_unroll / epoch_eval_time
    self._eval_walltime = self._eval_walltime + epoch_eval_time
    return {'eval/walltime': self._eval_walltime, **(training_metrics or {}), **metrics}
