"""SAC on the fused rollouts and a device replay queue
(`brax/training/agents/sac/train.py`).

`train` keeps the reference's arguments, defaults, checks, step accounting and
evaluation schedule on one device. One training step is

* `get_experience`: one `policy_rollout(k=1)` (the reference's
  `acting.actor_step`), the normaliser update from the observation the policy
  read, and one `UniformSamplingQueue.insert` launch;
* one `sample` launch of `batch_size * grad_updates_per_step` rows;
* `grad_updates_per_step` times `sgd_step`: the alpha, critic and actor Adam
  steps and the target network's update,

after which the policy's weights are copied into the acting `MLPPolicy` in
place. The two buffer launches remove small launches and the dependence on a
generator's state; the updates, 3 Adam steps of torch MLPs per gradient step,
are where a training step's time goes.

The acting launch: `policy_rollout`'s kernel takes layers up to
`abi.POLICY_MAX_WIDTH` = 128 wide, so the reference's default `(256, 256)`
policy acts through `policy_rollout`'s chained path (one `bx_normal_slabs`
launch, the torch MLP and `env.step`), and `(128, 128)` or narrower acts in the
fused launch. The noise and the results are the same by construction.
"""
import dataclasses
from typing import Callable, List, Mapping, Optional, Tuple

import numpy as np
import torch

from brax_amd.envs import wrappers
from brax_amd.envs.policy import policy_rollout
from brax_amd.fused import use_kernel
from brax_amd.training import driver, optim, sac_head, sac_losses, sac_networks
from brax_amd.training.networks import Layers, detached, parameters
from brax_amd.training.running_statistics import RunningStatistics
from brax_amd.training.replay_buffers import UniformSamplingQueue, transition_fields

ALPHA_LEARNING_RATE = 3e-4  # train.py:178


@dataclasses.dataclass(frozen=True)
class StepAccounting:
  """`sac/train.py:139-159`."""
  max_replay_size: int
  env_steps_per_actor_step: int
  num_prefill_actor_steps: int
  num_prefill_env_steps: int
  num_evals_after_init: int
  num_training_steps_per_epoch: int


def step_accounting(num_timesteps: int, num_evals: int, min_replay_size: int, num_envs: int,
                    action_repeat: int, max_replay_size: Optional[int] = None) -> StepAccounting:
  if min_replay_size >= num_timesteps:
    raise ValueError('No training will happen because min_replay_size >= num_timesteps')
  if max_replay_size is None:
    max_replay_size = num_timesteps
  env_steps_per_actor_step = action_repeat * num_envs
  # ceil(min_replay_size / num_envs)
  num_prefill_actor_steps = -(-min_replay_size // num_envs)
  num_prefill_env_steps = num_prefill_actor_steps * env_steps_per_actor_step
  assert num_timesteps - num_prefill_env_steps >= 0
  num_evals_after_init = max(num_evals - 1, 1)
  # ceil((num_timesteps - num_prefill_env_steps) / (num_evals_after_init * env_steps_per_actor_step))
  num_training_steps_per_epoch = -(-(num_timesteps - num_prefill_env_steps)
                                   // (num_evals_after_init * env_steps_per_actor_step))
  return StepAccounting(int(max_replay_size), env_steps_per_actor_step, num_prefill_actor_steps,
                        num_prefill_env_steps, num_evals_after_init, num_training_steps_per_epoch)


@dataclasses.dataclass
class TrainingState:
  """`sac/train.py:53-65` without the normaliser and the env-step count (the
  `Learner` holds those): the parameters and their three optimisers, or, in
  their place (all three None), one `optim.FusedAdam` over the three groups
  that also owns the target update."""
  policy_layers: Layers
  q_layers: List[Layers]
  target_q_layers: List[Layers]
  log_alpha: torch.Tensor
  policy_optimizer: Optional[torch.optim.Optimizer]
  q_optimizer: Optional[torch.optim.Optimizer]
  alpha_optimizer: Optional[torch.optim.Optimizer]
  gradient_steps: int = 0
  fused_optimizer: Optional[optim.FusedAdam] = None


def init_training_state(observation_size: int, action_size: int, learning_rate: float = 1e-4,
                        network_factory=sac_networks.make_sac_networks, seed: int = 0,
                        device=None, dtype=torch.float32, fused_adam=False,
                        tau: float = 0.005) -> TrainingState:
  """`_init_training_state`: log_alpha 0, the target q network a copy of the
  q network, optax.adam's defaults (eps 1e-8, as torch's).

  `fused_adam` other than False puts one `optim.FusedAdam` in the three torch
  optimisers' place (True: that or NotImplementedError; None: that where it
  applies): log_alpha, the q tensors with their targets and `tau`, the policy
  tensors, in that order."""
  policy, q = network_factory(observation_size, action_size, seed=seed, device=device, dtype=dtype)
  target = [[(w.detach().clone(), b.detach().clone()) for w, b in c] for c in q]
  log_alpha = torch.zeros((), dtype=dtype, device=device, requires_grad=True)
  fused = optim.make_adam(
      [dict(params=[log_alpha], lr=ALPHA_LEARNING_RATE),
       dict(params=sac_networks.q_parameters(q), lr=learning_rate,
            targets=sac_networks.q_parameters(target), tau=tau),
       dict(params=parameters(policy), lr=learning_rate)], fused_adam)
  if fused is not None:
    return TrainingState(policy_layers=policy, q_layers=q, target_q_layers=target,
                         log_alpha=log_alpha, policy_optimizer=None, q_optimizer=None,
                         alpha_optimizer=None, fused_optimizer=fused)
  return TrainingState(
      policy_layers=policy, q_layers=q, target_q_layers=target, log_alpha=log_alpha,
      policy_optimizer=torch.optim.Adam(parameters(policy), lr=learning_rate, eps=1e-8),
      q_optimizer=torch.optim.Adam(sac_networks.q_parameters(q), lr=learning_rate, eps=1e-8),
      alpha_optimizer=torch.optim.Adam([log_alpha], lr=ALPHA_LEARNING_RATE, eps=1e-8))


def _apply(optimizer, params, grads):
  for p, g in zip(params, grads):
    p.grad = g
  optimizer.step()
  optimizer.zero_grad(set_to_none=True)


def _chained_gradients(ts: TrainingState, normalizer, transitions, eps, reward_scaling, discounting,
                       fused_mlp, fused_group=False):
  """The three losses as torch expressions (`sac_losses`) and autograd's
  gradients of them: `(a_grads, c_grads, p_grads, metrics)`."""
  eps_alpha, eps_critic, eps_actor = eps
  policy_params = parameters(ts.policy_layers)
  q_params = sac_networks.q_parameters(ts.q_layers)
  a_loss = sac_losses.alpha_loss(ts.log_alpha, ts.policy_layers, normalizer, transitions, eps_alpha,
                                 fused_mlp, fused_group)
  alpha = torch.exp(ts.log_alpha.detach())
  c_loss = sac_losses.critic_loss(ts.q_layers, ts.policy_layers, normalizer, ts.target_q_layers,
                                  alpha, transitions, eps_critic, reward_scaling, discounting,
                                  fused_mlp, fused_group)
  p_loss = sac_losses.actor_loss(ts.policy_layers, normalizer, ts.q_layers, alpha, transitions,
                                 eps_actor, fused_mlp, fused_group)
  a_grads = torch.autograd.grad(a_loss, [ts.log_alpha])
  c_grads = torch.autograd.grad(c_loss, q_params)
  p_grads = torch.autograd.grad(p_loss, policy_params)
  return a_grads, c_grads, p_grads, {'critic_loss': c_loss.detach(), 'actor_loss': p_loss.detach(),
                                     'alpha_loss': a_loss.detach()}


def _gradients(ts, normalizer, transitions, eps, reward_scaling, discounting, fused_mlp, fused_head,
               fused_group=False):
  if use_kernel(fused_head, 'sac head',
                lambda: sac_head.fused_supported(ts, normalizer, transitions, eps)):
    return sac_head.gradients(ts, normalizer, transitions, eps, reward_scaling, discounting,
                              fused_mlp, fused_group)
  return _chained_gradients(ts, normalizer, transitions, eps, reward_scaling, discounting, fused_mlp,
                            fused_group)


def sgd_step(ts: TrainingState, normalizer, transitions: Mapping[str, torch.Tensor],
             eps: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], reward_scaling: float = 1.0,
             discounting: float = 0.9, tau: float = 0.005, fused_mlp=False, fused_head=False,
             fused_group=False):
  """One gradient step in the reference's order (`train.py:214-269`).

  The alpha update comes first, but the critic and actor losses read `exp` of
  the OLD `log_alpha`; the critic reads the old policy and the actor the OLD q
  parameters. Every loss is therefore a function of the state before the step:
  the three gradients are taken first and the three Adam steps applied after,
  which is that order with in-place optimisers. Then target = target * (1 -
  tau) + q * tau with the new q, and the metric `alpha` is `exp` of the NEW
  `log_alpha`.

  With `ts.fused_optimizer` the three Adam steps and the target update are its
  one `step` call (one launch); `tau` must then be the one it was built with.

  Args:
    normalizer: `(mean, std)` or None.
    eps: the standard-normal draws `(B, A)` of the alpha, critic and actor
      losses' samples (the reference's three keys).
    fused_mlp: the losses' `fused_mlp` (`networks.mlp`'s `fused`).
    fused_head: how the three gradients are taken (False: `sac_losses` and
      autograd; True: `sac_head.gradients`, four launches between the networks,
      or NotImplementedError; None: that where it applies).
    fused_group: networks evaluated at the same point of the step share
      launches (`networks.mlp_many`): with the head the critics' twelve launches
      become three, without it each `q_apply` groups its critics. It needs the
      MLP kernels: with `fused_mlp=False`, True raises and None falls back.
  Returns:
    the metrics (detached tensors): critic_loss, actor_loss, alpha_loss, alpha;
    from the kernels a `sac_head.Metrics`, whose `vector` is the three losses.
  """
  if ts.fused_optimizer is not None and tau != ts.fused_optimizer.groups[1]['tau']:
    raise ValueError(f"tau {tau} is not the fused optimiser's {ts.fused_optimizer.groups[1]['tau']}")
  policy_params = parameters(ts.policy_layers)
  q_params = sac_networks.q_parameters(ts.q_layers)
  a_grads, c_grads, p_grads, metrics = _gradients(ts, normalizer, transitions, eps, reward_scaling,
                                                  discounting, fused_mlp, fused_head, fused_group)
  if ts.fused_optimizer is not None:
    ts.fused_optimizer.step(grads=[*a_grads, *c_grads, *p_grads])
  else:
    _apply(ts.alpha_optimizer, [ts.log_alpha], a_grads)
    _apply(ts.q_optimizer, q_params, c_grads)
    _apply(ts.policy_optimizer, policy_params, p_grads)
    with torch.no_grad():
      for tc, qc in zip(ts.target_q_layers, ts.q_layers):
        for t_wb, q_wb in zip(tc, qc):
          for t, q in zip(t_wb, q_wb):
            t.copy_(t * (1 - tau) + q * tau)
  ts.gradient_steps += 1
  metrics['alpha'] = torch.exp(ts.log_alpha.detach())
  return metrics


class Learner(driver.GradientLearner):
  """The state of one SAC run and the phases of a training step."""

  policy_kwargs = dict(activation=sac_networks.ACTIVATION, min_std=sac_losses.MIN_STD)

  def __init__(self, env, num_envs: int, batch_size: int = 256, grad_updates_per_step: int = 1,
               max_replay_size: int = 1 << 20, num_prefill_actor_steps: int = 0,
               learning_rate: float = 1e-4, discounting: float = 0.9, reward_scaling: float = 1.0,
               tau: float = 0.005, normalize_observations: bool = False, seed: int = 0,
               network_factory=sac_networks.make_sac_networks, device=None,
               action_repeat: int = 1, fused_buffer: Optional[bool] = None, fused_mlp=False,
               fused_adam=False, fused_head=False, fused_group=False):
    self.env, self.device = env, torch.device(device)
    self.num_envs, self.action_repeat = int(num_envs), int(action_repeat)
    self.batch_size, self.grad_updates_per_step = int(batch_size), int(grad_updates_per_step)
    self.num_prefill_actor_steps = int(num_prefill_actor_steps)
    self.seed, self.fused_buffer, self.fused_mlp = int(seed), fused_buffer, fused_mlp
    self.loss_kwargs = dict(reward_scaling=reward_scaling, discounting=discounting, tau=tau)
    O, A = env.observation_size, env.action_size
    self.fused_adam, self.fused_head, self.fused_group = fused_adam, fused_head, fused_group
    self.ts = init_training_state(O, A, learning_rate, network_factory, seed, self.device,
                                  fused_adam=fused_adam, tau=tau)
    self.normalizer = RunningStatistics(O, self.device) if normalize_observations else None
    self.buffer = UniformSamplingQueue(max_replay_size, transition_fields(O, A),
                                       self.batch_size * self.grad_updates_per_step, seed=seed,
                                       device=self.device)
    self.actor = self.make_policy(self.params)
    self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
    self._noise_offset = 0
    self.state = None
    self.env_steps = 0

  @property
  def params(self):
    """(normaliser, policy layers), the reference's returned `params`."""
    return self.normalizer, self.ts.policy_layers

  def get_experience(self):
    """`get_experience` (`train.py:271-287`): one actor step, the normaliser
    update from the observation the policy read, the insert."""
    obs0 = self.state.obs
    self.state, traj, extras = policy_rollout(self.env, self.state, self.actor, 1, seed=self.seed,
                                              offset=self._noise_offset, fused=None)
    self._noise_offset += 2 * self.num_envs * self.env.action_size
    if self.normalizer is not None:
      self.normalizer.update(obs0)
    self.buffer.insert(
        {'observation': obs0, 'action': extras.action[0], 'reward': traj.reward[0],
         'discount': 1 - traj.done[0], 'next_observation': traj.obs[0],
         'truncation': traj.truncation[0]}, fused=self.fused_buffer)
    self.env_steps += self.action_repeat * self.num_envs

  def prefill(self):
    """`prefill_replay_buffer`: `num_prefill_actor_steps` actor steps with the
    initial policy, no updates."""
    for _ in range(self.num_prefill_actor_steps):
      self.get_experience()

  def update(self, transitions: Mapping[str, torch.Tensor]):
    """`grad_updates_per_step` gradient steps on consecutive `batch_size`
    slices of the sample; returns the mean of each metric (device tensors)."""
    A = self.env.action_size
    sums = {}
    for g in range(self.grad_updates_per_step):
      mb = {k: v[g * self.batch_size:(g + 1) * self.batch_size] for k, v in transitions.items()}
      eps = tuple(torch.randn((self.batch_size, A), generator=self._gen, device=self.device)
                  for _ in range(3))
      metrics = sgd_step(self.ts, self._mean_std, mb, eps, fused_mlp=self.fused_mlp,
                         fused_head=self.fused_head, fused_group=self.fused_group,
                         **self.loss_kwargs)
      # (the fused head's three losses in one addition, alpha in another)
      driver.add_metrics(sums, metrics)
    self.actor.load_(detached(self.ts.policy_layers))
    return driver.mean_metrics(sums, self.grad_updates_per_step, sac_head.METRICS)

  def training_step(self):
    """`training_step` (`train.py:289-313`)."""
    self.get_experience()
    metrics = self.update(self.buffer.sample(fused=self.fused_buffer))
    metrics['buffer_current_size'] = self.buffer.size
    metrics['buffer_current_position'] = self.buffer.position
    return metrics


def train(environment, num_timesteps: int, episode_length: int, action_repeat: int = 1,
          num_envs: int = 1, num_eval_envs: int = 128, learning_rate: float = 1e-4,
          discounting: float = 0.9, seed: int = 0, batch_size: int = 256, num_evals: int = 1,
          normalize_observations: bool = False, max_devices_per_host: Optional[int] = None,
          reward_scaling: float = 1.0, tau: float = 0.005, min_replay_size: int = 0,
          max_replay_size: Optional[int] = None, grad_updates_per_step: int = 1,
          deterministic_eval: bool = False, network_factory=sac_networks.make_sac_networks,
          progress_fn: Callable[[int, dict], None] = lambda *args: None,
          checkpoint_logdir: Optional[str] = None, eval_env=None, device=None,
          fused_buffer: Optional[bool] = None, fused_mlp=False, fused_adam=False,
          fused_head=False, fused_group=False):
  """SAC training; the reference's arguments and defaults
  (`sac/train.py:106-129`).

  Args:
    environment: an env name (created with the Episode / Vector / AutoReset
      wrappers at `num_envs`), or such a batched env.
    max_devices_per_host: accepted and ignored (one device).
    max_replay_size: the queue's capacity in rows (default `num_timesteps`).
    network_factory: `make_sac_networks`; with its default `(256, 256)` the
      policy is wider than `abi.POLICY_MAX_WIDTH` = 128 and acts through
      `policy_rollout`'s chained path, `(128, 128)` or narrower in the fused
      launch (`functools.partial(make_sac_networks, hidden_layer_sizes=...)`).
    checkpoint_logdir: must be None (io is out of scope).
    eval_env: with a batched `environment`, the same env batched at
      `num_eval_envs` (a name is created at both sizes).
    device: the GPU (default `cuda`).
    fused_buffer: the queue's `fused` (None: the kernels).
    fused_mlp: the losses' networks through `fused_mlp.fused_mlp` (False: chained
      torch; True: the kernels or NotImplementedError; None: the kernels where
      they apply).
    fused_adam: the three Adam steps and the target update of a gradient step
      (False: three `torch.optim.Adam` and a loop over the target tensors; True:
      one `optim.FusedAdam` step, one launch, or NotImplementedError; None: that
      where it applies).
    fused_head: the three losses and their gradients between the networks
      (False: `sac_losses` and autograd; True: `sac_head.gradients`, four
      launches, or NotImplementedError; None: that where it applies).
    fused_group: `sgd_step`'s: the critics evaluated at the same point of a
      gradient step share launches (off by default; it needs `fused_mlp`).
  Returns:
    `(make_policy, params, metrics)`: `make_policy(params, deterministic=False)`
    gives an `MLPPolicy`; `params` is (the normaliser or None, the policy
    layers); `metrics` the last evaluation's dict with `training/sps`,
    `training/walltime`, the epoch's mean losses and alpha,
    `training/buffer_current_size` and `training/buffer_current_position`.
  """
  del max_devices_per_host
  if checkpoint_logdir is not None:
    raise NotImplementedError('checkpoint_logdir: saving parameters (brax.io) is out of scope')
  acct = step_accounting(num_timesteps, num_evals, min_replay_size, num_envs, action_repeat,
                         max_replay_size)
  dev = torch.device('cuda' if device is None else device)
  env, eval_env = driver.make_envs(environment, eval_env, num_envs, num_eval_envs, episode_length,
                                   action_repeat, dev)
  learner = Learner(env, num_envs, batch_size=batch_size,
                    grad_updates_per_step=grad_updates_per_step,
                    max_replay_size=acct.max_replay_size,
                    num_prefill_actor_steps=acct.num_prefill_actor_steps,
                    learning_rate=learning_rate, discounting=discounting,
                    reward_scaling=reward_scaling, tau=tau,
                    normalize_observations=normalize_observations, seed=seed,
                    network_factory=network_factory, device=dev, action_repeat=action_repeat,
                    fused_buffer=fused_buffer, fused_mlp=fused_mlp, fused_adam=fused_adam,
                    fused_head=fused_head, fused_group=fused_group)
  # jax.random.PRNGKey(seed) layout; the evaluator's key is the split's other half
  learner.reset(wrappers.split_key(np.array([0, int(seed)], np.uint32))[0])
  eval_policy = learner.make_policy(deterministic=True) if deterministic_eval else learner.actor
  evaluator = driver.make_evaluator(eval_env, eval_policy, seed, num_eval_envs, episode_length,
                                    action_repeat, dev)

  def prefill():
    learner.prefill()
    assert learner.buffer.size >= min_replay_size
  metrics = driver.run_epochs(
      learner, eval_policy, evaluator, acct.num_evals_after_init,
      acct.num_training_steps_per_epoch,
      acct.env_steps_per_actor_step * acct.num_training_steps_per_epoch, num_timesteps,
      num_evals > 1, progress_fn, prefill=prefill)
  return learner.make_policy, learner.params, metrics
