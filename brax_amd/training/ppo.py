"""PPO on the fused rollouts (`brax/training/agents/ppo/train.py`).

`train` keeps the reference's arguments, asserts, step accounting and
evaluation schedule on one device. One training step is

* `batch_size * num_minibatches // num_envs` consecutive `policy_rollout`
  launches of `unroll_length` steps (envs the kernel refuses take its chained
  path),
* the normaliser update from the unroll's observations,
* `num_updates_per_batch` passes, each one permutation of the sequences and
  `num_minibatches` Adam steps on `ppo_loss`,

after which the policy's weights are copied into the acting `MLPPolicy` in
place (`load_`: the buffer the rollout kernel reads keeps its address).
`Learner` holds that state and exposes the three phases; `train` is the loop
around it with `Evaluator` as the reference's `acting.Evaluator`.
"""
import dataclasses
from typing import Callable, Optional

import numpy as np
import torch

from brax_amd.envs import wrappers
from brax_amd.envs.policy import policy_rollout
from brax_amd.training import driver
from brax_amd.training import networks as ppo_networks
from brax_amd.training import optim
from brax_amd.training.losses import Transition, ppo_loss
from brax_amd.training.ppo_head import METRICS
from brax_amd.training.running_statistics import RunningStatistics


@dataclasses.dataclass(frozen=True)
class StepAccounting:
  """`ppo/train.py:103-110`."""
  env_step_per_training_step: int
  num_evals_after_init: int
  num_training_steps_per_epoch: int
  unrolls_per_training_step: int


def step_accounting(num_timesteps: int, num_evals: int, batch_size: int, unroll_length: int,
                    num_minibatches: int, action_repeat: int, num_envs: int) -> StepAccounting:
  assert batch_size * num_minibatches % num_envs == 0
  env_step_per_training_step = batch_size * unroll_length * num_minibatches * action_repeat
  num_evals_after_init = max(num_evals - 1, 1)
  # ceil(num_timesteps / (num_evals * env_step_per_training_step))
  num_training_steps_per_epoch = -(-num_timesteps // (num_evals_after_init
                                                      * env_step_per_training_step))
  return StepAccounting(env_step_per_training_step, num_evals_after_init,
                        num_training_steps_per_epoch, batch_size * num_minibatches // num_envs)


def transitions(obs0: torch.Tensor, traj, extras) -> Transition:
  """One unroll as `acting.actor_step` records it (`training/acting.py:30-50`),
  leading dimensions `[B, T]` (views of the trajectory, no copies but the
  observation shift): observation_t is the obs before step t (`obs0`, then the
  trajectory's), next_observation_t the obs after it (under AutoReset the
  reset obs), discount = 1 - done."""
  observation = torch.cat([obs0[None].to(traj.obs.dtype), traj.obs[:-1]], dim=0)
  t = Transition(observation=observation, action=extras.action, reward=traj.reward,
                 discount=1 - traj.done, next_observation=traj.obs, truncation=traj.truncation,
                 raw_action=extras.raw_action, log_prob=extras.log_prob)
  return t.map(lambda x: x.transpose(0, 1))


def make_optimizer(params, learning_rate: float, fused_adam=False):
  """Adam over `params`: `torch.optim.Adam` (`fused_adam` False), or
  `optim.FusedAdam`, one launch per step (True: that or NotImplementedError;
  None: that where it applies). Both have `zero_grad` and `step`."""
  return (optim.make_adam([dict(params=params, lr=learning_rate)], fused_adam)
          or torch.optim.Adam(params, lr=learning_rate, eps=1e-8))


class Learner(driver.GradientLearner):
  """The state of one PPO run and the three phases of a training step."""

  policy_kwargs = dict(activation='swish')

  def __init__(self, env, num_envs: int, unroll_length: int, batch_size: int,
               num_minibatches: int, num_updates_per_batch: int, learning_rate: float = 1e-4,
               entropy_cost: float = 1e-4, discounting: float = 0.9, reward_scaling: float = 1.0,
               clipping_epsilon: float = 0.3, gae_lambda: float = 0.95,
               normalize_observations: bool = False, normalize_advantage: bool = True,
               seed: int = 0, network_factory=ppo_networks.make_ppo_networks, device=None,
               fused_gae: Optional[bool] = None, action_repeat: int = 1, fused_mlp=False,
               fused_head=False, fused_adam=False, fused_group=False):
    assert batch_size * num_minibatches % num_envs == 0
    self.env, self.device = env, torch.device(device)
    self.action_repeat = int(action_repeat)
    self.num_envs, self.unroll_length = int(num_envs), int(unroll_length)
    self.batch_size, self.num_minibatches = int(batch_size), int(num_minibatches)
    self.num_updates_per_batch = int(num_updates_per_batch)
    self.unrolls = batch_size * num_minibatches // num_envs
    self.seed, self.fused_gae, self.fused_mlp = int(seed), fused_gae, fused_mlp
    self.fused_head, self.fused_adam, self.fused_group = fused_head, fused_adam, fused_group
    self.loss_kwargs = dict(entropy_cost=entropy_cost, discounting=discounting,
                            reward_scaling=reward_scaling, gae_lambda=gae_lambda,
                            clipping_epsilon=clipping_epsilon,
                            normalize_advantage=normalize_advantage)
    O, A = env.observation_size, env.action_size
    self.policy_layers, self.value_layers = network_factory(O, A, seed=seed, device=self.device)
    self.normalizer = RunningStatistics(O, self.device) if normalize_observations else None
    # optax.adam's defaults (eps 1e-8, as torch's)
    self.optimizer = make_optimizer(
        ppo_networks.parameters(self.policy_layers, self.value_layers), learning_rate, fused_adam)
    self.actor = self.make_policy(self.params)
    self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
    self._noise_offset = 0
    self.state = None
    self.env_steps = 0

  @property
  def params(self):
    """(normaliser, policy layers, value layers)."""
    return self.normalizer, self.policy_layers, self.value_layers

  def collect(self) -> Transition:
    """The unroll phase: `[batch_size * num_minibatches, unroll_length]`
    transitions from consecutive `policy_rollout` launches."""
    parts = []
    A = self.env.action_size
    for _ in range(self.unrolls):
      obs0 = self.state.obs
      self.state, traj, extras = policy_rollout(
          self.env, self.state, self.actor, self.unroll_length, seed=self.seed,
          offset=self._noise_offset, fused=None)
      self._noise_offset += self.unroll_length * 2 * self.num_envs * A
      parts.append(transitions(obs0, traj, extras))
    if len(parts) == 1:
      return parts[0]
    names = [f.name for f in dataclasses.fields(Transition)]
    return Transition(**{n: torch.cat([getattr(p, n) for p in parts], dim=0) for n in names})

  def update_normalizer(self, data: Transition):
    if self.normalizer is not None:
      self.normalizer.update(data.observation)

  def update(self, data: Transition):
    """The update phase: `num_updates_per_batch` x `num_minibatches` Adam
    steps; returns the mean of each loss metric (device tensors)."""
    n, bs = data.reward.shape[0], self.batch_size
    A = data.action.shape[-1]
    sums = {}
    for _ in range(self.num_updates_per_batch):
      perm = torch.randperm(n, generator=self._gen, device=self.device)
      shuffled = data.map(lambda x, perm=perm: x[perm])
      for m in range(self.num_minibatches):
        mb = shuffled.map(lambda x, m=m: x[m * bs:(m + 1) * bs])
        eps = torch.randn((bs, self.unroll_length, A), generator=self._gen, device=self.device)
        loss, metrics = ppo_loss(self.policy_layers, self.value_layers, self._mean_std, mb, eps,
                                 fused=self.fused_gae, fused_mlp=self.fused_mlp,
                                 fused_head=self.fused_head, fused_group=self.fused_group,
                                 **self.loss_kwargs)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        # (the fused head's four metrics are one (4,) tensor: one add, not four)
        driver.add_metrics(sums, metrics)
    self.actor.load_(ppo_networks.detached(self.policy_layers))
    return driver.mean_metrics(sums, self.num_updates_per_batch * self.num_minibatches, METRICS)

  def training_step(self):
    data = self.collect()
    self.update_normalizer(data)
    metrics = self.update(data)
    self.env_steps += data.reward.numel() * self.action_repeat
    return metrics


def train(environment, num_timesteps: int, episode_length: int, action_repeat: int = 1,
          num_envs: int = 1, max_devices_per_host: Optional[int] = None,
          num_eval_envs: int = 128, learning_rate: float = 1e-4, entropy_cost: float = 1e-4,
          discounting: float = 0.9, seed: int = 0, unroll_length: int = 10, batch_size: int = 32,
          num_minibatches: int = 16, num_updates_per_batch: int = 2, num_evals: int = 1,
          normalize_observations: bool = False, reward_scaling: float = 1.0,
          clipping_epsilon: float = 0.3, gae_lambda: float = 0.95,
          deterministic_eval: bool = False, network_factory=ppo_networks.make_ppo_networks,
          progress_fn: Callable[[int, dict], None] = lambda *args: None,
          normalize_advantage: bool = True, eval_env=None, device=None,
          fused_gae: Optional[bool] = None, fused_mlp=False, fused_head=False, fused_adam=False,
          fused_group=False):
  """PPO training; the reference's arguments and defaults
  (`ppo/train.py:61-86`).

  Args:
    environment: an env name (created with the Episode / Vector / AutoReset
      wrappers at `num_envs`), or such a batched env.
    max_devices_per_host: accepted and ignored (one device).
    eval_env: with a batched `environment`, the same env batched at
      `num_eval_envs` (a name is created at both sizes).
    device: the GPU (default `cuda`).
    fused_gae: `compute_gae`'s `fused` (None: the kernel).
    fused_mlp: the loss's networks through `fused_mlp.fused_mlp` (False: chained
      torch; True: the kernels or NotImplementedError; None: the kernels where
      they apply).
    fused_head: the loss after the networks through `ppo_head.ppo_head` (False:
      chained torch; True: `bx_ppo_head` or NotImplementedError; None: the
      kernel where it applies); where the kernel is taken it runs its own GAE
      scan and `fused_gae` is not consulted.
    fused_adam: the optimiser (False: `torch.optim.Adam`; True:
      `optim.FusedAdam`, one launch per Adam step, or NotImplementedError; None:
      `FusedAdam` where it applies).
    fused_group: `ppo_loss`'s: the loss's three network evaluations share one
      forward launch, the two networks' backward passes two (off by default; it
      needs `fused_mlp`).
  Returns:
    `(make_policy, params, metrics)`: `make_policy(params, deterministic=False)`
    gives an `MLPPolicy`; `params` is (the normaliser or None, the policy
    layers, the value layers); `metrics` the last evaluation's dict with
    `training/sps` and `training/walltime`.
  """
  del max_devices_per_host
  acct = step_accounting(num_timesteps, num_evals, batch_size, unroll_length, num_minibatches,
                         action_repeat, num_envs)
  dev = torch.device('cuda' if device is None else device)
  env, eval_env = driver.make_envs(environment, eval_env, num_envs, num_eval_envs, episode_length,
                                   action_repeat, dev)
  learner = Learner(env, num_envs, unroll_length, batch_size, num_minibatches,
                    num_updates_per_batch, learning_rate=learning_rate, entropy_cost=entropy_cost,
                    discounting=discounting, reward_scaling=reward_scaling,
                    clipping_epsilon=clipping_epsilon, gae_lambda=gae_lambda,
                    normalize_observations=normalize_observations,
                    normalize_advantage=normalize_advantage, seed=seed,
                    network_factory=network_factory, device=dev, fused_gae=fused_gae,
                    action_repeat=action_repeat, fused_mlp=fused_mlp, fused_head=fused_head,
                    fused_adam=fused_adam, fused_group=fused_group)
  # jax.random.PRNGKey(seed) layout; the evaluator's key is the split's other half
  learner.reset(wrappers.split_key(np.array([0, int(seed)], np.uint32))[0])
  eval_policy = learner.make_policy(deterministic=True) if deterministic_eval else learner.actor
  evaluator = driver.make_evaluator(eval_env, eval_policy, seed, num_eval_envs, episode_length,
                                    action_repeat, dev)
  metrics = driver.run_epochs(
      learner, eval_policy, evaluator, acct.num_evals_after_init,
      acct.num_training_steps_per_epoch,
      acct.num_training_steps_per_epoch * acct.env_step_per_training_step, num_timesteps,
      num_evals > 1, progress_fn)
  return learner.make_policy, learner.params, metrics
