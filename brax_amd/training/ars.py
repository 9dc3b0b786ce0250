"""Augmented random search on the one-launch population episode
(`brax/training/agents/ars/train.py`, https://arxiv.org/pdf/1803.07055.pdf).

The policy is `obs @ W` with `W` starting at zeros: an `MLPPolicy` of one
layer with the identity head, packed as `(W, zeros)`. The bias is frozen: the
perturbation leaves it at zero, the weighted noise sum gives it no update, and
its counters are skipped, so `W`'s noise does not depend on it.

An epoch is `es.py`'s with ARS's optimiser half: the `top_directions`
directions of the largest `max(r+, r-)` (ties to the lower index) weigh `r+ -
r-`, the others 0 (the kernel skips them), and `theta += step_size * sum /
(top_directions * reward_std)`, `reward_std` the population std of the `2 *
top_directions` selected scores (zero gives what IEEE gives, as in the
reference). `train` keeps the reference's arguments, defaults, asserts and its
own evaluation schedule (no initial evaluation).
"""
import dataclasses
from typing import Callable, Optional, Tuple

import torch

from brax_amd.training import driver, es


def ars_weights(scores: torch.Tensor, top_directions: int
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """`ars/train.py:176-191` in float64: of `(2 * directions,)` scores, the
  direction weights `reward_weight * (r+ - r-)`, the 0 / 1 `reward_weight`
  (rank of `-max(r+, r-)` below `top_directions`, stable) and `reward_std`,
  the population std of the scores whose direction is selected."""
  s = scores.reshape(-1).to(torch.float64)
  half = s.shape[0] // 2
  plus, minus = s[:half], s[half:]
  rank = torch.argsort(torch.argsort(-torch.maximum(plus, minus), stable=True), stable=True)
  reward_weight = (rank < top_directions).to(torch.float64)
  chosen = torch.cat([reward_weight, reward_weight]) != 0
  reward_std = s[chosen].std(unbiased=False)
  return reward_weight * (plus - minus), reward_weight, reward_std


@dataclasses.dataclass(frozen=True)
class EvalSchedule:
  """`ars/train.py:87-88`: no initial evaluation."""
  num_env_steps_between_evals: int
  first_eval_step: int


def eval_schedule(num_timesteps: int, num_evals: int) -> EvalSchedule:
  between = num_timesteps // num_evals
  return EvalSchedule(between, num_timesteps - (num_evals - 1) * between)


def make_policy_network(observation_size: int, action_size: int, seed: int = 0, device=None,
                        dtype=torch.float32):
  """`ars/networks.py:27-40`: `W = zeros((observation_size, action_size))`,
  as one layer with a zero bias."""
  del seed
  return [(torch.zeros((observation_size, action_size), device=device, dtype=dtype),
           torch.zeros((action_size,), device=device, dtype=dtype))]


class Learner(es.EvolutionLearner):
  """The state of one ARS run; `epoch()` is one `training_epoch`."""

  head = 'identity'

  def __init__(self, env, number_of_directions: int = 60, top_directions: int = 20,
               step_size: float = 0.015, episode_length: int = 1000, action_repeat: int = 1,
               exploration_noise_std: float = 0.025, seed: int = 0,
               normalize_observations: bool = False, reward_shift: float = 0.0,
               network_factory=make_policy_network, device=None, fused: Optional[bool] = None):
    dev = torch.device('cuda' if device is None else device)
    layers = network_factory(env.observation_size, env.action_size, seed=seed, device=dev)
    if len(layers) != 1:
      raise ValueError('the ARS policy is one matrix')
    w, b = layers[0]
    frozen = torch.cat([torch.zeros(w.numel(), dtype=torch.uint8),
                        torch.ones(b.numel(), dtype=torch.uint8)])
    self.reward_shift = float(reward_shift)
    super().__init__(env, layers, number_of_directions, episode_length, action_repeat,
                     exploration_noise_std, seed, normalize_observations, dev, frozen=frozen,
                     fused=fused)
    self.number_of_directions = int(number_of_directions)
    self.top_directions = min(int(top_directions), self.number_of_directions)
    self.step_size = float(step_size)

  def step(self, delta, reward_std):
    """`ars/train.py:193-195` in float32, the frozen bias left alone."""
    new = self.theta + self.step_size * delta / (self.top_directions * reward_std.to(delta.dtype))
    return torch.where(self.frozen.bool(), self.theta, new)

  def epoch(self):
    """One training epoch. Returns its diagnostics: `scores` (2 P,) float32,
    `weights` (P,) float64, `delta` (n_params,) float32 (the weighted noise
    sum), `reward_weight`, `reward_std`, `metrics` (the reference's four),
    `result` and the keys and counters the episodes used."""
    result, used = self.run_episodes()
    scores = result.scores
    weights, reward_weight, reward_std = ars_weights(scores, self.top_directions)
    delta = self.noise_sum(weights)
    self.theta.copy_(self.step(delta, reward_std))
    self.publish()
    return dict(scores=scores, weights=weights, delta=delta, reward_weight=reward_weight,
                reward_std=reward_std, result=result,
                metrics=self.training_metrics(scores, reward_weight), **used)


def train(environment, num_timesteps: int = 100, episode_length: int = 1000,
          action_repeat: int = 1, max_devices_per_host: Optional[int] = None,
          number_of_directions: int = 60, top_directions: int = 20, step_size: float = 0.015,
          num_eval_envs: int = 128, exploration_noise_std: float = 0.025, seed: int = 0,
          normalize_observations: bool = False, num_evals: int = 1, reward_shift: float = 0.0,
          network_factory=make_policy_network,
          progress_fn: Callable[[int, dict], None] = lambda *args: None, eval_env=None,
          device=None, fused: Optional[bool] = None):
  """ARS training; the reference's arguments and defaults
  (`ars/train.py:51-70`).

  Args:
    environment: an env name (created with the Episode / Vector / AutoReset
      wrappers at `2 * number_of_directions`), or such a batched env.
    max_devices_per_host: accepted and ignored (one device).
    eval_env: with a batched `environment`, the same env batched at
      `num_eval_envs` (a name is created at both sizes).
    device: the GPU (default `cuda`).
    fused: `perturb_`'s and `weighted_noise_sum`'s `fused` (None: the kernels).
  Returns:
    `(make_policy, params, metrics)`: `make_policy(params)` gives an
    `MLPPolicy` with the identity head; `params` is (the normaliser or None,
    `[(W, zero bias)]`); `metrics` the last evaluation's dict.
  """
  del max_devices_per_host
  num_envs = number_of_directions * 2  # noise + anti noise
  sched = eval_schedule(num_timesteps, num_evals)
  dev = torch.device('cuda' if device is None else device)
  env, eval_env = driver.make_envs(environment, eval_env, num_envs, num_eval_envs, episode_length,
                                   action_repeat, dev)
  learner = Learner(env, number_of_directions, top_directions, step_size, episode_length,
                    action_repeat, exploration_noise_std, seed, normalize_observations,
                    reward_shift, network_factory, dev, fused)
  evaluator = driver.make_evaluator(eval_env, learner.policy, seed, num_eval_envs, episode_length,
                                    action_repeat, dev)
  metrics = driver.run(learner, learner.policy, evaluator, num_timesteps, sched.first_eval_step,
                       sched.num_env_steps_between_evals, False, progress_fn)
  return learner.make_policy, learner.params, metrics
