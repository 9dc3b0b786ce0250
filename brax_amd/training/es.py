"""Evolution strategies on the one-launch population episode
(`brax/training/agents/es/train.py`, https://arxiv.org/pdf/1703.03864.pdf).

`train` keeps the reference's arguments, defaults, asserts and evaluation
schedule on one device. One epoch is

1. `env.reset` with a fresh key,
2. `PolicyPopulation.perturb_`: rows theta +- sigma eps, eps regenerated on
   chip from the counter RNG (`bx_population_perturb`),
3. ONE `population_rollout` of `episode_length // action_repeat` steps (envs
   the population kernel refuses take its chained path),
4. the normaliser update from the launch's on-chip moments,
5. the fitness weights, in float64 (`es_weights`),
6. `weighted_noise_sum`: sum_p w_p eps_p with the same eps regenerated
   (`bx_population_delta`), so no `(population, n_params)` array is ever
   written or read,
7. Adam (optax's defaults) on `-(sum / population_size - l2coeff theta)`,
8. `policy.load_` in place: the buffer the kernels read keeps its address,
9. `num_env_steps += sum(obs_count) * action_repeat`.

The parameter noise of epoch e sits at counters `[e, e + 1) * 2 * population *
n_params` of its own seed; the action noise has another seed. `Learner` holds
the state and runs one epoch at a time; `train` is the loop around it with
`Evaluator` as the reference's `acting.Evaluator`.
"""
import dataclasses
import enum
import math
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from brax_amd.envs import wrappers
from brax_amd.envs.policy import MLPPolicy
from brax_amd.envs.population import PolicyPopulation, population_rollout
from brax_amd.training import driver, networks
from brax_amd.training.driver import run
from brax_amd.training.running_statistics import RunningStatistics

_SEED_MASK = 0x7FFFFFFFFFFFFFFF


def _ranks(x: torch.Tensor) -> torch.Tensor:
  """`jnp.argsort(jnp.argsort(x))`: rank 0 the smallest, ties in index order
  (both sorts stable, as jnp's)."""
  return torch.argsort(torch.argsort(x, stable=True), stable=True)


def centered_rank(x: torch.Tensor) -> torch.Tensor:
  """`es/train.py:54-57`, https://arxiv.org/pdf/1703.03864.pdf."""
  r = _ranks(x).to(torch.float64)
  return r / (len(x) - 1) - .5


def wierstra(x: torch.Tensor) -> torch.Tensor:
  """`es/train.py:62-65`,
  https://www.jmlr.org/papers/volume15/wierstra14a/wierstra14a.pdf."""
  n = len(x)
  r = (n - _ranks(x)).to(torch.float64)
  u = torch.clamp_min(math.log(n / 2.0 + 1) - torch.log(r), 0.)
  return u / u.sum() - 1.0 / n


class FitnessShaping(enum.Enum):
  ORIGINAL = 'original'
  CENTERED_RANK = 'centered_rank'
  WIERSTRA = 'wierstra'

  def __call__(self, x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.float64)
    if self is FitnessShaping.CENTERED_RANK:
      return centered_rank(x)
    if self is FitnessShaping.WIERSTRA:
      return wierstra(x)
    return x


def es_weights(scores: torch.Tensor, fitness_shaping: FitnessShaping = FitnessShaping.ORIGINAL,
               center_fitness: bool = False) -> torch.Tensor:
  """The `(population_size,)` float64 direction weights of `(2 *
  population_size,)` scores (`es/train.py:238-246`): shaped, optionally
  standardised with the population std, then noise half minus anti-noise
  half."""
  w = fitness_shaping(scores.reshape(-1))
  if center_fitness:
    w = (w - w.mean()) / (1e-6 + w.std(unbiased=False))
  half = w.shape[0] // 2
  return w[:half] - w[half:]


@dataclasses.dataclass(frozen=True)
class EvalSchedule:
  """`es/train.py:112-116`: an evaluation after the epoch that takes
  `num_env_steps` to `first_eval_step`, then every
  `num_env_steps_between_evals`."""
  num_evals_after_init: int
  num_env_steps_between_evals: int
  first_eval_step: int


def eval_schedule(num_timesteps: int, num_evals: int) -> EvalSchedule:
  num_evals_after_init = max(num_evals - 1, 1)
  between = num_timesteps // num_evals_after_init
  return EvalSchedule(num_evals_after_init, between,
                      num_timesteps - (num_evals_after_init - 1) * between)


def make_es_networks(observation_size: int, action_size: int,
                     hidden_layer_sizes: Sequence[int] = (32,) * 4, seed: int = 0, device=None,
                     dtype=torch.float32) -> networks.Layers:
  """`es/networks.py:52-70`: the policy MLP ending in `2 * action_size`
  NormalTanh parameters (relu between the layers, flax's `Dense` defaults)."""
  g = torch.Generator(device='cpu').manual_seed(int(seed))
  return networks.make_layers((observation_size, *hidden_layer_sizes, 2 * action_size), g, device,
                              dtype)


def unpack(flat: torch.Tensor, sizes):
  """Views `[(W (in, out), b (out,)), ...]` of a packed parameter vector
  (`MLPPolicy.params`' layout)."""
  out, o = [], 0
  for i, n in sizes:
    out.append((flat[o:o + i * n].view(i, n), flat[o + i * n:o + (i + 1) * n]))
    o += (i + 1) * n
  return out


class EvolutionLearner:
  """What ES and ARS share: the acting policy, its population of `2 *
  directions` rows, the normaliser, the keys and counters, and the episode
  phase of an epoch."""

  activation = 'relu'
  head = 'normal_tanh'

  def __init__(self, env, layers, directions: int, episode_length: int, action_repeat: int,
               perturbation_std: float, seed: int, normalize_observations: bool, device,
               frozen=None, fused: Optional[bool] = None):
    self.env, self.device = env, torch.device(device)
    self.directions, self.num_envs = int(directions), 2 * int(directions)
    self.episode_length, self.action_repeat = int(episode_length), int(action_repeat)
    self.perturbation_std, self.fused = float(perturbation_std), fused
    self.normalizer = (RunningStatistics(env.observation_size, self.device)
                       if normalize_observations else None)
    self.policy = self.make_policy((self.normalizer, layers))
    self.population = PolicyPopulation(self.policy, self.num_envs)
    self.frozen = None if frozen is None else torch.as_tensor(frozen).to(self.device, torch.uint8)
    self.theta = self.policy.params.clone()
    self._workspace = (self.population.delta_workspace() if self.policy.params.is_cuda
                       and fused is not False else None)
    # jax.random.PRNGKey(seed) layout; the evaluator's key is the other half
    # of this split (`train`)
    key = wrappers.split_key(np.array([0, int(seed)], np.uint32))[0]
    self._key, noise_key = wrappers.split_key(key)
    param_key, action_key = wrappers.split_key(noise_key)
    self.param_seed = wrappers.key_to_seed(param_key) & _SEED_MASK
    self.action_seed = wrappers.key_to_seed(action_key) & _SEED_MASK
    self.param_offset = self.action_offset = 0
    self.num_env_steps = 0

  @property
  def layers(self):
    """Views of the current parameters, `[(W, b), ...]`."""
    return unpack(self.theta, self.policy.sizes)

  @property
  def params(self):
    """(normaliser or None, policy layers)."""
    return self.normalizer, self.layers

  def make_policy(self, params=None, deterministic: bool = False) -> MLPPolicy:
    """`make_inference_fn`: an acting `MLPPolicy` from `params` (default: the
    learner's current ones), sharing the normaliser's device buffers."""
    normalizer, layers = self.params if params is None else params
    return driver.acting_policy(normalizer, layers, self.device, activation=self.activation,
                                deterministic=deterministic, head=self.head)

  def run_episodes(self):
    """Steps 1-4 and 9 of an epoch: returns the `PopulationResult` and the
    seeds that reproduce it."""
    self._key, reset_key = wrappers.split_key(self._key)
    state = self.env.reset(reset_key)
    if state.obs.shape[0] != self.num_envs:
      raise ValueError(f'the env holds {state.obs.shape[0]} envs, the population {self.num_envs}')
    used = dict(reset_key=reset_key, param_seed=self.param_seed, param_offset=self.param_offset,
                action_seed=self.action_seed, action_offset=self.action_offset)
    self.population.perturb_(self.perturbation_std, self.param_seed, self.param_offset, True,
                             frozen=self.frozen, fused=self.fused)
    K = self.episode_length // self.action_repeat
    _, result = population_rollout(self.env, state, self.population, K, seed=self.action_seed,
                                   offset=self.action_offset, reward_shift=self.reward_shift)
    self.action_offset += K * 2 * self.num_envs * self.env.action_size
    if self.normalizer is not None:
      self.normalizer.update_from_moments(result)
    self.num_env_steps += int(result.obs_count.double().sum().item()) * self.action_repeat
    return result, used

  def noise_sum(self, weights):
    """Step 6, then the parameter noise's counters move on to the next
    epoch's."""
    delta = self.population.weighted_noise_sum(
        weights, self.param_seed, self.param_offset, True, frozen=self.frozen, fused=self.fused,
        workspace=self._workspace)
    self.param_offset += 2 * self.directions * self.population.n_params
    return delta

  def publish(self):
    """Step 8: theta into the acting policy's buffer, in place."""
    self.policy.load_(self.layers)

  def training_metrics(self, scores, weights):
    return {'params_norm': torch.linalg.vector_norm(self.theta), 'eval_scores_mean': scores.mean(),
            'eval_scores_std': scores.std(unbiased=False), 'weights': weights.mean()}


class Learner(EvolutionLearner):
  """The state of one ES run; `epoch()` is one `training_epoch`."""

  reward_shift = 0.0

  def __init__(self, env, population_size: int = 128, episode_length: int = 1000,
               action_repeat: int = 1, l2coeff: float = 0, learning_rate: float = 1e-3,
               fitness_shaping: FitnessShaping = FitnessShaping.ORIGINAL,
               perturbation_std: float = 0.1, seed: int = 0, normalize_observations: bool = False,
               center_fitness: bool = False, network_factory=make_es_networks, device=None,
               fused: Optional[bool] = None):
    dev = torch.device('cuda' if device is None else device)
    layers = network_factory(env.observation_size, env.action_size, seed=seed, device=dev)
    super().__init__(env, layers, population_size, episode_length, action_repeat, perturbation_std,
                     seed, normalize_observations, dev, fused=fused)
    self.population_size, self.l2coeff = int(population_size), float(l2coeff)
    self.fitness_shaping, self.center_fitness = fitness_shaping, bool(center_fitness)
    # optax.adam's defaults (eps 1e-8, as torch's)
    self.optimizer = torch.optim.Adam([self.theta], lr=learning_rate, eps=1e-8)

  def gradient(self, delta):
    """`compute_delta` (`es/train.py:181-207`) of the weighted noise sum: what
    the optimiser descends."""
    return -(delta / self.population_size - self.l2coeff * self.theta)

  def epoch(self):
    """One training epoch. Returns its diagnostics: `scores` (2 P,) float32,
    `weights` (P,) float64, `delta` (n_params,) float32 (the weighted noise
    sum), `metrics` (the reference's four), `result` and the keys and
    counters the episodes used."""
    result, used = self.run_episodes()
    scores = result.scores
    weights = es_weights(scores, self.fitness_shaping, self.center_fitness)
    delta = self.noise_sum(weights)
    self.theta.grad = self.gradient(delta)
    self.optimizer.step()
    self.publish()
    return dict(scores=scores, weights=weights, delta=delta, result=result,
                metrics=self.training_metrics(scores, weights), **used)


def train(environment, num_timesteps: int = 100, episode_length: int = 1000,
          action_repeat: int = 1, l2coeff: float = 0, max_devices_per_host: Optional[int] = None,
          population_size: int = 128, learning_rate: float = 1e-3,
          fitness_shaping: FitnessShaping = FitnessShaping.ORIGINAL, num_eval_envs: int = 128,
          perturbation_std: float = 0.1, seed: int = 0, normalize_observations: bool = False,
          num_evals: int = 1, center_fitness: bool = False, deterministic_eval: bool = False,
          network_factory=make_es_networks,
          progress_fn: Callable[[int, dict], None] = lambda *args: None, eval_env=None,
          device=None, fused: Optional[bool] = None):
  """ES training; the reference's arguments and defaults
  (`es/train.py:75-96`).

  Args:
    environment: an env name (created with the Episode / Vector / AutoReset
      wrappers at `2 * population_size`), or such a batched env.
    max_devices_per_host: accepted and ignored (one device).
    eval_env: with a batched `environment`, the same env batched at
      `num_eval_envs` (a name is created at both sizes).
    device: the GPU (default `cuda`).
    fused: `perturb_`'s and `weighted_noise_sum`'s `fused` (None: the kernels).
  Returns:
    `(make_policy, params, metrics)`: `make_policy(params, deterministic=False)`
    gives an `MLPPolicy`; `params` is (the normaliser or None, the policy
    layers); `metrics` the last evaluation's dict.
  """
  del max_devices_per_host
  num_envs = population_size * 2  # noise + anti noise
  sched = eval_schedule(num_timesteps, num_evals)
  dev = torch.device('cuda' if device is None else device)
  env, eval_env = driver.make_envs(environment, eval_env, num_envs, num_eval_envs, episode_length,
                                   action_repeat, dev)
  learner = Learner(env, population_size, episode_length, action_repeat, l2coeff, learning_rate,
                    fitness_shaping, perturbation_std, seed, normalize_observations,
                    center_fitness, network_factory, dev, fused)
  eval_policy = learner.make_policy(deterministic=True) if deterministic_eval else learner.policy
  evaluator = driver.make_evaluator(eval_env, eval_policy, seed, num_eval_envs, episode_length,
                                    action_repeat, dev)
  metrics = run(learner, eval_policy, evaluator, num_timesteps, sched.first_eval_step,
                sched.num_env_steps_between_evals, num_evals > 1, progress_fn)
  return learner.make_policy, learner.params, metrics
