"""The PPO loss (`brax/training/agents/ppo/losses.py:96-182`) in torch.

`ppo_loss` is `compute_ppo_loss` with the reference's defaults: dtype-generic,
differentiable in the two networks' parameters, its GAE targets from
`compute_gae` (one `bx_compute_gae` launch for float32 device tensors). The
NormalTanh log-prob is `MLPPolicy.forward`'s (`brax_amd.envs.policy`), so the
log-prob recomputed here for the recorded `raw_action` is the one the rollout
kernel recorded, up to float32 rounding.
"""
import dataclasses
from typing import Any, Dict, Optional, Tuple

import torch

from brax_amd.envs.policy import head_scale, normal_tanh_log_prob  # noqa: F401 (re-exported)
from brax_amd.training.gae import compute_gae
from brax_amd.training.networks import Layers, mlp, mlp_many  # noqa: F401 (mlp re-exported)
from brax_amd.training.ppo_head import entropy, ppo_head  # noqa: F401 (entropy re-exported)


@dataclasses.dataclass(frozen=True)
class Transition:
  """`types.Transition` with the extras `compute_ppo_loss` reads, flat; the
  leading dimensions are `[B, T]` as the reference's loss takes them
  (`acting.actor_step`, `training/acting.py:30-50`):

    observation (B, T, O)       the obs the policy read before step t
    action, raw_action (B, T, A)  action = tanh(raw_action)
    reward, discount (B, T)     discount = 1 - done
    next_observation (B, T, O)  the obs after step t (under AutoReset: the
                                reset obs)
    truncation (B, T)           extras['state_extras']['truncation']
    log_prob (B, T)             extras['policy_extras']['log_prob']
  """
  observation: Any
  action: Any
  reward: Any
  discount: Any
  next_observation: Any
  truncation: Any
  raw_action: Any
  log_prob: Any

  def map(self, fn):
    return Transition(**{f.name: fn(getattr(self, f.name)) for f in dataclasses.fields(self)})


def normalize(obs, normalizer):
  """`running_statistics.normalize`: `normalizer` is `(mean, std)` or None."""
  if normalizer is None:
    return obs
  mean, std = normalizer
  return (obs - mean.to(obs.dtype)) / std.to(obs.dtype)


def ppo_loss(policy_layers: Layers, value_layers: Layers, normalizer, data: Transition, eps,
             entropy_cost: float = 1e-4, discounting: float = 0.9, reward_scaling: float = 1.0,
             gae_lambda: float = 0.95, clipping_epsilon: float = 0.3,
             normalize_advantage: bool = True, activation: str = 'swish', min_std: float = 1e-3,
             fused: Optional[bool] = None,
             fused_mlp=False, fused_head=False,
             fused_group=False) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
  """`(loss, metrics)` of one minibatch.

  Args:
    policy_layers, value_layers: `[(W (in, out), b), ...]` torch parameters.
    normalizer: `(mean, std)` of the observations, or None.
    data: a `Transition`, leading dimensions `[B, T]`.
    eps: `(B, T, A)` standard-normal draws for the entropy term's sample (the
      reference's `rng`, explicit).
    fused: passed to `compute_gae`.
    fused_mlp: `networks.mlp`'s `fused` for the three network evaluations.
    fused_head: `ppo_head.ppo_head`'s `fused` for everything after them (False:
      chained torch; True: `bx_ppo_head` or NotImplementedError; None: the
      kernel where it applies). The kernel runs its own GAE scan, so `fused`
      is not consulted where it is taken.
    fused_group: the three network evaluations in one forward launch and the
      two networks' backward passes in two (`networks.mlp_many`). It needs the
      MLP kernels: with `fused_mlp=False`, True raises and None falls back.
  """
  data = data.map(lambda x: x.transpose(0, 1))  # time first
  eps = eps.transpose(0, 1)
  obs = normalize(data.observation, normalizer)
  logits, baseline, bootstrap_value = mlp_many(
      [(policy_layers, obs, activation), (value_layers, obs, activation),
       (value_layers, normalize(data.next_observation[-1], normalizer), activation)],
      fused_mlp, fused_group)
  return ppo_head(logits, baseline.squeeze(-1), bootstrap_value.squeeze(-1), data, eps, entropy_cost=entropy_cost,
                  discounting=discounting, reward_scaling=reward_scaling, gae_lambda=gae_lambda,
                  clipping_epsilon=clipping_epsilon, normalize_advantage=normalize_advantage,
                  min_std=min_std, fused=fused_head, fused_gae=fused, gae=compute_gae)
