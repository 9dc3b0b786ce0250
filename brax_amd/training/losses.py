"""The PPO loss (`brax/training/agents/ppo/losses.py:96-182`) in torch.

`ppo_loss` is `compute_ppo_loss` with the reference's defaults: dtype-generic,
differentiable in the two networks' parameters, its GAE targets from
`compute_gae` (one `bx_compute_gae` launch for float32 device tensors). The
NormalTanh log-prob is `MLPPolicy.forward`'s (`brax_amd.envs.policy`), so the
log-prob recomputed here for the recorded `raw_action` is the one the rollout
kernel recorded, up to float32 rounding.
"""
import dataclasses
import math
from typing import Any, Dict, Optional, Tuple

import torch

from brax_amd.envs.policy import head_scale, normal_tanh_log_prob, tanh_log_det
from brax_amd.training.gae import compute_gae
from brax_amd.training.networks import Layers, mlp


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


def entropy(loc, scale, eps):
  """`ParametricDistribution.entropy` (`training/distribution.py:83-91`): the
  Normal's entropy plus the tanh log-det at the sample loc + scale * eps,
  summed over the actions."""
  normal = 0.5 + (0.5 * math.log(2.0 * math.pi) + torch.log(scale))
  return (normal + tanh_log_det(loc + scale * eps)).sum(-1)


def ppo_loss(policy_layers: Layers, value_layers: Layers, normalizer, data: Transition, eps,
             entropy_cost: float = 1e-4, discounting: float = 0.9, reward_scaling: float = 1.0,
             gae_lambda: float = 0.95, clipping_epsilon: float = 0.3,
             normalize_advantage: bool = True, activation: str = 'swish', min_std: float = 1e-3,
             fused: Optional[bool] = None,
             fused_mlp=False) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
  """`(loss, metrics)` of one minibatch.

  Args:
    policy_layers, value_layers: `[(W (in, out), b), ...]` torch parameters.
    normalizer: `(mean, std)` of the observations, or None.
    data: a `Transition`, leading dimensions `[B, T]`.
    eps: `(B, T, A)` standard-normal draws for the entropy term's sample (the
      reference's `rng`, explicit).
    fused: passed to `compute_gae`.
    fused_mlp: `networks.mlp`'s `fused` for the three network evaluations.
  """
  data = data.map(lambda x: x.transpose(0, 1))  # time first
  eps = eps.transpose(0, 1)
  obs = normalize(data.observation, normalizer)
  logits = mlp(policy_layers, obs, activation, fused_mlp)
  baseline = mlp(value_layers, obs, activation, fused_mlp).squeeze(-1)
  bootstrap_value = mlp(value_layers, normalize(data.next_observation[-1], normalizer),
                        activation, fused_mlp).squeeze(-1)
  loc, s = torch.chunk(logits, 2, dim=-1)
  scale = head_scale(s, min_std)
  target_log_probs = normal_tanh_log_prob(loc, scale, data.raw_action).sum(-1)
  # termination = (1 - discount) * (1 - truncation): compute_gae forms the
  # product from done = 1 - discount; the reward scaling is folded in as well
  vs, advantages = compute_gae(
      truncation=data.truncation, termination=1 - data.discount, rewards=data.reward,
      values=baseline, bootstrap_value=bootstrap_value, lambda_=gae_lambda,
      discount=discounting, reward_scaling=reward_scaling, fused=fused)
  if normalize_advantage:
    advantages = (advantages - advantages.mean()) / (advantages.std(unbiased=False) + 1e-8)
  rho_s = torch.exp(target_log_probs - data.log_prob)
  surrogate_loss1 = rho_s * advantages
  surrogate_loss2 = torch.clamp(rho_s, 1 - clipping_epsilon, 1 + clipping_epsilon) * advantages
  policy_loss = -torch.mean(torch.minimum(surrogate_loss1, surrogate_loss2))
  v_error = vs - baseline
  v_loss = torch.mean(v_error * v_error) * 0.5 * 0.5
  entropy_loss = entropy_cost * -torch.mean(entropy(loc, scale, eps.to(loc.dtype)))
  total_loss = policy_loss + v_loss + entropy_loss
  return total_loss, {'total_loss': total_loss, 'policy_loss': policy_loss, 'v_loss': v_loss,
                      'entropy_loss': entropy_loss}
