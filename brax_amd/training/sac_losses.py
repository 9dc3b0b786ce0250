"""The SAC losses (`brax/training/agents/sac/losses.py:40-94`) in torch.

Line for line the reference's, dtype-generic, with the sample's standard-normal
draw `eps` explicit where the reference takes a key. `transitions` is a mapping
with the replay row's fields (`replay_buffers.transition_fields`):
observation and next_observation (B, O), action (B, A), reward, discount and
truncation (B,) or (B, 1). `normalizer` is `(mean, std)` or None. The NormalTanh
formulae are `brax_amd.envs.policy`'s, the ones the acting policy uses.
"""
from typing import List, Mapping

import torch

from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
from brax_amd.training.losses import normalize
from brax_amd.training.networks import Layers, mlp
from brax_amd.training.sac_networks import ACTIVATION, q_apply

MIN_STD = 1e-3  # NormalTanhDistribution's default (distribution.py:136)


def target_entropy(action_size: int) -> float:
  return -0.5 * action_size


def _scalar(t):
  return t.reshape(t.shape[0])


def _sample(policy_layers, obs, eps, fused_mlp=False):
  """`sample_no_postprocessing` and `log_prob` of it: (raw action, log_prob)."""
  loc, s = torch.chunk(mlp(policy_layers, obs, ACTIVATION, fused_mlp), 2, dim=-1)
  scale = head_scale(s, MIN_STD)
  raw = loc + scale * eps.to(loc.dtype)
  return raw, normal_tanh_log_prob(loc, scale, raw).sum(-1)


def alpha_loss(log_alpha: torch.Tensor, policy_layers: Layers, normalizer,
               transitions: Mapping[str, torch.Tensor], eps: torch.Tensor,
               fused_mlp=False, fused_group=False) -> torch.Tensor:
  """Eq 18 of arXiv:1812.05905 (`losses.py:40-51`); differentiable in `log_alpha`.
  (`fused_group` has nothing to group here: one network.)"""
  del fused_group
  action_size = eps.shape[-1]
  _, log_prob = _sample(policy_layers, normalize(transitions['observation'], normalizer), eps,
                        fused_mlp)
  alpha = torch.exp(log_alpha)
  loss = alpha * (-log_prob - target_entropy(action_size)).detach()
  return torch.mean(loss)


def critic_loss(q_layers: List[Layers], policy_layers: Layers, normalizer,
                target_q_layers: List[Layers], alpha: torch.Tensor,
                transitions: Mapping[str, torch.Tensor], eps: torch.Tensor,
                reward_scaling: float = 1.0, discounting: float = 0.9,
                fused_mlp=False, fused_group=False) -> torch.Tensor:
  """`losses.py:53-79`; differentiable in `q_layers` (the target is held).
  `fused_group`: each `q_apply`'s critics share their launches."""
  obs = normalize(transitions['observation'], normalizer)
  next_obs = normalize(transitions['next_observation'], normalizer)
  q_old_action = q_apply(q_layers, obs, transitions['action'], fused_mlp, fused_group)
  next_raw, next_log_prob = _sample(policy_layers, next_obs, eps, fused_mlp)
  next_action = torch.tanh(next_raw)
  next_q = q_apply(target_q_layers, next_obs, next_action, fused_mlp, fused_group)
  next_v = torch.min(next_q, dim=-1).values - alpha * next_log_prob
  target_q = (_scalar(transitions['reward']) * reward_scaling
              + _scalar(transitions['discount']) * discounting * next_v).detach()
  q_error = q_old_action - target_q.unsqueeze(-1)
  # Better bootstrapping for truncated episodes.
  q_error = q_error * (1 - _scalar(transitions['truncation'])).unsqueeze(-1)
  return 0.5 * torch.mean(torch.square(q_error))


def actor_loss(policy_layers: Layers, normalizer, q_layers: List[Layers], alpha: torch.Tensor,
               transitions: Mapping[str, torch.Tensor], eps: torch.Tensor,
               fused_mlp=False, fused_group=False) -> torch.Tensor:
  """`losses.py:81-94`; differentiable in `policy_layers`. `fused_group` as
  `critic_loss`'s."""
  obs = normalize(transitions['observation'], normalizer)
  raw, log_prob = _sample(policy_layers, obs, eps, fused_mlp)
  action = torch.tanh(raw)
  q_action = q_apply(q_layers, obs, action, fused_mlp, fused_group)
  min_q = torch.min(q_action, dim=-1).values
  return torch.mean(alpha * log_prob - min_q)
