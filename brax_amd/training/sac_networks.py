"""The SAC networks as plain lists of torch parameters.

The reference's `make_sac_networks` (`training/agents/sac/networks.py:53-78`,
`training/networks.py:83-103`, `:126-162`): a policy MLP ending in `2 *
action_size` NormalTanh parameters, and a q network of two critics, each an
MLP `[O + A, *hidden, 1]` over `cat(normalised obs, action)` whose outputs are
concatenated to `(B, 2)`; relu, flax's `Dense` defaults (`make_layers`). The
policy is `[(W, b), ...]` as PPO's, the q network a list of two such lists.
"""
from typing import List, Sequence, Tuple

import torch

from brax_amd.training.networks import Layers, make_layers, mlp_many

ACTIVATION = 'relu'


def make_sac_networks(observation_size: int, action_size: int,
                      hidden_layer_sizes: Sequence[int] = (256, 256), seed: int = 0, device=None,
                      dtype=torch.float32, n_critics: int = 2) -> Tuple[Layers, List[Layers]]:
  """`(policy_layers, q_layers)` with the reference's default sizes."""
  g = torch.Generator(device='cpu').manual_seed(int(seed))
  policy = make_layers((observation_size, *hidden_layer_sizes, 2 * action_size), g, device, dtype)
  q = [make_layers((observation_size + action_size, *hidden_layer_sizes, 1), g, device, dtype)
       for _ in range(n_critics)]
  return policy, q


def q_apply(q_layers: List[Layers], obs: torch.Tensor, action: torch.Tensor,
            fused_mlp=False, fused_group=False) -> torch.Tensor:
  """`QModule.__call__` on observations that are already normalised: (B,
  n_critics). With `fused_group` the critics share their launches
  (`networks.mlp_many`)."""
  hidden = torch.cat([obs, action], dim=-1)
  return torch.cat(mlp_many([(c, hidden, ACTIVATION) for c in q_layers], fused_mlp, fused_group),
                   dim=-1)


def q_parameters(q_layers: List[Layers]) -> List[torch.Tensor]:
  return [t for c in q_layers for wb in c for t in wb]
