"""The PPO networks as plain lists of torch parameters.

The reference's `make_ppo_networks` (`training/agents/ppo/networks.py:62-88`):
a policy MLP `(32,) * 4` ending in `2 * action_size` NormalTanh parameters and
a value MLP `(256,) * 5` ending in one output, swish, flax's `Dense` defaults
(lecun-uniform kernels, `U(+-sqrt(3 / fan_in))`, zero biases;
`training/networks.py:37-57`). A network here is `[(W (in, out), b (out,)),
...]` in flax's kernel layout, which is what `MLPPolicy` packs, so the learner's
policy is copied into the acting one with `MLPPolicy.load_`.
"""
import math
from typing import List, Sequence, Tuple

import torch

from brax_amd.envs.policy import _ACTIVATIONS

Layers = List[Tuple[torch.Tensor, torch.Tensor]]


def make_layers(sizes: Sequence[int], generator: torch.Generator, device=None,
                dtype=torch.float32) -> Layers:
  """An MLP `sizes[0] -> ... -> sizes[-1]` of leaf tensors that require grad;
  the draws come from `generator` (a CPU generator: the same weights on every
  device)."""
  layers = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    lim = math.sqrt(3.0 / i)
    w = (torch.rand((i, o), generator=generator, dtype=torch.float64) * 2 - 1) * lim
    layers.append((w.to(device=device, dtype=dtype).requires_grad_(),
                   torch.zeros((o,), device=device, dtype=dtype).requires_grad_()))
  return layers


def make_ppo_networks(observation_size: int, action_size: int,
                      policy_hidden_layer_sizes: Sequence[int] = (32,) * 4,
                      value_hidden_layer_sizes: Sequence[int] = (256,) * 5, seed: int = 0,
                      device=None, dtype=torch.float32) -> Tuple[Layers, Layers]:
  """`(policy_layers, value_layers)` with the reference's default sizes."""
  g = torch.Generator(device='cpu').manual_seed(int(seed))
  policy = make_layers((observation_size, *policy_hidden_layer_sizes, 2 * action_size), g, device,
                       dtype)
  value = make_layers((observation_size, *value_hidden_layer_sizes, 1), g, device, dtype)
  return policy, value


def mlp(layers: Layers, x: torch.Tensor, activation: str = 'swish', fused=False) -> torch.Tensor:
  """`networks.MLP.__call__`: the activation after every layer but the last
  (`MLPPolicy.forward`'s loop). `fused` other than False goes through
  `fused_mlp.fused_mlp` (True: the kernels or NotImplementedError; None: the
  kernels where they apply, else the loop below)."""
  if fused is not False:
    from brax_amd.training.fused_mlp import fused_mlp  # pylint: disable=import-outside-toplevel
    return fused_mlp(layers, x, activation, fused)
  fn = _ACTIVATIONS[activation]
  for k, (w, b) in enumerate(layers):
    x = x @ w + b
    if k + 1 < len(layers):
      x = fn(x)
  return x


def mlp_many(members, fused=False, fused_group=False) -> List[torch.Tensor]:
  """`[mlp(layers, x, activation, fused) for layers, x, activation in members]`
  for networks evaluated at the same point of a step. `fused_group` other than
  False gives them shared launches through `fused_mlp.mlp_group` (True: the
  group kernels or NotImplementedError, also where `fused` is False; None: them
  where they apply, else the loop)."""
  if fused_group is not False:
    from brax_amd.training import fused_mlp  # pylint: disable=import-outside-toplevel
    if fused_mlp.use_group(fused_group, fused, members):
      return fused_mlp.apply_group(members)
  return [mlp(layers, x, activation, fused) for layers, x, activation in members]


def parameters(*networks: Layers) -> List[torch.Tensor]:
  return [t for layers in networks for wb in layers for t in wb]


def detached(layers: Layers) -> Layers:
  """The layers' tensors without their autograd history (views, no copies)."""
  return [(w.detach(), b.detach()) for w, b in layers]
