"""Generalised advantage estimation, the whole unroll in ONE launch.

`compute_gae` is the reference's (`brax/training/agents/ppo/losses.py:37-93`):
a reverse scan over a `(T, B)` unroll that `compute_ppo_loss` calls once per
minibatch per update. Under `jit` the scan is fused; as chained torch
operations it is a handful of small launches per time step. `bx_compute_gae`
runs it with one lane per env sequence, float32, every operation rounded on
its own and in the reference's order, so its outputs are bit for bit the
chained form's (`tests/test_gpu_training.py`).

The recurrences, for t = T-1 .. 0, with v_next = t == T-1 ? bootstrap :
values[t+1], vs_next likewise, acc starting at 0:

    r     = rewards[t] * reward_scaling
    mask  = 1 - truncation[t]
    term  = termination[t] * mask
    g     = discount * (1 - term)
    delta = ((r + g * v_next) - values[t]) * mask
    acc   = delta + ((g * mask) * lambda_) * acc
    vs[t] = acc + values[t]
    advantages[t] = ((r + g * vs_next) - values[t]) * mask

`termination` may be the reference's `(1 - discount_t) * (1 - truncation)` or
the plain `done = 1 - discount_t`: the `* mask` maps both to the same value for
the 0 / 1 flags the wrappers write. `reward_scaling` folds `compute_ppo_loss`'s
`rewards = data.reward * reward_scaling` into the same launch (1: the
reference's function exactly).
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from brax_amd import abi
from brax_amd.fused import use_kernel
from brax_amd.system import launch


def _seq(t):
  return abi.BxSeq(t.data_ptr(), t.stride(0), t.stride(1))


def fused_supported(*tensors) -> Optional[str]:
  """None when the kernel takes these tensors, else why not."""
  dev = tensors[0].device
  for t in tensors:
    if t.dtype != torch.float32:
      return f'{t.dtype} is not float32'
    if not t.is_cuda:
      return 'a CPU tensor'
    if t.device != dev:
      return f'tensors on {dev} and {t.device}'
  return None


def _chained(truncation, termination, rewards, values, bootstrap_value, lambda_, discount,
             reward_scaling):
  """The recurrences as separate torch operations in the inputs' dtype: the
  public fallback and the kernel's yardstick. Everything that does not depend
  on the scan is one operation over the whole (T, B) array, which rounds each
  element exactly as a per-step loop would."""
  mask = 1 - truncation
  r = rewards * reward_scaling
  term = termination * mask
  g = discount * (1 - term)
  v_next = torch.cat([values[1:], bootstrap_value[None]], dim=0)
  delta = ((r + g * v_next) - values) * mask
  coef = (g * mask) * lambda_
  acc = torch.zeros_like(bootstrap_value)
  rows = []
  for t in range(values.shape[0] - 1, -1, -1):
    acc = delta[t] + coef[t] * acc
    rows.append(acc)
  vs = torch.stack(rows[::-1]) + values
  vs_next = torch.cat([vs[1:], bootstrap_value[None]], dim=0)
  advantages = ((r + g * vs_next) - values) * mask
  return vs, advantages


def compute_gae(truncation, termination, rewards, values, bootstrap_value, lambda_: float = 1.0,
                discount: float = 0.99, reward_scaling: float = 1.0, fused: Optional[bool] = None,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
  """`(vs, advantages)`, both `(T, B)` and without gradient.

  Args:
    truncation, termination, rewards, values: `(T, B)` tensors of one dtype,
      any strides (a transposed `[B, T]` array passes without a copy).
    bootstrap_value: `(B,)`, the value estimate at time T.
    lambda_, discount: as the reference's.
    reward_scaling: multiplies `rewards` first (see the module's text).
    fused: None takes the kernel for float32 tensors on one GPU, else the
      chained form; True raises NotImplementedError where the kernel does not
      apply; False forces the chained form.
    out: optional `(vs, advantages)` float tensors of shape `(T, B)` to write
      (any layout that does not overlap itself or the inputs).
  """
  seqs = (truncation, termination, rewards, values)
  T, B = values.shape
  for t in seqs:
    if tuple(t.shape) != (T, B):
      raise ValueError(f'expected four ({T}, {B}) tensors, got {tuple(t.shape)}')
  if tuple(bootstrap_value.shape) != (B,):
    raise ValueError(f'bootstrap_value {tuple(bootstrap_value.shape)} != ({B},)')
  if T < 1:
    raise ValueError('compute_gae needs at least one time step')
  if out is not None:
    for o in out:
      if tuple(o.shape) != (T, B) or o.dtype != values.dtype or o.device != values.device:
        raise ValueError(f'out must be two ({T}, {B}) {values.dtype} tensors on {values.device}')
  seqs = tuple(t.detach() for t in seqs)
  boot = bootstrap_value.detach()
  if not use_kernel(fused, 'compute_gae', lambda: fused_supported(*seqs, boot)):
    with torch.no_grad():
      vs, adv = _chained(*seqs, boot, lambda_, discount, reward_scaling)
      # (elementwise results take their inputs' layout; the kernel's fresh
      # outputs are row-major, and a later reduction's summation order follows
      # the layout, so both forms hand out the same one)
      vs, adv = vs.contiguous(), adv.contiguous()
      if out is not None:
        vs, adv = out[0].copy_(vs), out[1].copy_(adv)
    return vs, adv
  dev = values.device
  if out is None:
    out = (torch.empty((T, B), dtype=torch.float32, device=dev),
           torch.empty((T, B), dtype=torch.float32, device=dev))
  vs, adv = out
  if B == 0:
    return vs, adv
  boot = boot.contiguous()
  tr, term, rew, val = seqs
  args = [_seq(t) for t in (rew, term, tr, val, vs, adv)]
  launch(dev, 'bx_compute_gae', T, B, C.byref(args[0]), C.byref(args[1]), C.byref(args[2]),
         C.byref(args[3]), boot.data_ptr(), C.byref(args[4]), C.byref(args[5]), reward_scaling,
         discount, lambda_)
  return vs, adv
