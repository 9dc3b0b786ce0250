"""The fused optimiser step: Adam for every parameter, and SAC's target
update, in one launch.

`torch.optim.Adam` walks its tensors in `multi_tensor_apply` launches (8 for
PPO's 22 tensors), and SAC applies three such optimisers and then four
launches per target tensor. `FusedAdam` is one `bx_adam_step` call
(`include/brax_amd.h`) per 32 tensors: the table of pointers travels in the
kernel's arguments, so a step allocates nothing, copies nothing and does not
synchronise. The arithmetic is `torch.optim.Adam`'s default path (no weight
decay, no amsgrad) with the bias corrections taken on the host in double;
`reference_step` restates it in torch for any dtype.

    opt = FusedAdam([dict(params=q_params, lr=3e-4, targets=target_params, tau=0.005),
                     dict(params=policy_params, lr=3e-4)])
    opt.step(grads)          # or loss.backward(); opt.step()
"""
import math
from typing import List, Optional, Sequence

import torch

from brax_amd import _native, abi
from brax_amd.fused import use_kernel
from brax_amd.system import launch

_ALIGN = 4  # float32 elements: every arena slice starts on a 16-byte boundary


def _normalised(groups):
  """The groups as dicts with every key, `params` / `targets` as lists."""
  if isinstance(groups, dict):
    groups = [groups]
  out = []
  for g in groups:
    unknown = set(g) - {'params', 'lr', 'targets', 'tau'}
    if unknown:
      raise ValueError(f'unknown group keys {sorted(unknown)}')
    params = list(g['params'])
    targets = g.get('targets')
    out.append(dict(params=params, lr=float(g['lr']),
                    targets=None if targets is None else list(targets),
                    tau=float(g.get('tau', 0.0))))
  return out


def supported(groups, device: bool = True) -> Optional[str]:
  """None when `FusedAdam` takes these groups, else why not. With `device`
  False the tensors' devices are not looked at."""
  groups = _normalised(groups)
  named = []
  for k, g in enumerate(groups):
    if g['targets'] is not None and len(g['targets']) != len(g['params']):
      return f"group {k}: {len(g['targets'])} targets for {len(g['params'])} params"
    for i, p in enumerate(g['params']):
      named.append((f'group {k} param {i}', p))
      if g['targets'] is not None:
        t = g['targets'][i]
        if tuple(t.shape) != tuple(p.shape):
          return f'group {k} target {i} {tuple(t.shape)} is not shaped as its param {tuple(p.shape)}'
        named.append((f'group {k} target {i}', t))
  if not named:
    return 'no parameters'
  for name, t in named:
    if t.dtype != torch.float32:
      return f'{name}: {t.dtype} is not float32'
  for name, t in named:
    if not t.is_contiguous():
      return f'{name} is not contiguous'
  if not device:
    return None
  # (the device last, so the reasons above can be read off CPU tensors too)
  first = named[0][1].device
  for name, t in named:
    if not t.is_cuda:
      return f'{name} is a CPU tensor'
    if t.device != first:
      return f'tensors on {first} and {t.device}'
  return None


def _scalar(x: float, dtype) -> torch.Tensor:
  """A host double narrowed once to `dtype`, as the C entry point narrows."""
  return torch.tensor(x, dtype=torch.float64).to(dtype)


def reference_step(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor],
                   exp_avgs: Sequence[torch.Tensor], exp_avg_sqs: Sequence[torch.Tensor],
                   step: int, lr, betas=(0.9, 0.999), eps: float = 1e-8, targets=None, tau=0.0):
  """`bx_adam_step`'s arithmetic (the header's lines, in its order) in torch,
  in place on `params`, `exp_avgs`, `exp_avg_sqs` and `targets`, in the
  tensors' own dtype: the scalars are formed in double and narrowed once.

  Args:
    step: the count after this step, >= 1.
    lr, tau: one value, or one per tensor.
    targets: None, or one entry per tensor (None: no target update).
  """
  beta1, beta2 = betas
  n = len(params)
  lrs = list(lr) if isinstance(lr, (list, tuple)) else [lr] * n
  taus = list(tau) if isinstance(tau, (list, tuple)) else [tau] * n
  targets = [None] * n if targets is None else list(targets)
  bc1 = 1.0 - beta1 ** step
  bc2 = 1.0 - beta2 ** step
  with torch.no_grad():
    for k, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
      dt = p.dtype
      g = g.detach().to(dt)
      w1, w2 = _scalar(1.0 - beta1, dt), _scalar(1.0 - beta2, dt)
      b2, c2 = _scalar(beta2, dt), _scalar(math.sqrt(bc2), dt)
      s, e = _scalar(lrs[k] / bc1, dt), _scalar(eps, dt)
      m.copy_(m + (g - m) * w1)
      v.copy_(v * b2 + (g * g) * w2)
      denom = torch.sqrt(v) / c2 + e
      p.copy_(p - s * (m / denom))
      if targets[k] is not None:
        t = targets[k]
        t.copy_(t * _scalar(1.0 - taus[k], dt) + p * _scalar(taus[k], dt))


def arena_offsets(sizes: Sequence[int]):
  """The element offsets of tensors of `sizes` in one arena, each rounded up
  to a 16-byte boundary, and the arena's length."""
  offsets, at = [], 0
  for n in sizes:
    offsets.append(at)
    at += -(-max(int(n), 1) // _ALIGN) * _ALIGN
  return offsets, at


class FusedAdam:
  """Adam over `groups`, each `dict(params=[...], lr=..., targets=None |
  [...], tau=0.0)`; a group with targets also does `target = target * (1 -
  tau) + param * tau` with the parameter just written.

  The moments are slices of two flat zeroed float32 arenas (`exp_avg(i)`,
  `exp_avg_sq(i)`, `i` counting the tensors across the groups in order). The
  step count is a host value. The optimiser holds the parameters' addresses:
  they are updated in place and must keep their storage.
  """

  def __init__(self, groups, betas=(0.9, 0.999), eps: float = 1e-8):
    self.groups = _normalised(groups)
    why = supported(self.groups, device=False)
    if why is not None:
      raise NotImplementedError(f'no fused Adam: {why}')
    self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
    self.params: List[torch.Tensor] = []
    self.targets: List[Optional[torch.Tensor]] = []
    self.lrs: List[float] = []
    self.taus: List[float] = []
    for g in self.groups:
      for i, p in enumerate(g['params']):
        self.params.append(p)
        self.targets.append(None if g['targets'] is None else g['targets'][i])
        self.lrs.append(g['lr'])
        self.taus.append(g['tau'] if g['targets'] is not None else 0.0)
    self.device = self.params[0].device
    self.step_count = 0
    offsets, total = arena_offsets([p.numel() for p in self.params])
    self._m = torch.zeros((total,), dtype=torch.float32, device=self.device)
    self._v = torch.zeros((total,), dtype=torch.float32, device=self.device)
    self._slices = [(o, p.numel(), tuple(p.shape)) for o, p in zip(offsets, self.params)]
    # the written tensors, whose autograd versions a step bumps
    self._written = self.params + [t for t in self.targets if t is not None]
    # one table per call of at most OPT_MAX_TENSORS tensors, filled once but
    # for the gradient pointers
    self._tables = []
    for lo in range(0, len(self.params), abi.OPT_MAX_TENSORS):
      hi = min(lo + abi.OPT_MAX_TENSORS, len(self.params))
      table = (abi.BxOptTensor * (hi - lo))()
      for k in range(lo, hi):
        e = table[k - lo]
        e.p = self.params[k].data_ptr()
        e.m = self.exp_avg(k).data_ptr()
        e.v = self.exp_avg_sq(k).data_ptr()
        e.target = None if self.targets[k] is None else self.targets[k].data_ptr()
        e.lr, e.tau = self.lrs[k], self.taus[k]
      self._tables.append((lo, hi, table))

  def _slice(self, arena, i):
    o, n, shape = self._slices[i]
    return arena[o:o + n].view(shape)

  def exp_avg(self, i: int) -> torch.Tensor:
    """Tensor `i`'s first moment (a view of the arena, shaped as the tensor)."""
    return self._slice(self._m, i)

  def exp_avg_sq(self, i: int) -> torch.Tensor:
    """Tensor `i`'s second moment."""
    return self._slice(self._v, i)

  def zero_grad(self, set_to_none: bool = True):
    for p in self.params:
      if p.grad is None:
        continue
      if set_to_none:
        p.grad = None
      else:
        p.grad.detach_()
        p.grad.zero_()

  def step(self, grads: Optional[Sequence[torch.Tensor]] = None):
    """One Adam step (and target update) of every tensor: one launch per 32
    tensors. `grads` lists one gradient per tensor across the groups in order
    (None: `p.grad`); a tensor whose gradient is None is left as it is, as
    `torch.optim.Adam` leaves it."""
    if self.device.type != 'cuda':
      raise _native.NativeError('FusedAdam.step needs CUDA tensors: brax_amd has no CPU fallback')
    if grads is None:
      grads = [p.grad for p in self.params]
    elif len(grads) != len(self.params):
      raise ValueError(f'{len(grads)} gradients for {len(self.params)} tensors')
    held = []  # (until the launches are queued: contiguous copies are fresh tensors)
    for p, g in zip(self.params, grads):
      if g is None:
        held.append(None)
        continue
      if g.dtype != torch.float32 or g.device != p.device or g.numel() != p.numel():
        raise ValueError(f'gradient {tuple(g.shape)} {g.dtype} on {g.device} for a parameter '
                         f'{tuple(p.shape)} float32 on {p.device}')
      held.append(g if g.is_contiguous() else g.contiguous())
    self.step_count += 1
    for lo, hi, table in self._tables:
      for k in range(lo, hi):
        e, g = table[k - lo], held[k]
        if g is None:
          e.g, e.n = None, 0
        else:
          e.g, e.n = g.data_ptr(), self._slices[k][1]
      launch(self.device, 'bx_adam_step', table, hi - lo, self.step_count, self.betas[0],
             self.betas[1], self.eps)
    # the writes went around torch
    torch.autograd.graph.increment_version(self._written)
    del held


def make_adam(groups, fused_adam) -> Optional[FusedAdam]:
  """`FusedAdam(groups)` with optax.adam's defaults (eps 1e-8, as torch's)
  where `fused_adam` takes it (the usual rule, see `brax_amd.fused`), else
  None: the caller builds torch's optimisers."""
  if use_kernel(fused_adam, 'Adam', lambda: supported(groups)):
    return FusedAdam(groups, eps=1e-8)
  return None
