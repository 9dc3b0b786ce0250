"""A whole MLP forward in ONE launch and backward in two.

`networks.mlp` as autograd is about three launches per layer forward and
twice that backward, on batches of a few thousand rows where each launch is
shorter than its own dispatch. `fused_mlp` is the same function over
`bx_mlp_forward` / `bx_mlp_backward` (`include/brax_amd.h`): float32, the
products on gfx950's f32-input MFMA (a k-ordered fmaf chain, so no precision
is traded), the row tile's activations in LDS between layers. The layers stay
the separate `(W (in, out), b (out,))` tensors `make_layers` creates and are
read in place, so an optimiser that updates them in place is seen by the next
call (and by a captured graph's next replay).

Forward saves the hidden layers' pre-activations `(rows, sum of hidden
widths)` when a gradient will be wanted and nothing under `torch.no_grad()`.
Backward launch (i) is the reverse chain per row tile (`dx`, and the
pre-activation gradients into a torch-allocated workspace); launch (ii) is
every layer's `dW` and `db` in one grouped launch. `needs_input_grad` switches
either off: SAC's actor loss wants `dx` through the critics, PPO wants the
parameter gradients alone. No floating-point atomics anywhere: the same
inputs give the same bits.
"""
import ctypes as C
from typing import Optional

import torch

from brax_amd import _native, abi
from brax_amd.fused import use_kernel
from brax_amd.system import launch
from brax_amd.training import networks


def fused_supported(layers, x, activation: str = 'swish') -> Optional[str]:
  """None when the kernels take this network and input, else why not."""
  if activation not in abi.POLICY_ACTIVATIONS:
    return f'activation {activation!r} not in {sorted(abi.POLICY_ACTIVATIONS)}'
  if not 1 <= len(layers) <= abi.MLP_MAX_LAYERS:
    return f'{len(layers)} layers, the kernels take 1..{abi.MLP_MAX_LAYERS}'
  tensors = [x] + [t for wb in layers for t in wb]
  for t in tensors:
    if t.dtype != torch.float32:
      return f'{t.dtype} is not float32'
  if x.dim() < 1:
    return 'x has no feature dimension'
  width = x.shape[-1]
  if not 1 <= width <= abi.MLP_MAX_IN:
    return f'input width {width} outside 1..{abi.MLP_MAX_IN}'
  if x.stride(-1) != 1 and width > 1:
    return f'x has inner stride {x.stride(-1)}, not 1'
  for w, b in layers:
    if w.dim() != 2 or b.dim() != 1 or w.shape[0] != width or b.shape[0] != w.shape[1]:
      return f'layer shapes {tuple(w.shape)}, {tuple(b.shape)} after width {width}'
    width = w.shape[1]
    if not 1 <= width <= abi.MLP_MAX_WIDTH:
      return f'layer width {width} outside 1..{abi.MLP_MAX_WIDTH}'
    if not w.is_contiguous() or not b.is_contiguous():
      return 'a layer that is not contiguous'
  # (the device last, so the reasons above can be read off CPU tensors too)
  for t in tensors:
    if not t.is_cuda:
      return 'a CPU tensor'
    if t.device != x.device:
      return f'tensors on {x.device} and {t.device}'
  return None


def _net(params, activation):
  n = abi.BxMlp()
  n.n_layers = len(params) // 2
  n.activation = abi.POLICY_ACTIVATIONS[activation]
  for l in range(n.n_layers):
    w, b = params[2 * l], params[2 * l + 1]
    getattr(n, 'in')[l], n.out[l] = w.shape
    n.w[l], n.b[l] = w.data_ptr(), b.data_ptr()
  return n


def _rows2d(x):
  """x as (rows, width) with unit inner stride and one row pitch, without a
  copy where its layout already is that (a column slice of a wider buffer)."""
  width = x.shape[-1]
  if x.dim() == 2 and (x.stride(1) == 1 or width == 1) and x.stride(0) >= width:
    return x
  return x.reshape(-1, width).contiguous()


class _FusedMlp(torch.autograd.Function):
  """`(x2, activation, want, *params)` -> y; x2 is (rows, in) as `_rows2d`
  leaves it, `want` whether a backward pass can follow (the caller's grad
  mode: inside `forward` it is always off)."""

  @staticmethod
  def forward(ctx, x2, activation, want, *params):
    dev = x2.device
    params = tuple(p.detach() for p in params)
    rows = x2.shape[0]
    hidden = sum(w.shape[1] for w in params[0:-2:2])
    y = torch.empty((rows, params[-1].shape[0]), dtype=torch.float32, device=dev)
    saved = torch.empty((rows, hidden), dtype=torch.float32, device=dev) if want else None
    if rows:
      net = _net(params, activation)
      launch(dev, 'bx_mlp_forward', C.byref(net), rows, x2.data_ptr(), x2.stride(0), y.data_ptr(),
             saved.data_ptr() if want and hidden else None)
    ctx.activation = activation
    if want:
      ctx.save_for_backward(x2, saved, *params)
    return y

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, dy):
    x2, saved, *params = ctx.saved_tensors
    dev = x2.device
    rows = x2.shape[0]
    need = ctx.needs_input_grad
    dy = dy.contiguous()
    dx = torch.empty((rows, x2.shape[1]), dtype=torch.float32, device=dev) if need[0] else None
    grads = [torch.empty_like(p) if need[3 + k] else None for k, p in enumerate(params)]
    if rows == 0:
      return (dx, None, None, *[None if g is None else g.zero_() for g in grads])
    net = _net(params, ctx.activation)
    g = abi.BxMlpGrads()
    for l in range(net.n_layers):
      g.dw[l] = None if grads[2 * l] is None else grads[2 * l].data_ptr()
      g.db[l] = None if grads[2 * l + 1] is None else grads[2 * l + 1].data_ptr()
    nbytes = C.c_int64(0)
    _native.check(_native.lib().bx_mlp_backward(C.byref(net), rows, None, x2.stride(0), None, None,
                                                None, None, None, C.byref(nbytes), None))
    work = torch.empty(((nbytes.value + 3) // 4,), dtype=torch.float32, device=dev)
    launch(dev, 'bx_mlp_backward', C.byref(net), rows, x2.data_ptr(), x2.stride(0),
           saved.data_ptr() or None, dy.data_ptr(), None if dx is None else dx.data_ptr(),
           C.byref(g), work.data_ptr(), C.byref(nbytes))
    return (dx, None, None, *grads)


def fused_mlp(layers, x: torch.Tensor, activation: str = 'swish',
              fused: Optional[bool] = None) -> torch.Tensor:
  """`networks.mlp(layers, x, activation)` through the fused kernels.

  Args:
    layers: `[(W (in, out), b (out,)), ...]`, as `make_layers` creates them.
    x: `(..., in)`; the leading dimensions are flattened to rows.
    fused: None takes the kernels where `fused_supported` has no objection,
      else `networks.mlp`; True raises NotImplementedError where they do not
      apply; False is `networks.mlp`.
  """
  if not use_kernel(fused, 'mlp', lambda: fused_supported(layers, x, activation)):
    return networks.mlp(layers, x, activation)
  params = [t for wb in layers for t in wb]
  want = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + params)
  y = _FusedMlp.apply(_rows2d(x), activation, want, *params)
  return y.reshape(*x.shape[:-1], y.shape[-1])
