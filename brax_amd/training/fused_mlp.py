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

from brax_amd import _native, abi, abi_mlp_group
from brax_amd.fused import use_kernel
from brax_amd.system import launch
from brax_amd.training import networks


def fused_supported(layers, x, activation: str = 'swish') -> Optional[str]:
  """None when the kernels take this network and input, else why not."""
  # (the device last, so the other reasons can be read off CPU tensors too)
  return _why_not_shapes(layers, x, activation) or _why_not_device(layers, x)


def _why_not_shapes(layers, x, activation):
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
  return None


def _why_not_device(layers, x):
  for t in [x] + [t for wb in layers for t in wb]:
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


# ---- several networks in one forward and two backward launches ----------------------------------
# A group is up to `abi_mlp_group.MLP_MAX_GROUP` members `(layers, x,
# activation)`, each a whole problem of its own (`include/
# brax_amd_mlp_group.h`): the launches cover every member's tiles, and a tile
# runs the single-network kernels' code, so a member's bits are `fused_mlp`'s.


def _member(m, activation):
  return (m[0], m[1], m[2] if len(m) > 2 else activation)


def group_supported(members, activation: str = 'swish') -> Optional[str]:
  """None when the group kernels take these `(layers, x[, activation])`
  members (`activation` is that of a member without its own), else why not:
  the group's own limits, then `fused_supported` per member."""
  if not 1 <= len(members) <= abi_mlp_group.MLP_MAX_GROUP:
    return f'{len(members)} members, the kernels take 1..{abi_mlp_group.MLP_MAX_GROUP}'
  members = [_member(m, activation) for m in members]
  for why_not in (_why_not_shapes, lambda layers, x, act: _why_not_device(layers, x)):
    for i, (layers, x, act) in enumerate(members):
      why = why_not(layers, x, act)
      if why is not None:
        return f'member {i}: {why}'
  dev = members[0][1].device
  for i, (_, x, _) in enumerate(members):
    if x.device != dev:
      return f'member {i}: tensors on {dev} and {x.device}'
  return None


def _table(members):
  """The member table of `[(params, x2, activation)]` with net, rows and x
  set, and what must outlive the call."""
  table = (abi_mlp_group.BxMlpMember * len(members))()
  nets = [_net(params, act) for params, _, act in members]
  for m, net, (_, x2, _) in zip(table, nets, members):
    m.net = C.pointer(net)
    m.rows, m.x, m.x_stride = x2.shape[0], x2.data_ptr(), x2.stride(0)
  return table, nets


def _hidden(params):
  return sum(w.shape[1] for w in params[0:-2:2])


def group_forward(members, save):
  """`bx_mlp_group_forward`, no autograd: `members` is `[(params, x2,
  activation)]` with `params` the flat `[W0, b0, W1, ...]` and `x2` as
  `_rows2d` leaves it; `save[i]` whether member i's pre-activations are kept.
  Returns `(ys, saveds)`, `saveds[i]` None where not kept."""
  dev = members[0][1].device
  new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
  ys = [new(x2.shape[0], params[-1].shape[0]) for params, x2, _ in members]
  saveds = [new(x2.shape[0], _hidden(params)) if keep else None
            for (params, x2, _), keep in zip(members, save)]
  table, keep_alive = _table(members)
  for m, y, s in zip(table, ys, saveds):
    m.y = y.data_ptr()
    m.saved = s.data_ptr() if s is not None and s.numel() else None
  if any(x2.shape[0] for _, x2, _ in members):
    launch(dev, 'bx_mlp_group_forward', table, len(members))
  del keep_alive
  return ys, saveds


def group_backward(members, saveds, dys, want_dx, want_params):
  """`bx_mlp_group_backward`, no autograd: `members` and `saveds` as
  `group_forward` took and returned them; `dys[i]` is member i's `(rows, out)`
  gradient or None (the member is switched off); `want_dx[i]` whether its
  input gradient is wanted, `want_params[i]` one bool per tensor of its
  `params`. Returns `(dxs, grads)`: None where not wanted, `grads[i]` a list
  as `params`."""
  dev = members[0][1].device
  new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
  on = [dy is not None for dy in dys]
  dys = [dy.contiguous() if dy is not None else None for dy in dys]
  dxs = [new(*x2.shape) if k and dx else None for (_, x2, _), k, dx in zip(members, on, want_dx)]
  grads = [[torch.empty_like(p) if k and w else None for p, w in zip(params, wants)]
           for (params, _, _), k, wants in zip(members, on, want_params)]
  table, keep_alive = _table(members)
  lib = _native.lib()
  _native.check(lib.bx_mlp_group_backward(table, len(members), 1, None))
  offsets, total = [], 0
  for m in table:  # each member's slice of one workspace, 16-byte aligned
    offsets.append(total)
    total += (m.workspace_bytes + 15) // 16 * 4
  work = new(total)
  for i, m in enumerate(table):
    m.workspace = work.data_ptr() + 4 * offsets[i]
    if not on[i]:
      continue
    s = saveds[i]
    m.saved = s.data_ptr() if s is not None and s.numel() else None
    m.dy = dys[i].data_ptr()
    m.dx = None if dxs[i] is None else dxs[i].data_ptr()
    g = abi.BxMlpGrads()
    for l in range(len(grads[i]) // 2):
      g.dw[l] = None if grads[i][2 * l] is None else grads[i][2 * l].data_ptr()
      g.db[l] = None if grads[i][2 * l + 1] is None else grads[i][2 * l + 1].data_ptr()
    keep_alive.append(g)
    m.grads = C.pointer(g)
  for i, (_, x2, _) in enumerate(members):
    if x2.shape[0] == 0:  # no rows: the sums over nothing
      for t in grads[i]:
        if t is not None:
          t.zero_()
  if any(k and x2.shape[0] for k, (_, x2, _) in zip(on, members)):
    launch(dev, 'bx_mlp_group_backward', table, len(members), 0)
  del keep_alive
  return dxs, grads


class _FusedMlpGroup(torch.autograd.Function):
  """`(spec, *flat)` -> the members' y. `spec` is one `(activation, want,
  n_params)` per member, `flat` each member's `x2` then its params; `want` is
  whether a backward pass through that member can follow."""

  @staticmethod
  def forward(ctx, spec, *flat):
    members, at = [], 0
    for act, _, n in spec:
      members.append(([p.detach() for p in flat[at + 1:at + 1 + n]], flat[at], act))
      at += 1 + n
    ys, saveds = group_forward(members, [want for _, want, _ in spec])
    ctx.spec = spec
    ctx.set_materialize_grads(False)
    kept = []
    for (params, x2, _), s, (_, want, _) in zip(members, saveds, spec):
      if want:
        kept += [x2, s, *params]
    ctx.save_for_backward(*kept)
    ctx.mark_non_differentiable(*[y for y, (_, want, _) in zip(ys, spec) if not want])
    return tuple(ys)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, *dys):
    kept, need = list(ctx.saved_tensors), ctx.needs_input_grad
    members, saveds, on_dys, want_dx, want_params, where = [], [], [], [], [], []
    at, k = 1, 0
    for (act, want, n), dy in zip(ctx.spec, dys):
      if want and dy is not None:
        x2, s, params = kept[k], kept[k + 1], kept[k + 2:k + 2 + n]
        members.append((params, x2, act))
        saveds.append(s)
        on_dys.append(dy)
        want_dx.append(need[at])
        want_params.append(need[at + 1:at + 1 + n])
        where.append(at)
      if want:
        k += 2 + n
      at += 1 + n
    out = [None] * at
    if members:
      dxs, grads = group_backward(members, saveds, on_dys, want_dx, want_params)
      for a, dx, g in zip(where, dxs, grads):
        out[a] = dx
        out[a + 1:a + 1 + len(g)] = g
    return tuple(out)


def mlp_group(members, fused: Optional[bool] = None):
  """`[networks.mlp(layers, x, activation) for layers, x, activation in
  members]` in one forward launch (and at most two backward launches for the
  whole group).

  Args:
    members: `[(layers, x, activation), ...]`, each as `fused_mlp` takes them.
    fused: None takes the kernels where `group_supported` has no objection,
      else `networks.mlp` per member; True raises NotImplementedError where
      they do not apply; False is `networks.mlp` per member.
  """
  members = [_member(m, 'swish') for m in members]
  if not use_kernel(fused, 'mlp group', lambda: group_supported(members)):
    return [networks.mlp(layers, x, act) for layers, x, act in members]
  return apply_group(members)


def apply_group(members):
  """`mlp_group` through the kernels for `(layers, x, activation)` members that
  have passed `group_supported` (`use_group` or `mlp_group` checked them)."""
  grad = torch.is_grad_enabled()
  spec, flat, rows2d = [], [], {}
  for layers, x, act in members:
    params = [t for wb in layers for t in wb]
    if id(x) not in rows2d:  # members that share an x share its (rows, in) form
      rows2d[id(x)] = _rows2d(x)
    x2 = rows2d[id(x)]
    spec.append((act, grad and any(t.requires_grad for t in [x2] + params), len(params)))
    flat += [x2, *params]
  ys = _FusedMlpGroup.apply(tuple(spec), *flat)
  return [y.reshape(*x.shape[:-1], y.shape[-1]) for y, (_, x, _) in zip(ys, members)]


def use_group(fused_group, fused_mlp, members, activation: str = 'swish') -> bool:
  """The one decision of a learner's `fused_group` switch, by the rule of
  `brax_amd.fused`: whether these members take the group kernels. The switch
  needs the MLP kernels, so with `fused_mlp=False` it is unsupported, as it is
  where `group_supported` objects (True raises, None falls back). The support
  check runs once, here."""
  return use_kernel(
      fused_group, 'mlp group',
      lambda: 'fused_mlp is off' if fused_mlp is False else group_supported(members, activation))
