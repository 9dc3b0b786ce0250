"""The fused MLP without a GPU: the ABI mirror of `bx_mlp_forward` /
`bx_mlp_backward`, their refusals (host pointers: a launch would fault),
`fused_supported`'s reasons, and the chained fallbacks' bits."""
import ctypes as C

import pytest
import torch

from brax_amd import _native, abi
from brax_amd.envs.policy import _ACTIVATIONS
from brax_amd.training import fused_mlp as fm
from brax_amd.training import networks


def test_header_abi_and_exports():
  # (names, types, fields and the BX_MLP_MAX_* macros: tests/test_abi.py)
  assert (abi.MLP_MAX_LAYERS, abi.MLP_MAX_WIDTH, abi.MLP_MAX_IN) == (8, 256, 1024)
  # the struct sizes as the library was compiled
  a, b = C.c_int32(0), C.c_int32(0)
  assert _native.lib().bx_mlp_sizes(C.byref(a), C.byref(b)) == 0
  assert (a.value, b.value) == (C.sizeof(abi.BxMlp), C.sizeof(abi.BxMlpGrads))
  # additive: the version stays
  assert abi.ABI_VERSION == 14 and _native.lib().bx_abi_version() == 14


def _net(sizes, ptr, activation=0):
  n = abi.BxMlp()
  n.n_layers = len(sizes) - 1
  n.activation = activation
  for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
    if l < abi.MLP_MAX_LAYERS:
      getattr(n, 'in')[l], n.out[l], n.w[l], n.b[l] = i, o, ptr, ptr
  return n


def test_refusals_before_any_launch():
  """Every refusal sets bx_last_error and returns before a device call (the
  pointers here are host memory: a launch would fault)."""
  lib = _native.lib()
  buf = (C.c_float * 64)()
  p = C.addressof(buf)
  nbytes = C.c_int64(1 << 30)

  def forward(net, rows=4, x=p, stride=None, y=p):
    stride = getattr(net, 'in')[0] if stride is None else stride
    return lib.bx_mlp_forward(None if net is None else C.byref(net), rows, x, stride, y, None, None)

  def backward(net, rows=4, x=p, stride=None, saved=p, dy=p, ws=p, nb=nbytes):
    stride = getattr(net, 'in')[0] if stride is None else stride
    return lib.bx_mlp_backward(None if net is None else C.byref(net), rows, x, stride, saved, dy,
                               None, None, ws, None if nb is None else C.byref(nb), None)
  ok = _net((5, 3, 2), p)
  no_w, no_b = _net((5, 3, 2), p), _net((5, 3, 2), p)
  no_w.w[1] = None
  no_b.b[0] = None
  broken = _net((5, 3, 2), p)
  getattr(broken, 'in')[1] = 4
  nine = _net((5,) + (3,) * 9, p)
  small = C.c_int64(8)
  cases = [
      (forward, dict(net=None, stride=5), b'null'),
      (forward, dict(net=ok, x=None), b'null'),
      (forward, dict(net=ok, y=None), b'null'),
      (forward, dict(net=no_w), b'null weight or bias'),
      (forward, dict(net=no_b), b'null weight or bias'),
      (forward, dict(net=_net((5, 257, 2), p)), b'width 257 outside 1..256'),
      (forward, dict(net=_net((5, 0, 2), p)), b'width 0 outside 1..256'),
      (forward, dict(net=_net((1025, 3), p)), b'input width 1025 outside 1..1024'),
      (forward, dict(net=_net((0, 3), p)), b'input width 0 outside 1..1024'),
      (forward, dict(net=nine), b'n_layers 9 outside 1..8'),
      (forward, dict(net=_net((5,), p)), b'n_layers 0 outside 1..8'),
      (forward, dict(net=ok, stride=4), b'x_stride 4 below the input width 5'),
      (forward, dict(net=broken), b'in 4 != the previous out 3'),
      (forward, dict(net=_net((5, 3, 2), p, activation=3)), b'unknown activation 3'),
      (forward, dict(net=_net((5, 3, 2), p, activation=-1)), b'unknown activation -1'),
      (forward, dict(net=ok, rows=-1), b'negative rows'),
      (backward, dict(net=None, stride=5), b'null'),
      (backward, dict(net=ok, nb=None), b'null'),
      (backward, dict(net=ok, x=None), b'null'),
      (backward, dict(net=ok, dy=None), b'null'),
      (backward, dict(net=ok, saved=None), b'null saved'),
      (backward, dict(net=no_w), b'null weight or bias'),
      (backward, dict(net=_net((5, 257, 2), p)), b'width 257 outside 1..256'),
      (backward, dict(net=_net((1025, 3), p)), b'input width 1025 outside 1..1024'),
      (backward, dict(net=nine), b'n_layers 9 outside 1..8'),
      (backward, dict(net=ok, stride=4), b'x_stride 4 below the input width 5'),
      (backward, dict(net=broken), b'in 4 != the previous out 3'),
      (backward, dict(net=_net((5, 3, 2), p, activation=7)), b'unknown activation 7'),
      (backward, dict(net=ok, rows=-1), b'negative rows'),
      (backward, dict(net=ok, nb=small), b'workspace of 8 bytes, 48 needed'),
      (backward, dict(net=ok, ws=p + 4), b'workspace not 16-byte aligned'),
  ]
  for fn, kw, word in cases:
    assert fn(**kw) != 0 and word in lib.bx_last_error(), (kw, lib.bx_last_error())
  # zero rows: a successful no-op, whatever the pointers
  assert forward(ok, rows=0, x=None, y=None) == 0
  assert backward(ok, rows=0, x=None, saved=None, dy=None) == 0
  # the size query: 4 bytes per row and hidden unit, at least 16
  for sizes, rows, want in (((5, 3, 2), 4, 48), ((5, 3, 7, 2), 100, 4000), ((5, 2), 100, 16),
                            ((5, 3, 2), 0, 16)):
    q = C.c_int64(-1)
    assert backward(_net(sizes, p), rows=rows, x=None, saved=None, dy=None, ws=None, nb=q) == 0
    assert q.value == want


def _layers(sizes, dtype=torch.float32, seed=0):
  return networks.make_layers(sizes, torch.Generator().manual_seed(seed), dtype=dtype)


def test_fused_supported_names_the_reason():
  x = torch.zeros((4, 5))
  assert fm.fused_supported(_layers((5, 3, 2)), x) == 'a CPU tensor'
  assert 'float64' in fm.fused_supported(_layers((5, 3, 2), torch.float64), x.double())
  assert 'float64' in fm.fused_supported(_layers((5, 3, 2)), x.double())
  assert 'width 257 outside 1..256' in fm.fused_supported(_layers((5, 257, 2)), x)
  assert 'width 1025 outside 1..1024' in fm.fused_supported(_layers((1025, 2)), torch.zeros((4, 1025)))
  assert '9 layers' in fm.fused_supported(_layers((5,) + (3,) * 9), x)
  assert 'inner stride 2' in fm.fused_supported(_layers((5, 3, 2)), torch.zeros((4, 10))[:, ::2])
  assert 'activation' in fm.fused_supported(_layers((5, 3, 2)), x, 'gelu')
  assert 'layer shapes' in fm.fused_supported(_layers((6, 3, 2)), x)


def test_fused_true_refuses_cpu_tensors():
  with pytest.raises(NotImplementedError, match='a CPU tensor'):
    fm.fused_mlp(_layers((5, 3, 2)), torch.zeros((4, 5)), fused=True)
  with pytest.raises(NotImplementedError, match='a CPU tensor'):
    networks.mlp(_layers((5, 3, 2)), torch.zeros((4, 5)), 'swish', fused=True)


def _restated(layers, x, activation):
  """`networks.mlp`'s loop as the parent commit has it."""
  fn = _ACTIVATIONS[activation]
  for k, (w, b) in enumerate(layers):
    x = x @ w + b
    if k + 1 < len(layers):
      x = fn(x)
  return x


def _value_and_grads(f, layers, x):
  x = x.clone().requires_grad_()
  y = f(layers, x)
  g = torch.autograd.grad(y.square().sum(), [x] + networks.parameters(layers))
  return [y.detach()] + list(g)


@pytest.mark.parametrize('activation', sorted(_ACTIVATIONS))
def test_cpu_paths_are_the_chained_bits(activation):
  layers = _layers((7, 33, 5, 2), seed=3)
  x = torch.randn((2, 6, 7), generator=torch.Generator().manual_seed(4))
  want = _value_and_grads(lambda l, v: _restated(l, v, activation), layers, x)
  forms = {
      'mlp': lambda l, v: networks.mlp(l, v, activation),
      'mlp fused=False': lambda l, v: networks.mlp(l, v, activation, fused=False),
      'mlp fused=None': lambda l, v: networks.mlp(l, v, activation, fused=None),
      'fused_mlp None': lambda l, v: fm.fused_mlp(l, v, activation),
      'fused_mlp False': lambda l, v: fm.fused_mlp(l, v, activation, fused=False),
  }
  for name, f in forms.items():
    got = _value_and_grads(f, layers, x)
    assert len(got) == len(want)
    for g, w in zip(got, want):
      assert torch.equal(g, w), name
