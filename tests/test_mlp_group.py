"""The MLP group entry points without a GPU: the mirror of
`include/brax_amd_mlp_group.h` against that header, the refusals (host
pointers: a launch would fault), the size query, `group_supported`'s reasons
and the learners' `fused_group` switch on CPU tensors."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from brax_amd import _native, abi, abi_mlp_group
from brax_amd.training import fused_mlp as fm
from brax_amd.training import losses, networks, sac_networks
from tests.helpers import HEADER_PATH, Header
from tests.test_abi import SCALARS, accepts

GROUP_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), 'brax_amd_mlp_group.h')
GROUP_HEADER = Header(GROUP_HEADER_PATH)
MAX = abi_mlp_group.MLP_MAX_GROUP


def test_mirror_is_the_group_headers(tmp_path):
  """Names, order and types of every declaration, the struct's layout as the
  host compiler has it, the macro, and the library's own sizeof."""
  assert list(GROUP_HEADER.functions) == list(abi_mlp_group.ARGS) == [
      'bx_mlp_group_sizes', 'bx_mlp_group_forward', 'bx_mlp_group_backward']
  assert list(GROUP_HEADER.structs) == ['bx_mlp_member']
  assert GROUP_HEADER.constants == {'BX_MLP_MAX_GROUP': MAX} and MAX == 8
  for name, (res, params) in GROUP_HEADER.functions.items():
    table = abi_mlp_group.ARGS[name]
    assert res == 'int' and [n for n, _ in table] == [n for _, n, _ in params]
    for (ctype, arg, dim), (_, t) in zip(params, table):
      if ctype.replace('const ', '') == 'bx_mlp_member*':
        assert t is C.POINTER(abi_mlp_group.BxMlpMember)
      else:
        assert accepts(ctype, dim, t), (arg, ctype, t)
    fn = getattr(_native.lib(), name)
    assert list(fn.argtypes) == [t for _, t in table] and fn.restype is C.c_int
  cls, fields = abi_mlp_group.BxMlpMember, GROUP_HEADER.structs['bx_mlp_member']
  assert [f for f, _ in cls._fields_] == [f for _, f, _ in fields]
  mirrors = {'const bx_mlp*': C.POINTER(abi.BxMlp), 'const bx_mlp_grads*': C.POINTER(abi.BxMlpGrads)}
  for (ctype, f, _), (_, t) in zip(fields, cls._fields_):
    assert t is (mirrors.get(ctype) or SCALARS.get(ctype) or C.c_void_p), (f, ctype, t)
  lines = ['std::printf("%zu\\n", sizeof(bx_mlp_member));']
  want = [str(C.sizeof(cls))]
  for _, f, _ in fields:
    lines.append(f'std::printf("%zu %zu\\n", offsetof(bx_mlp_member, {f}), '
                 f'sizeof(((bx_mlp_member*)0)->{f}));')
    want.append(f'{getattr(cls, f).offset} {getattr(cls, f).size}')
  src = tmp_path / 'layout.cpp'
  src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() {\n  %s\n}\n'
                 % (GROUP_HEADER_PATH, '\n  '.join(lines)))
  exe = tmp_path / 'layout'
  subprocess.run([os.environ.get('HOSTCXX', 'c++'), '-std=c++17', str(src), '-o', str(exe)],
                 check=True, timeout=120)
  got = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
  assert got.splitlines() == want
  n = C.c_int32(0)
  assert _native.lib().bx_mlp_group_sizes(C.byref(n)) == 0 and n.value == C.sizeof(cls)
  assert _native.lib().bx_mlp_group_sizes(None) != 0
  # additive: the version stays
  assert _native.lib().bx_abi_version() == abi.ABI_VERSION == 14


def _net(sizes, ptr, activation=0):
  n = abi.BxMlp()
  n.n_layers = len(sizes) - 1
  n.activation = activation
  for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
    if l < abi.MLP_MAX_LAYERS:
      getattr(n, 'in')[l], n.out[l], n.w[l], n.b[l] = i, o, ptr, ptr
  return n


class _Group:
  """Members over host buffers, every pointer distinct and 16-byte aligned."""

  def __init__(self, nets, rows=4):
    self.buf = (C.c_float * 4096)()
    self.nets, self.grads = nets, [abi.BxMlpGrads() for _ in nets]
    self.table = (abi_mlp_group.BxMlpMember * max(len(nets), 1))()
    base = (C.addressof(self.buf) + 15) & ~15
    self.base = base
    for i, (m, net) in enumerate(zip(self.table, nets)):
      at = base + 1024 * i
      m.net = C.pointer(net) if net is not None else None
      m.rows = rows
      m.x, m.x_stride = base, 0 if net is None else getattr(net, 'in')[0]
      m.y, m.saved, m.dy, m.dx, m.workspace = at, at + 64, base, at + 128, at + 256
      m.workspace_bytes = 1 << 20
      self.grads[i].dw[0], self.grads[i].db[0] = at + 512, at + 640
      m.grads = C.pointer(self.grads[i])

  def forward(self, n=None):
    return _native.lib().bx_mlp_group_forward(self.table, len(self.nets) if n is None else n, None)

  def backward(self, n=None, query=0):
    return _native.lib().bx_mlp_group_backward(self.table, len(self.nets) if n is None else n,
                                               query, None)


def _three(p=1 << 12):
  return _Group([_net((5, 3, 2), p), _net((7, 2), p), _net((5, 3, 2), p)])


def _refused(rc, word):
  msg = _native.lib().bx_last_error()
  assert rc != 0 and word in msg, msg


def test_group_refusals_before_any_launch():
  lib = _native.lib()
  _refused(lib.bx_mlp_group_forward(None, 2, None), b'null')
  _refused(lib.bx_mlp_group_backward(None, 2, 0, None), b'null')
  for n in (0, -1, MAX + 1):
    _refused(_three().forward(n), b'n_members %d outside 1..8' % n)
    _refused(_three().backward(n), b'n_members %d outside 1..8' % n)
    _refused(_three().backward(n, query=1), b'n_members %d outside 1..8' % n)
  # every refusal of the single entry points, as the member's
  p = 1 << 12
  no_w = _net((5, 3, 2), p)
  no_w.w[1] = None
  broken = _net((5, 3, 2), p)
  getattr(broken, 'in')[1] = 4
  for bad, word in ((None, b'null'), (no_w, b'null weight or bias'),
                    (_net((5, 257, 2), p), b'layer 0: width 257 outside 1..256'),
                    (_net((1025, 3), p), b'input width 1025 outside 1..1024'),
                    (_net((5,) + (3,) * 9, p), b'n_layers 9 outside 1..8'),
                    (broken, b'layer 1: in 4 != the previous out 3'),
                    (_net((5, 3, 2), p, activation=3), b'unknown activation 3')):
    for where in (0, 2):
      nets = [_net((5, 3, 2), p), _net((7, 2), p), _net((5, 3, 2), p)]
      nets[where] = bad
      for call in (lambda g: g.forward(), lambda g: g.backward(), lambda g: g.backward(query=1)):
        _refused(call(_Group(nets)), b'member %d: ' % where + word)

  def edited(field, value, member=1):
    g = _three()
    setattr(g.table[member], field, value)
    return g
  _refused(edited('rows', -1).forward(), b'member 1: negative rows')
  _refused(edited('rows', -1).backward(), b'member 1: negative rows')
  _refused(edited('x_stride', 6).forward(), b'member 1: x_stride 6 below the input width 7')
  _refused(edited('x_stride', 4, 2).backward(), b'member 2: x_stride 4 below the input width 5')
  _refused(edited('x', None).forward(), b'member 1: null argument')
  _refused(edited('y', None, 0).forward(), b'member 0: null argument')
  _refused(edited('x', None, 2).backward(), b'member 2: null argument')
  _refused(edited('saved', None, 2).backward(), b'member 2: null saved with hidden layers')
  _refused(edited('workspace_bytes', 8, 0).backward(), b'member 0: workspace of 8 bytes, 48 needed')
  g = _three()
  g.table[2].workspace += 4
  _refused(g.backward(), b'member 2: workspace not 16-byte aligned')
  # a member without hidden layers needs no saved
  g = edited('saved', None, 1)
  g.table[0].net = None
  _refused(g.backward(), b'member 0: null')
  # two members that write the same array
  for field, call in (('y', 'forward'), ('saved', 'forward'), ('dx', 'backward'),
                      ('workspace', 'backward')):
    g = _three()
    setattr(g.table[2], field, getattr(g.table[0], field))
    _refused(getattr(g, call)(), b'members 0 and 2 write the same array')
  for name in ('dw', 'db'):
    g = _three()
    getattr(g.grads[1], name)[0] = getattr(g.grads[0], name)[0]
    _refused(g.backward(), b'members 0 and 1 write the same array')
  g = _three()
  g.grads[2].db[1] = g.grads[0].dw[0]
  _refused(g.backward(), b'members 0 and 2 write the same array (dw, db)')


def test_members_that_take_no_part_launch_nothing():
  """Zero rows, and in the backward call a null dy: successful no-ops whatever
  the other pointers (host memory here: a launch would fault)."""
  g = _three()
  for m in g.table:
    m.rows, m.x, m.y = 0, None, None
  assert g.forward() == 0 and g.backward() == 0
  g = _three()
  for m in g.table:
    m.dy, m.x, m.saved, m.workspace = None, None, None, None
  assert g.backward() == 0
  # ... and such members may name the arrays of one another
  g = _three()
  for m in g.table:
    m.dy, m.dx = None, g.table[0].dx
  assert g.backward() == 0


def test_query_writes_each_members_workspace_size():
  """max(16, 4 * rows * H) per member, as bx_mlp_backward's query."""
  p = 1 << 12
  cases = [((5, 3, 2), 4), ((5, 3, 7, 2), 100), ((5, 2), 100), ((5, 3, 2), 0),
           ((33, 256, 256, 1), 130), ((7, 3, 2), 1), ((1024, 40, 3), 31), ((35, 129, 1, 255, 4), 65)]
  g = _Group([_net(s, p) for s, _ in cases])
  for m, (_, rows) in zip(g.table, cases):
    m.rows, m.workspace, m.workspace_bytes, m.x, m.dy = rows, None, -1, None, None
  assert g.backward(query=1) == 0
  for m, (sizes, rows) in zip(g.table, cases):
    assert m.workspace_bytes == max(16, 4 * rows * sum(sizes[1:-1])), (sizes, rows)
    single = C.c_int64(-1)
    assert _native.lib().bx_mlp_backward(m.net, rows, None, sizes[0], None, None, None, None, None,
                                         C.byref(single), None) == 0
    assert single.value == m.workspace_bytes


def _layers(sizes, dtype=torch.float32, seed=0):
  return networks.make_layers(sizes, torch.Generator().manual_seed(seed), dtype=dtype)


def test_group_supported_names_the_reason():
  x = torch.zeros((4, 5))
  ok = (_layers((5, 3, 2)), x, 'relu')
  assert fm.group_supported([]) == '0 members, the kernels take 1..8'
  assert fm.group_supported([ok] * 9) == '9 members, the kernels take 1..8'
  assert fm.group_supported([ok]) == 'member 0: a CPU tensor'
  assert fm.group_supported([ok, (_layers((5, 257, 2)), x, 'relu')]) == (
      'member 1: layer width 257 outside 1..256')
  assert 'member 2: activation' in fm.group_supported([ok, ok, (ok[0], x, 'gelu')])
  # a member without an activation takes the group's
  assert 'member 0: activation' in fm.group_supported([ok[:2]], 'gelu')
  assert 'member 1: torch.float64' in fm.group_supported([ok, (ok[0], x.double(), 'relu')])
  assert 'member 0: layer shapes' in fm.group_supported([(_layers((6, 3, 2)), x, 'swish')])
  with pytest.raises(NotImplementedError, match='no fused mlp group: member 0: a CPU tensor'):
    fm.mlp_group([ok], fused=True)


@pytest.mark.parametrize('fused', [None, False])
def test_mlp_group_falls_back_to_the_loop_on_cpu(fused):
  members = [(_layers((5, 3, 2)), torch.randn((4, 5)), 'relu'),
             (_layers((7, 2), seed=1), torch.randn((2, 3, 7)), 'tanh')]
  got = fm.mlp_group(members, fused=fused)
  for y, (layers, x, act) in zip(got, members):
    assert torch.equal(y, networks.mlp(layers, x, act))


def _ppo_inputs(B=3, T=4, O=5, A=2):
  g = torch.Generator().manual_seed(0)
  r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
  data = losses.Transition(
      observation=r(B, T, O), action=torch.tanh(r(B, T, A)), reward=r(B, T),
      discount=torch.ones(B, T), next_observation=r(B, T, O), truncation=torch.zeros(B, T),
      raw_action=r(B, T, A), log_prob=r(B, T))
  policy, value = networks.make_ppo_networks(O, A, (8, 8), (8,), seed=1)
  return policy, value, data, r(B, T, A)


def test_fused_group_needs_the_mlp_kernels():
  """`fused_group=True` with `fused_mlp=False` is unsupported: it raises; None
  falls back to the ungrouped form."""
  q = sac_networks.make_sac_networks(5, 2, (8, 8), seed=0)[1]
  obs, action = torch.randn((4, 5)), torch.randn((4, 2))
  with pytest.raises(NotImplementedError, match='no fused mlp group: fused_mlp is off'):
    sac_networks.q_apply(q, obs, action, fused_mlp=False, fused_group=True)
  policy, value, data, eps = _ppo_inputs()
  with pytest.raises(NotImplementedError, match='no fused mlp group: fused_mlp is off'):
    losses.ppo_loss(policy, value, None, data, eps, fused=False, fused_group=True)
  with pytest.raises(NotImplementedError, match='no fused mlp group: fused_mlp is off'):
    networks.mlp_many([(q[0], torch.randn((4, 7)), 'relu')], False, True)
  want = sac_networks.q_apply(q, obs, action)
  assert torch.equal(sac_networks.q_apply(q, obs, action, fused_mlp=False, fused_group=None), want)
  # with the kernels wanted, the group's own reason
  with pytest.raises(NotImplementedError, match='no fused mlp group: member 0: a CPU tensor'):
    sac_networks.q_apply(q, obs, action, fused_mlp=True, fused_group=True)
  assert torch.equal(sac_networks.q_apply(q, obs, action, fused_mlp=None, fused_group=None), want)


def test_fused_group_off_is_the_call_without_it():
  q = sac_networks.make_sac_networks(5, 2, (8, 8), seed=0)[1]
  obs, action = torch.randn((4, 5)), torch.randn((4, 2))
  want = sac_networks.q_apply(q, obs, action)
  assert torch.equal(sac_networks.q_apply(q, obs, action, fused_group=False), want)
  policy, value, data, eps = _ppo_inputs()
  params = networks.parameters(policy, value)
  out = []
  for kw in ({}, {'fused_group': False}, {'fused_group': None}):
    loss, metrics = losses.ppo_loss(policy, value, None, data, eps, fused=False, **kw)
    grads = torch.autograd.grad(loss, params)
    out.append((loss.detach(), grads, metrics))
  for loss, grads, metrics in out[1:]:
    assert torch.equal(loss, out[0][0])
    assert all(torch.equal(a, b) for a, b in zip(grads, out[0][1]))
    assert metrics.keys() == out[0][2].keys()
    assert all(torch.equal(metrics[k], out[0][2][k]) for k in metrics)
