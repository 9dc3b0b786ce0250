"""The MLP group launches (`bx_mlp_group_forward` / `bx_mlp_group_backward`) on
the GPU: every output of every member is bit for bit what `bx_mlp_forward` /
`bx_mlp_backward` write for that member alone.

The grid walk goes over a prefix table of the members' 32-row tiles (forward,
launch (i)) and of their (layer, 32 x 64) tiles (launch (ii)), so: members of
different shapes and row counts below, at and across a tile (1, 31, 32, 33, 64,
65, 130), a member without rows in the middle, the full 8 members, an input
wider than the LDS image, and members that share an x or their weights.
"""
import ctypes as C
import functools

import pytest
import torch

from brax_amd import abi, abi_mlp_group
from brax_amd.system import launch
from brax_amd.training import fused_mlp as fm
from brax_amd.training import losses, networks, ppo, sac, sac_head, sac_networks

pytestmark = pytest.mark.gpu

SENTINEL = 777.25
PAD = 64
GROUP_A = (((5, 1), 1), ((7, 3, 2), 33), ((35, 129, 1, 255, 4), 65), ((1024, 40, 3), 31),
           ((33, 256, 256, 1), 130))
GROUP_B = tuple(((7, 3, 2), rows) for rows in (1, 31, 32, 33, 0, 64, 65, 130))
ALL = dict(saved=True, dx=True, grads='all', dy=True)


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


class Member:
  """One problem on the device: the layers, x as a column slice of a wider
  NaN-filled buffer, dy; `switches` say which outputs are asked for."""

  def __init__(self, sizes, rows, activation, seed, dev, layers=None, x=None, **switches):
    g = torch.Generator().manual_seed(seed)
    self.sizes, self.rows, self.activation = sizes, rows, activation
    if layers is None:
      layers = networks.make_layers(sizes, g, device=dev)
      with torch.no_grad():
        for _, b in layers:
          b.copy_((torch.randn(b.shape, generator=g) * 0.1).to(dev))
    self.layers = layers
    self.params = [t.detach() for wb in layers for t in wb]
    if x is None:
      wide = torch.full((rows, sizes[0] + 3), float('nan'), device=dev)
      x = wide[:, 2:2 + sizes[0]]
      x.copy_(torch.randn((rows, sizes[0]), generator=g).to(dev))
    self.x = x
    self.dy = torch.randn((rows, sizes[-1]), generator=g).to(dev)
    self.switches = dict(ALL, **switches)
    self.hidden = sum(sizes[1:-1])

  def wanted(self, k):
    """Whether the gradient of params[k] is asked for."""
    mode = self.switches['grads']
    return mode == 'all' or (mode == 'odd' and k % 3 != 1) or (mode == 'last' and k >= len(self.params) - 2)

  def outputs(self):
    """Fresh outputs, each inside PAD sentinel words on either side."""
    dev = self.x.device
    shapes = {'y': (self.rows, self.sizes[-1]), 'saved': (self.rows, self.hidden),
              'dx': (self.rows, self.sizes[0])}
    shapes.update({f'g{k}': tuple(p.shape) for k, p in enumerate(self.params)})
    out = {}
    for name, shape in shapes.items():
      n = 1
      for s in shape:
        n *= s
      full = torch.full((2 * PAD + n,), SENTINEL, device=dev)
      out[name] = (full, full[PAD:PAD + n].view(shape))
    return out

  def fill(self, m, net, grads, out, work):
    """The member struct over these outputs; off outputs are null."""
    sw = self.switches
    m.net = C.pointer(net)
    m.rows, m.x, m.x_stride = self.rows, self.x.data_ptr(), max(self.x.stride(0), self.sizes[0])
    m.y = out['y'][1].data_ptr()
    m.saved = out['saved'][1].data_ptr() if self.hidden and (sw['saved'] or sw['dy']) else None
    m.dy = self.dy.data_ptr() if sw['dy'] else None
    m.dx = out['dx'][1].data_ptr() if sw['dx'] else None
    for k in range(len(self.params)):
      if self.wanted(k):
        (grads.dw if k % 2 == 0 else grads.db)[k // 2] = out[f'g{k}'][1].data_ptr()
    m.grads = C.pointer(grads)
    m.workspace, m.workspace_bytes = work.data_ptr(), work.numel() * 4


def _work(member, dev):
  return torch.empty((max(4, member.rows * member.hidden),), device=dev)


def run_single(member, dev):
  """{name: the padded buffer} after bx_mlp_forward and bx_mlp_backward."""
  out, work = member.outputs(), _work(member, dev)
  net, grads = fm._net(member.params, member.activation), abi.BxMlpGrads()
  m = abi_mlp_group.BxMlpMember()
  member.fill(m, net, grads, out, work)
  launch(dev, 'bx_mlp_forward', m.net, m.rows, m.x, m.x_stride, m.y, m.saved)
  if member.switches['dy']:
    nbytes = C.c_int64(m.workspace_bytes)
    launch(dev, 'bx_mlp_backward', m.net, m.rows, m.x, m.x_stride, m.saved, m.dy, m.dx, m.grads,
           m.workspace, C.byref(nbytes))
  torch.cuda.synchronize(dev)
  return {k: full for k, (full, _) in out.items()}


def run_group(members, dev, backward=True):
  outs, works = [m.outputs() for m in members], [_work(m, dev) for m in members]
  nets = [fm._net(m.params, m.activation) for m in members]
  grads = [abi.BxMlpGrads() for _ in members]
  table = (abi_mlp_group.BxMlpMember * len(members))()
  for args in zip(members, table, nets, grads, outs, works):
    args[0].fill(*args[1:])
  launch(dev, 'bx_mlp_group_forward', table, len(members))
  if backward:
    launch(dev, 'bx_mlp_group_backward', table, len(members), 0)
  torch.cuda.synchronize(dev)
  return [{k: full for k, (full, _) in out.items()} for out in outs]


def _same(a, b):
  """Bit equality (a NaN equals itself)."""
  return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_members_equal_single(members, dev, got=None):
  got = run_group(members, dev) if got is None else got
  for i, (member, g) in enumerate(zip(members, got)):
    want = run_single(member, dev)
    sw = member.switches
    for name, full in g.items():
      assert _same(full, want[name]), (i, member.sizes, member.rows, name)
      assert bool((full[:PAD] == SENTINEL).all()) and bool((full[-PAD:] == SENTINEL).all()), (i, name)
      inner = full[PAD:len(full) - PAD]
      off = (member.rows == 0 or (name == 'saved' and not (sw['saved'] or sw['dy'])) or (name == 'dx' and not (sw['dx'] and sw['dy']))
             or (name[0] == 'g' and not (sw['dy'] and member.wanted(int(name[1:])))))  # noqa: E129
      if off:  # an output nobody asked for stays untouched
        assert bool((inner == SENTINEL).all()), (i, name)
      elif inner.numel():
        assert not bool((inner == SENTINEL).any()), (i, name)
  return got


def _group_a(dev, activation, **switches):
  return [Member(sizes, rows, activation, 11 * k + rows, dev, **switches)
          for k, (sizes, rows) in enumerate(GROUP_A)]


def _group_b(dev, **switches):
  return [Member(sizes, rows, 'swish', 7 * k + 1, dev, **switches) for k, (sizes, rows) in enumerate(GROUP_B)]


def _group_c(dev, **switches):
  """The SAC pattern: two critics on one x, the same two again on another."""
  sizes, rows = (33, 256, 256, 1), 130
  q = [Member(sizes, rows, 'relu', 40 + c, dev, **switches) for c in range(2)]
  first = [q[0], Member(sizes, rows, 'relu', 42, dev, layers=q[1].layers, x=q[0].x, **switches)]
  other = Member(sizes, rows, 'relu', 43, dev, layers=q[0].layers, **switches)
  return first + [other, Member(sizes, rows, 'relu', 44, dev, layers=q[1].layers, x=other.x, **switches)]


@pytest.mark.parametrize('activation', ['relu', 'swish', 'tanh'])
def test_group_a_members_are_the_single_launches(dev, activation):
  members = _group_a(dev, activation)
  got = assert_members_equal_single(members, dev)
  again = run_group(members, dev)  # two runs, the same bits
  for g, a in zip(got, again):
    for name in g:
      assert _same(g[name], a[name]), name


def test_eight_members_and_one_without_rows(dev):
  members = _group_b(dev)
  assert len(members) == abi_mlp_group.MLP_MAX_GROUP
  assert_members_equal_single(members, dev)


def test_members_that_share_an_x_or_their_weights(dev):
  assert_members_equal_single(_group_c(dev), dev)


def test_per_member_switches(dev):
  """Null saved, dx and gradient entries per member; one member without dy."""
  members = _group_a(dev, 'swish')
  members[0].switches.update(dx=False)
  members[1].switches.update(grads='odd')
  members[2].switches.update(dy=False, saved=False)
  members[3].switches.update(grads='none')
  members[4].switches.update(dx=False, grads='odd')
  assert_members_equal_single(members, dev)
  # forward alone, nothing saved
  members = _group_b(dev, saved=False, dy=False)
  assert_members_equal_single(members, dev)


def _mlp_kernels(fn, dev):
  from torch.autograd import DeviceType
  from torch.profiler import ProfilerActivity, profile
  torch.cuda.synchronize(dev)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize(dev)
  return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and 'mlp_' in e.name]


def test_a_launch_nobody_needs_is_skipped(dev):
  # no dx and no hidden layer's gradient: launch (i) is left out
  members = _group_c(dev, dx=False, grads='last') + _group_a(dev, 'relu', dx=False, grads='last')[:2]
  assert_members_equal_single(members, dev)
  names = _mlp_kernels(lambda: run_group(members, dev), dev)
  assert len(names) == 2 and 'group_forward' in names[0] and 'group_grad' in names[1], names
  # no parameter gradient: launch (ii) is left out
  members = _group_c(dev, grads='none')
  assert_members_equal_single(members, dev)
  names = _mlp_kernels(lambda: run_group(members, dev), dev)
  assert len(names) == 2 and 'group_forward' in names[0] and 'group_backward' in names[1], names
  # nothing at all
  members = _group_c(dev, dx=False, grads='none')
  assert_members_equal_single(members, dev)
  assert len(_mlp_kernels(lambda: run_group(members, dev), dev)) == 1


def test_a_nan_row_stays_in_its_member(dev):
  members = _group_a(dev, 'swish')
  clean = run_group(members, dev)
  members[2].x[40] = float('nan')
  got = run_group(members, dev)
  for i, (g, c) in enumerate(zip(got, clean)):
    for name in g:
      if i != 2:
        assert bool(torch.isfinite(g[name]).all()) and _same(g[name], c[name]), (i, name)
  assert bool(torch.isnan(got[2]['y']).any())
  assert_members_equal_single(members, dev, got)


# ---- the autograd function ----------------------------------------------------------------------

def _autograd_members(dev):
  ms = _group_a(dev, 'tanh')[1:] + _group_c(dev)[:2]
  out = []
  for m in ms:
    layers = [(w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_())
              for w, b in m.layers]
    out.append((layers, m.x.detach().clone().requires_grad_(), m.activation, m.dy))
  return out


def test_mlp_group_gradients_are_fused_mlps(dev):
  members = _autograd_members(dev)
  leaves = [[x] + networks.parameters(layers) for layers, x, _, _ in members]
  ys = fm.mlp_group([m[:3] for m in members], fused=True)
  loss = sum((y * m[3]).sum() for y, m in zip(ys, members))
  got = torch.autograd.grad(loss, [t for ls in leaves for t in ls])
  at = 0
  for (layers, x, act, dy), ls, y in zip(members, leaves, ys):
    want_y = fm.fused_mlp(layers, x, act, fused=True)
    want = torch.autograd.grad((want_y * dy).sum(), ls)
    assert torch.equal(y, want_y)
    for g, w in zip(got[at:at + len(ls)], want):
      assert torch.equal(g, w)
    at += len(ls)
  # under no_grad: the same bits, no graph
  with torch.no_grad():
    for y0, y in zip(fm.mlp_group([m[:3] for m in members], fused=True), ys):
      assert not y0.requires_grad and torch.equal(y0, y)


def test_an_unused_member_gets_no_backward_work(dev):
  members = _autograd_members(dev)
  frozen = [(w.detach(), b.detach()) for w, b in members[1][0]]  # no gradient can be wanted
  members[1] = (frozen, members[1][1].detach(), *members[1][2:])
  ys = fm.mlp_group([m[:3] for m in members], fused=True)
  assert not ys[1].requires_grad
  used = (0, 3)
  loss = sum((ys[i] * members[i][3]).sum() for i in used)
  leaves = [t for layers, x, _, _ in members for t in [x] + networks.parameters(layers)
            if t.requires_grad]
  names = []

  def backward():
    names.append(torch.autograd.grad(loss, leaves, allow_unused=True))
  kernels = _mlp_kernels(backward, dev)
  assert len(kernels) == 2 and all('group' in k for k in kernels), kernels
  at = 0
  for i, (layers, x, act, dy) in enumerate(members):
    ls = [t for t in [x] + networks.parameters(layers) if t.requires_grad]
    grads = names[0][at:at + len(ls)]
    at += len(ls)
    if i in used:
      want = torch.autograd.grad((fm.fused_mlp(layers, x, act, fused=True) * dy).sum(), ls)
      assert all(torch.equal(g, w) for g, w in zip(grads, want)), i
    else:
      assert all(g is None for g in grads), i


def test_graph_capture_replays_the_eager_bits(dev):
  """Forward plus backward captured on one stream: the replay gives the eager
  bits and sees weights changed in place."""
  members = _autograd_members(dev)[:3]
  leaves = [t for layers, x, _, _ in members for t in [x] + networks.parameters(layers)]
  params = [t for layers, _, _, _ in members for t in networks.parameters(layers)]

  def step():
    ys = fm.mlp_group([m[:3] for m in members], fused=True)
    loss = sum((y * m[3]).sum() for y, m in zip(ys, members))
    return [y.detach() for y in ys] + list(torch.autograd.grad(loss, leaves))
  side = torch.cuda.Stream(dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side):
    step()
  torch.cuda.current_stream(dev).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, capture_error_mode='thread_local'):
    outs = step()
  for _ in range(2):
    graph.replay()
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(outs, step())):
      assert torch.equal(g, w), k
    with torch.no_grad():  # an optimiser's in-place update
      for p in params:
        p.mul_(1.25).add_(0.01)


# ---- the learners -------------------------------------------------------------------------------

def _sac_case(dev, B=130, O=87, A=8):
  ts = sac.init_training_state(O, A, 1e-3, sac_networks.make_sac_networks, 3, device=dev)
  g = torch.Generator().manual_seed(5)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  with torch.no_grad():
    for t in networks.parameters(ts.policy_layers, *ts.q_layers):
      if t.dim() == 1:
        t.copy_(0.1 * r(*t.shape))
    for t in networks.parameters(*ts.target_q_layers):
      t.add_(0.05 * r(*t.shape))
  flags = lambda p: (torch.rand((B,), generator=g) < p).float().to(dev)  # noqa: E731
  trans = {'observation': r(B, O), 'action': torch.tanh(r(B, A)), 'reward': r(B),
           'discount': 1 - flags(0.2), 'next_observation': r(B, O), 'truncation': flags(0.2)}
  normalizer = (r(O), (0.5 + 1.5 * torch.rand((O,), generator=g)).to(dev))
  return ts, normalizer, trans, (r(B, A), r(B, A), r(B, A))


def test_sac_gradients_grouped_are_the_ungrouped_bits(dev):
  case = _sac_case(dev)
  runs, counts = {}, {}
  for group in (False, True):
    call = functools.partial(sac_head.gradients, *case, 1.5, 0.95, fused_mlp=True, fused_group=group)
    a, c, p, metrics = call()
    runs[group] = [t.clone() for t in (*a, *c, *p, metrics.vector)]
    counts[group] = len(_mlp_kernels(call, dev))
  assert len(runs[True]) == len(runs[False]) == 1 + 12 + 6 + 1
  for k, (g, w) in enumerate(zip(runs[True], runs[False])):
    assert torch.equal(g, w), k
  assert bool(torch.isfinite(torch.cat([t.reshape(-1) for t in runs[True]])).all())
  assert counts == {True: 7, False: 16}
  # the chained losses: q_apply groups its critics
  obs, action = case[2]['observation'], case[2]['action']
  want = sac_networks.q_apply(case[0].q_layers, obs, action, fused_mlp=True)
  got = sac_networks.q_apply(case[0].q_layers, obs, action, fused_mlp=True, fused_group=True)
  assert torch.equal(got, want)
  params = sac_networks.q_parameters(case[0].q_layers)
  for g, w in zip(torch.autograd.grad(got.square().sum(), params),
                  torch.autograd.grad(want.square().sum(), params)):
    assert torch.equal(g, w)


def _ppo_case(dev, B=5, T=33, O=27, A=4):
  g = torch.Generator().manual_seed(9)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  done = (torch.rand((B, T), generator=g) < 0.1).float().to(dev)
  data = losses.Transition(
      observation=r(B, T, O), action=torch.tanh(r(B, T, A)), reward=r(B, T), discount=1 - done,
      next_observation=r(B, T, O), truncation=done * (torch.rand((B, T), generator=g) < 0.5).float().to(dev),
      raw_action=r(B, T, A), log_prob=r(B, T) - 3)
  policy, value = networks.make_ppo_networks(O, A, seed=2, device=dev)
  normalizer = (r(O), (0.5 + torch.rand((O,), generator=g)).to(dev))
  return policy, value, normalizer, data, r(B, T, A)


def test_ppo_loss_grouped_is_the_ungrouped_bits(dev):
  policy, value, normalizer, data, eps = _ppo_case(dev)
  params = networks.parameters(policy, value)
  runs, counts = {}, {}
  for group in (False, True):
    kw = dict(fused_mlp=True, fused_head=True)
    if group:
      kw['fused_group'] = True

    def step():
      for p in params:
        p.grad = None
      loss, _ = losses.ppo_loss(policy, value, normalizer, data, eps, **kw)
      loss.backward()
      return loss
    loss = step()
    runs[group] = [loss.detach().clone()] + [p.grad.clone() for p in params]
    counts[group] = len(_mlp_kernels(step, dev))
  for k, (g, w) in enumerate(zip(runs[True], runs[False])):
    assert torch.equal(g, w), k
  assert bool(torch.isfinite(torch.cat([t.reshape(-1) for t in runs[True]])).all())
  assert counts == {True: 3, False: 7}


def _flat(params):
  return torch.cat([t.detach().reshape(-1) for t in params])


def test_sac_train_end_to_end(dev):
  factory = functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=(32, 32))
  kw = dict(num_timesteps=2000, episode_length=50, num_envs=16, num_eval_envs=16, batch_size=32,
            grad_updates_per_step=2, min_replay_size=64, num_evals=2, seed=1, device=dev,
            normalize_observations=True, network_factory=factory, fused_mlp=True, fused_adam=True,
            fused_head=True)
  runs = {}
  for name, more in (('plain', {}), ('off', {'fused_group': False}), ('on', {'fused_group': True})):
    _, params, metrics = sac.train('inverted_pendulum', **kw, **more)
    runs[name] = _flat(networks.parameters(params[1]))
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in metrics.values()), name
  assert torch.equal(runs['off'], runs['plain'])
  O, A = params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2
  init = _flat(networks.parameters(factory(O, A, seed=1, device=dev)[0]))
  assert runs['on'].shape == init.shape and not torch.equal(runs['on'], init)
  assert bool(torch.isfinite(runs['on']).all())
  assert torch.equal(runs['on'], runs['plain'])  # each member's bits are the ungrouped call's


def test_ppo_train_end_to_end(dev):
  kw = dict(num_timesteps=1900, episode_length=50, num_eval_envs=32, seed=1, device=dev, num_envs=64,
            unroll_length=5, batch_size=32, num_minibatches=4, num_updates_per_batch=2, num_evals=2,
            normalize_observations=True, fused_mlp=True, fused_head=True)
  runs = {}
  for name, more in (('plain', {}), ('off', {'fused_group': False}), ('on', {'fused_group': True})):
    _, params, metrics = ppo.train('inverted_pendulum', **kw, **more)
    runs[name] = _flat(networks.parameters(*params[1:]))
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in metrics.values()), name
  assert torch.equal(runs['off'], runs['plain'])
  O, A = params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2
  init = _flat(networks.parameters(*networks.make_ppo_networks(O, A, seed=1, device=dev)))
  assert runs['on'].shape == init.shape and not torch.equal(runs['on'], init)
  assert bool(torch.isfinite(runs['on']).all())
  assert torch.equal(runs['on'], runs['plain'])
