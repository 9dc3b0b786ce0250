"""The fused optimiser step on the GPU (`bx_adam_step`, `optim.FusedAdam`) and
the learners' `fused_adam` switches.

A workgroup owns `abi.OPT_CHUNK` = 1024 elements of one tensor and a lane 4 of
them in the 16-byte form, so the sizes are: a 0-dim tensor, 3 and 6 (only the
tail lane's scalar loop, 3 and 2 elements), 255 (63 full lanes and a tail of
3), 1023 / 1024 / 1025 (a chunk less one, exactly one, one and a lane of one
element in the next), 2050 (a tail of 2 in the third chunk) and 4097 (five
workgroups). 1, 7, 32 and 33 tensors: one, a few, a full table, and a table
and a second call.
"""
import math
import types

import numpy as np
import pytest
import torch

from brax_amd import _native, abi
from brax_amd.training import FusedAdam, optim

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
SIZES = [(), (3,), (255,), (1023,), (1024,), (1025,), (4097,), (6,), (2050,)]
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
SENTINEL = 0x7FC0BEEF  # a NaN with a payload, as int32
KERNEL = 'adam_step_kernel'


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _held(got, ref, yard, what, ratios=None):
  """max |got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|)
  (`test_gpu_ppo_head._held`'s rule)."""
  err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
  unit = max(float((yard.double() - ref).abs().max()) if ref.numel() else 0.0,
             EPS * (float(ref.abs().max()) if ref.numel() else 0.0))
  ratio = err / unit if unit else (0.0 if err == 0 else math.inf)
  if ratios is not None:
    ratios.append((ratio, what))
  assert ratio <= 8, (what, err, unit)


def _shapes(count):
  return [SIZES[k % len(SIZES)] for k in range(count)]


def _randn(shapes, g, dev):
  return [torch.randn(s, generator=g).to(dev) for s in shapes]


# ---- 1. accuracy ----------------------------------------------------------------------------

@pytest.mark.parametrize('count', [1, 7, 32, 33])
def test_five_steps_against_float64(dev, count):
  """p, m and v after each of 5 steps against `reference_step` in float64,
  `torch.optim.Adam(foreach=True)` in float32 as the yardstick; two groups at
  lr 3e-4 and 1e-2; the gradients through `p.grad` on odd steps and through
  `step(grads)` on even ones.

  The rule's maxima run over all the elements of a case's tensors of one kind
  (all p, all m, all v) at one step. The step is elementwise and treats every
  element of every tensor alike, so they are one population; a tensor on its
  own is not, where it is 0-dim: the yardstick's error on one element is a
  single draw that lands arbitrarily near zero, and m of a scalar (a moving
  average of zero-mean gradients of size 1) is far smaller than the
  gradients whose float32 rounding, 2^-24 |g| (1 - beta1), it carries. The
  one-tensor case is therefore the 4097-element tensor; the 0-dim one is in
  the other three."""
  g = torch.Generator().manual_seed(100 + count)
  shapes = _shapes(count) if count > 1 else [(4097,)]
  half = (count + 1) // 2
  params = _randn(shapes, g, dev)
  yard = [p.clone().requires_grad_() for p in params]
  ref = [p.double() for p in params]
  ref_m, ref_v = [torch.zeros_like(p) for p in ref], [torch.zeros_like(p) for p in ref]
  groups = [dict(params=params[:half], lr=3e-4)] + (
      [dict(params=params[half:], lr=1e-2)] if count > 1 else [])
  lrs = [3e-4] * half + [1e-2] * (count - half)
  opt = FusedAdam(groups, betas=BETAS, eps=ADAM_EPS)
  adam = torch.optim.Adam(
      [dict(params=yard[:half], lr=3e-4)] + ([dict(params=yard[half:], lr=1e-2)] if count > 1 else []),
      betas=BETAS, eps=ADAM_EPS, foreach=True)
  ratios = []
  for step in range(1, 6):
    grads = _randn(shapes, g, dev)
    versions = [p._version for p in params]  # pylint: disable=protected-access
    if step % 2:
      for p, gr in zip(params, grads):
        p.grad = gr
      opt.step()
      opt.zero_grad()
      assert all(p.grad is None for p in params)
    else:
      opt.step(grads)
    assert all(p._version > v for p, v in zip(params, versions))  # pylint: disable=protected-access
    for p, gr in zip(yard, grads):
      p.grad = gr.clone()
    adam.step()
    optim.reference_step(ref, [x.double() for x in grads], ref_m, ref_v, step, lrs, BETAS, ADAM_EPS)
    assert opt.step_count == step
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
    states = [adam.state[y] for y in yard]
    _held(cat(params), cat(ref), cat(yard), f'p step {step}', ratios)
    _held(cat([opt.exp_avg(k) for k in range(count)]), cat(ref_m),
          cat([s['exp_avg'] for s in states]), f'm step {step}', ratios)
    _held(cat([opt.exp_avg_sq(k) for k in range(count)]), cat(ref_v),
          cat([s['exp_avg_sq'] for s in states]), f'v step {step}', ratios)
  print(f'{count} tensors: worst error ratio', max(ratios))


# ---- the C entry point on arrays of any alignment -------------------------------------------

class _Arrays:
  """p, g, m, v and target of every tensor as views at element `offset[k]` of
  sentinel-filled buffers of their own: offset 4 is 16-byte aligned, offset 1
  is 4-byte aligned only. `offset[k]` may be one int or a dict per array name."""
  NAMES = ('p', 'g', 'm', 'v', 't')

  def __init__(self, shapes, values, offsets, dev):
    self.bufs, self.views, self.shapes = [], [], shapes
    for k, shape in enumerate(shapes):
      n = int(np.prod(shape, dtype=np.int64))
      bufs, views = {}, {}
      for name in self.NAMES:
        off = offsets[k][name] if isinstance(offsets[k], dict) else offsets[k]
        buf = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=dev)
        view = buf.view(torch.float32)[off:off + n]
        view.copy_(values[name][k].reshape(-1))
        bufs[name], views[name] = (buf, off, n), view
        assert view.data_ptr() % 16 == (0 if off % 4 == 0 else 4 * (off % 4))
      self.bufs.append(bufs)
      self.views.append(views)

  def call(self, step, lrs, taus, with_target, stream=None):
    """One bx_adam_step over all tensors (at most 32)."""
    table = (abi.BxOptTensor * len(self.views))()
    for k, (e, v) in enumerate(zip(table, self.views)):
      e.p, e.g, e.m, e.v = (v[n].data_ptr() for n in 'pgmv')
      e.target = v['t'].data_ptr() if with_target[k] else None
      e.n, e.lr, e.tau = v['p'].numel(), lrs[k], taus[k]
    _native.check(_native.lib().bx_adam_step(table, len(self.views), step, BETAS[0], BETAS[1],
                                             ADAM_EPS, stream))
    torch.cuda.synchronize()

  def guards_intact(self):
    for bufs in self.bufs:
      for name, (buf, off, n) in bufs.items():
        if not (bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())):
          return False, name
    return True, None

  def get(self, name):
    return [v[name].clone() for v in self.views]


def _values(shapes, g, dev):
  """Random p, g and target, and moments as after some steps (m any sign, v >= 0)."""
  vals = {'p': _randn(shapes, g, dev), 'g': _randn(shapes, g, dev), 't': _randn(shapes, g, dev)}
  vals['m'] = [0.1 * x for x in _randn(shapes, g, dev)]
  vals['v'] = [0.01 * x * x for x in _randn(shapes, g, dev)]
  return vals


def _case(dev, seed=7, count=9):
  g = torch.Generator().manual_seed(seed)
  shapes = _shapes(count)
  vals = _values(shapes, g, dev)
  lrs = [3e-4 if k % 2 else 1e-2 for k in range(count)]
  return shapes, vals, lrs


# ---- 2. the target update -------------------------------------------------------------------

@pytest.mark.parametrize('tau', [0.005, 1.0, 0.0])
def test_target_update_is_three_float32_operations(dev, tau):
  shapes, vals, lrs = _case(dev)
  n = len(shapes)
  with_target = [k % 2 == 0 for k in range(n)]
  a = _Arrays(shapes, vals, [4] * n, dev)
  a.call(3, lrs, [tau] * n, with_target)
  assert a.guards_intact() == (True, None)
  for k in range(n):
    t_old, p_new, got = vals['t'][k].reshape(-1), a.views[k]['p'], a.views[k]['t']
    assert not torch.equal(p_new, vals['p'][k].reshape(-1))
    if with_target[k]:
      assert torch.equal(got, t_old * (1 - tau) + p_new * tau), (k, tau)
    else:
      assert torch.equal(got, t_old)  # not in the table: untouched
  if tau == 1.0:
    assert torch.equal(a.views[0]['t'], a.views[0]['p'])
  if tau == 0.0:
    assert torch.equal(a.views[0]['t'], vals['t'][0].reshape(-1))


# ---- 3. layout ------------------------------------------------------------------------------

def test_unaligned_and_mixed_layouts_give_the_aligned_bits(dev):
  shapes, vals, lrs = _case(dev)
  n = len(shapes)
  taus, with_target = [0.005] * n, [k % 3 != 1 for k in range(n)]
  mixed = [4 if k % 2 else 1 for k in range(n)]
  # one array alone off the 16-byte grid sends its tensor down the float path
  mixed[3] = {'p': 4, 'g': 1, 'm': 4, 'v': 4, 't': 4}
  mixed[5] = {'p': 4, 'g': 4, 'm': 4, 'v': 4, 't': 2}
  mixed[7] = {'p': 4, 'g': 4, 'm': 3, 'v': 4, 't': 4}
  results = []
  for offsets in ([4] * n, [1] * n, mixed):
    a = _Arrays(shapes, vals, offsets, dev)
    a.call(2, lrs, taus, with_target)
    assert a.guards_intact() == (True, None), offsets
    results.append({name: a.get(name) for name in 'pmvt'})
    for k in range(n):
      assert torch.equal(a.views[k]['g'], vals['g'][k].reshape(-1))
      assert not bool(torch.isnan(a.views[k]['p']).any())
  for other in results[1:]:
    for name in 'pmvt':
      for x, y in zip(results[0][name], other[name]):
        assert torch.equal(x, y), name


# ---- 4. determinism and isolation -----------------------------------------------------------

@pytest.mark.parametrize('bad', [math.nan, math.inf, -math.inf])
def test_a_non_finite_gradient_element_stays_in_its_element(dev, bad):
  shapes, vals, lrs = _case(dev)
  n = len(shapes)
  taus, with_target = [0.005] * n, [True] * n

  def run(values, offset):
    a = _Arrays(shapes, values, [offset] * n, dev)
    a.call(4, lrs, taus, with_target)
    return {name: a.get(name) for name in 'pmvt'}
  clean, again = run(vals, 4), run(vals, 4)
  for name in 'pmvt':
    for x, y in zip(clean[name], again[name]):
      assert torch.equal(x, y)  # two runs, the same bits
  # tensor 5 (1025 elements): element 1024 is the next workgroup's tail lane
  # in the 16-byte form; element 517 sits inside a full lane's four
  for offset, (k, i) in ((4, (5, 1024)), (4, (5, 517)), (1, (6, 4096))):
    dirty = dict(vals, g=[x.clone() for x in vals['g']])
    dirty['g'][k].reshape(-1)[i] = bad
    got = run(dirty, offset)
    for name in 'pmvt':
      for j, (x, y) in enumerate(zip(got[name], clean[name])):
        if j == k:
          keep = torch.ones(x.numel(), dtype=torch.bool, device=dev)
          keep[i] = False
          assert torch.equal(x[keep], y[keep]), (name, j)
        else:
          assert torch.equal(x, y), (name, j)
    # the element itself: the float64 restatement's class
    one = lambda name: vals[name][k].reshape(-1)[i:i + 1].double().clone()  # noqa: E731
    p, m, v, t = one('p'), one('m'), one('v'), one('t')
    optim.reference_step([p], [torch.tensor([bad], dtype=torch.float64, device=dev)], [m], [v], 4,
                         lrs[k], BETAS, ADAM_EPS, targets=[t], tau=taus[k])
    for name, want in (('p', p), ('m', m), ('v', v), ('t', t)):
      x = got[name][k][i:i + 1]
      assert bool(torch.isnan(x)) == bool(torch.isnan(want)), (name, bad)
      assert bool(torch.isinf(x)) == bool(torch.isinf(want)), (name, bad)
      if bool(torch.isinf(want)):
        assert bool(x > 0) == bool(want > 0)
    assert bool(torch.isnan(got['p'][k][i]))


# ---- 5. empty tensors and split lists -------------------------------------------------------

def test_empty_tensors_and_a_list_longer_than_one_table(dev):
  g = torch.Generator().manual_seed(11)
  shapes = _shapes(33)
  params, grads = _randn(shapes, g, dev), _randn(shapes, g, dev)
  empty = lambda: torch.zeros((0,), device=dev)  # noqa: E731

  def run(build):
    ps = [p.clone() for p in params]
    opt, gs = build(ps)
    opt.step(gs)
    opt.step(gs)
    torch.cuda.synchronize()
    return ps, opt
  whole, opt = run(lambda ps: (FusedAdam([dict(params=ps, lr=1e-2)]), grads))
  assert opt.step_count == 2 and len(opt._tables) == 2  # pylint: disable=protected-access
  # two optimisers over the first 32 and the last one
  ps = [p.clone() for p in params]
  first, last = FusedAdam([dict(params=ps[:32], lr=1e-2)]), FusedAdam([dict(params=ps[32:], lr=1e-2)])
  for _ in range(2):
    first.step(grads[:32])
    last.step(grads[32:])
  for x, y in zip(whole, ps):
    assert torch.equal(x, y)
  assert torch.equal(opt.exp_avg_sq(32), last.exp_avg_sq(0))
  # empty tensors among them, and a tensor without a gradient, change nothing else
  def with_empties(ps):
    mixed = [empty()] + ps[:5] + [empty(), empty()] + ps[5:] + [empty()]
    gs = [empty()] + grads[:5] + [empty(), empty()] + grads[5:] + [empty()]
    return FusedAdam([dict(params=mixed, lr=1e-2)]), gs
  padded, _ = run(with_empties)
  for x, y in zip(whole, padded):
    assert torch.equal(x, y)
  skipped, opt = run(lambda ps: (FusedAdam([dict(params=ps, lr=1e-2)]),
                                 [None if k == 4 else x for k, x in enumerate(grads)]))
  for k, (x, y) in enumerate(zip(whole, skipped)):
    assert torch.equal(y, params[k] if k == 4 else x)
  assert not bool(opt.exp_avg(4).any())


# ---- 6. graph capture -----------------------------------------------------------------------

def test_a_captured_step_replays_the_eager_bits(dev):
  """One `step` captured on a single stream, its gradients in persistent
  buffers. The step count is a host value baked into the captured launch's
  arguments (the bias corrections), so a replay repeats THAT step: the test
  replays step 1 on restored state and on new gradients written into the same
  buffers, and compares with eager step 1. Capture across a changing step
  count is out of scope."""
  g = torch.Generator().manual_seed(13)
  shapes = _shapes(9)
  start, targets0 = _randn(shapes, g, dev), _randn(shapes, g, dev)
  grads_a, grads_b = _randn(shapes, g, dev), _randn(shapes, g, dev)

  def fresh():
    ps, ts = [p.clone() for p in start], [t.clone() for t in targets0]
    return ps, ts, FusedAdam([dict(params=ps, lr=1e-2, targets=ts, tau=0.005)])
  eager = {}
  for name, gs in (('a', grads_a), ('b', grads_b)):
    ps, ts, opt = fresh()
    opt.step(gs)
    eager[name] = (ps, ts, opt.exp_avg_sq(8).clone())
  ps, ts, opt = fresh()
  buffers = [x.clone() for x in grads_a]
  graph = torch.cuda.CUDAGraph()
  torch.cuda.synchronize()
  with torch.cuda.graph(graph):
    opt.step(buffers)
  assert opt.step_count == 1
  for x, y in zip(ps, start):
    assert torch.equal(x, y)  # captured, not run
  graph.replay()
  torch.cuda.synchronize()
  for got, want in zip(ps + ts, eager['a'][0] + eager['a'][1]):
    assert torch.equal(got, want)
  # restored state, other gradients in the same buffers
  with torch.no_grad():
    for x, y in zip(ps + ts + buffers, start + targets0 + grads_b):
      x.copy_(y)
    opt._m.zero_()  # pylint: disable=protected-access
    opt._v.zero_()  # pylint: disable=protected-access
  graph.replay()
  torch.cuda.synchronize()
  for got, want in zip(ps + ts, eager['b'][0] + eager['b'][1]):
    assert torch.equal(got, want)
  assert torch.equal(opt.exp_avg_sq(8), eager['b'][2])


# ---- 7. the learners ------------------------------------------------------------------------

HIDDEN = (16, 16)


def _sac_factory():
  import functools
  from brax_amd.training import sac_networks
  return functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=HIDDEN)


def _sac_tensors(ts):
  from brax_amd.training import sac_networks
  return sac_networks.q_parameters([ts.policy_layers] + ts.q_layers + ts.target_q_layers) + [
      ts.log_alpha]


def _sac_run(dev, dtype, steps=3, **kw):
  from brax_amd.training import sac
  O, A, B, tau = 5, 2, 8, 0.05
  ts = sac.init_training_state(O, A, 1e-3, _sac_factory(), 3, dev, dtype=dtype, tau=tau, **kw)
  g = torch.Generator().manual_seed(17)
  r = lambda *s: torch.randn(s, generator=g).to(device=dev, dtype=dtype)  # noqa: E731
  out = []
  for _ in range(steps):
    batch = {'observation': r(B, O), 'action': torch.tanh(r(B, A)), 'reward': r(B),
             'discount': (torch.rand((B,), generator=g) < 0.8).to(device=dev, dtype=dtype),
             'next_observation': r(B, O),
             'truncation': (torch.rand((B,), generator=g) < 0.2).to(device=dev, dtype=dtype)}
    eps = tuple(r(B, A) for _ in range(3))
    metrics = sac.sgd_step(ts, None, batch, eps, reward_scaling=0.5, discounting=0.95, tau=tau)
    out.append(([t.detach().clone() for t in _sac_tensors(ts)], metrics))
  return ts, out


def test_sac_sgd_step_with_the_fused_optimizer(dev):
  ts64, ref = _sac_run(dev, torch.float64)
  ts32, yard = _sac_run(dev, torch.float32)
  tsf, got = _sac_run(dev, torch.float32, fused_adam=True)
  assert tsf.fused_optimizer is not None and tsf.q_optimizer is None
  assert tsf.policy_optimizer is None and tsf.alpha_optimizer is None
  assert len(tsf.fused_optimizer.params) == 19 and tsf.gradient_steps == 3
  assert sum(t is not None for t in tsf.fused_optimizer.targets) == 12
  assert tsf.fused_optimizer.step_count == 3 and ts32.fused_optimizer is None
  ratios = []
  for step, ((g_, gm), (r_, _), (y_, _)) in enumerate(zip(got, ref, yard)):
    for k, (a, b, c) in enumerate(zip(g_, r_, y_)):
      _held(a, b, c, f'sac tensor {k} step {step}', ratios)
    assert torch.equal(gm['alpha'], torch.exp(g_[-1]))
    assert all(math.isfinite(float(v)) for v in gm.values())
  print('sac: worst error ratio', max(ratios))
  assert not torch.equal(got[-1][0][-1], torch.zeros((), device=dev))
  from brax_amd.training import sac
  with pytest.raises(ValueError, match='tau'):
    sac.sgd_step(tsf, None, {}, (None, None, None), tau=0.5)
  # the switch off is the call without it, bit for bit
  _, off = _sac_run(dev, torch.float32, fused_adam=False)
  for a, b in zip(off[-1][0], yard[-1][0]):
    assert torch.equal(a, b)
  with pytest.raises(NotImplementedError, match='float64'):
    _sac_run(dev, torch.float64, steps=0, fused_adam=True)
  assert _sac_run(dev, torch.float64, steps=0, fused_adam=None)[0].fused_optimizer is None


def _ppo_learner(dev, **kw):
  from brax_amd.training import ppo
  env = types.SimpleNamespace(observation_size=7, action_size=2)
  return ppo.Learner(env, num_envs=8, unroll_length=3, batch_size=4, num_minibatches=2,
                     num_updates_per_batch=1, learning_rate=1e-3, entropy_cost=1e-2, seed=5,
                     device=dev, **kw)


def _ppo_data(dev):
  from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
  from brax_amd.training import networks
  from brax_amd.training.losses import Transition
  B, T, O, A = 8, 3, 7, 2
  g = torch.Generator().manual_seed(19)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  policy, _ = networks.make_ppo_networks(O, A, seed=5, device=dev)
  obs, raw = r(B, T, O), r(B, T, A)
  with torch.no_grad():
    loc, s = torch.chunk(networks.mlp(policy, obs), 2, dim=-1)
    log_prob = normal_tanh_log_prob(loc, head_scale(s, 1e-3), raw).sum(-1) + 0.2 * r(B, T)
  flags = lambda p: (torch.rand((B, T), generator=g) < p).float().to(dev)  # noqa: E731
  return Transition(observation=obs, action=torch.tanh(raw), reward=r(B, T),
                    discount=1 - flags(0.2), next_observation=r(B, T, O), truncation=flags(0.2),
                    raw_action=raw, log_prob=log_prob)


def test_ppo_update_with_the_fused_optimizer(dev):
  from brax_amd.training import networks
  from brax_amd.training.losses import ppo_loss
  data = _ppo_data(dev)
  fused, torch_form, default = (_ppo_learner(dev, fused_adam=True),
                                _ppo_learner(dev, fused_adam=False), _ppo_learner(dev))
  assert isinstance(fused.optimizer, FusedAdam) and len(fused.optimizer.params) == 22
  assert isinstance(torch_form.optimizer, torch.optim.Adam)
  before = fused.actor.params.clone()
  # the float64 reference: the layers cast to double, the update loop's own
  # draws (the same generator seed), stepped with reference_step
  cast = lambda layers: [(w.detach().double().requires_grad_(), b.detach().double().requires_grad_())  # noqa: E731
                         for w, b in layers]
  pl, vl = cast(fused.policy_layers), cast(fused.value_layers)
  p64 = networks.parameters(pl, vl)
  m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
  gen = torch.Generator(device=dev).manual_seed(5)
  perm = torch.randperm(8, generator=gen, device=dev)
  shuffled = data.map(lambda x: x[perm].double())
  for m in range(2):
    mb = shuffled.map(lambda x, m=m: x[m * 4:(m + 1) * 4])
    eps = torch.randn((4, 3, 2), generator=gen, device=dev)
    loss, _ = ppo_loss(pl, vl, None, mb, eps.double(), fused=False, **fused.loss_kwargs)
    grads = torch.autograd.grad(loss, p64)
    optim.reference_step(p64, grads, m64, v64, m + 1, 1e-3, BETAS, ADAM_EPS)
  metrics = [l.update(data) for l in (fused, torch_form, default)]
  torch.cuda.synchronize()
  ratios = []
  for k, (a, b, c) in enumerate(zip(networks.parameters(fused.policy_layers, fused.value_layers), p64,
                                    networks.parameters(torch_form.policy_layers,
                                                        torch_form.value_layers))):
    _held(a.detach(), b.detach(), c.detach(), f'ppo tensor {k}', ratios)
  print('ppo: worst error ratio', max(ratios))
  assert fused.optimizer.step_count == 2
  assert all(math.isfinite(float(v)) for v in metrics[0].values())
  # the acting policy reads the new weights
  assert not torch.equal(fused.actor.params, before)
  assert torch.equal(fused.actor.params, fused.make_policy().params)
  # the switch off is the call without it, bit for bit
  for a, b in zip(networks.parameters(torch_form.policy_layers, torch_form.value_layers),
                  networks.parameters(default.policy_layers, default.value_layers)):
    assert torch.equal(a, b)
  assert torch.equal(torch_form.actor.params, default.actor.params)


def _flat(layer_lists):
  return torch.cat([t.detach().reshape(-1) for layers in layer_lists for wb in layers for t in wb])


@pytest.mark.parametrize('others', [False, True])
def test_ppo_train_end_to_end(dev, others):
  from brax_amd.training import networks, ppo
  make_policy, params, metrics = ppo.train(
      'inverted_pendulum', num_timesteps=1900, episode_length=50, num_eval_envs=32, seed=1,
      device=dev, num_envs=64, unroll_length=5, batch_size=32, num_minibatches=4,
      num_updates_per_batch=2, num_evals=2, normalize_observations=True, fused_adam=True,
      fused_mlp=others, fused_head=others)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  learner = make_policy.__self__
  assert isinstance(learner.optimizer, FusedAdam) and learner.optimizer.step_count > 0
  got = _flat(params[1:])
  init = _flat(networks.make_ppo_networks(params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2,
                                          seed=1, device=dev))
  assert torch.isfinite(got).all() and got.shape == init.shape and not torch.equal(got, init)
  assert torch.equal(learner.actor.params, make_policy(params).params)


@pytest.mark.parametrize('others', [False, True])
def test_sac_train_end_to_end(dev, others):
  from brax_amd.training import sac
  make_policy, params, metrics = sac.train(
      'inverted_pendulum', num_timesteps=2000, episode_length=50, num_envs=16, num_eval_envs=32,
      batch_size=32, num_evals=2, min_replay_size=100, max_replay_size=512,
      grad_updates_per_step=1, normalize_observations=True, network_factory=_sac_factory(),
      device=dev, fused_adam=True, fused_mlp=others)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  learner = make_policy.__self__
  opt = learner.ts.fused_optimizer
  assert opt is not None and opt.step_count == learner.ts.gradient_steps > 0
  O, A = learner.env.observation_size, learner.env.action_size
  init = sac.init_training_state(O, A, 1e-4, _sac_factory(), 0, dev)
  for got, was in zip(_sac_tensors(learner.ts), _sac_tensors(init)):
    assert torch.isfinite(got).all() and not torch.equal(got.detach(), was.detach())
  assert torch.equal(learner.actor.params, make_policy(params).params)


# ---- 8. one launch per step -----------------------------------------------------------------

def _launches(fn, dev):
  from torch.autograd import DeviceType
  from torch.profiler import ProfilerActivity, profile
  torch.cuda.synchronize(dev)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize(dev)
  return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and KERNEL in e.name)


def test_one_launch_per_step(dev):
  data, learner = _ppo_data(dev), _ppo_learner(dev, fused_adam=True)
  learner.update(data)  # (first calls: module loads outside the profile)
  assert _launches(lambda: learner.update(data), dev) == 2  # 2 minibatches, 1 pass: 2 Adam steps
  assert _launches(lambda: _sac_run(dev, torch.float32, steps=3, fused_adam=True), dev) == 3
  assert _launches(lambda: _sac_run(dev, torch.float32, steps=3), dev) == 0
