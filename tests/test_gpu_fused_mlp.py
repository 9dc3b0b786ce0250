"""The fused MLP kernels (`bx_mlp_forward` / `bx_mlp_backward`) on the GPU.

A workgroup owns 32 rows and its four waves split a layer's columns in tiles
of 32 (`brax_amd/csrc/mlp_kernels.hip`); the gradient launch gives a workgroup
a (32 in, 64 out) tile of one layer's dW and each of its 8 waves an eighth of
the rows. So: rows 1, 31, 33, 65, 130 (below, around and across row tiles; at
130 every gradient wave holds rows), widths that are no multiple of 32 or of
4 (129, 255, 3, 1), a one-column hidden layer, 8 layers, no hidden layer, and
an input wider than the 256-column LDS image (1024, walked in 4 chunks).
"""
import ctypes as C
import math

import pytest
import torch

from brax_amd import _native, abi
from brax_amd.training import fused_mlp as fm
from brax_amd.training import networks

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 33, 65, 130)
SIZES = ((5, 1), (7, 3, 2), (87, 32, 32, 32, 32, 16), (33, 256, 256, 1), (35, 129, 1, 255, 4),
         (12,) + (16,) * 7 + (3,), (1024, 40, 3))
ACTIVATIONS = ('relu', 'swish', 'tanh')
EPS = 2.0 ** -23
SENTINEL = 777.25
PAD = 64


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _ids(v):
  return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _to(layers, device=None, dtype=None):
  return [(w.detach().to(device=device, dtype=dtype).requires_grad_(),
           b.detach().to(device=device, dtype=dtype).requires_grad_()) for w, b in layers]


def _run(layers, x, dy, activation, fused):
  """[y, dx, dW_0, db_0, ...] of sum(y * dy)."""
  x = x.detach().clone().requires_grad_()
  y = networks.mlp(layers, x, activation, fused=fused)
  grads = torch.autograd.grad((y * dy).sum(), [x] + networks.parameters(layers))
  return [y.detach()] + list(grads)


def _names(layers):
  return ['y', 'dx'] + [f'{n}{l}' for l in range(len(layers)) for n in ('dW', 'db')]


def _random_case(sizes, rows, seed, dev):
  g = torch.Generator().manual_seed(seed)
  layers = networks.make_layers(sizes, g)
  with torch.no_grad():
    for _, b in layers:  # make_layers' biases are zero
      b.copy_(torch.randn(b.shape, generator=g) * 0.1)
  x = torch.randn((rows, sizes[0]), generator=g)
  dy = torch.randn((rows, sizes[-1]), generator=g)
  return _to(layers, dev), x.to(dev), dy.to(dev)


# ---- 1. the exact check ---------------------------------------------------------------------

def _integer_case(sizes, rows, seed):
  """Small integers. Up to 4 layers the weights are dense; deeper networks get
  sparse ones (about 4 non-zeros a column), so the magnitudes stay below 2^24
  through 8 layers."""
  g = torch.Generator().manual_seed(seed)
  layers = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    keep = torch.rand((i, o), generator=g) < (1.0 if len(sizes) <= 5 else min(1.0, 4.0 / i))
    w = torch.randint(-1, 2, (i, o), generator=g).float() * keep
    layers.append((w.requires_grad_(), torch.randint(0, 3, (o,), generator=g).float().requires_grad_()))
  x = torch.randint(-2, 3, (rows, sizes[0]), generator=g).float()
  dy = torch.randint(-2, 3, (rows, sizes[-1]), generator=g).float()
  return layers, x, dy


def _assert_exact_inputs(layers, x, dy):
  """On the CPU: the chained float32 form equals float64, and every partial
  sum in ANY order stays below 2^24: the network of absolute values (all
  pre-activations positive, so relu and its derivative are the identity)
  bounds every partial sum of the forward pass, and its gradients bound those
  of the backward pass."""
  got = _run(layers, x, dy, 'relu', False)
  want = _run(_to(layers, dtype=torch.float64), x.double(), dy.double(), 'relu', False)
  for g, w in zip(got, want):
    assert torch.equal(g.double(), w)
  mags = [(w.detach().abs().double().requires_grad_(), b.detach().abs().double().requires_grad_())
          for w, b in layers]
  bound = _run(mags, x.abs().double(), dy.abs().double(), 'relu', False)
  assert max(float(t.max()) for t in bound) < 2 ** 24


@pytest.mark.parametrize('sizes', SIZES, ids=_ids)
def test_exact_on_integer_data(dev, sizes):
  for rows in ROWS:
    layers, x, dy = _integer_case(sizes, rows, seed=rows)
    _assert_exact_inputs(layers, x, dy)
    want = _run(layers, x, dy, 'relu', False)
    dl = _to(layers, dev)
    chained = _run(dl, x.to(dev), dy.to(dev), 'relu', False)
    got = _run(dl, x.to(dev), dy.to(dev), 'relu', True)
    for name, g, c, w in zip(_names(layers), got, chained, want):
      assert torch.equal(c.cpu(), w), (rows, name, 'chained on the GPU')
      assert torch.equal(g, c), (rows, name)


# ---- 2. accuracy on random inputs -----------------------------------------------------------

def _held(got, ref, yard, what, ratios=None):
  """max |got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|)."""
  err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
  unit = max(float((yard.double() - ref).abs().max()) if ref.numel() else 0.0,
             EPS * (float(ref.abs().max()) if ref.numel() else 0.0))
  ratio = err / unit if unit else (0.0 if err == 0 else math.inf)
  if ratios is not None:
    ratios.append((ratio, what))
  assert ratio <= 8, (what, err, unit)


@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('sizes', SIZES, ids=_ids)
def test_accuracy_against_float64(dev, sizes, activation):
  ratios = []
  for rows in ROWS:
    layers, x, dy = _random_case(sizes, rows, seed=rows, dev=dev)
    ref = _run(_to(layers, dtype=torch.float64), x.double(), dy.double(), activation, False)
    yard = _run(layers, x, dy, activation, False)
    got = _run(layers, x, dy, activation, True)
    for name, g, r, y in zip(_names(layers), got, ref, yard):
      assert g.shape == r.shape and g.dtype == torch.float32
      _held(g, r, y, (rows, name), ratios)
  print('worst error ratio', _ids(sizes), activation, max(ratios))


# ---- 3. determinism -------------------------------------------------------------------------

@pytest.mark.parametrize('sizes', SIZES, ids=_ids)
def test_two_runs_give_the_same_bits(dev, sizes):
  for rows in ROWS:
    layers, x, dy = _random_case(sizes, rows, seed=7, dev=dev)
    a = _run(layers, x, dy, 'swish', True)
    b = _run(layers, x, dy, 'swish', True)
    for name, s, t in zip(_names(layers), a, b):
      assert torch.equal(s.view(torch.int32), t.view(torch.int32)), (rows, name)


# ---- 4. boundaries --------------------------------------------------------------------------

def _guarded(shape, dev):
  """A tensor of `shape` inside a buffer of sentinels, PAD words either side."""
  n = math.prod(shape)
  buf = torch.full((n + 2 * PAD,), SENTINEL, device=dev)
  return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf, n):
  return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


def _raw(layers, x, dy, activation, dev):
  """Both entry points on guarded outputs; returns ([y, dx, dW_0, ...], all guards intact)."""
  lib = _native.lib()
  params = [t.detach() for wb in layers for t in wb]
  net = fm._net(params, activation)
  rows = x.shape[0]
  hidden = sum(w.shape[1] for w, _ in layers[:-1])
  outs = {'y': _guarded((rows, layers[-1][0].shape[1]), dev), 'saved': _guarded((rows, hidden), dev),
          'dx': _guarded((rows, x.shape[1]), dev)}
  for k, p in enumerate(params):
    outs[f'g{k}'] = _guarded(tuple(p.shape), dev)
  nbytes = C.c_int64(0)
  _native.check(lib.bx_mlp_backward(C.byref(net), rows, None, x.stride(0), None, None, None, None,
                                    None, C.byref(nbytes), None))
  assert nbytes.value == max(16, 4 * rows * hidden)
  outs['work'] = _guarded((nbytes.value // 4,), dev)
  stream = torch.cuda.current_stream(dev).cuda_stream
  _native.check(lib.bx_mlp_forward(C.byref(net), rows, x.data_ptr(), x.stride(0),
                                   outs['y'][1].data_ptr(), outs['saved'][1].data_ptr() or None,
                                   stream))
  g = abi.BxMlpGrads()
  for l in range(len(layers)):
    g.dw[l], g.db[l] = outs[f'g{2 * l}'][1].data_ptr(), outs[f'g{2 * l + 1}'][1].data_ptr()
  _native.check(lib.bx_mlp_backward(
      C.byref(net), rows, x.data_ptr(), x.stride(0), outs['saved'][1].data_ptr() or None,
      dy.data_ptr(), outs['dx'][1].data_ptr(), C.byref(g), outs['work'][1].data_ptr(),
      C.byref(nbytes), stream))
  torch.cuda.synchronize()
  intact = all(_intact(buf, view.numel()) for buf, view in outs.values())
  return [outs['y'][1], outs['dx'][1]] + [outs[f'g{k}'][1] for k in range(len(params))], intact


@pytest.mark.parametrize('sizes', SIZES, ids=_ids)
def test_strided_input_and_guarded_outputs(dev, sizes):
  for rows in ROWS:
    layers, x, dy = _random_case(sizes, rows, seed=11, dev=dev)
    wide = torch.full((rows, sizes[0] + 9), float('nan'), device=dev)
    wide[:, 4:4 + sizes[0]] = x
    view = wide[:, 4:4 + sizes[0]]
    assert view.stride(0) == sizes[0] + 9 or rows == 1
    want = _run(layers, x, dy, 'tanh', True)
    got, intact = _raw(layers, view, dy, 'tanh', dev)
    assert intact, rows
    for name, g, w in zip(_names(layers), got, want):
      assert torch.equal(g, w), (rows, name)
    # the autograd function takes the view as it is
    for name, g, w in zip(_names(layers), _run(layers, view, dy, 'tanh', True), want):
      assert torch.equal(g, w), (rows, name, 'view')


@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_a_nan_row_stays_in_its_row(dev, activation):
  """y of the row is NaN under every activation. dx of the row is NaN where
  the activation's derivative carries the NaN (swish, tanh); relu's backward
  is a select on the pre-activation, which passes the finite gradient through
  in the chained form too, so there dx is compared with the chained pattern."""
  for sizes in ((33, 256, 256, 1), (35, 129, 1, 255, 4), (1024, 40, 3)):
    for rows, bad in ((33, 31), (130, 64)):
      layers, x, dy = _random_case(sizes, rows, seed=13, dev=dev)
      x[bad, sizes[0] // 2] = float('nan')
      y, dx = _run(layers, x, dy, activation, True)[:2]
      others = torch.arange(rows, device=dev) != bad
      assert not torch.isfinite(y[bad]).any() and torch.isfinite(y[others]).all()
      assert torch.isfinite(dx[others]).all()
      if activation == 'relu':
        assert torch.equal(torch.isnan(dx), torch.isnan(_run(layers, x, dy, activation, False)[1]))
      else:
        assert not torch.isfinite(dx[bad]).any()


@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_an_inf_weight_gives_the_chained_pattern(dev, activation):
  for sizes in ((7, 3, 2), (33, 256, 256, 1), (87, 32, 32, 32, 32, 16)):
    layers, x, dy = _random_case(sizes, 65, seed=17, dev=dev)
    with torch.no_grad():
      layers[0][0][2, 1] = float('inf')
    want = _run(layers, x, dy, activation, False)
    got = _run(layers, x, dy, activation, True)
    for name, g, w in zip(_names(layers), got, want):
      assert torch.equal(torch.isnan(g), torch.isnan(w)), (sizes, name)
      assert torch.equal(torch.isinf(g), torch.isinf(w)), (sizes, name)
      assert torch.equal(torch.isinf(g) & (g > 0), torch.isinf(w) & (w > 0)), (sizes, name)


# ---- 5. the gradient switches ---------------------------------------------------------------

def test_gradient_switches(dev):
  sizes, rows = (35, 129, 1, 255, 4), 65
  layers, x, dy = _random_case(sizes, rows, seed=19, dev=dev)
  full = _run(layers, x, dy, 'swish', True)
  lib = _native.lib()
  # only x: dx as before, no parameter gradient
  frozen = [(w.detach(), b.detach()) for w, b in layers]
  xg = x.clone().requires_grad_()
  y = fm.fused_mlp(frozen, xg, 'swish', fused=True)
  (y * dy).sum().backward()
  assert torch.equal(y, full[0]) and torch.equal(xg.grad, full[1])
  # only the parameters: no dx, the same gradients
  y = fm.fused_mlp(layers, x, 'swish', fused=True)
  grads = torch.autograd.grad((y * dy).sum(), networks.parameters(layers))
  for g, w in zip(grads, full[2:]):
    assert torch.equal(g, w)
  # one layer's parameters alone
  part = [(w.detach(), b.detach()) for w, b in layers]
  part[2] = layers[2]
  y = fm.fused_mlp(part, x, 'swish', fused=True)
  gw, gb = torch.autograd.grad((y * dy).sum(), part[2])
  assert torch.equal(gw, full[2 + 4]) and torch.equal(gb, full[2 + 5])
  # no graph: the same bits, nothing saved
  with torch.no_grad():
    y0 = fm.fused_mlp(layers, x, 'swish', fused=True)
  assert not y0.requires_grad and torch.equal(y0, full[0])
  # the entry point itself writes only what is asked for
  net = fm._net([t.detach() for wb in layers for t in wb], 'swish')
  hidden = sum(sizes[1:-1])
  saved = torch.empty((rows, hidden), device=dev)
  yy = torch.empty((rows, sizes[-1]), device=dev)
  _native.check(lib.bx_mlp_forward(C.byref(net), rows, x.data_ptr(), x.stride(0), yy.data_ptr(),
                                   saved.data_ptr(), None))
  buf, dw1 = _guarded((129, 1), dev)
  g = abi.BxMlpGrads()
  g.dw[1] = dw1.data_ptr()
  work = torch.empty((rows * hidden,), device=dev)
  nbytes = C.c_int64(work.numel() * 4)
  _native.check(lib.bx_mlp_backward(C.byref(net), rows, x.data_ptr(), x.stride(0), saved.data_ptr(),
                                    dy.data_ptr(), None, C.byref(g), work.data_ptr(),
                                    C.byref(nbytes), None))
  torch.cuda.synchronize()
  assert torch.equal(dw1, full[2 + 2]) and _intact(buf, 129)


def test_leading_dimensions_and_empty_batches(dev):
  layers, x, dy = _random_case((7, 3, 2), 24, seed=23, dev=dev)
  want = _run(layers, x, dy, 'relu', True)
  got = _run(layers, x.view(2, 3, 4, 7), dy.view(2, 3, 4, 2), 'relu', True)
  assert got[0].shape == (2, 3, 4, 2) and got[1].shape == (2, 3, 4, 7)
  for g, w in zip(got, want):
    assert torch.equal(g.reshape(w.shape), w)
  # a transposed batch (ppo_loss's time-first view) is copied, not refused
  xt = x.view(4, 6, 7).transpose(0, 1)
  assert torch.equal(fm.fused_mlp(layers, xt, 'relu', fused=True),
                     networks.mlp(layers, xt.contiguous(), 'relu', fused=True))
  empty = _run(layers, x[:0], dy[:0], 'relu', True)
  assert empty[0].shape == (0, 2) and all(not t.any() for t in empty[2:])


# ---- 6. graph capture -----------------------------------------------------------------------

def test_graph_capture_replays_the_eager_bits(dev):
  sizes, rows = (87, 32, 32, 32, 32, 16), 130
  layers, x, dy = _random_case(sizes, rows, seed=29, dev=dev)
  xs = x.clone().requires_grad_()
  params = networks.parameters(layers)

  def step():
    y = fm.fused_mlp(layers, xs, 'swish', fused=True)
    return [y.detach()] + list(torch.autograd.grad((y * dy).sum(), [xs] + params))
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
    for name, g, w in zip(_names(layers), outs, _run(layers, x, dy, 'swish', True)):
      assert torch.equal(g, w), name
    with torch.no_grad():  # an optimiser's in-place update
      for p in params:
        p.mul_(1.25).add_(0.01)


# ---- 7. the losses --------------------------------------------------------------------------

def _loss_held(run, params64, params32):
  """run(params, fused_mlp, dtype) -> (loss, metrics dict); the loss, every
  metric and every gradient of the fused form are held to `_held` with the
  float64 form as the reference and the chained float32 form as the yardstick."""
  def everything(params, fused_mlp, dtype):
    loss, metrics = run(params, fused_mlp, dtype)
    grads = torch.autograd.grad(loss, params)
    return ([('loss', loss.detach())] + [(k, v.detach()) for k, v in sorted(metrics.items())]
            + [(f'grad{k}', g) for k, g in enumerate(grads)])
  ref = everything(params64, False, torch.float64)
  yard = everything(params32, False, torch.float32)
  got = everything(params32, True, torch.float32)
  ratios = []
  for (name, g), (_, r), (_, y) in zip(got, ref, yard):
    _held(g, r, y, name, ratios)
  print('worst error ratio', max(ratios))


def test_ppo_loss_through_the_kernels(dev):
  from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
  from brax_amd.training.losses import Transition, ppo_loss
  B, T, O, A = 8, 3, 27, 8
  g = torch.Generator().manual_seed(31)
  policy, value = networks.make_ppo_networks(O, A, seed=5, device=dev)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  obs, raw = r(B, T, O), r(B, T, A)
  with torch.no_grad():
    loc, s = torch.chunk(networks.mlp(policy, obs), 2, dim=-1)
    log_prob = normal_tanh_log_prob(loc, head_scale(s, 1e-3), raw).sum(-1) + 0.1 * r(B, T)
  flags = lambda p: (torch.rand((B, T), generator=g) < p).float().to(dev)  # noqa: E731
  data = Transition(observation=obs, action=torch.tanh(raw), reward=r(B, T), discount=1 - flags(0.2),
                    next_observation=r(B, T, O), truncation=flags(0.2), raw_action=raw,
                    log_prob=log_prob)
  eps = r(B, T, A)
  mean_std = (r(O) * 0.1, 1 + 0.1 * torch.rand((O,), generator=g).to(dev))

  def run(params, fused_mlp, dtype):
    n = len(policy) * 2
    pl = list(zip(params[0:n:2], params[1:n:2]))
    vl = list(zip(params[n::2], params[n + 1::2]))
    return ppo_loss(pl, vl, tuple(t.to(dtype) for t in mean_std), data.map(lambda t: t.to(dtype)),
                    eps.to(dtype), fused=False, fused_mlp=fused_mlp)
  p32 = networks.parameters(policy, value)
  p64 = [p.detach().double().requires_grad_() for p in p32]
  _loss_held(run, p64, p32)


@pytest.mark.parametrize('which', ['critic', 'actor'])
def test_sac_losses_through_the_kernels(dev, which):
  from brax_amd.training import sac_losses
  from brax_amd.training.sac_networks import make_sac_networks, q_parameters
  B, O, A = 64, 27, 8
  g = torch.Generator().manual_seed(37)
  policy, q = make_sac_networks(O, A, hidden_layer_sizes=(256, 256), seed=3, device=dev)
  _, target = make_sac_networks(O, A, hidden_layer_sizes=(256, 256), seed=4, device=dev)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  flags = lambda p: (torch.rand((B, 1), generator=g) < p).float().to(dev)  # noqa: E731
  tr = {'observation': r(B, O), 'action': torch.tanh(r(B, A)), 'reward': r(B, 1),
        'discount': 1 - flags(0.2), 'next_observation': r(B, O), 'truncation': flags(0.2)}
  eps = r(B, A)
  alpha = torch.tensor(0.7, device=dev)

  def cast(layers, dtype):
    return [(w.detach().to(dtype), b.detach().to(dtype)) for w, b in layers]

  def pairs(params):
    return list(zip(params[0::2], params[1::2]))

  def run(params, fused_mlp, dtype):
    t = {k: v.to(dtype) for k, v in tr.items()}
    if which == 'critic':
      qs = [pairs(params[:len(params) // 2]), pairs(params[len(params) // 2:])]
      loss = sac_losses.critic_loss(qs, cast(policy, dtype), None, [cast(c, dtype) for c in target],
                                    alpha.to(dtype), t, eps.to(dtype), fused_mlp=fused_mlp)
    else:
      loss = sac_losses.actor_loss(pairs(params), None, [cast(c, dtype) for c in q],
                                   alpha.to(dtype), t, eps.to(dtype), fused_mlp=fused_mlp)
    return loss, {}
  p32 = q_parameters(q) if which == 'critic' else networks.parameters(policy)
  p64 = [p.detach().double().requires_grad_() for p in p32]
  _loss_held(run, p64, p32)


# ---- 8. end to end --------------------------------------------------------------------------

def _flat(params):
  return torch.cat([t.detach().reshape(-1) for layers in params for wb in layers for t in wb])


def test_ppo_train_end_to_end(dev):
  from brax_amd.training import ppo
  cfg = dict(num_envs=64, unroll_length=5, batch_size=32, num_minibatches=4,
             num_updates_per_batch=2, num_evals=2, normalize_observations=True)
  run = lambda **kw: ppo.train('inverted_pendulum', num_timesteps=1900, episode_length=50,  # noqa: E731
                               num_eval_envs=32, seed=1, device=dev, **cfg, **kw)
  _, params, metrics = run(fused_mlp=True)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  got = _flat(params[1:])
  assert torch.isfinite(got).all()
  init = _flat(networks.make_ppo_networks(params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2,
                                          seed=1, device=dev))
  assert got.shape == init.shape and not torch.equal(got, init)
  plain, off = _flat(run()[1][1:]), _flat(run(fused_mlp=False)[1][1:])
  assert torch.equal(plain.view(torch.int32), off.view(torch.int32))
  assert not torch.equal(plain, init)


def test_sac_train_end_to_end(dev):
  from brax_amd.training import sac
  from brax_amd.training.sac_networks import make_sac_networks
  run = lambda **kw: sac.train(  # noqa: E731
      'inverted_pendulum', num_timesteps=2000, episode_length=50, num_envs=16, num_eval_envs=32,
      batch_size=32, num_evals=3, min_replay_size=100, max_replay_size=512, grad_updates_per_step=1,
      normalize_observations=True, device=dev, **kw)
  _, params, metrics = run(fused_mlp=True)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  got = _flat(params[1:])
  assert torch.isfinite(got).all()
  policy = params[1]
  init = _flat([make_sac_networks(policy[0][0].shape[0], policy[-1][0].shape[1] // 2, seed=0,
                                  device=dev)[0]])
  assert got.shape == init.shape and not torch.equal(got, init)
  plain, off = _flat(run()[1][1:]), _flat(run(fused_mlp=False)[1][1:])
  assert torch.equal(plain.view(torch.int32), off.view(torch.int32))
