"""The fused PPO loss head (`bx_ppo_head`) on the GPU.

A scan workgroup holds 256 envs (4 waves) and walks the sequence in chunks of
8 steps; a row workgroup holds 256 (t, env) rows. So `(T, B, A)`: (1, 1, 1)
(one row: a zero standard deviation, where both forms give zero advantages),
(3, 63, 8) (below one wave; 189 rows in one row workgroup), (9, 65, 8) (T
crosses a scan chunk, B a wave; 585 rows in three row workgroups) and
(2, 130, 17) (A odd and above 16; 260 rows, four in the second workgroup).

Inputs as `test_ppo_loss_through_the_kernels` builds them: random logits and
baseline, raw actions, a behaviour log-prob 0.2 randn off the current one (so
rows clip on either side of the 0.3 interval), 0/1 discount and truncation
flags at p = 0.2. The accuracy rule is `tests/test_gpu_fused_mlp.py`'s `_held`,
restated: max |got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|), ref the
chained form in float64, yard the chained form in float32 on the GPU.

Worst ratios measured on an MI355X (the worst of loss, metrics, dlogits and
dbaseline over the shapes): see DESIGN.md, "PPO loss head".
"""
import math

import pytest
import torch

from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
from brax_amd.training import networks
from brax_amd.training import ppo_head as ph
from brax_amd.training.gae import compute_gae
from brax_amd.training.losses import Transition, ppo_loss

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (3, 63, 8), (9, 65, 8), (2, 130, 17))
# chosen on the CPU so that the float64 reference meets `_precondition` under
# every variant below
SEEDS = {(1, 1, 1): 2, (3, 63, 8): 1, (9, 65, 8): 1, (2, 130, 17): 1}
HYPER = dict(entropy_cost=1e-2, discounting=0.97, reward_scaling=0.5, gae_lambda=0.95,
             clipping_epsilon=0.3, min_std=1e-3, normalize_advantage=True)
VARIANTS = {'default': {}, 'raw_advantages': dict(normalize_advantage=False),
            'no_entropy': dict(entropy_cost=0.0)}
NAMES = ('loss',) + ph.METRICS[1:] + ('dlogits', 'dbaseline')
EPS = 2.0 ** -23
SENTINEL = 777.25
PAD = 64


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _ids(v):
  return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _case(shape, seed=None, device=None, batch_major=True):
  """(logits, baseline, bootstrap, data, eps), time first; with `batch_major`
  views of [B, T] arrays as `ppo_loss` passes them, else contiguous."""
  T, B, A = shape
  g = torch.Generator().manual_seed(SEEDS[shape] if seed is None else seed)
  r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
  flags = lambda p: (torch.rand((B, T), generator=g) < p).float()  # noqa: E731
  logits, baseline, boot, raw, eps = r(B, T, 2 * A), r(B, T), r(B), r(B, T, A), r(B, T, A)
  loc, s = torch.chunk(logits.double(), 2, dim=-1)
  log_prob = (normal_tanh_log_prob(loc, head_scale(s, HYPER['min_std']), raw.double()).sum(-1)
              + 0.2 * r(B, T).double()).float()
  data = Transition(observation=None, action=None, reward=r(B, T), discount=1 - flags(0.2),
                    next_observation=None, truncation=flags(0.2), raw_action=raw,
                    log_prob=log_prob)
  def lay(x):
    if x is None:
      return None
    x = x.to(device).transpose(0, 1)
    return x if batch_major else x.contiguous()
  return lay(logits), lay(baseline), boot.to(device), data.map(lay), lay(eps)


def _cast(case, dtype):
  logits, baseline, boot, data, eps = case
  c = lambda x: None if x is None else x.to(dtype)  # noqa: E731
  return c(logits), c(baseline), c(boot), data.map(c), c(eps)


def _run(case, fused, **hyper):
  """{name: tensor} of NAMES for one evaluation and its backward pass."""
  logits, baseline, boot, data, eps = case
  logits = logits.detach().clone().requires_grad_()
  baseline = baseline.detach().clone().requires_grad_()
  loss, metrics = ph.ppo_head(logits, baseline, boot, data, eps, fused=fused, fused_gae=False,
                              **{**HYPER, **hyper})
  assert sorted(metrics) == sorted(ph.METRICS) and metrics['total_loss'] is loss
  grads = torch.autograd.grad(loss, [logits, baseline])
  out = [loss.detach()] + [metrics[k].detach() for k in ph.METRICS[1:]] + list(grads)
  return dict(zip(NAMES, out))


def _precondition(case64, **hyper):
  """In float64: no row's rho within 1e-4 (relative) of a clip edge, no row
  outside the interval with |A^| < 1e-6; returns the rows clipped below and
  above. A kink of the surrogate cannot then pass for an accuracy failure.
  Without normalisation a truncated step's advantage is the product with
  mask = 0, an exact zero in every precision: such a row's term and gradient
  are exact zeros in every form, so it is no kink and is not counted."""
  h = {**HYPER, **hyper}
  logits, baseline, boot, data, _ = case64
  loc, s = torch.chunk(logits, 2, dim=-1)
  lp = normal_tanh_log_prob(loc, head_scale(s, h['min_std']), data.raw_action).sum(-1)
  _, adv = compute_gae(data.truncation, 1 - data.discount, data.reward, baseline, boot,
                       h['gae_lambda'], h['discounting'], h['reward_scaling'], fused=False)
  masked = torch.zeros_like(adv, dtype=torch.bool)
  if h['normalize_advantage']:
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
  else:
    masked = (data.truncation == 1) & (adv == 0)
  rho = torch.exp(lp - data.log_prob)
  lo, hi = 1 - h['clipping_epsilon'], 1 + h['clipping_epsilon']
  assert float(torch.minimum((rho / lo - 1).abs(), (rho / hi - 1).abs()).min()) > 1e-4
  outside = (rho < lo) | (rho > hi)
  assert not bool((outside & ~masked & (adv.abs() < 1e-6)).any())
  return int((rho < lo).sum()), int((rho > hi).sum())


def _held(got, ref, yard, what, ratios=None):
  """max |got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|)."""
  err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
  unit = max(float((yard.double() - ref).abs().max()) if ref.numel() else 0.0,
             EPS * (float(ref.abs().max()) if ref.numel() else 0.0))
  ratio = err / unit if unit else (0.0 if err == 0 else math.inf)
  if ratios is not None:
    ratios.append((ratio, what))
  assert ratio <= 8, (what, err, unit)


@pytest.fixture(scope='module')
def references(dev):
  """{(shape, variant): (ref float64, yard float32)}, computed once."""
  out = {}
  for shape in SHAPES:
    case = _case(shape, device=dev)
    for name, hyper in VARIANTS.items():
      out[shape, name] = (_run(_cast(case, torch.float64), False, **hyper),
                          _run(case, False, **hyper))
  return out


# ---- 1. the GAE outputs are bx_compute_gae's bits -------------------------------------------

@pytest.mark.parametrize('batch_major', [True, False])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_gae_outputs_are_compute_gaes_bits(dev, shape, batch_major):
  logits, baseline, boot, data, eps = _case(shape, device=dev, batch_major=batch_major)
  h = {k: v for k, v in HYPER.items()}
  T, B, _ = shape
  out = {}
  if batch_major:  # the outputs as [B, T] views too
    out = {k: torch.empty((B, T), device=dev).transpose(0, 1) for k in ('vs', 'advantages')}
  _, _, _, vs, adv = ph.head_call(logits, baseline, boot, data, eps, want_gae=True, out=out, **h)
  want = compute_gae(data.truncation, 1 - data.discount, data.reward, baseline, boot,
                     h['gae_lambda'], h['discounting'], h['reward_scaling'], fused=True)
  assert torch.equal(vs, want[0]) and torch.equal(adv, want[1])


# ---- 2. accuracy, against float64 and autograd ----------------------------------------------

@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_accuracy_against_float64(dev, references, shape, variant):
  hyper = VARIANTS[variant]
  case = _case(shape, device=dev)
  below, above = _precondition(_cast(_case(shape), torch.float64), **hyper)
  if shape[0] * shape[1] >= 100:
    assert below >= 1 and above >= 1, (below, above)
  ref, yard = references[shape, variant]
  got = _run(case, True, **hyper)
  ratios = []
  for name in NAMES:
    assert got[name].shape == ref[name].shape and got[name].dtype == torch.float32
    _held(got[name], ref[name], yard[name], name, ratios)
  if shape == (1, 1, 1) and {**HYPER, **hyper}['normalize_advantage']:
    # a zero standard deviation: zero advantages in both forms
    assert float(got['policy_loss']) == 0 and float(yard['policy_loss']) == 0
  print('worst error ratio', _ids(shape), variant, max(ratios), 'clipped', below, above)


# ---- 3. determinism -------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_two_runs_give_the_same_bits(dev, shape):
  case = _case(shape, device=dev)
  a = ph.head_call(*case, want_gae=True, **HYPER)
  b = ph.head_call(*case, want_gae=True, **HYPER)
  for x, y in zip(a, b):
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- 4. guards ------------------------------------------------------------------------------

def _embedded(t):
  """`t` as a view of a wider NaN-filled buffer (same values, same shape)."""
  if t.dim() == 1:
    wide = torch.full((t.shape[0] + 9,), float('nan'), device=t.device)
    wide[4:4 + t.shape[0]] = t
    return wide[4:4 + t.shape[0]]
  wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 7,), float('nan'), device=t.device)
  wide[..., 3:3 + t.shape[-1]] = t
  return wide[..., 3:3 + t.shape[-1]]


def _guarded(shape, dev):
  n = math.prod(shape)
  buf = torch.full((n + 2 * PAD,), SENTINEL, device=dev)
  return buf, buf[PAD:PAD + n].view(shape)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_nothing_is_written_outside_the_outputs(dev, shape):
  T, B, A = shape
  logits, baseline, boot, data, eps = _case(shape, device=dev)
  want = ph.head_call(logits, baseline, boot, data, eps, want_gae=True, **HYPER)
  e = lambda x: None if x is None else _embedded(x)  # noqa: E731
  shapes = dict(losses=(4,), dlogits=(T, B, 2 * A), dbaseline=(T, B), vs=(T, B), advantages=(T, B))
  bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
  ws_buf, ws = _guarded((ph.workspace_floats(T, B),), dev)
  assert ws.data_ptr() % 16 == 0
  got = ph.head_call(e(logits), e(baseline), e(boot), data.map(e), e(eps), want_gae=True,
                     out={k: v[1] for k, v in bufs.items()}, workspace=ws, **HYPER)
  for g, w in zip(got, want):
    assert torch.equal(g.view(torch.int32), w.view(torch.int32))
  for name, (buf, view) in list(bufs.items()) + [('workspace', (ws_buf, ws))]:
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + view.numel():] == SENTINEL).all()), name


# ---- 5. NaN ---------------------------------------------------------------------------------

@pytest.mark.parametrize('normalize_advantage', [True, False])
def test_a_nan_reward_stays_in_its_envs_dbaseline(dev, normalize_advantage):
  shape = (9, 65, 8)
  logits, baseline, boot, data, eps = _case(shape, device=dev, batch_major=False)
  reward = data.reward.clone()
  reward[5, 17] = float('nan')
  data = Transition(**{**vars(data), 'reward': reward})
  case = (logits, baseline, boot, data, eps)
  got = _run(case, True, normalize_advantage=normalize_advantage)
  yard = _run(case, False, normalize_advantage=normalize_advantage)
  assert not math.isfinite(float(got['loss'])) and not math.isfinite(float(yard['loss']))
  finite = torch.isfinite(got['dbaseline'])
  assert torch.equal(finite, torch.isfinite(yard['dbaseline']))
  assert not finite[:6, 17].any() and finite[6:, 17].all() and finite[:, :17].all()


# ---- 6. autograd plumbing -------------------------------------------------------------------

def test_ppo_loss_through_both_kernels(dev):
  """`loss.backward()` through fused_mlp + fused_head on Ant-sized networks
  against the chained gradients, every parameter to the same bound."""
  B, T, O, A = 8, 3, 87, 8
  g = torch.Generator().manual_seed(41)
  policy, value = networks.make_ppo_networks(O, A, seed=5, device=dev)
  r = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
  obs, raw = r(B, T, O), r(B, T, A)
  with torch.no_grad():
    loc, s = torch.chunk(networks.mlp(policy, obs), 2, dim=-1)
    log_prob = normal_tanh_log_prob(loc, head_scale(s, 1e-3), raw).sum(-1) + 0.2 * r(B, T)
  flags = lambda p: (torch.rand((B, T), generator=g) < p).float().to(dev)  # noqa: E731
  data = Transition(observation=obs, action=torch.tanh(raw), reward=r(B, T), discount=1 - flags(0.2),
                    next_observation=r(B, T, O), truncation=flags(0.2), raw_action=raw,
                    log_prob=log_prob)
  eps = r(B, T, A)
  n = len(policy) * 2

  def everything(params, fused, dtype, scale=1.0):
    pl, vl = list(zip(params[0:n:2], params[1:n:2])), list(zip(params[n::2], params[n + 1::2]))
    loss, metrics = ppo_loss(pl, vl, None, data.map(lambda t: t.to(dtype)), eps.to(dtype),
                             fused=False, fused_mlp=fused, fused_head=fused, entropy_cost=1e-2)
    grads = torch.autograd.grad(scale * loss, params)
    return ([('loss', loss.detach())] + [(k, v.detach()) for k, v in sorted(metrics.items())]
            + [(f'grad{k}', g_) for k, g_ in enumerate(grads)])
  p32 = networks.parameters(policy, value)
  p64 = [p.detach().double().requires_grad_() for p in p32]
  ref, yard, got = everything(p64, False, torch.float64), everything(p32, False, torch.float32), \
      everything(p32, True, torch.float32)
  ratios = []
  for (name, g_), (_, r_), (_, y_) in zip(got, ref, yard):
    _held(g_, r_, y_, name, ratios)
  print('worst error ratio', max(ratios))
  # an upstream factor of 2.5 gives 2.5 times the gradients: the scaled run is
  # held to the scaled reference by the same rule
  scaled = everything(p32, True, torch.float32, scale=2.5)
  for (name, g_), (_, r_), (_, y_) in zip(scaled[5:], ref[5:], yard[5:]):
    _held(g_, 2.5 * r_, 2.5 * y_, name + ' x 2.5')
  assert not torch.equal(scaled[5][1], got[5][1])


def test_fused_true_refuses_what_the_kernel_does_not_take(dev):
  logits, baseline, boot, data, eps = _cast(_case((3, 63, 8), device=dev), torch.float64)
  with pytest.raises(NotImplementedError, match='float64 is not float32'):
    ph.ppo_head(logits, baseline, boot, data, eps, fused=True)
  loss, _ = ph.ppo_head(logits, baseline, boot, data, eps, fused=None)
  assert loss.dtype == torch.float64


# ---- 7. end to end --------------------------------------------------------------------------

def _flat(params):
  return torch.cat([t.detach().reshape(-1) for layers in params for wb in layers for t in wb])


def test_ppo_train_end_to_end(dev):
  from brax_amd.training import ppo
  _, params, metrics = ppo.train(
      'inverted_pendulum', num_timesteps=1900, episode_length=50, num_eval_envs=32, seed=1,
      device=dev, num_envs=64, unroll_length=5, batch_size=32, num_minibatches=4,
      num_updates_per_batch=2, num_evals=2, normalize_observations=True, fused_mlp=True,
      fused_head=True)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  assert {f'training/{k}' for k in ph.METRICS} <= set(metrics)
  got = _flat(params[1:])
  assert torch.isfinite(got).all()
  init = _flat(networks.make_ppo_networks(params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2,
                                          seed=1, device=dev))
  assert got.shape == init.shape and not torch.equal(got, init)
