"""The fused SAC loss heads (`bx_sac_head_*`) on the GPU.

A workgroup holds 256 rows (4 waves), a row per lane; the losses launch leaves
one partial per workgroup and the sample_backward launch's last workgroup sums
them, lane-strided (a second stride from 256 workgroups = 65,281 rows on, the
same loop). So `(B, O, A, C)`: (1, 3, 1, 2) (one row), (63, 11, 8, 2) (below a
wave), (65, 11, 8, 1) (crosses a wave, single critic), (260, 27, 17, 3) (four
rows in a second workgroup, A odd and above 16), (513, 5, 2, 2) (three
workgroups of partials).

Inputs: randn tensors, 0/1 discount and truncation at p = 0.2, log_alpha =
-0.7, reward_scaling 30, discounting 0.997, a normaliser with std in [0.5, 2].
The accuracy rule is `tests/test_gpu_ppo_head.py`'s `_held`, restated: max
|got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|), ref the chained form
in float64, yard the chained form in float32 on the GPU. Precondition, in
float64: every row's two smallest q_pi and two smallest next_q differ by more
than 1e-4 relative, so the min's kink cannot pass for an accuracy failure.

Worst ratios measured on an MI355X: see DESIGN.md, "SAC loss heads".
"""
import functools
import math

import pytest
import torch

from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
from brax_amd.training import sac, sac_head, sac_losses, sac_networks
from brax_amd.training.losses import normalize
from brax_amd.training.networks import parameters

pytestmark = pytest.mark.gpu

SHAPES = ((1, 3, 1, 2), (63, 11, 8, 2), (65, 11, 8, 1), (260, 27, 17, 3), (513, 5, 2, 2))
# chosen on the CPU so that the float64 reference meets `_precondition`
SEEDS = {(1, 3, 1, 2): 0, (63, 11, 8, 2): 0, (65, 11, 8, 1): 0, (260, 27, 17, 3): 0,
         (513, 5, 2, 2): 0}
STEP_SHAPE, STEP_SEED = (65, 11, 8, 2), 0
SCALING, DISCOUNTING, LOG_ALPHA = 30.0, 0.997, -0.7
EPS = 2.0 ** -23
SENTINEL = 777.25
PAD = 64


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _ids(v):
  return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _case(shape, seed=None, device=None, dtype=torch.float32):
  """Everything the four calls read, as a dict; the draws come from a CPU
  generator (the same values on every device)."""
  B, O, A, C = shape
  g = torch.Generator().manual_seed(SEEDS[shape] if seed is None else seed)
  r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
  flags = lambda p: (torch.rand((B,), generator=g) < p).float()  # noqa: E731
  case = dict(
      obs=r(B, O), next_obs=r(B, O), action=torch.tanh(r(B, A)), reward=r(B),
      discount=1 - flags(0.2), truncation=flags(0.2), mean=r(O),
      std=0.5 + 1.5 * torch.rand((O,), generator=g), logits=[r(B, 2 * A) for _ in range(2)],
      eps=[r(B, A) for _ in range(3)], lps=[r(B) - A for _ in range(3)],
      q_old=[r(B) for _ in range(C)], next_q=[r(B) for _ in range(C)],
      q_pi=[r(B) for _ in range(C)], da=[r(B, A) for _ in range(C)], g=r(B),
      log_alpha=torch.tensor(LOG_ALPHA))
  to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
  return {k: [to(t) for t in v] if isinstance(v, list) else to(v) for k, v in case.items()}


def _two_smallest_apart(qs):
  """qs: C (B,) float64 tensors; every row's two smallest differ by more than
  1e-4 relative (nothing to ask of one critic)."""
  if len(qs) < 2:
    return True
  low = torch.stack(qs, -1).sort(-1).values[:, :2]
  return bool(((low[:, 1] - low[:, 0]) > 1e-4 * low.abs().max(-1).values).all())


def _precondition(case64):
  assert _two_smallest_apart(case64['q_pi']) and _two_smallest_apart(case64['next_q'])


def _held(got, ref, yard, what, ratios=None):
  """max |got - ref| <= 8 max(max |yard - ref|, 2^-23 max |ref|)."""
  assert got.shape == ref.shape and got.dtype == torch.float32, what
  err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
  unit = max(float((yard.double() - ref).abs().max()) if ref.numel() else 0.0,
             EPS * (float(ref.abs().max()) if ref.numel() else 0.0))
  ratio = err / unit if unit else (0.0 if err == 0 else math.inf)
  if ratios is not None:
    ratios.append((ratio, what))
  assert ratio <= 8, (what, err, unit)


# ---- the chained forms (dtype-generic: float64 is ref, float32 on the GPU is yard) ------------

def _jobs(case):
  """(logits, eps) of the alpha, critic and actor jobs."""
  cur, nxt = case['logits']
  return [(cur, case['eps'][0]), (nxt, case['eps'][1]), (cur, case['eps'][2])]


def _sample_chained(logits, eps):
  loc, s = torch.chunk(logits, 2, dim=-1)
  scale = head_scale(s, sac_losses.MIN_STD)
  raw = loc + scale * eps
  return torch.tanh(raw), normal_tanh_log_prob(loc, scale, raw).sum(-1)


def _losses_chained(case):
  """`sac_losses`' three losses from the networks' outputs on, and autograd's
  gradients of them."""
  B, C = case['reward'].shape[0], len(case['q_old'])
  A = case['eps'][0].shape[1]
  lp_alpha, lp_next, lp_pi = case['lps']
  log_alpha = case['log_alpha'].clone().requires_grad_()
  q_old = torch.stack(case['q_old'], -1).requires_grad_()
  q_pi = torch.stack(case['q_pi'], -1).requires_grad_()
  lp_pi = lp_pi.clone().requires_grad_()
  a_loss = torch.mean(torch.exp(log_alpha) * (-lp_alpha - sac_losses.target_entropy(A)).detach())
  alpha = torch.exp(log_alpha.detach())
  next_v = torch.min(torch.stack(case['next_q'], -1), dim=-1).values - alpha * lp_next
  target_q = (case['reward'] * SCALING + case['discount'] * DISCOUNTING * next_v).detach()
  q_error = (q_old - target_q.unsqueeze(-1)) * (1 - case['truncation']).unsqueeze(-1)
  c_loss = 0.5 * torch.mean(torch.square(q_error))
  p_loss = torch.mean(alpha * lp_pi - torch.min(q_pi, dim=-1).values)
  dq_old, = torch.autograd.grad(c_loss, q_old)
  dq_pi, g_lp = torch.autograd.grad(p_loss, [q_pi, lp_pi])
  dlog_alpha, = torch.autograd.grad(a_loss, log_alpha)
  assert dq_old.shape == (B, C)
  return dict(losses=torch.stack([c_loss, p_loss, a_loss]).detach(), dq_old=dq_old, dq_pi=dq_pi,
              g_lp=g_lp, dlog_alpha=dlog_alpha)


def _backward_chained(case):
  logits = case['logits'][0].clone().requires_grad_()
  loc, s = torch.chunk(logits, 2, dim=-1)
  scale = head_scale(s, sac_losses.MIN_STD)
  raw = loc + scale * case['eps'][2]
  lp = normal_tanh_log_prob(loc, scale, raw).sum(-1)
  th = torch.tanh(raw)
  return torch.autograd.grad((case['g'] * lp).sum() + sum((d * th).sum() for d in case['da']),
                             logits)[0]


# ---- the calls --------------------------------------------------------------------------------

def _new(dev, *shape):
  return torch.full(shape, SENTINEL, device=dev)


def _run_prep(case, normalizer=True, out=None):
  B, O = case['obs'].shape
  A = case['action'].shape[1]
  dev = case['obs'].device
  xs = out or [_new(dev, B, O + A) for _ in range(3)]
  sac_head.prep_call(case['obs'], case['next_obs'], case['action'],
                     (case['mean'], case['std']) if normalizer else None, *xs)
  return xs


def _run_sample(case, out=None):
  """The three jobs; the critic's and the actor's actions land in the action
  columns of two (B, O + A) buffers. Returns (x_next, x_pi, [lp] * 3)."""
  B, O = case['obs'].shape
  A = case['action'].shape[1]
  dev = case['obs'].device
  x_next, x_pi, lps = out or (_new(dev, B, O + A), _new(dev, B, O + A), [_new(dev, B) for _ in range(3)])
  jobs = _jobs(case)
  sac_head.sample_call([(*jobs[0], None, lps[0]), (*jobs[1], x_next[:, O:], lps[1]),
                        (*jobs[2], x_pi[:, O:], lps[2])])
  return x_next, x_pi, lps


def _run_losses(case, out=None, workspace=None):
  """`losses`, then `sample_backward` on the same workspace for the sums."""
  B, C = case['reward'].shape[0], len(case['q_old'])
  A = case['eps'][0].shape[1]
  dev = case['reward'].device
  o = out or dict(dq_old=[_new(dev, B) for _ in range(C)], dq_pi=[_new(dev, B) for _ in range(C)],
                  g_lp=_new(dev, B), losses=_new(dev, 3), dlog_alpha=_new(dev),
                  dlogits=_new(dev, B, 2 * A))
  ws = _new(dev, max(sac_head.workspace_floats(B), 4)) if workspace is None else workspace
  sac_head.losses_call(case['lps'], case['q_old'], case['next_q'], case['q_pi'], case['reward'],
                       case['discount'], case['truncation'], case['log_alpha'], SCALING,
                       DISCOUNTING, sac_losses.target_entropy(A), o['dq_old'], o['dq_pi'],
                       o['g_lp'], ws)
  sac_head.sample_backward_call(case['logits'][0], case['eps'][2], o['g_lp'], case['da'],
                                o['dlogits'], o['losses'], o['dlog_alpha'], ws)
  return dict(losses=o['losses'], dq_old=torch.stack(o['dq_old'], -1),
              dq_pi=torch.stack(o['dq_pi'], -1), g_lp=o['g_lp'], dlog_alpha=o['dlog_alpha'])


def _run_backward(case, dlogits=None, workspace=None):
  B, A = case['eps'][0].shape
  dev = case['reward'].device
  dlogits = _new(dev, B, 2 * A) if dlogits is None else dlogits
  ws = torch.zeros(max(sac_head.workspace_floats(B), 4), device=dev) if workspace is None else workspace
  sac_head.sample_backward_call(case['logits'][0], case['eps'][2], case['g'], case['da'], dlogits,
                                _new(dev, 3), _new(dev), ws)
  return dlogits


@pytest.fixture(scope='module')
def references(dev):
  """{shape: {name: (ref float64, yard float32)}}, computed once."""
  out = {}
  for shape in SHAPES:
    c32, c64 = _case(shape, device=dev), _case(shape, device=dev, dtype=torch.float64)
    _precondition(c64)
    both = lambda fn: (fn(c64), fn(c32))  # noqa: E731
    ref = {'losses': both(_losses_chained), 'backward': both(_backward_chained)}
    for k, (lg, ep) in enumerate(_jobs(c64)):
      ref['sample', k] = (_sample_chained(lg, ep), _sample_chained(*_jobs(c32)[k]))
    out[shape] = ref
  return out


def test_the_seeds_meet_the_precondition():
  for shape in SHAPES:
    _precondition(_case(shape, dtype=torch.float64))


# ---- 1. prep ------------------------------------------------------------------------------------

@pytest.mark.parametrize('normalizer', [True, False])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_prep_is_the_chained_bits(dev, shape, normalizer):
  case = _case(shape, device=dev)
  O = shape[1]
  x_cur, x_next, x_pi = _run_prep(case, normalizer)
  n = (case['mean'], case['std']) if normalizer else None
  obs, next_obs = normalize(case['obs'], n), normalize(case['next_obs'], n)
  bits = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731
  assert bits(x_cur, torch.cat([obs, case['action']], dim=-1))
  assert bits(x_pi[:, :O], obs) and bits(x_next[:, :O], next_obs)
  assert bool((x_pi[:, O:] == SENTINEL).all()) and bool((x_next[:, O:] == SENTINEL).all())


# ---- 2. sample ----------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_sample_against_float64(dev, references, shape):
  case = _case(shape, device=dev)
  O = shape[1]
  x_next, x_pi, lps = _run_sample(case)
  ratios = []
  for k, action in enumerate((None, x_next[:, O:], x_pi[:, O:])):
    (ref_a, ref_lp), (yard_a, yard_lp) = references[shape]['sample', k]
    _held(lps[k], ref_lp, yard_lp, f'log_prob {k}', ratios)
    if action is not None:
      _held(action, ref_a, yard_a, f'action {k}', ratios)
  # the actions land in the action columns and nowhere else in the row
  assert bool((x_pi[:, :O] == SENTINEL).all()) and bool((x_next[:, :O] == SENTINEL).all())
  assert not bool((x_pi[:, O:] == SENTINEL).any())
  print('worst error ratio, sample', _ids(shape), max(ratios))


# ---- 3. losses ----------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_losses_against_float64(dev, references, shape):
  case = _case(shape, device=dev)
  ref, yard = references[shape]['losses']
  got = _run_losses(case)
  ratios = []
  for name in ('losses', 'dq_old', 'dq_pi', 'dlog_alpha', 'g_lp'):
    _held(got[name], ref[name], yard[name], name, ratios)
  for k, name in enumerate(('critic', 'actor', 'alpha')):
    _held(got['losses'][k], ref['losses'][k], yard['losses'][k], name)
  print('worst error ratio, losses', _ids(shape), max(ratios))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_every_row_truncated_is_exact_zeros(dev, shape):
  case = _case(shape, device=dev)
  case['truncation'] = torch.ones_like(case['truncation'])
  got, yard = _run_losses(case), _losses_chained(case)
  for form in (got, yard):
    assert float(form['losses'][0]) == 0 and bool((form['dq_old'] == 0).all())
  assert float(got['losses'][1]) != 0 and float(got['losses'][2]) != 0


# ---- 4. sample_backward -------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_sample_backward_against_float64(dev, references, shape):
  case = _case(shape, device=dev)
  ref, yard = references[shape]['backward']
  ratios = []
  _held(_run_backward(case), ref, yard, 'dlogits', ratios)
  print('worst error ratio, sample_backward', _ids(shape), max(ratios))


# ---- 5. the whole step's gradients ------------------------------------------------------------

def _step_case(dev, dtype=torch.float32, seed=STEP_SEED, fused_adam=False):
  """A training state with (32, 32) networks, non-zero biases, targets off the
  critics and log_alpha = -0.7, and a minibatch at STEP_SHAPE."""
  B, O, A, C = STEP_SHAPE
  factory = functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=(32, 32),
                              n_critics=C)
  ts = sac.init_training_state(O, A, 1e-2, factory, seed + 1, device=dev, dtype=dtype,
                               fused_adam=fused_adam)
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(s, generator=g).to(device=dev, dtype=dtype)  # noqa: E731
  with torch.no_grad():
    for t in parameters(ts.policy_layers, *ts.q_layers):
      if t.dim() == 1:
        t.copy_(0.1 * r(*t.shape))
    for t in parameters(*ts.target_q_layers):
      t.add_(0.05 * r(*t.shape))
    ts.log_alpha.fill_(LOG_ALPHA)
  flags = lambda p: (torch.rand((B,), generator=g) < p).to(device=dev, dtype=dtype)  # noqa: E731
  trans = {'observation': r(B, O), 'action': torch.tanh(r(B, A)), 'reward': r(B),
           'discount': 1 - flags(0.2), 'next_observation': r(B, O), 'truncation': flags(0.2)}
  normalizer = (r(O), 0.5 + 1.5 * torch.rand((O,), generator=g).to(device=dev, dtype=dtype))
  return ts, normalizer, trans, (r(B, A), r(B, A), r(B, A))


def _step_precondition(ts, normalizer, trans, eps):
  with torch.no_grad():
    obs, nxt = normalize(trans['observation'], normalizer), normalize(trans['next_observation'], normalizer)
    q_pi = sac_networks.q_apply(ts.q_layers, obs, torch.tanh(sac_losses._sample(ts.policy_layers, obs, eps[2])[0]))
    next_q = sac_networks.q_apply(ts.target_q_layers, nxt,
                                  torch.tanh(sac_losses._sample(ts.policy_layers, nxt, eps[1])[0]))
  assert _two_smallest_apart(list(q_pi.unbind(-1))) and _two_smallest_apart(list(next_q.unbind(-1)))


def test_the_step_seed_meets_the_precondition():
  _step_precondition(*_step_case(None, torch.float64))


@pytest.fixture(scope='module')
def step_references(dev):
  def chained(dtype):
    ts, normalizer, trans, eps = _step_case(dev, dtype)
    a, c, p, m = sac._chained_gradients(ts, normalizer, trans, eps, SCALING, DISCOUNTING, False)
    return [*a, *c, *p] + [m[k] for k in sac_head.METRICS]
  _step_precondition(*_step_case(dev, torch.float64))
  return chained(torch.float64), chained(torch.float32)


@pytest.mark.parametrize('fused_mlp', [True, False])
def test_gradients_against_the_chained_float64_step(dev, step_references, fused_mlp):
  ref, yard = step_references
  ts, normalizer, trans, eps = _step_case(dev)
  a, c, p, m = sac_head.gradients(ts, normalizer, trans, eps, SCALING, DISCOUNTING, fused_mlp)
  got = [*a, *c, *p] + [m[k] for k in sac_head.METRICS]
  assert len(got) == len(ref) == 1 + 12 + 6 + 3
  assert torch.equal(m.vector, torch.stack([m[k] for k in sac_head.METRICS]))
  ratios = []
  for k, (g, r, y) in enumerate(zip(got, ref, yard)):
    _held(g, r, y, f'tensor {k}', ratios)
  print('worst error ratio, gradients, fused_mlp', fused_mlp, max(ratios))


def test_a_fused_step_updates_everything(dev):
  tau = 0.25
  ts, normalizer, trans, eps = _step_case(dev)
  q, target, rest = (parameters(*ts.q_layers), parameters(*ts.target_q_layers),
                     [ts.log_alpha] + parameters(ts.policy_layers))
  old = [t.detach().clone() for t in q + rest]
  old_target = [t.detach().clone() for t in target]
  m = sac.sgd_step(ts, normalizer, trans, eps, SCALING, DISCOUNTING, tau, fused_mlp=True,
                   fused_head=True)
  assert list(m) == ['critic_loss', 'actor_loss', 'alpha_loss', 'alpha']
  assert float(m['alpha']) == float(torch.exp(ts.log_alpha.detach())) != math.exp(LOG_ALPHA)
  for t, o in zip(q + rest, old):
    assert bool(torch.isfinite(t).all()) and not torch.equal(t.detach(), o)
  for t, o, qn in zip(target, old_target, q):
    assert torch.equal(t, o * (1 - tau) + qn.detach() * tau)


# ---- 6. determinism -----------------------------------------------------------------------------

def _everything(case, **kw):
  """Every output of the four calls, flat."""
  x_next, x_pi, lps = _run_sample(case, kw.get('sample'))
  losses = _run_losses(case, kw.get('losses'), kw.get('workspace'))
  return ([*_run_prep(case, out=kw.get('prep')), x_next, x_pi, *lps] + list(losses.values())
          + [_run_backward(case, kw.get('dlogits'), kw.get('workspace'))])


def _same_bits(a, b):
  return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_two_runs_give_the_same_bits(dev, shape):
  case = _case(shape, device=dev)
  for x, y in zip(_everything(case), _everything(case)):
    assert _same_bits(x, y)


# ---- 7. guards ----------------------------------------------------------------------------------

def _embedded(t):
  """`t` as a view of a wider NaN-filled buffer (same values, same shape)."""
  if t.dim() == 0:
    return t
  if t.dim() == 1:
    wide = torch.full((t.shape[0] + 9,), float('nan'), device=t.device)
    wide[4:4 + t.shape[0]] = t
    return wide[4:4 + t.shape[0]]
  wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 7,), float('nan'), device=t.device)
  wide[..., 3:3 + t.shape[-1]] = t
  return wide[..., 3:3 + t.shape[-1]]


def _guarded(shape, dev, bufs):
  n = math.prod(shape)
  buf = torch.full((n + 2 * PAD,), SENTINEL, device=dev)
  bufs.append((buf, n))
  return buf[PAD:PAD + n].view(shape)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_nothing_is_written_outside_the_outputs(dev, shape):
  B, O, A, C = shape
  case = _case(shape, device=dev)
  want = _everything(case)
  # the (B,) arrays the losses launch reads with a stride of one stay contiguous
  # where the entry point has no stride for them; the rest sit in NaN
  wide = {k: [_embedded(t) for t in v] if isinstance(v, list) else _embedded(v)
          for k, v in case.items() if k not in ('lps', 'q_old', 'next_q', 'q_pi', 'g', 'mean', 'std')}
  wide = {**case, **wide}
  bufs = []
  G = lambda *s: _guarded(s, dev, bufs)  # noqa: E731
  ws = G(max(sac_head.workspace_floats(B), 4))
  assert ws.data_ptr() % 16 == 0
  got = _everything(
      wide, prep=[G(B, O + A) for _ in range(3)],
      sample=(G(B, O + A), G(B, O + A), [G(B) for _ in range(3)]),
      losses=dict(dq_old=[G(B) for _ in range(C)], dq_pi=[G(B) for _ in range(C)], g_lp=G(B),
                  losses=G(3), dlog_alpha=G(), dlogits=G(B, 2 * A)),
      dlogits=G(B, 2 * A), workspace=ws)
  for g, w in zip(got, want):
    assert _same_bits(g, w)
  for buf, n in bufs:
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


# ---- 8. NaN -------------------------------------------------------------------------------------

def test_a_nan_reward_stays_in_its_row(dev):
  shape = (65, 11, 8, 1)
  for C in (1, 2):
    case = _case((65, 11, 8, C), seed=SEEDS[shape], device=dev)
    case['reward'][17] = float('nan')
    got, yard = _run_losses(case), _losses_chained(case)
    for form in (got, yard):
      assert not math.isfinite(float(form['losses'][0]))
      assert math.isfinite(float(form['losses'][1])) and math.isfinite(float(form['losses'][2]))
    finite = torch.isfinite(got['dq_old'])
    assert torch.equal(finite, torch.isfinite(yard['dq_old']))
    assert not finite[17].any() and int((~finite).sum()) == C
    assert bool(torch.isfinite(got['dq_pi']).all()) and bool(torch.isfinite(got['g_lp']).all())


# ---- 9. the switch ------------------------------------------------------------------------------

def test_fused_true_refuses_what_the_kernels_do_not_take(dev):
  ts, normalizer, trans, eps = _step_case(dev, torch.float64)
  with pytest.raises(NotImplementedError, match='float64 is not float32'):
    sac.sgd_step(ts, normalizer, trans, eps, fused_head=True)
  m = sac.sgd_step(ts, normalizer, trans, eps, fused_head=None)
  assert m['critic_loss'].dtype == torch.float64 and ts.gradient_steps == 1


# ---- 10. end to end -----------------------------------------------------------------------------

def test_sac_train_end_to_end(dev):
  factory = functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=(32, 32))
  _, params, metrics = sac.train(
      'inverted_pendulum', num_timesteps=2000, episode_length=50, num_envs=16, num_eval_envs=16,
      batch_size=32, grad_updates_per_step=2, min_replay_size=64, num_evals=2, seed=1, device=dev,
      normalize_observations=True, network_factory=factory, fused_mlp=True, fused_adam=True,
      fused_head=True)
  for k, v in metrics.items():
    assert math.isfinite(float(v)), k
  assert {f'training/{k}' for k in sac_head.METRICS + ('alpha',)} <= set(metrics)
  got = torch.cat([t.detach().reshape(-1) for t in parameters(params[1])])
  init = torch.cat([t.detach().reshape(-1) for t in parameters(
      factory(params[1][0][0].shape[0], params[1][-1][0].shape[1] // 2, seed=1, device=dev)[0])])
  assert bool(torch.isfinite(got).all()) and got.shape == init.shape and not torch.equal(got, init)
