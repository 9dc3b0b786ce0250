"""The evolution trainers on the device (`brax_amd.training.es` / `ars`,
`bx_population_perturb`, `bx_population_delta`). Needs an MI355X.

`perturb_` is compared bit for bit with its torch expression (`fused=False`)
over `bx_normal_slabs`' noise. `weighted_noise_sum` is compared with the
float64 chained form r_j = sum_p w_p eps_pj under

    |got - r_j| <= 2^-23 |r_j| + P 2^-50 sum_p |w_p eps_pj|

the first term one float32 rounding of the sum, the second the float64
reassociation of P terms (each partial sum is within P 2^-53 of relative error
of the absolute sum, in either order). One epoch of each learner is checked
against a direct `population_rollout` with the same keys and numpy
restatements of the reference's optimiser halves.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SHAPES = {18: (5, 3), 323: (14, 12, 11)}  # n_params: layer widths
CHUNK = 64


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _policy(dev, n_params, seed=5):
  from brax_amd.envs.policy import MLPPolicy
  sizes = SHAPES[n_params]
  g = torch.Generator(device='cpu').manual_seed(seed)
  layers = [(torch.randn((i, o), generator=g), torch.randn((o,), generator=g))
            for i, o in zip(sizes[:-1], sizes[1:])]
  pol = MLPPolicy(layers, activation='relu', head='identity', device=dev)
  assert pol.params.numel() == n_params
  return pol


def _bias_mask(pol):
  """The last layer's bias."""
  m = torch.zeros(pol.params.numel(), dtype=torch.bool, device=pol.params.device)
  m[-pol.sizes[-1][1]:] = True
  return m


def _bits(x):
  return x.detach().contiguous().view(torch.int32).cpu()


def _sentinel_population(pol, n_members):
  from brax_amd.envs.population import PolicyPopulation
  pop = PolicyPopulation(pol, n_members)
  pop.rows.fill_(SENTINEL)
  return pop


# ---- perturb --------------------------------------------------------------------------------

def test_the_chunk_is_the_librarys():
  from brax_amd import abi
  assert abi.POPULATION_DELTA_CHUNK == CHUNK


@pytest.mark.parametrize('offset', [0, 2 ** 32 - 6])
@pytest.mark.parametrize('n_members,antithetic', [(2, True), (6, True), (5, False)])
@pytest.mark.parametrize('n_params', [18, 323])
def test_perturb_equals_the_torch_expression(dev, n_params, n_members, antithetic, offset):
  pol = _policy(dev, n_params)
  for frozen in (None, _bias_mask(pol)):
    for sigma in (0.1, -0.25, 0.0):
      a = _sentinel_population(pol, n_members)
      b = _sentinel_population(pol, n_members)
      assert a.stride > n_params  # there is padding to keep
      a.perturb_(sigma, 7, offset, antithetic, frozen=frozen, fused=True)
      b.perturb_(sigma, 7, offset, antithetic, frozen=frozen, fused=False)
      what = (n_params, n_members, offset, sigma, frozen is not None)
      assert torch.equal(_bits(a.rows), _bits(b.rows)), what
      assert (a.rows[:, n_params:] == SENTINEL).all(), what
      if frozen is not None:
        assert torch.equal(_bits(a.rows[:, :n_params][:, frozen]),
                           _bits(pol.params[frozen].expand(n_members, -1))), what
      if sigma != 0.0:
        free = slice(0, n_params) if frozen is None else ~frozen
        assert (a.rows[:, :n_params][:, free] != pol.params[free]).any(), what
  # fused=None takes the kernel on the device: the same rows again
  c = _sentinel_population(pol, n_members).perturb_(0.1, 7, offset, antithetic)
  d = _sentinel_population(pol, n_members).perturb_(0.1, 7, offset, antithetic, fused=False)
  assert torch.equal(_bits(c.rows), _bits(d.rows))


def test_perturb_is_the_noise_of_normal_slabs(dev):
  """Frozen parameters skip their counters: the free ones keep theirs."""
  pol = _policy(dev, 323)
  pop = _sentinel_population(pol, 6)
  frozen = _bias_mask(pol)
  pop.perturb_(0.5, 11, 40, True, frozen=frozen)
  eps = pop.noise(11, 40).double()
  want = (pol.params.double() + 0.5 * eps).float()
  got = pop.rows[:3, :323]
  assert torch.equal(_bits(got[:, ~frozen]), _bits(want[:, ~frozen]))


def test_perturb_rows_off_16_bytes(dev):
  """Rows whose base is not 16-byte aligned take the word-by-word stores."""
  pol = _policy(dev, 323)
  a = _sentinel_population(pol, 6)
  big = torch.full((6 * a.stride + 8,), SENTINEL, dtype=torch.float32, device=dev)
  a.rows = big[1:1 + 6 * a.stride].view(6, a.stride)
  assert a.rows.data_ptr() % 16 == 4
  b = _sentinel_population(pol, 6)
  a.perturb_(0.1, 3, 10, True, fused=True)
  b.perturb_(0.1, 3, 10, True, fused=False)
  assert torch.equal(_bits(a.rows), _bits(b.rows))
  assert big[0] == SENTINEL and (big[1 + 6 * a.stride:] == SENTINEL).all()


# ---- delta ----------------------------------------------------------------------------------

def _weights(P, seed, zeros=True):
  g = torch.Generator(device='cpu').manual_seed(seed)
  w = torch.randn((P,), generator=g)
  if zeros and P > 2:
    w[torch.randperm(P, generator=g)[:P // 3]] = 0.
  return w


def _check_delta(pop, got, w, seed, offset, frozen=None):
  P = w.numel()
  eps = pop.noise(seed, offset).double()
  terms = w.to(eps.device).float().double()[:, None] * eps
  ref, mag = terms.sum(0), terms.abs().sum(0)
  if frozen is not None:
    frozen = frozen.to(got.device)
    assert (got[frozen] == 0).all()
    got, ref, mag = got[~frozen], ref[~frozen], mag[~frozen]
  err = (got.double() - ref).abs()
  bound = 2.0 ** -23 * ref.abs() + P * 2.0 ** -50 * mag
  k = int(torch.argmax(err - bound))
  print(f'delta P={P} n={got.numel()}: worst error {err[k].item():.3e}, its bound {bound[k].item():.3e}')
  assert (err <= bound).all(), (P, err[k].item(), bound[k].item())


@pytest.mark.parametrize('P', [1, CHUNK, CHUNK + 1, 2 * CHUNK + 2])
@pytest.mark.parametrize('n_params', [18, 323])
def test_delta_against_the_float64_chained_form(dev, n_params, P):
  from brax_amd.envs.population import PolicyPopulation
  pol = _policy(dev, n_params)
  pop = PolicyPopulation(pol, 2 * P)
  seed, offset = 21, 2 ** 32 - 6
  for w in (_weights(P, P, zeros=False), _weights(P, P + 1)):
    got = pop.weighted_noise_sum(w, seed, offset, fused=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n_params,)
    _check_delta(pop, got, w, seed, offset)
    # the chained form under the same bound, and fused=None is the kernel
    _check_delta(pop, pop.weighted_noise_sum(w, seed, offset, fused=False), w, seed, offset)
    again = pop.weighted_noise_sum(w, seed, offset, workspace=pop.delta_workspace())
    assert torch.equal(_bits(got), _bits(again))
  # zeros: skipped directions are exact
  zero = pop.weighted_noise_sum(torch.zeros(P), seed, offset, fused=True)
  assert (zero == 0).all() and not torch.signbit(zero).any()
  # a frozen mask: exact zeros there, the others unchanged
  frozen = _bias_mask(pol)
  w = _weights(P, 3)
  plain = pop.weighted_noise_sum(w, seed, offset, fused=True)
  masked = pop.weighted_noise_sum(w, seed, offset, frozen=frozen, fused=True)
  _check_delta(pop, masked, w, seed, offset, frozen=frozen)
  assert torch.equal(_bits(masked[~frozen]), _bits(plain[~frozen]))
  chained = pop.weighted_noise_sum(w, seed, offset, frozen=frozen, fused=False)
  assert (chained[frozen] == 0).all()


@pytest.mark.parametrize('P', [3, 2 * CHUNK + 2])
@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_a_non_finite_weight_reaches_every_output_and_no_other_call(dev, P, bad):
  from brax_amd.envs.population import PolicyPopulation
  pol = _policy(dev, 323)
  pop = PolicyPopulation(pol, 2 * P)
  ws = pop.delta_workspace()
  frozen = _bias_mask(pol)
  w = _weights(P, 9)
  clean = pop.weighted_noise_sum(w, 4, 0, frozen=frozen, workspace=ws)
  for at in (0, P - 1):
    wb = w.clone()
    wb[at] = bad
    got = pop.weighted_noise_sum(wb, 4, 0, frozen=frozen, workspace=ws)
    assert not torch.isfinite(got[~frozen]).any(), (at, bad)
    assert (got[frozen] == 0).all()
    # the same workspace, clean weights: nothing of the bad call is left
    again = pop.weighted_noise_sum(w, 4, 0, frozen=frozen, workspace=ws)
    assert torch.equal(_bits(again), _bits(clean))
  assert torch.isfinite(clean).all()


def test_a_short_workspace_is_refused(dev):
  from brax_amd import _native
  from brax_amd.envs.population import PolicyPopulation
  pop = PolicyPopulation(_policy(dev, 18), 2 * (CHUNK + 1))
  assert pop.delta_workspace().numel() == 2 * 18
  with pytest.raises(_native.NativeError, match='workspace'):
    pop.weighted_noise_sum(torch.ones(CHUNK + 1), 0,
                           workspace=torch.empty(2 * 18 - 1, dtype=torch.float64, device=dev))


# ---- one epoch ------------------------------------------------------------------------------

P8, EP = 8, 20
# a pendulum that starts within 0.01 of upright stands for 20 steps under
# ARS's default noise (0.025): every score is equal and reward_std is 0. This
# much feedback topples some of the 16 early.
ARS_STD = 5.0


def _env(dev, B, ar=1):
  from brax_amd import envs
  return envs.create('inverted_pendulum', batch_size=B, episode_length=EP, action_repeat=ar,
                     device=dev)


def _replay(learner, env, theta0, out, shift, K, norm):
  """The epoch's scores from a direct `population_rollout` with its keys."""
  from brax_amd.envs.population import PolicyPopulation, population_rollout
  from brax_amd.training import es
  pol = learner.make_policy((None, es.unpack(theta0, learner.policy.sizes)))
  if norm:  # the normaliser as the epoch's episodes read it: its initial state
    O = env.observation_size
    pol.obs_mean = torch.zeros(O, device=theta0.device)
    pol.obs_std = torch.ones(O, device=theta0.device)
  pop = PolicyPopulation(pol, 2 * P8)
  pop.perturb_(learner.perturbation_std, out['param_seed'], out['param_offset'], True,
               frozen=learner.frozen, fused=False)
  st = env.reset(out['reset_key'])
  _, res = population_rollout(env, st, pop, K, seed=out['action_seed'],
                              offset=out['action_offset'], reward_shift=shift)
  return pop, res


def test_es_epoch(dev):
  from brax_amd.training import es
  ar = 2
  env = _env(dev, 2 * P8, ar)
  L = es.Learner(env, population_size=P8, episode_length=EP, action_repeat=ar, l2coeff=0.01,
                 learning_rate=1e-2, fitness_shaping=es.FitnessShaping.CENTERED_RANK,
                 perturbation_std=0.1, seed=3, normalize_observations=True, device=dev)
  assert L.policy.activation == 'relu' and L.policy.head == 'normal_tanh'
  assert [n for _, n in L.policy.sizes] == [32] * 4 + [2 * env.action_size]
  theta0, addr = L.theta.clone(), L.policy.params.data_ptr()
  assert torch.equal(theta0, L.policy.params)
  out = L.epoch()
  pop, res = _replay(L, env, theta0, out, 0.0, EP // ar, norm=True)
  assert torch.equal(_bits(out['scores']), _bits(res.scores))
  print('es scores', out['scores'].tolist())
  assert out['scores'].unique().numel() > 2  # (episodes end early: the ranks are not all ties)
  assert (out['param_offset'], out['action_offset']) == (0, 0)
  assert L.param_offset == 2 * P8 * pop.n_params
  assert L.action_offset == (EP // ar) * 2 * (2 * P8) * env.action_size
  assert out['param_seed'] != out['action_seed']
  # the weights: centred ranks of the 16 scores, half minus half
  s = out['scores'].cpu().numpy().astype(np.float64)
  ranks = np.argsort(np.argsort(s, kind='stable'), kind='stable')
  w = ranks / (2 * P8 - 1) - .5
  np.testing.assert_allclose(out['weights'].cpu().numpy(), w[:P8] - w[P8:], rtol=1e-12, atol=0)
  assert out['weights'].dtype == torch.float64
  _check_delta(pop, out['delta'], out['weights'].cpu(), out['param_seed'], out['param_offset'])
  # Adam on -(delta / population - l2coeff theta), from a fresh optimiser
  t = theta0.clone()
  opt = torch.optim.Adam([t], lr=1e-2, eps=1e-8)
  t.grad = -(out['delta'] / P8 - 0.01 * theta0)
  opt.step()
  assert torch.equal(_bits(L.theta), _bits(t))
  assert torch.equal(_bits(L.policy.params), _bits(t))
  assert L.policy.params.data_ptr() == addr
  count = float(res.obs_count.double().sum())
  assert count > 0 and L.num_env_steps == int(count) * ar
  assert L.normalizer.count == count
  assert set(out['metrics']) == {'params_norm', 'eval_scores_mean', 'eval_scores_std', 'weights'}
  assert all(np.isfinite(float(v)) for v in out['metrics'].values())
  # the next epoch's parameter noise starts where this one's ended
  assert L.epoch()['param_offset'] == 2 * P8 * pop.n_params


def test_ars_epoch(dev):
  from brax_amd.training import ars
  env = _env(dev, 2 * P8)
  assert ars.Learner(env, P8, 30, episode_length=EP, device=dev).top_directions == P8
  L = ars.Learner(env, number_of_directions=P8, top_directions=3, step_size=0.015,
                  episode_length=EP, exploration_noise_std=ARS_STD, seed=4, reward_shift=0.5,
                  device=dev)
  O, A = env.observation_size, env.action_size
  assert L.policy.head == 'identity' and L.policy.sizes == [(O, A)]
  assert (L.theta == 0).all() and L.frozen.tolist() == [0] * (O * A) + [1] * A
  theta0, addr = L.theta.clone(), L.policy.params.data_ptr()
  out = L.epoch()
  pop, res = _replay(L, env, theta0, out, 0.5, EP, norm=False)
  # the frozen bias is not perturbed
  assert (pop.rows[:, O * A:O * A + A] == 0).all() and (L.population.rows[:, O * A:O * A + A] == 0).all()
  assert torch.equal(_bits(out['scores']), _bits(res.scores))
  print('ars scores', out['scores'].tolist())
  assert out['scores'].unique().numel() > 2 and float(out['reward_std']) > 0
  s = out['scores'].cpu().numpy().astype(np.float64)
  plus, minus = s[:P8], s[P8:]
  rank = np.argsort(np.argsort(-np.maximum(plus, minus), kind='stable'), kind='stable')
  rw = (rank < 3).astype(np.float64)
  np.testing.assert_allclose(out['weights'].cpu().numpy(), rw * (plus - minus), rtol=1e-12, atol=0)
  assert rw.sum() == 3
  std = np.std(np.concatenate([plus[rw > 0], minus[rw > 0]]))
  np.testing.assert_allclose(float(out['reward_std']), std, rtol=1e-12, atol=0)
  _check_delta(pop, out['delta'], out['weights'].cpu(), out['param_seed'], out['param_offset'],
               frozen=L.frozen.bool())
  want = theta0 + 0.015 * out['delta'] / (3 * out['reward_std'].float())
  want[O * A:] = 0.
  assert torch.equal(_bits(L.theta), _bits(want))
  assert torch.equal(_bits(L.policy.params), _bits(want))
  assert L.policy.params.data_ptr() == addr
  assert L.num_env_steps == int(float(res.obs_count.double().sum()))
  assert float(out['metrics']['weights']) == 3 / P8


# ---- end to end -----------------------------------------------------------------------------

def _record_epochs(monkeypatch, cls):
  steps = []
  orig = cls.epoch

  def epoch(self):
    out = orig(self)
    steps.append(self.num_env_steps)
    return out
  monkeypatch.setattr(cls, 'epoch', epoch)
  return steps


def _expected_calls(steps, first, between, initial):
  """The reference's loop over the recorded step counts: one evaluation after
  an epoch that reaches the next evaluation step."""
  calls, nxt = ([0] if initial else []), first
  for s in steps:
    if s >= nxt:
      calls.append(s)
      nxt += between
  return calls


def _finite(metrics):
  assert metrics
  for k, v in metrics.items():
    assert np.isfinite(float(v)), k


def _evaluates(dev, policy):
  from brax_amd.envs.evaluator import Evaluator
  from brax_amd.envs.policy import MLPPolicy
  assert isinstance(policy, MLPPolicy)
  m = Evaluator('inverted_pendulum', policy, num_eval_envs=16, episode_length=EP,
                device=dev).run_evaluation()
  assert np.isfinite(float(m['eval/episode_reward']))


# an epoch is at most 2 * 8 * 20 = 320 env steps: 641 takes three or more
STEPS = 641


def test_es_train(dev, monkeypatch):
  from brax_amd.training import es
  steps, calls = _record_epochs(monkeypatch, es.Learner), []
  make_policy, params, metrics = es.train(
      'inverted_pendulum', num_timesteps=STEPS, episode_length=EP, population_size=P8,
      fitness_shaping=es.FitnessShaping.WIERSTRA, center_fitness=True, num_eval_envs=16,
      normalize_observations=True, num_evals=2, deterministic_eval=True, seed=1,
      max_devices_per_host=8, progress_fn=lambda n, m: calls.append((n, dict(m))), device=dev)
  assert len(steps) >= 3 and steps[-1] >= STEPS > steps[-2]
  # num_evals 2: one evaluation after the initial one, at 641
  assert [n for n, _ in calls] == _expected_calls(steps, 641, 641, True) == [0, steps[-1]]
  for _, m in calls:
    _finite(m)
  _finite(metrics)
  assert 'training/sps' in metrics and 'training/params_norm' in metrics
  assert 'eval/episode_reward' in metrics
  _evaluates(dev, make_policy(params))
  _evaluates(dev, make_policy(params, deterministic=True))


def test_ars_train(dev, monkeypatch):
  from brax_amd.training import ars
  steps, calls = _record_epochs(monkeypatch, ars.Learner), []
  make_policy, params, metrics = ars.train(
      'inverted_pendulum', num_timesteps=STEPS, episode_length=EP, number_of_directions=P8,
      top_directions=3, exploration_noise_std=ARS_STD, num_eval_envs=16,
      normalize_observations=True, num_evals=2, seed=1, max_devices_per_host=8, progress_fn=lambda n, m: calls.append((n, dict(m))), device=dev)
  assert len(steps) >= 3 and steps[-1] >= STEPS > steps[-2]
  # 641 // 2 = 320 between evaluations, the first at 641 - 320; none at 0
  want = _expected_calls(steps, 321, 320, False)
  assert [n for n, _ in calls] == want and want[0] > 0 and len(want) <= 2
  for _, m in calls:
    _finite(m)
  _finite(metrics)
  assert 'training/sps' in metrics and 'eval/episode_reward' in metrics
  policy = make_policy(params)
  assert policy.head == 'identity'
  _evaluates(dev, policy)
