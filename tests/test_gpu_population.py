"""One episode per perturbed policy in one launch
(`brax_amd.envs.population`: `bx_env_eval_population`). Needs an MI355X.

The yardstick is the parent's own trajectory kernel. For member e,
`policy_rollout(env, st0, population.member(e), K, seed, offset, fused=True)`
runs on the whole batch and env e's row of its trajectory is taken: batch
independence and the per-env noise key make that env e's true trajectory. An
identity head has no trajectory kernel, so there each step's action row is the
`raw_action` (= loc, the same FMA chains) of a one-step `policy_rollout` of the
member as a deterministic NormalTanh policy, applied with `env.step`. The
recurrences of the kernel (shifted reward sum, `EvalWrapper`'s sums, the
observation moments) are then applied in float32 torch. Everything compares
bit for bit.
"""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


_ENVS = {}


def _make(dev, name, B, ep=3, ar=1, lift=None):
  """The env (Episode, Vector, AutoReset) and its reset state; `lift`: that
  env's bodies raised out of a healthy z range (an early `done`)."""
  from brax_amd import envs
  from brax_amd.base import PackedQP
  from brax_amd.envs.policy import _packed
  key = (name, B, ep, ar)
  if key not in _ENVS:
    _ENVS[key] = envs.create(name, batch_size=B, episode_length=ep, action_repeat=ar,
                             auto_reset=True, device=dev)
  env = _ENVS[key]
  st = env.reset(np.array([2, 9], np.uint32))
  if lift is not None:
    buf = _packed(st, dev).clone()
    buf[lift, :, 2] += 3.0
    st = st.replace(qp=PackedQP(buf))
  return env, st


def _theta(env, dev, hidden, head, seed=11, deterministic=False, norm=False):
  from brax_amd.envs.policy import MLPPolicy
  O, A = env.observation_size, env.action_size
  sizes = (O,) + tuple(hidden) + (A if head == 'identity' else 2 * A,)
  g = torch.Generator(device='cpu').manual_seed(seed)
  layers = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    lim = math.sqrt(3.0 / i)
    layers.append(((torch.rand((i, o), generator=g) * 2 - 1) * lim,
                   (torch.rand((o,), generator=g) * 2 - 1) * 0.1))
  kw = {}
  if norm:
    kw = dict(obs_mean=torch.rand((O,), generator=g) - 0.5, obs_std=torch.rand((O,), generator=g) + 0.5)
  return MLPPolicy(layers, activation='relu', deterministic=deterministic, head=head, device=dev, **kw)


def _population(policy, B, seed=3, scale=0.2):
  """Distinct random rows: theta plus member-wise uniform noise."""
  from brax_amd.envs.population import PolicyPopulation
  pp = PolicyPopulation(policy, B)
  g = torch.Generator(device='cpu').manual_seed(seed)
  noise = (torch.rand((B, pp.n_params), generator=g) * 2 - 1) * scale
  return pp.set_(policy.params.cpu()[None] + noise)


def _member_steps(env, st0, member, K, seed, offset):
  """The member's K steps on the whole batch as per-step tensors: obs (K, B,
  O), reward, done, steps, truncation (K, B), metrics (K, B, M), qp (K, B, N,
  16), rng."""
  from brax_amd.envs.policy import _packed, policy_rollout
  if member.head == 'normal_tanh':
    _, tr, _ = policy_rollout(env, st0, member, K, seed=seed, offset=offset, fused=True)
    return dict(obs=tr.obs, reward=tr.reward, done=tr.done, steps=tr.steps,
                truncation=tr.truncation, metrics=tr.metrics, qp=tr.qp,
                rng=tr.rng)
  det = copy.copy(member)
  det.head, det.deterministic = 'normal_tanh', True
  keys = tuple(env.unwrapped.metric_keys)
  rec = {k: [] for k in ('obs', 'reward', 'done', 'steps', 'truncation', 'metrics', 'qp', 'rng')}
  st = st0
  dev = st0.obs.device
  for _ in range(K):
    _, _, ex = policy_rollout(env, st, det, 1, fused=True)
    st = env.step(st, ex.raw_action[0].clone())
    rec['obs'].append(st.obs.clone())
    rec['reward'].append(st.reward.clone())
    rec['done'].append(st.done.clone())
    rec['steps'].append(st.info['steps'].clone())
    rec['truncation'].append(st.info['truncation'].clone())
    rec['metrics'].append(torch.stack([st.metrics[k] for k in keys], -1) if keys
                          else torch.zeros((st.obs.shape[0], 0), device=dev))
    rec['qp'].append(_packed(st, dev).clone())
    rec['rng'].append(st.info['rng'].clone() if st.info.get('rng') is not None else None)
  out = {k: torch.stack(v) for k, v in rec.items() if k != 'rng'}
  out['rng'] = None if rec['rng'][0] is None else torch.stack(rec['rng'])
  return out


def _expected(env, st0, pp, K, seed, offset, shift, members, carry=None):
  """Per member e of `members`: env e's row of everything the launch writes."""
  policy = pp.policy
  mean = policy.obs_mean
  want = {}
  for e in members:
    tr = _member_steps(env, st0, pp.member(e), K, seed, offset)
    B, M = tr['reward'].shape[1], tr['metrics'].shape[2]
    dev = tr['reward'].device
    sums = [torch.zeros(B, device=dev) for _ in range(M)]
    score = torch.zeros(B, device=dev)
    active = torch.ones(B, device=dev)
    esteps = torch.zeros(B, device=dev)
    O = st0.obs.shape[1]
    s1, s2 = torch.zeros((B, O), device=dev), torch.zeros((B, O), device=dev)
    cnt = torch.zeros(B, device=dev)
    sh = torch.tensor(shift, dtype=torch.float32, device=dev)
    flipped = False
    for t in range(K):
      o = st0.obs if t == 0 else tr['obs'][t - 1]
      d = o if mean is None else o - mean
      q = d * d
      s1 = s1 + active[:, None] * d
      s2 = s2 + active[:, None] * q
      cnt = cnt + active
      esteps = torch.where(active != 0, tr['steps'][t], esteps)
      sums = [s + tr['metrics'][t, :, k] * active for k, s in enumerate(sums)]
      score = score + (tr['reward'][t] - sh) * active
      active = active * (1 - tr['done'][t])
      flipped = flipped or (t < K - 1 and float(active[e]) == 0.0)
    want[e] = dict(scores=score[e], active=active[e], episode_steps=esteps[e],
                   sums=[s[e] for s in sums], s1=s1[e], s2=s2[e], count=cnt[e],
                   qp=tr['qp'][K - 1, e, :, :13], obs=tr['obs'][K - 1, e],
                   reward=tr['reward'][K - 1, e], done=tr['done'][K - 1, e],
                   steps=tr['steps'][K - 1, e], truncation=tr['truncation'][K - 1, e],
                   metrics=tr['metrics'][K - 1, e],
                   rng=None if tr['rng'] is None else tr['rng'][K - 1, e], flipped=flipped)
  return want


def _bits(x):
  return x.contiguous().view(torch.int32)


def _same(a, b, what):
  assert torch.equal(_bits(a), _bits(b)), what


def _rows(final, res, e):
  """Env e's row of a fused result, under `_expected`'s names."""
  from brax_amd.envs.policy import _packed
  keys = res.metric_keys
  return dict(scores=res.scores[e], active=res.active[e], episode_steps=res.episode_steps[e],
              sums=[res.metric_sums[k][e] for k in keys],
              s1=None if res.obs_s1 is None else res.obs_s1[e],
              s2=None if res.obs_s2 is None else res.obs_s2[e],
              count=None if res.obs_count is None else res.obs_count[e],
              qp=_packed(final, final.obs.device)[e, :, :13], obs=final.obs[e],
              reward=final.reward[e], done=final.done[e], steps=final.info['steps'][e],
              truncation=final.info['truncation'][e],
              metrics=(torch.stack([final.metrics[k][e] for k in keys]) if keys
                       else torch.zeros((0,), device=final.obs.device)),
              rng=None if final.info.get('rng') is None else final.info['rng'][e])


def _check_rows(got, want, what):
  for k, w in want.items():
    if k == 'flipped':
      continue
    g = got[k]
    if k == 'sums':
      assert len(g) == len(w)
      for i, (x, y) in enumerate(zip(g, w)):
        _same(x, y, (what, k, i))
    elif w is None:
      assert g is None, (what, k)
    else:
      _same(g, w, (what, k))


def _same_results(a, b, rows=None):
  (fa, ra), (fb, rb) = a, b
  B = fa.obs.shape[0]
  for e in (range(B) if rows is None else rows):
    _check_rows(_rows(fa, ra, e), _rows(fb, rb, e), e)


def _run_case(dev, name, B, K, hidden, head, det=False, norm=False, shift=0.0, ep=3, ar=1,
              lift=None, members=None, staged=None):
  from brax_amd.envs.population import population_rollout
  env, st0 = _make(dev, name, B, ep, ar, lift)
  pp = _population(_theta(env, dev, hidden, head, deterministic=det, norm=norm), B)
  seed, offset = 5, 1000
  got = population_rollout(env, st0, pp, k=K, seed=seed, offset=offset, reward_shift=shift, fused=True)
  torch.cuda.synchronize()
  if staged is not None:
    assert got[1].staged is staged
  members = range(B) if members is None else members
  want = _expected(env, st0, pp, K, seed, offset, shift, members)
  for e in members:
    _check_rows(_rows(got[0], got[1], e), want[e], (name, e))
  return env, st0, pp, got, want


ANT = dict(name='ant', B=6, K=7, lift=2)  # one and a half workgroups


@pytest.mark.parametrize('hidden,head,det,norm,shift,staged', [
    ((8,), 'normal_tanh', False, False, 0.0, True),
    ((32,) * 4, 'normal_tanh', False, False, 0.0, False),  # ES's default net: global reads
    ((32,) * 4, 'normal_tanh', True, False, 0.0, False),
    ((), 'identity', False, False, 0.25, True),  # ARS's linear policy
    ((), 'identity', False, True, 0.25, True),
])
def test_ant_members_vs_their_own_trajectories(dev, hidden, head, det, norm, shift, staged):
  _, _, pp, (_, res), want = _run_case(dev, hidden=hidden, head=head, det=det, norm=norm, shift=shift,
                                       staged=staged, **ANT)
  if not hidden:
    assert pp.stride == 704  # 87 x 8 + 8
  elif len(hidden) == 4:
    assert pp.n_params == 6512
  # `done` fired inside the run: `active` flipped before the last step
  assert any(w['flipped'] for w in want.values())
  assert float(res.active.max()) == 0.0
  # the members differ
  assert len({float(s) for s in res.scores}) > 1


def test_staged_and_global_rows_give_the_same_bits(dev):
  from brax_amd.envs.population import population_rollout
  env, st0 = _make(dev, ANT['name'], ANT['B'], lift=ANT['lift'])
  pp = _population(_theta(env, dev, (8,), 'normal_tanh'), ANT['B'])
  a = population_rollout(env, st0, pp, k=ANT['K'], seed=5, offset=1000, fused=True)
  b = population_rollout(env, st0, pp, k=ANT['K'], seed=5, offset=1000, fused=True, stage=False)
  assert a[1].staged is True and b[1].staged is False
  _same_results(a, b)
  _same(a[1].eval_buf, b[1].eval_buf, 'eval')
  _same(a[1].mom_buf, b[1].mom_buf, 'moments')


@pytest.mark.parametrize('det', [False, True])
def test_equal_rows_and_stride_zero_equal_the_evaluation_kernel(dev, det):
  from brax_amd import envs
  from brax_amd.envs import eval_rollout
  from brax_amd.envs.population import PolicyPopulation, population_rollout
  B, K = 21, 7
  env = envs.create('ant', batch_size=B, episode_length=3, auto_reset=True, eval_metrics=True,
                    device=dev)
  st0 = env.reset(np.array([2, 9], np.uint32))
  theta = _theta(env, dev, (32, 32), 'normal_tanh', deterministic=det)
  ref = eval_rollout(env, st0, k=K, policy=theta, seed=5, offset=1000, fused=True)
  em = ref.info['eval_metrics']
  for population in (PolicyPopulation(theta, B), theta):
    final, res = population_rollout(env, st0, population, k=K, seed=5, offset=1000, fused=True)
    _same(res.scores, em.episode_metrics['reward'], 'reward')
    for k in res.metric_keys:
      _same(res.metric_sums[k], em.episode_metrics[k], k)
    _same(res.active, em.active_episodes, 'active')
    _same(res.episode_steps, em.episode_steps, 'episode_steps')
    _same(final.obs, ref.obs, 'obs')
    _same(final.qp.pos, ref.qp.pos, 'pos')
    _same(final.reward, ref.reward, 'reward')
    _same(final.info['steps'], ref.info['steps'], 'steps')


@pytest.mark.parametrize('name,ar', [('halfcheetah', 1), ('pusher', 1), ('hopper', 1), ('fetch', 1),
                                     ('ur5e', 2), ('inverted_pendulum', 1)])
def test_other_kernel_families(dev, name, ar):
  _run_case(dev, name, 5, 6, (8,), 'identity', shift=0.5, ar=ar)


def test_wide_ant_kernel(dev):
  B = 4160
  assert (B + 3) // 4 > 4 * torch.cuda.get_device_properties(dev).multi_processor_count
  _run_case(dev, 'ant', B, 4, (8,), 'normal_tanh', ep=2, lift=63, members=(0, 63, 64, 4159))


def test_continuation_through_carry(dev):
  from brax_amd.envs.population import population_rollout
  env, st0 = _make(dev, ANT['name'], ANT['B'], lift=ANT['lift'])
  pp = _population(_theta(env, dev, (8,), 'normal_tanh', norm=True), ANT['B'])
  B, A = ANT['B'], env.action_size
  whole = population_rollout(env, st0, pp, k=7, seed=5, offset=1000, reward_shift=0.25, fused=True)
  mid, r1 = population_rollout(env, st0, pp, k=3, seed=5, offset=1000, reward_shift=0.25, fused=True)
  assert float(r1.active.min()) == 0.0
  two = population_rollout(env, mid, pp, k=4, seed=5, offset=1000 + 3 * 2 * B * A, reward_shift=0.25,
                           carry=r1, fused=True)
  _same_results(two, whole)


@pytest.mark.parametrize('B', [6, 3, 1])
@pytest.mark.parametrize('moments', [True, False])
def test_no_stores_outside_the_documented_buffers(dev, B, moments):
  from brax_amd.envs.population import population_rollout
  env, st0 = _make(dev, 'ant', B)
  pp = _population(_theta(env, dev, (8,), 'normal_tanh'), B)
  u = env.unwrapped
  N, O, M = u.sys.num_bodies, u.obs_size, len(u.metric_keys)
  block = B * (N * 16 + O + 4 + M)
  pad = 64
  bufs = {n: torch.full((size + 2 * pad,), SENTINEL, device=dev)
          for n, size in (('out', block), ('ev', (M + 3) * B), ('mom', B * (2 * O + 1)))}
  final, res = population_rollout(
      env, st0, pp, k=4, seed=1, fused=True, moments=moments, out=bufs['out'][pad:pad + block],
      eval_out=bufs['ev'][pad:pad + (M + 3) * B].view(M + 3, B),
      mom_out=bufs['mom'][pad:pad + B * (2 * O + 1)].view(B, 2 * O + 1))
  torch.cuda.synchronize()
  for n, t in bufs.items():
    assert bool((t[:pad] == SENTINEL).all()) and bool((t[-pad:] == SENTINEL).all()), n
  if moments:
    assert res.mom_buf.data_ptr() == bufs['mom'][pad:].data_ptr()
    assert bool(torch.isfinite(res.mom_buf).all()) and float(res.obs_count.min()) >= 1.0
  else:
    assert res.mom_buf is None and bool((bufs['mom'] == SENTINEL).all())
  assert bool(torch.isfinite(res.eval_buf).all())
  ref = population_rollout(env, st0, pp, k=4, seed=1, fused=True, moments=moments)
  _same_results((final, res), ref)


def test_a_nan_row_poisons_its_own_env_alone(dev):
  from brax_amd.envs.population import population_rollout
  env, st0 = _make(dev, ANT['name'], ANT['B'], lift=ANT['lift'])
  pp = _population(_theta(env, dev, (8,), 'normal_tanh'), ANT['B'])
  clean = population_rollout(env, st0, pp, k=5, seed=5, fused=True)
  bad = 1
  pp.rows[bad, 17] = float('nan')
  got = population_rollout(env, st0, pp, k=5, seed=5, fused=True)
  assert not math.isfinite(float(got[1].scores[bad]))
  assert not bool(torch.isfinite(got[1].obs_s1[bad]).all())
  assert not bool(torch.isfinite(got[1].obs_s2[bad]).all())
  _same_results(got, clean, rows=[e for e in range(ANT['B']) if e != bad])


def test_antithetic_rows_at_sigma_zero_are_twins(dev):
  from brax_amd.envs.population import PolicyPopulation, population_rollout
  B = 6
  env, st0 = _make(dev, 'ant', B)
  # twins need twin start states (and no noise, no reset: K below the episode
  # length, a deterministic head), which a reset does not give: copy them
  from brax_amd.base import PackedQP
  from brax_amd.envs.policy import _packed
  buf = _packed(st0, dev).clone()
  buf[3:] = buf[:3]
  st = st0.replace(qp=PackedQP(buf), obs=torch.cat([st0.obs[:3], st0.obs[:3]]))
  theta = _theta(env, dev, (8,), 'normal_tanh', deterministic=True)
  pp = PolicyPopulation(theta, B).perturb_(0.0, seed=4)
  assert torch.equal(pp.rows[:3], pp.rows[3:])
  assert torch.equal(pp.rows[:, :pp.n_params], theta.params.expand(B, -1))
  _, res = population_rollout(env, st, pp, k=2, fused=True)
  _same(res.scores[:3], res.scores[3:], 'scores')
  _same(res.obs_s1[:3], res.obs_s1[3:], 's1')
  _same(res.obs_s2[:3], res.obs_s2[3:], 's2')
  # and a real perturbation is what `noise` says, on the device's own RNG
  pp.perturb_(0.05, seed=4, offset=10)
  eps = pp.noise(4, 10)
  th = theta.params.double()
  assert torch.equal(pp.rows[:3, :pp.n_params], (th + 0.05 * eps.double()).float())
  assert torch.equal(pp.rows[3:, :pp.n_params], (th - 0.05 * eps.double()).float())
  assert float(eps.std()) > 0.5


@pytest.mark.parametrize('name', ['humanoid', 'swimmer', 'grasp'])
def test_refused_kinds_run_chained(dev, name):
  from brax_amd.envs import eval_rollout, wrappers
  from brax_amd.envs.population import population_rollout, population_supported
  B, K = 4, 3
  env, st0 = _make(dev, name, B)
  pp = _population(_theta(env, dev, (8,), 'normal_tanh', deterministic=True), B)
  why = population_supported(env, pp)
  assert why and 'reads the action row' in why
  with pytest.raises(NotImplementedError, match='reads the action row'):
    population_rollout(env, st0, pp, k=K, fused=True)
  final, res = population_rollout(env, st0, pp, k=K)
  assert res.staged is None and bool(torch.isfinite(res.scores).all())
  assert tuple(res.obs_s1.shape) == (B, env.observation_size)
  if name == 'humanoid':
    eenv = wrappers.EvalWrapper(env)
    est0 = eenv.reset(np.array([2, 9], np.uint32))
    _same(est0.obs, st0.obs, 'the same reset')
    for e in range(B):
      ref = eval_rollout(eenv, est0, k=K, policy=pp.member(e), fused=None)
      _same(res.scores[e], ref.info['eval_metrics'].episode_metrics['reward'][e], e)


def test_bad_stride_and_head_are_refused(dev):
  from brax_amd.envs.population import population_supported
  env, _ = _make(dev, 'ant', 6)
  pp = _population(_theta(env, dev, (8,), 'normal_tanh'), 6)
  assert population_supported(env, pp) is None
  assert pp.n_params % 4 == 0
  for stride in (pp.n_params - 4, pp.n_params + 2, -4):
    why = population_supported(env, pp, param_stride=stride)
    assert why and 'param_stride' in why, stride
  assert population_supported(env, pp, param_stride=pp.n_params + 8) is None
  why = population_supported(env, pp, head='softmax')
  assert why and 'unknown head' in why
  # an identity head wants an A-wide last layer
  why = population_supported(env, pp, head='identity')
  assert why and 'identity' in why


def test_identity_head_in_the_evaluator(dev):
  from brax_amd.envs import Evaluator, eval_supported
  B, ep = 6, 4
  from brax_amd import envs
  env = envs.create('ant', batch_size=B, episode_length=ep, auto_reset=True, eval_metrics=True,
                    device=dev)
  policy = _theta(env, dev, (), 'identity', norm=True)
  assert eval_supported(env, policy) is None
  fused = Evaluator(env, policy, num_eval_envs=B, episode_length=ep, seed=3, fused=True)
  chained = Evaluator(env, policy, num_eval_envs=B, episode_length=ep, seed=3, fused=False)
  a = fused.run_evaluation(aggregate_episodes=False)
  b = chained.run_evaluation(aggregate_episodes=False)
  timing = ('eval/epoch_eval_time', 'eval/sps', 'eval/walltime')
  assert sorted(a) == sorted(b)
  for k in a:
    if k not in timing:
      torch.testing.assert_close(a[k], b[k], rtol=1e-3, atol=1e-3, msg=k)
  # every recorded sum, bit for bit, against the float32 recurrences on the
  # yardstick trajectory
  st0 = fused.first_state
  tr = _member_steps(env.env, st0, policy, ep, 0, 0)
  keys = tuple(env.unwrapped.metric_keys)
  active = torch.ones(B, device=dev)
  sums = {k: torch.zeros(B, device=dev) for k in keys + ('reward',)}
  esteps = torch.zeros(B, device=dev)
  for t in range(ep):
    esteps = torch.where(active != 0, tr['steps'][t], esteps)
    for i, k in enumerate(keys):
      sums[k] = sums[k] + tr['metrics'][t, :, i] * active
    sums['reward'] = sums['reward'] + tr['reward'][t] * active
    active = active * (1 - tr['done'][t])
  em = fused.state.info['eval_metrics']
  assert list(em.episode_metrics) == list(keys + ('reward',))
  for k, w in sums.items():
    _same(em.episode_metrics[k], w, k)
    _same(a[f'eval/episode_{k}'], w, k)
  _same(em.active_episodes, active, 'active')
  _same(em.episode_steps, esteps, 'episode_steps')
  _same(fused.state.obs, tr['obs'][ep - 1], 'obs')
