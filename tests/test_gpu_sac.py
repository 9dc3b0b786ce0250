"""SAC and its replay queue on the GPU.

`bx_replay_insert` and `bx_replay_sample` against the chained form
(`fused=False`) on the same device tensors, compared on an int32 view: the
kernels only copy words, so every bit is checked and NaN payloads must arrive
unchanged. A wave takes whole rows, its lanes along the row's words, 256 words
per pass (`REPLAY_CHUNK` x 64, `brax_amd/csrc/replay_kernels.hip`), four waves
per workgroup: row_words 1 and 5 use a few lanes of one piece, 67 two pieces,
185 (Ant's row) three; 1 and 3 rows leave waves of the one workgroup idle, 64
and 65 rows are 16 workgroups and 16 plus one wave.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_sac import reference_rows

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF  # a NaN with a payload, as int32
WIDTHS = {1: [1], 5: [2, 1, 1, 1], 67: [30, 5, 1, 1, 29, 1], 185: [87, 8, 1, 1, 87, 1]}


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _bits(shape, g, dev):
  """Random 32-bit patterns as float32 (NaNs with payloads, infinities and
  denormals among them)."""
  return torch.randint(-2**31, 2**31 - 1, shape, generator=g, dtype=torch.int64).to(
      torch.int32).view(torch.float32).to(dev)


def _queue(capacity, widths, n_samples, dev, seed=0):
  from brax_amd.training.replay_buffers import UniformSamplingQueue
  q = UniformSamplingQueue(capacity, {f'f{k}': w for k, w in enumerate(widths)}, n_samples,
                           seed=seed, device=dev)
  q.data.view(torch.int32).fill_(SENTINEL)
  return q


def _sliced_batch(widths, n, g, dev):
  """Each field a column slice of a wider buffer of its own: unequal row
  strides, none equal to the width."""
  batch = {}
  for k, w in enumerate(widths):
    wide = _bits((n, w + 1 + k), g, dev)
    batch[f'f{k}'] = wide[:, (k % 2):(k % 2) + w]
    assert batch[f'f{k}'].stride(0) == w + 1 + k
  return batch


@pytest.mark.parametrize('row_words', [1, 5, 67, 185])
def test_insert_equals_the_chained_form_bit_for_bit(dev, row_words):
  widths = WIDTHS[row_words]
  g = torch.Generator().manual_seed(row_words)
  for capacity in (7, 64, 130):
    for n in (1, 3, 64, 65):
      if n > capacity:
        continue
      # the start, a batch that ends on the last row, one that wraps after its
      # first row, one that wraps before its last
      for position in sorted({0, capacity - n, capacity - 1, (capacity - n + 1) % capacity}):
        fused, chained = _queue(capacity, widths, 1, dev), _queue(capacity, widths, 1, dev)
        fused.position = chained.position = position
        batch = _sliced_batch(widths, n, g, dev)
        fused.insert(batch, fused=True)
        chained.insert(batch, fused=False)
        what = (capacity, n, position)
        assert (fused.position, fused.size) == (chained.position, chained.size) == (
            (position + n) % capacity, n), what
        got, want = fused.data.view(torch.int32), chained.data.view(torch.int32)
        assert torch.equal(got, want), what
        rows = (position + torch.arange(n, device=dev)) % capacity
        flat = torch.cat(list(batch.values()), dim=1).view(torch.int32)
        assert torch.equal(got[rows], flat), what
        untouched = torch.ones(capacity, dtype=torch.bool, device=dev)
        untouched[rows] = False
        assert bool((got[untouched] == SENTINEL).all()), what
  # n_rows == capacity from a position inside the ring: every row written once
  q = _queue(64, widths, 1, dev)
  q.position = 40
  batch = _sliced_batch(widths, 64, g, dev)
  q.insert(batch, fused=True)
  flat = torch.cat(list(batch.values()), dim=1).view(torch.int32)
  assert torch.equal(q.data.view(torch.int32)[(40 + torch.arange(64, device=dev)) % 64], flat)
  assert (q.position, q.size) == (40, 64)


def _filled(capacity, widths, n_samples, live, position, dev, g, seed=5):
  """A queue whose `live` rows end at `position`, random bits in them and the
  NaN sentinel in the dead rows."""
  q = _queue(capacity, widths, n_samples, dev, seed=seed)
  rows = (position - live + torch.arange(live, device=dev)) % capacity
  q.data[rows] = _bits((live, sum(widths)), g, dev)
  q.position, q.size = position, live
  return q


@pytest.mark.parametrize('row_words', [1, 5, 67, 185])
@pytest.mark.parametrize('n_samples', [1, 63, 257])
def test_sample_equals_the_restatement_and_the_chained_form(dev, row_words, n_samples):
  widths = WIDTHS[row_words]
  g = torch.Generator().manual_seed(row_words * 1000 + n_samples)
  # (capacity, live rows, position): full; partly filled; one live row; a
  # live range that wraps past the end; position - size negative
  for capacity, live, position in ((7, 7, 3), (64, 20, 20), (64, 1, 0), (130, 100, 30),
                                   (130, 129, 2)):
    q = _filled(capacity, widths, n_samples, live, position, dev, g)
    for offset in (0, (1 << 32) - 3, (1 << 64) - 3):
      what = (capacity, live, position, offset)
      q.counter = offset
      idx = torch.full((n_samples,), -1, dtype=torch.int64, device=dev)
      got = q.sample(fused=True, indices=idx)
      assert q.counter == (offset + n_samples) % (1 << 64), what
      want_idx = reference_rows(q.seed, offset, n_samples, position, live, capacity)
      assert idx.tolist() == want_idx, what
      q.counter = offset
      idx2 = torch.empty_like(idx)
      want = q.sample(fused=False, indices=idx2)
      assert torch.equal(idx2, idx), what
      flat = q.data.view(torch.int32)[idx]
      o = 0
      for k, w in enumerate(widths):
        t = got[f'f{k}']
        assert t.is_contiguous() and tuple(t.shape) == (n_samples, w)
        assert torch.equal(t.view(torch.int32), flat[:, o:o + w]), (what, k)
        assert torch.equal(t.view(torch.int32), want[f'f{k}'].view(torch.int32)), (what, k)
        assert not bool((t.view(torch.int32) == SENTINEL).any()), (what, k)  # no dead row
        o += w
      if live == 1:
        assert set(want_idx) == {(position - 1) % capacity}


def test_sample_scatters_into_strided_views_and_repeats(dev):
  widths = WIDTHS[185]
  g = torch.Generator().manual_seed(9)
  n = 257
  q = _filled(130, widths, n, 100, 30, dev, g)
  # every destination field a strided view inside ONE flat buffer, a gap of
  # k + 1 sentinel words after field k's columns
  stride = sum(widths) + sum(k + 1 for k in range(len(widths)))
  flat = torch.empty((n, stride), dtype=torch.float32, device=dev)
  flat.view(torch.int32).fill_(SENTINEL)
  out, gaps, o = {}, torch.zeros(stride, dtype=torch.bool, device=dev), 0
  for k, w in enumerate(widths):
    out[f'f{k}'] = flat[:, o:o + w]
    gaps[o + w:o + w + k + 1] = True
    o += w + k + 1
  idx = torch.empty((n,), dtype=torch.int64, device=dev)
  got = q.sample(fused=True, out=out, indices=idx)
  assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
  assert bool((flat.view(torch.int32)[:, gaps] == SENTINEL).all())
  rows = q.data.view(torch.int32)[idx]
  assert torch.equal(flat.view(torch.int32)[:, ~gaps], rows)
  # the same counter gives the same bits; consecutive calls advance it
  assert q.counter == n
  second = {k: v.clone() for k, v in q.sample(fused=True).items()}
  assert q.counter == 2 * n
  q.counter = 0
  again = q.sample(fused=True)
  for k in out:
    assert torch.equal(again[k].view(torch.int32), out[k].view(torch.int32))
  q.counter = n
  again2 = q.sample(fused=True)
  assert all(torch.equal(again2[k].view(torch.int32), second[k].view(torch.int32)) for k in out)
  assert any(not torch.equal(second[k].view(torch.int32), again[k].view(torch.int32)) for k in out)
  # (n,) destinations for the fields of width 1, and fused=None takes the kernel
  out1 = {f'f{k}': torch.empty((n,) if w == 1 else (n, w), dtype=torch.float32, device=dev)
          for k, w in enumerate(widths)}
  q.counter = 0
  q.sample(out=out1)
  for k, w in enumerate(widths):
    assert torch.equal(out1[f'f{k}'].reshape(n, w).view(torch.int32), out[f'f{k}'].view(torch.int32))
  with pytest.raises(NotImplementedError):
    q.sample(fused=True, out={k: v.double() for k, v in out1.items()})


# ---- the learner ------------------------------------------------------------------------------

HIDDEN = (16, 16)  # within POLICY_MAX_WIDTH: the acting launch is the fused one


def _factory(hidden=HIDDEN):
  from brax_amd.training import sac_networks
  return functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=hidden)


def test_training_step_equals_its_restatement(dev):
  from brax_amd import envs
  from brax_amd.envs import wrappers
  from brax_amd.envs.policy import MLPPolicy, fused_supported, policy_rollout
  from brax_amd.training import sac, sac_networks
  from brax_amd.training.replay_buffers import UniformSamplingQueue, transition_fields
  B, batch, G, seed = 8, 4, 2, 3
  kw = dict(learning_rate=1e-3, discounting=0.95, reward_scaling=0.5, tau=0.05)
  env = envs.create('inverted_pendulum', episode_length=50, action_repeat=1, batch_size=B,
                    device=dev)
  O, A = env.observation_size, env.action_size
  key = wrappers.split_key(np.array([0, seed], np.uint32))[0]
  learner = sac.Learner(env, B, batch_size=batch, grad_updates_per_step=G, max_replay_size=20,
                        num_prefill_actor_steps=1, normalize_observations=True, seed=seed,
                        network_factory=_factory(), device=dev, **kw)
  assert fused_supported(env, learner.actor) is None
  learner.reset(key)
  learner.prefill()
  steps = [learner.training_step() for _ in range(2)]
  torch.cuda.synchronize()
  assert learner.env_steps == 3 * B
  assert steps[-1]['buffer_current_size'] == 20 and steps[-1]['buffer_current_position'] == 4

  # the restatement: policy_rollout, the chained queue, sgd_step, the same seeds
  ts = sac.init_training_state(O, A, kw['learning_rate'], _factory(), seed, dev)
  norm = sac.RunningStatistics(O, dev)
  actor = MLPPolicy([(w.detach(), b.detach()) for w, b in ts.policy_layers], activation='relu',
                    device=dev, obs_mean=norm.mean_t, obs_std=norm.std_t)
  actor.obs_mean, actor.obs_std = norm.mean_t, norm.std_t
  queue = UniformSamplingQueue(20, transition_fields(O, A), batch * G, seed=seed, device=dev)
  gen = torch.Generator(device=dev).manual_seed(seed)
  state, offset, metrics = env.reset(key), 0, None
  for step in range(3):
    obs0 = state.obs
    state, traj, extras = policy_rollout(env, state, actor, 1, seed=seed, offset=offset)
    offset += 2 * B * A
    norm.update(obs0)
    queue.insert({'observation': obs0, 'action': extras.action[0], 'reward': traj.reward[0],
                  'discount': 1 - traj.done[0], 'next_observation': traj.obs[0],
                  'truncation': traj.truncation[0]}, fused=False)
    if step == 0:
      continue  # the prefill step
    sample = queue.sample(fused=False)
    for g_ in range(G):
      mb = {k: v[g_ * batch:(g_ + 1) * batch] for k, v in sample.items()}
      eps = tuple(torch.randn((batch, A), generator=gen, device=dev) for _ in range(3))
      metrics = sac.sgd_step(ts, (norm.mean_t, norm.std_t), mb, eps,
                             reward_scaling=kw['reward_scaling'], discounting=kw['discounting'],
                             tau=kw['tau'])
    actor.load_([(w.detach(), b.detach()) for w, b in ts.policy_layers])
  assert (queue.position, queue.size, queue.counter) == (
      learner.buffer.position, learner.buffer.size, learner.buffer.counter) == (4, 20, 2 * batch * G)
  assert torch.equal(queue.data.view(torch.int32), learner.buffer.data.view(torch.int32))
  assert not bool(torch.isnan(queue.data).any()) and float(queue.data.abs().max()) > 0
  for got, want in zip(
      sac_networks.q_parameters([learner.ts.policy_layers] + learner.ts.q_layers
                                + learner.ts.target_q_layers) + [learner.ts.log_alpha],
      sac_networks.q_parameters([ts.policy_layers] + ts.q_layers + ts.target_q_layers)
      + [ts.log_alpha]):
    assert torch.equal(got, want)
  assert torch.equal(learner.actor.params, actor.params)
  assert torch.equal(learner.normalizer.mean_t, norm.mean_t)
  assert float(learner.ts.log_alpha.detach()) != 0 and learner.ts.gradient_steps == 2 * G
  # the last step's metrics: the mean over its G gradient steps ends in the last one's alpha
  assert float(steps[-1]['alpha']) > 0 and np.isfinite(float(steps[-1]['critic_loss']))
  assert float(metrics['alpha']) == float(torch.exp(learner.ts.log_alpha.detach()))


@pytest.mark.parametrize('hidden,normalize', [(HIDDEN, True), ((256, 256), False)])
def test_train_end_to_end(dev, hidden, normalize):
  """(256, 256), the reference's default, is wider than the policy kernel
  takes: the acting step goes through `policy_rollout`'s chained path."""
  from brax_amd import envs
  from brax_amd.envs.policy import fused_supported
  from brax_amd.training import sac
  num_timesteps, num_envs, min_replay, capacity = 2000, 16, 100, 512
  acct = sac.step_accounting(num_timesteps, 3, min_replay, num_envs, 1, capacity)
  assert (acct.num_prefill_actor_steps, acct.num_training_steps_per_epoch) == (7, 59)
  calls = []
  factory = sac.sac_networks.make_sac_networks if hidden == (256, 256) else _factory(hidden)
  make_policy, params, metrics = sac.train(
      'inverted_pendulum', num_timesteps=num_timesteps, episode_length=50, num_envs=num_envs,
      num_eval_envs=32, batch_size=32, num_evals=3, min_replay_size=min_replay,
      max_replay_size=capacity, grad_updates_per_step=1, normalize_observations=normalize,
      network_factory=factory, device=dev, progress_fn=lambda step, m: calls.append((step, m)))
  prefill = 7 * num_envs
  assert [s for s, _ in calls] == [0, prefill + 59 * num_envs, prefill + 2 * 59 * num_envs]
  assert calls[-1][0] >= num_timesteps
  assert metrics is calls[-1][1]
  want_keys = {'eval/episode_reward', 'training/sps', 'training/walltime', 'training/critic_loss',
               'training/actor_loss', 'training/alpha_loss', 'training/alpha',
               'training/buffer_current_size', 'training/buffer_current_position'}
  assert want_keys <= set(metrics)
  for k in want_keys:
    assert np.isfinite(float(metrics[k])), k
  assert float(metrics['training/sps']) > 0 and float(metrics['training/walltime']) > 0
  assert not any(k.startswith('training/') for k in calls[0][1])  # the initial evaluation
  # the epoch means of min(capacity, rows inserted) and of the write position
  for epoch, (_, m) in enumerate(calls[1:]):
    inserted = [prefill + num_envs * (epoch * 59 + i + 1) for i in range(59)]
    assert float(m['training/buffer_current_size']) == pytest.approx(
        np.mean([min(capacity, r) for r in inserted]), rel=1e-12)
    assert float(m['training/buffer_current_position']) == pytest.approx(
        np.mean([r % capacity for r in inserted]), rel=1e-12)
  assert float(calls[-1][1]['training/buffer_current_size']) == capacity  # full all epoch
  normalizer, policy_layers = params
  assert (normalizer is not None) == normalize
  assert [w.shape[1] for w, _ in policy_layers][:-1] == list(hidden)
  policy = make_policy(params, deterministic=True)
  env = envs.create('inverted_pendulum', episode_length=50, batch_size=num_envs, device=dev)
  why = fused_supported(env, policy)
  assert (why is None) == (hidden == HIDDEN), why
