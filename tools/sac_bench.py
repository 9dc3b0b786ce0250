"""SAC trainer timings on one GPU (a tool, not a test; `bench.py` is
untouched).

  (a) `UniformSamplingQueue.insert` and `.sample`, fused (one `bx_replay_insert`
      / `bx_replay_sample` launch) against chained (the same rows through torch
      operations) on the same build: Ant's row (185 words) in a queue of 2^20
      rows, 4,096 rows inserted, 256 x 64 rows sampled; and the sizes of the
      reference's own buffer test (10 rows, batches of 2). A timed region is
      `--calls` back-to-back calls ending in one device synchronise; the figure
      is microseconds per call, median (min .. max) of `--runs` regions after a
      warm-up, the two forms alternating.
  (b) one SAC training step on Ant (4,096 envs, batch 256 x 64 gradient
      updates by default, `--updates` to change) split into its phases, each
      ending in a synchronise: act, normaliser, insert, sample, updates;
      median (min .. max) of `--steps` steps, the buffer's two forms
      alternating.
  `--learn`: a short run on `inverted_pendulum`, the evaluation reward at every
      evaluation.

Prints one JSON line per measurement.

    python tools/sac_bench.py [--runs 7] [--calls 50] [--steps 3] [--learn]
"""
import functools
import time

import torch

from measure import (ANT_ACT, ANT_OBS, SAC_ANT, alternate, ant_env, emit, sac_learner, spread, start,
                     timed, tool_args)


def bench_buffer(dev, fields, capacity, n_insert, n_sample, runs, calls, label):
  from brax_amd.training.replay_buffers import UniformSamplingQueue  # pylint: disable=import-outside-toplevel
  g = torch.Generator().manual_seed(capacity)
  q = {form: UniformSamplingQueue(capacity, fields, n_sample, seed=1, device=dev)
       for form in ('fused', 'chained')}
  batch = {k: torch.randn((n_insert, w), generator=g).to(dev) for k, w in fields.items()}
  flag = {'fused': True, 'chained': False}
  for _ in range(-(-capacity // n_insert)):  # fill both, the same rows
    for form, b in q.items():
      b.insert(batch, fused=flag[form])
  same = torch.equal(q['fused'].data.view(torch.int32), q['chained'].data.view(torch.int32))
  out = {form: {k: torch.empty((n_sample, w), device=dev) for k, w in fields.items()} for form in q}
  s = {form: b.sample(fused=flag[form], out=out[form]) for form, b in q.items()}
  same_sample = all(torch.equal(s['fused'][k].view(torch.int32), s['chained'][k].view(torch.int32))
                    for k in fields)
  words = sum(fields.values())
  head = {'case': label, 'capacity': capacity, 'row_words': words, 'unit': 'us per call',
          'runs': runs, 'calls_per_region': calls}
  t = alternate({form: functools.partial(b.insert, batch, fused=flag[form]) for form, b in q.items()},
                runs, calls, dev, warmup_calls=max(calls // 4, 1))
  res = {'measure': 'insert', **head, 'rows': n_insert, 'bit_identical': same,
         'bytes_moved': 2 * n_insert * words * 4}
  res.update({k: spread(v, 1e6) for k, v in t.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  res['fused_GB_per_s'] = round(res['bytes_moved'] / res['fused']['median'] / 1e3, 1)
  emit(res)
  t = alternate({form: functools.partial(b.sample, fused=flag[form], out=out[form])
                 for form, b in q.items()}, runs, calls, dev, warmup_calls=max(calls // 4, 1))
  res = {'measure': 'sample', **head, 'rows': n_sample, 'bit_identical': same_sample,
         'bytes_moved': 2 * n_sample * words * 4}
  res.update({k: spread(v, 1e6) for k, v in t.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  res['fused_GB_per_s'] = round(res['bytes_moved'] / res['fused']['median'] / 1e3, 1)
  emit(res)


def bench_step(dev, num_envs, batch_size, updates, hidden, steps):
  from brax_amd.envs.policy import fused_supported, policy_rollout  # pylint: disable=import-outside-toplevel
  from brax_amd.training import sac_networks  # pylint: disable=import-outside-toplevel
  env = ant_env(dev, num_envs)
  # (the one SAC setup that starts on an empty queue and names its hidden sizes)
  L = sac_learner(dev, env, prefill=0, num_envs=num_envs, batch_size=batch_size,
                  grad_updates_per_step=updates,
                  network_factory=functools.partial(sac_networks.make_sac_networks,
                                                    hidden_layer_sizes=hidden))
  why = fused_supported(env, L.actor)

  def phases(fused):
    out = {}
    obs0 = L.state.obs

    def act():
      r = policy_rollout(env, L.state, L.actor, 1, seed=L.seed, offset=L._noise_offset)  # pylint: disable=protected-access
      L._noise_offset += 2 * num_envs * env.action_size  # pylint: disable=protected-access
      return r
    out['act'], (L.state, traj, extras) = timed(act, dev)
    out['normaliser'], _ = timed(lambda: L.normalizer.update(obs0), dev)
    row = {'observation': obs0, 'action': extras.action[0], 'reward': traj.reward[0],
           'discount': 1 - traj.done[0], 'next_observation': traj.obs[0],
           'truncation': traj.truncation[0]}
    out['insert'], _ = timed(lambda: L.buffer.insert(row, fused=fused), dev)
    out['sample'], sample = timed(lambda: L.buffer.sample(fused=fused), dev)
    out['updates'], _ = timed(lambda: L.update(sample), dev)
    return out
  phases(None), phases(False)  # warm-up
  rec = {None: [], False: []}
  for _ in range(steps):
    for fused in (None, False):
      rec[fused].append(phases(fused))
  both = rec[None] + rec[False]
  res = {'measure': 'sac_training_step', 'env': 'ant', 'num_envs': num_envs,
         'batch_size': batch_size, 'grad_updates_per_step': updates, 'hidden': list(hidden),
         'unit': 'ms', 'steps': steps, 'act_in_one_launch': why is None, 'chained_reason': why}
  for name in ('act', 'normaliser', 'updates'):
    res[name] = spread([r[name] for r in both], 1e3, 3)
  for name in ('insert', 'sample'):
    res[name + '_fused'] = spread([r[name] for r in rec[None]], 1e3, 3)
    res[name + '_chained'] = spread([r[name] for r in rec[False]], 1e3, 3)
  total = lambda recs: [sum(r.values()) for r in recs]  # noqa: E731
  res['step_fused'] = spread(total(rec[None]), 1e3, 3)
  res['step_chained'] = spread(total(rec[False]), 1e3, 3)
  emit(res)


def learn(dev, num_timesteps, num_evals):
  from brax_amd.training import sac, sac_networks  # pylint: disable=import-outside-toplevel
  curve = []

  def progress(step, m):
    curve.append({'env_steps': step, 'eval/episode_reward': round(float(m['eval/episode_reward']), 2),
                  'eval/avg_episode_length': round(float(m['eval/avg_episode_length']), 1)})
    emit({'measure': 'learn_progress', 'agent': 'sac', **curve[-1]})
  cfg = dict(num_envs=64, batch_size=128, grad_updates_per_step=4, min_replay_size=1024,
             max_replay_size=1 << 16, learning_rate=6e-4, discounting=0.99,
             normalize_observations=True)
  hidden = (64, 64)
  t = time.perf_counter()
  _, _, metrics = sac.train(
      'inverted_pendulum', num_timesteps=num_timesteps, episode_length=1000, num_eval_envs=128,
      seed=1, num_evals=num_evals, device=dev, progress_fn=progress,
      network_factory=functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=hidden),
      **cfg)
  emit({'measure': 'learn', 'agent': 'sac', 'env': 'inverted_pendulum', **cfg,
        'hidden': list(hidden), 'num_timesteps': num_timesteps,
        'wall_s': round(time.perf_counter() - t, 1),
        'training/sps': round(float(metrics['training/sps'])), 'curve': curve})


def main():
  ap = tool_args(__doc__, runs=7, calls=50, steps=3)
  ap.add_argument('--envs', type=int, default=SAC_ANT['num_envs'])
  ap.add_argument('--updates', type=int, default=SAC_ANT['updates'])
  ap.add_argument('--learn', action='store_true')
  ap.add_argument('--learn-timesteps', type=int, default=40_000)
  ap.add_argument('--learn-evals', type=int, default=6)
  ap.add_argument('--skip-step', action='store_true')
  a, dev = start('sac_bench', ap)
  from brax_amd.training.replay_buffers import transition_fields  # pylint: disable=import-outside-toplevel
  bench_buffer(dev, transition_fields(ANT_OBS, ANT_ACT), 1 << 20, 4096, 256 * 64, a.runs, a.calls,
               'ant')
  bench_buffer(dev, {'a': 1, 'b': 3}, 10, 2, 2, a.runs, a.calls, "the reference's buffer test")
  if not a.skip_step:
    for hidden in ((256, 256), (128, 128)):
      bench_step(dev, a.envs, SAC_ANT['batch_size'], a.updates, hidden, a.steps)
  if a.learn:
    learn(dev, a.learn_timesteps, a.learn_evals)


if __name__ == '__main__':
  main()
