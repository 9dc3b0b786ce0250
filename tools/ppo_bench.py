"""PPO learner timings on one GPU (a tool, not a test; `bench.py` is untouched).

  (a) `compute_gae`, fused (one `bx_compute_gae` launch) against chained (the
      same recurrences as separate torch operations) on the same device
      tensors: the minibatch of the Ant notebook configuration, (5, 1024), and
      the whole batch of one training step, (5, 32768). A timed region is
      `--calls` back-to-back calls ending in a device synchronise; the figure
      is microseconds per call, median (min .. max) of `--runs` regions after
      a warm-up, the two forms alternating.
  (b) one `train` training step on Ant at the notebook's hyper-parameters
      (2,048 envs, unroll 5, batch 1,024 x 32 minibatches, 8 updates per
      batch, normalised observations), split into unroll, normaliser and
      updates, each ending in a synchronise; the update phase with fused and
      with chained GAE, alternating, median (min .. max) of `--steps` steps.
  `--learn`: a longer `inverted_pendulum` run, its evaluation reward after
      every epoch.

Prints one JSON line per measurement.

    python tools/ppo_bench.py [--runs 7] [--calls 200] [--steps 3] [--learn]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from brax_amd import envs  # noqa: E402
from brax_amd.training import compute_gae, ppo  # noqa: E402

ANT = dict(num_envs=2048, unroll_length=5, batch_size=1024, num_minibatches=32,
           num_updates_per_batch=8, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97,
           reward_scaling=10.0, normalize_observations=True)


def spread(xs, scale=1.0, digits=2):
  return {'median': round(statistics.median(xs) * scale, digits),
          'min': round(min(xs) * scale, digits), 'max': round(max(xs) * scale, digits)}


def region(fn, calls, dev):
  torch.cuda.synchronize(dev)
  t = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize(dev)
  return (time.perf_counter() - t) / calls


def bench_gae(dev, T, B, runs, calls):
  g = torch.Generator().manual_seed(T * 7919 + B)
  done = (torch.rand((T, B), generator=g) < 0.1).float()
  trunc = done * (torch.rand((T, B), generator=g) < 0.5).float()
  args = [x.to(dev) for x in (trunc, done, torch.randn((T, B), generator=g),
                              torch.randn((T, B), generator=g), torch.randn((B,), generator=g))]
  kw = dict(lambda_=0.95, discount=0.97, reward_scaling=10.0)
  forms = {'fused': lambda: compute_gae(*args, fused=True, **kw),
           'chained': lambda: compute_gae(*args, fused=False, **kw)}
  a, b = forms['fused'](), forms['chained']()
  same = all(torch.equal(x, y) for x, y in zip(a, b))
  times = {k: [] for k in forms}
  for k, fn in forms.items():
    region(fn, calls, dev)  # warm-up
  for _ in range(runs):
    for k, fn in forms.items():
      times[k].append(region(fn, calls, dev))
  res = {'measure': 'compute_gae', 'shape': [T, B], 'unit': 'us per call', 'runs': runs,
         'calls_per_region': calls, 'bit_identical': same}
  res.update({k: spread(v, 1e6) for k, v in times.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  print(json.dumps(res), flush=True)


def bench_step(dev, steps):
  env = envs.create('ant', episode_length=1000, batch_size=ANT['num_envs'], device=dev)
  learner = ppo.Learner(env, device=dev, seed=0, **ANT)
  learner.reset(np.array([0, 1], np.uint32))

  def phases(fused):
    learner.fused_gae = fused
    out = {}
    for name, fn in (('unroll', learner.collect), ('normaliser', None), ('updates', None)):
      torch.cuda.synchronize(dev)
      t = time.perf_counter()
      if name == 'unroll':
        data = fn()
      elif name == 'normaliser':
        learner.update_normalizer(data)
      else:
        metrics = learner.update(data)
      torch.cuda.synchronize(dev)
      out[name] = time.perf_counter() - t
    out['total_loss'] = float(metrics['total_loss'])
    return out
  phases(None), phases(False)  # warm-up: code objects, the allocator, Adam's state
  rec = {None: [], False: []}
  for _ in range(steps):
    for fused in (None, False):
      rec[fused].append(phases(fused))
  n = ANT['num_updates_per_batch'] * ANT['num_minibatches']
  res = {'measure': 'training_step', 'env': 'ant', **ANT, 'unit': 'ms', 'steps': steps,
         'gae_calls_per_step': n,
         'env_steps_per_training_step': ANT['batch_size'] * ANT['num_minibatches'] * ANT['unroll_length']}
  both = rec[None] + rec[False]
  res['unroll'] = spread([r['unroll'] for r in both], 1e3)
  res['normaliser'] = spread([r['normaliser'] for r in both], 1e3)
  res['updates_fused_gae'] = spread([r['updates'] for r in rec[None]], 1e3)
  res['updates_chained_gae'] = spread([r['updates'] for r in rec[False]], 1e3)
  res['updates_chained_over_fused'] = round(
      res['updates_chained_gae']['median'] / res['updates_fused_gae']['median'], 3)
  res['last_total_loss'] = {'fused': rec[None][-1]['total_loss'], 'chained': rec[False][-1]['total_loss']}
  print(json.dumps(res), flush=True)


def learn(dev, num_timesteps, num_evals):
  curve = []

  def progress(step, m):
    curve.append({'env_steps': step, 'eval/episode_reward': round(float(m['eval/episode_reward']), 2),
                  'eval/avg_episode_length': round(float(m['eval/avg_episode_length']), 1)})
    print(json.dumps({'measure': 'learn_progress', **curve[-1]}), flush=True)
  t = time.perf_counter()
  _, _, metrics = ppo.train(
      'inverted_pendulum', num_timesteps=num_timesteps, episode_length=1000, num_envs=2048,
      num_eval_envs=128, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97, seed=1,
      unroll_length=5, batch_size=1024, num_minibatches=8, num_updates_per_batch=4,
      num_evals=num_evals, normalize_observations=True, reward_scaling=10.0, device=dev,
      progress_fn=progress)
  print(json.dumps({'measure': 'learn', 'env': 'inverted_pendulum', 'num_timesteps': num_timesteps,
                    'wall_s': round(time.perf_counter() - t, 1),
                    'training/sps': round(float(metrics['training/sps'])), 'curve': curve}),
        flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--calls', type=int, default=200)
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--learn', action='store_true')
  ap.add_argument('--learn-timesteps', type=int, default=2_000_000)
  ap.add_argument('--learn-evals', type=int, default=6)
  ap.add_argument('--skip-step', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('ppo_bench needs a GPU: a CPU run gives no time')
  dev = torch.device('cuda', 0)
  for T, B in ((5, 1024), (5, 32768)):
    bench_gae(dev, T, B, a.runs, a.calls)
  if not a.skip_step:
    bench_step(dev, a.steps)
  if a.learn:
    learn(dev, a.learn_timesteps, a.learn_evals)


if __name__ == '__main__':
  main()
