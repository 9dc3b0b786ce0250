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
  `--group`: only the update phase of such a step with every switch on
      (`fused_mlp`, `fused_head`, `fused_adam`), `fused_group` on and off on
      one learner, alternating; with `--parent` the same learner with
      `fused_group` not named (a tree from before the keyword).
  `--learn`: a longer `inverted_pendulum` run, its evaluation reward after
      every epoch.

Prints one JSON line per measurement.

    python tools/ppo_bench.py [--runs 7] [--calls 200] [--steps 3] [--learn]
    python tools/ppo_bench.py --group [--parent] [--steps 7]
"""
import time

import torch

from measure import ANT_PPO, alternate, emit, ppo_learner, spread, start, timed, tool_args


def bench_gae(dev, T, B, runs, calls):
  from brax_amd.training import compute_gae  # pylint: disable=import-outside-toplevel
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
  times = alternate(forms, runs, calls, dev)
  res = {'measure': 'compute_gae', 'shape': [T, B], 'unit': 'us per call', 'runs': runs,
         'calls_per_region': calls, 'bit_identical': same}
  res.update({k: spread(v, 1e6) for k, v in times.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  emit(res)


def bench_step(dev, steps):
  learner = ppo_learner(dev)

  def phases(fused):
    learner.fused_gae = fused
    out = {}
    out['unroll'], data = timed(learner.collect, dev)
    out['normaliser'], _ = timed(lambda: learner.update_normalizer(data), dev)
    out['updates'], metrics = timed(lambda: learner.update(data), dev)
    out['total_loss'] = float(metrics['total_loss'])
    return out
  phases(None), phases(False)  # warm-up: code objects, the allocator, Adam's state
  rec = {None: [], False: []}
  for _ in range(steps):
    for fused in (None, False):
      rec[fused].append(phases(fused))
  n = ANT_PPO['num_updates_per_batch'] * ANT_PPO['num_minibatches']
  res = {'measure': 'training_step', 'env': 'ant', **ANT_PPO, 'unit': 'ms', 'steps': steps,
         'gae_calls_per_step': n,
         'env_steps_per_training_step':
             ANT_PPO['batch_size'] * ANT_PPO['num_minibatches'] * ANT_PPO['unroll_length']}
  both = rec[None] + rec[False]
  res['unroll'] = spread([r['unroll'] for r in both], 1e3)
  res['normaliser'] = spread([r['normaliser'] for r in both], 1e3)
  res['updates_fused_gae'] = spread([r['updates'] for r in rec[None]], 1e3)
  res['updates_chained_gae'] = spread([r['updates'] for r in rec[False]], 1e3)
  res['updates_chained_over_fused'] = round(
      res['updates_chained_gae']['median'] / res['updates_fused_gae']['median'], 3)
  res['last_total_loss'] = {'fused': rec[None][-1]['total_loss'], 'chained': rec[False][-1]['total_loss']}
  emit(res)


def bench_group(dev, steps, parent):
  learner = ppo_learner(dev, fused_mlp=True, fused_head=True, fused_adam=True)
  forms = {'parent': None} if parent else {'grouped': True, 'ungrouped': False}

  def update(form):
    if not parent:
      learner.fused_group = forms[form]
    data = learner.collect()
    learner.update_normalizer(data)
    t, metrics = timed(lambda: learner.update(data), dev)
    return t, float(metrics['total_loss'])
  for form in forms:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in forms}
  for _ in range(steps):
    for form in forms:
      rec[form].append(update(form))
  n = ANT_PPO['num_updates_per_batch'] * ANT_PPO['num_minibatches']
  res = {'measure': 'ppo_update_phase_grouped', 'env': 'ant', **ANT_PPO, 'fused_mlp': True,
         'fused_head': True, 'fused_adam': True, 'unit': 'ms', 'steps': steps, 'adam_steps': n}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['ungrouped_over_grouped'] = round(res['ungrouped']['median'] / res['grouped']['median'], 3)
  emit(res)


def learn(dev, num_timesteps, num_evals):
  from brax_amd.training import ppo  # pylint: disable=import-outside-toplevel
  curve = []

  def progress(step, m):
    curve.append({'env_steps': step, 'eval/episode_reward': round(float(m['eval/episode_reward']), 2),
                  'eval/avg_episode_length': round(float(m['eval/avg_episode_length']), 1)})
    emit({'measure': 'learn_progress', **curve[-1]})
  t = time.perf_counter()
  _, _, metrics = ppo.train(
      'inverted_pendulum', num_timesteps=num_timesteps, episode_length=1000, num_envs=2048,
      num_eval_envs=128, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97, seed=1,
      unroll_length=5, batch_size=1024, num_minibatches=8, num_updates_per_batch=4,
      num_evals=num_evals, normalize_observations=True, reward_scaling=10.0, device=dev,
      progress_fn=progress)
  emit({'measure': 'learn', 'env': 'inverted_pendulum', 'num_timesteps': num_timesteps,
        'wall_s': round(time.perf_counter() - t, 1),
        'training/sps': round(float(metrics['training/sps'])), 'curve': curve})


def main():
  ap = tool_args(__doc__, runs=7, calls=200, steps=3)
  ap.add_argument('--learn', action='store_true')
  ap.add_argument('--learn-timesteps', type=int, default=2_000_000)
  ap.add_argument('--learn-evals', type=int, default=6)
  ap.add_argument('--skip-step', action='store_true')
  ap.add_argument('--group', action='store_true', help='the update phase, fused_group on and off')
  ap.add_argument('--parent', action='store_true', help='with --group: fused_group not named')
  a, dev = start('ppo_bench', ap)
  if a.group:
    bench_group(dev, a.steps, a.parent)
    return
  for T, B in ((5, 1024), (5, 32768)):
    bench_gae(dev, T, B, a.runs, a.calls)
  if not a.skip_step:
    bench_step(dev, a.steps)
  if a.learn:
    learn(dev, a.learn_timesteps, a.learn_evals)


if __name__ == '__main__':
  main()
