"""PPO loss head timings on one GPU (a tool, not a test; `bench.py` is untouched).

  head      forward plus backward of the head alone at (T, B, A) = (5, 1024, 8),
            `ppo_head(fused=True)` against the chained form on the same
            tensors, alternating. A region is `--calls` iterations ending in a
            synchronise; microseconds per iteration, median (min .. max) of
            `--runs` regions after a warm-up.
  launches  the kernel launches of one iteration of both forms, counted with
            `torch.profiler` (a run of its own: the profiler's cost is in no
            timing).
  ppo       the update phase of one Ant training step at the notebook's
            hyper-parameters (`tools/mlp_bench.py`'s), `fused_mlp=True`,
            `fused_head` on and off alternating on one learner, `--steps`
            steps each.
  split     one update phase of each form under `torch.profiler`: the kernels'
            count and device time by owner (the networks' kernels, the head,
            Adam, other torch).
  `--parent` runs ppo without naming `fused_head` at all, so the same file
  measures a tree from before the keyword existed.

Prints one JSON line per measurement.

    python tools/ppo_head_bench.py [--parts head,launches,ppo,split] [--runs 7] [--calls 100]
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from brax_amd import envs  # noqa: E402
from brax_amd.training import ppo  # noqa: E402
from brax_amd.training.losses import Transition  # noqa: E402

ANT = dict(num_envs=2048, unroll_length=5, batch_size=1024, num_minibatches=32,
           num_updates_per_batch=8, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97,
           reward_scaling=10.0, normalize_observations=True)
SHAPE = (5, 1024, 8)


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


def _forms(dev):
  from brax_amd.training import ppo_head  # pylint: disable=import-outside-toplevel
  T, B, A = SHAPE
  g = torch.Generator().manual_seed(0)
  r = lambda *s: torch.randn(s, generator=g).to(dev).transpose(0, 1)  # noqa: E731 ([B, T] views)
  flags = lambda: (torch.rand((B, T), generator=g) < 0.2).float().to(dev).transpose(0, 1)  # noqa: E731
  logits, baseline = r(B, T, 2 * A).requires_grad_(), r(B, T).requires_grad_()
  boot = torch.randn((B,), generator=g).to(dev)
  data = Transition(observation=None, action=None, reward=r(B, T), discount=1 - flags(),
                    next_observation=None, truncation=flags(), raw_action=r(B, T, A),
                    log_prob=-8 + r(B, T))
  eps = r(B, T, A)

  def step(fused):
    loss, _ = ppo_head.ppo_head(logits, baseline, boot, data, eps, entropy_cost=1e-2,
                                discounting=0.97, reward_scaling=10.0, fused=fused)
    return torch.autograd.grad(loss, [logits, baseline])
  return {'fused': functools.partial(step, True), 'chained': functools.partial(step, False)}


def bench_head(dev, runs, calls):
  forms = _forms(dev)
  times = {k: [] for k in forms}
  for fn in forms.values():
    region(fn, calls, dev)  # warm-up
  for _ in range(runs):
    for k, fn in forms.items():
      times[k].append(region(fn, calls, dev))
  res = {'measure': 'ppo_head_forward_backward', 'shape_T_B_A': list(SHAPE),
         'unit': 'us per iteration', 'runs': runs, 'calls_per_region': calls}
  res.update({k: spread(v, 1e6) for k, v in times.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  print(json.dumps(res), flush=True)


def _kernels(fn, dev, repeat=1):
  from torch.autograd import DeviceType  # pylint: disable=import-outside-toplevel
  from torch.profiler import ProfilerActivity, profile  # pylint: disable=import-outside-toplevel
  torch.cuda.synchronize(dev)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(repeat):
      fn()
    torch.cuda.synchronize(dev)
  return [e for e in prof.events() if e.device_type == DeviceType.CUDA
          and not e.name.lower().startswith(('memcpy', 'memset'))]


def count_launches(dev):
  res = {'measure': 'launches_per_iteration', 'shape_T_B_A': list(SHAPE)}
  for form, fn in _forms(dev).items():
    fn()
    kernels = _kernels(fn, dev, repeat=4)
    res[form] = len(kernels) / 4
    res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:12]
  print(json.dumps(res), flush=True)


def _timed(fn, dev):
  torch.cuda.synchronize(dev)
  t = time.perf_counter()
  r = fn()
  torch.cuda.synchronize(dev)
  return time.perf_counter() - t, r


def _learner(dev):
  env = envs.create('ant', episode_length=1000, batch_size=ANT['num_envs'], device=dev)
  learner = ppo.Learner(env, device=dev, seed=0, fused_mlp=True, **ANT)
  learner.reset(np.array([0, 1], np.uint32))
  return learner


def bench_ppo(dev, steps, parent):
  learner = _learner(dev)
  forms = ('parent',) if parent else ('fused_head', 'chained_head')

  def update(form):
    if not parent:
      learner.fused_head = form == 'fused_head'
    data = learner.collect()
    learner.update_normalizer(data)
    t, metrics = _timed(lambda: learner.update(data), dev)
    return t, float(metrics['total_loss'])
  for form in forms:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in forms}
  for _ in range(steps):
    for form in forms:
      rec[form].append(update(form))
  n = ANT['num_updates_per_batch'] * ANT['num_minibatches']
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT, 'fused_mlp': True, 'unit': 'ms',
         'steps': steps, 'adam_steps': n}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained_head']['median'] / res['fused_head']['median'], 2)
  print(json.dumps(res), flush=True)


def _owner(name):
  n = name.lower()
  if 'ppo_head' in n:
    return 'head kernels'
  if 'mlp_' in n:
    return 'network kernels'
  if 'compute_gae' in n:
    return 'gae kernel'
  if 'multi_tensor' in n or 'adam' in n:
    return 'adam'
  return 'other torch'


def split_update(dev):
  learner = _learner(dev)
  n = ANT['num_updates_per_batch'] * ANT['num_minibatches']
  for form in (True, False):
    learner.fused_head = form
    data = learner.collect()
    learner.update_normalizer(data)
    learner.update(data)  # warm-up; the second update is profiled
    kernels = _kernels(lambda: learner.update(data), dev)  # pylint: disable=cell-var-from-loop
    res = {'measure': 'ppo_update_split', 'fused_head': form, 'adam_steps': n,
           'unit': 'per Adam step: launches, device us'}
    for owner in ('network kernels', 'head kernels', 'gae kernel', 'adam', 'other torch'):
      own = [e for e in kernels if _owner(e.name) == owner]
      res[owner] = [round(len(own) / n, 1), round(sum(e.device_time for e in own) / n, 1)]
    print(json.dumps(res), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parts', default='head,launches,ppo,split')
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--calls', type=int, default=100)
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--parent', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('ppo_head_bench needs a GPU: a CPU run gives no time')
  dev = torch.device('cuda', 0)
  parts = a.parts.split(',')
  if a.parent:
    parts = [p for p in parts if p == 'ppo']
  if 'head' in parts:
    bench_head(dev, a.runs, a.calls)
  if 'launches' in parts:
    count_launches(dev)
  if 'ppo' in parts:
    bench_ppo(dev, a.steps, a.parent)
  if 'split' in parts:
    split_update(dev)


if __name__ == '__main__':
  main()
