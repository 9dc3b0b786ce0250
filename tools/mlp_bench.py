"""Fused MLP timings on one GPU (a tool, not a test; `bench.py` is untouched).

  mlp       forward plus backward of one network, `fused_mlp` against chained
            autograd on the same tensors, alternating: the PPO value net 87 ->
            (256,) * 5 -> 1 at 6,144 rows, the PPO policy net 87 -> (32,) * 4
            -> 16 at 5,120 rows, a SAC critic 95 -> 256 -> 256 -> 1 at 512
            rows. A region is `--calls` iterations ending in a synchronise;
            microseconds per iteration, median (min .. max) of `--runs`
            regions after a warm-up.
  launches  the kernel launches of one iteration of both forms, counted with
            `torch.profiler` (a run of its own: the profiler's cost is in no
            timing).
  ppo       the update phase of one Ant training step at the notebook's
            hyper-parameters (`tools/ppo_bench.py`'s), `fused_mlp` on and off
            alternating on one learner, `--steps` steps each.
  sac       the gradient updates of one Ant SAC step (`tools/sac_bench.py`'s
            setting: 4,096 envs, batch 256, 64 updates, (256, 256)), likewise.
  `--parent` runs ppo and sac without naming `fused_mlp` at all, so the same
  file measures a tree from before the keyword existed.

Prints one JSON line per measurement.

    python tools/mlp_bench.py [--parts mlp,launches,ppo,sac] [--runs 7] [--calls 100] [--steps 3]
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
from brax_amd.envs import wrappers  # noqa: E402
from brax_amd.training import networks, ppo, sac, sac_networks  # noqa: E402

ANT = dict(num_envs=2048, unroll_length=5, batch_size=1024, num_minibatches=32,
           num_updates_per_batch=8, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97,
           reward_scaling=10.0, normalize_observations=True)
NETS = (('ppo value', (87,) + (256,) * 5 + (1,), 6144, 'swish'),
        ('ppo policy', (87,) + (32,) * 4 + (16,), 5120, 'swish'),
        ('sac critic', (95, 256, 256, 1), 512, 'relu'))


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


def _forms(sizes, rows, activation, dev):
  g = torch.Generator().manual_seed(rows)
  layers = networks.make_layers(sizes, g, device=dev)
  params = networks.parameters(layers)
  x = torch.randn((rows, sizes[0]), generator=g).to(dev)
  dy = torch.randn((rows, sizes[-1]), generator=g).to(dev)

  def step(fused):
    y = networks.mlp(layers, x, activation, fused=fused)
    return torch.autograd.grad((y * dy).sum(), params)
  return {'fused': functools.partial(step, True), 'chained': functools.partial(step, False)}


def bench_mlp(dev, runs, calls):
  for name, sizes, rows, activation in NETS:
    forms = _forms(sizes, rows, activation, dev)
    times = {k: [] for k in forms}
    for fn in forms.values():
      region(fn, calls, dev)  # warm-up
    for _ in range(runs):
      for k, fn in forms.items():
        times[k].append(region(fn, calls, dev))
    flop = 6 * rows * sum(i * o for i, o in zip(sizes[:-1], sizes[1:]))
    res = {'measure': 'mlp_forward_backward', 'net': name, 'sizes': list(sizes), 'rows': rows,
           'activation': activation, 'unit': 'us per iteration', 'runs': runs,
           'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
    res['fused_TFLOP_per_s'] = round(flop / res['fused']['median'] / 1e6, 2)
    print(json.dumps(res), flush=True)


def count_launches(dev):
  from torch.autograd import DeviceType  # pylint: disable=import-outside-toplevel
  from torch.profiler import ProfilerActivity, profile  # pylint: disable=import-outside-toplevel
  for name, sizes, rows, activation in NETS:
    res = {'measure': 'launches_per_iteration', 'net': name}
    for form, fn in _forms(sizes, rows, activation, dev).items():
      fn()
      torch.cuda.synchronize(dev)
      with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(4):
          fn()
        torch.cuda.synchronize(dev)
      kernels = [e for e in prof.events() if e.device_type == DeviceType.CUDA
                 and not e.name.lower().startswith(('memcpy', 'memset'))]
      res[form] = len(kernels) / 4
      res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:12]
    print(json.dumps(res), flush=True)


def _timed(fn, dev):
  torch.cuda.synchronize(dev)
  t = time.perf_counter()
  r = fn()
  torch.cuda.synchronize(dev)
  return time.perf_counter() - t, r


def bench_ppo(dev, steps, parent):
  env = envs.create('ant', episode_length=1000, batch_size=ANT['num_envs'], device=dev)
  learner = ppo.Learner(env, device=dev, seed=0, **ANT)
  learner.reset(np.array([0, 1], np.uint32))
  forms = ('parent',) if parent else ('fused', 'chained')

  def update(form):
    if not parent:
      learner.fused_mlp = form == 'fused'
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
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT, 'unit': 'ms', 'steps': steps,
         'adam_steps': n}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  print(json.dumps(res), flush=True)


def bench_sac(dev, steps, parent, num_envs=4096, batch_size=256, updates=64):
  env = envs.create('ant', episode_length=1000, batch_size=num_envs, device=dev)
  L = sac.Learner(env, num_envs, batch_size=batch_size, grad_updates_per_step=updates,
                  max_replay_size=1 << 20, normalize_observations=True, seed=0,
                  network_factory=sac_networks.make_sac_networks, device=dev)
  L.reset(wrappers.split_key(np.array([0, 0], np.uint32))[0])
  forms = ('parent',) if parent else ('fused', 'chained')

  def update(form):
    if not parent:
      L.fused_mlp = form == 'fused'
    L.get_experience()
    sample = L.buffer.sample()
    t, metrics = _timed(lambda: L.update(sample), dev)
    return t, float(metrics['critic_loss'])
  for _ in range(4):
    L.get_experience()
  for form in forms:
    update(form)
  rec = {form: [] for form in forms}
  for _ in range(steps):
    for form in forms:
      rec[form].append(update(form))
  res = {'measure': 'sac_gradient_updates', 'env': 'ant', 'num_envs': num_envs,
         'batch_size': batch_size, 'grad_updates_per_step': updates, 'hidden': [256, 256],
         'unit': 'ms', 'steps': steps}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / updates, 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  print(json.dumps(res), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parts', default='mlp,launches,ppo,sac')
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--calls', type=int, default=100)
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--parent', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('mlp_bench needs a GPU: a CPU run gives no time')
  dev = torch.device('cuda', 0)
  parts = a.parts.split(',')
  if a.parent:
    parts = [p for p in parts if p in ('ppo', 'sac')]
  if 'mlp' in parts:
    bench_mlp(dev, a.runs, a.calls)
  if 'launches' in parts:
    count_launches(dev)
  if 'ppo' in parts:
    bench_ppo(dev, a.steps, a.parent)
  if 'sac' in parts:
    bench_sac(dev, a.steps, a.parent)


if __name__ == '__main__':
  main()
