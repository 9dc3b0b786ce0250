"""Fused optimiser step timings on one GPU (a tool, not a test; `bench.py` is untouched).

  step      the optimiser step alone on random gradients: PPO's 22 tensors
            (Ant: policy (32,) * 4, value (256,) * 5), `FusedAdam` against
            `torch.optim.Adam(foreach=True)`; SAC's 19 tensors with the 12
            targets (Ant, (256, 256)), `FusedAdam` against three foreach Adams
            plus the target loop. Forms alternate; a region is `--calls` steps
            ending in a synchronise; microseconds per step, median (min .. max)
            of `--runs` regions after a warm-up.
  launches  the kernel launches of one step of each form, counted with
            `torch.profiler` (a run of its own: the profiler's cost is in no
            timing).
  ppo       the update phase of one Ant training step at the README's
            hyper-parameters with `fused_mlp` and `fused_head` on, `fused_adam`
            on and off on two learners over one env, alternating, `--steps`
            steps each.
  sac       the 64 gradient updates of one Ant training step at 4,096 envs,
            batch 256, (256, 256), `fused_mlp` on, `fused_adam` on and off on two
            learners, alternating.
  split     one PPO update phase and one SAC update phase of each form under
            `torch.profiler`: the kernels' count and device time by owner, per
            Adam step / per gradient step.
  `--parent` runs ppo and sac without naming `fused_adam` at all, so the same
  file measures a tree from before the keyword existed.

Prints one JSON line per measurement.

    python tools/optim_bench.py [--parts step,launches,ppo,sac,split] [--runs 7] [--calls 100]
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
from brax_amd.envs import wrappers  # noqa: E402
from brax_amd.training import networks, ppo, sac, sac_networks  # noqa: E402

ANT = dict(num_envs=2048, unroll_length=5, batch_size=1024, num_minibatches=32,
           num_updates_per_batch=8, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97,
           reward_scaling=10.0, normalize_observations=True)
SAC = dict(num_envs=4096, batch_size=256, updates=64)
ANT_OBS, ANT_ACT = 87, 8
TAU = 0.005


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


def _ppo_forms(dev):
  from brax_amd.training import optim  # pylint: disable=import-outside-toplevel
  make = lambda: networks.parameters(  # noqa: E731
      *networks.make_ppo_networks(ANT_OBS, ANT_ACT, seed=0, device=dev))
  a, b = make(), make()
  grads = [torch.randn_like(p) for p in a]
  fused = optim.FusedAdam([dict(params=a, lr=3e-4)])
  adam = torch.optim.Adam(b, lr=3e-4, eps=1e-8, foreach=True)
  for p, g in zip(b, grads):
    p.grad = g
  return {'fused': lambda: fused.step(grads), 'torch': adam.step}, sum(p.numel() for p in a)


def _sac_forms(dev):
  from brax_amd.training import optim  # pylint: disable=import-outside-toplevel

  def make():
    policy, q = sac_networks.make_sac_networks(ANT_OBS, ANT_ACT, seed=0, device=dev)
    target = [[(w.detach().clone(), b.detach().clone()) for w, b in c] for c in q]
    alpha = torch.zeros((), device=dev, requires_grad=True)
    return [alpha], sac_networks.q_parameters(q), networks.parameters(policy), \
        sac_networks.q_parameters(target)
  (a1, q1, p1, t1), (a2, q2, p2, t2) = make(), make()
  grads = [torch.randn_like(p) for p in a1 + q1 + p1]
  fused = optim.FusedAdam([dict(params=a1, lr=3e-4), dict(params=q1, lr=6e-4, targets=t1, tau=TAU),
                           dict(params=p1, lr=6e-4)])
  adams = [torch.optim.Adam(ps, lr=lr, eps=1e-8, foreach=True)
           for ps, lr in ((a2, 3e-4), (q2, 6e-4), (p2, 6e-4))]
  for p, g in zip(a2 + q2 + p2, grads):
    p.grad = g

  def torch_step():
    for o in adams:
      o.step()
    with torch.no_grad():
      for t, q in zip(t2, q2):
        t.copy_(t * (1 - TAU) + q * TAU)
  return {'fused': lambda: fused.step(grads), 'torch': torch_step}, sum(p.numel() for p in a1 + q1 + p1)


def bench_step(dev, runs, calls):
  for name, (forms, n) in (('ppo_22_tensors', _ppo_forms(dev)),
                           ('sac_19_tensors_12_targets', _sac_forms(dev))):
    times = {k: [] for k in forms}
    for fn in forms.values():
      region(fn, calls, dev)  # warm-up
    for _ in range(runs):
      for k, fn in forms.items():
        times[k].append(region(fn, calls, dev))
    res = {'measure': 'optimiser_step', 'case': name, 'parameters': n, 'unit': 'us per step',
           'runs': runs, 'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['torch_over_fused'] = round(res['torch']['median'] / res['fused']['median'], 2)
    print(json.dumps(res), flush=True)


def _kernels(fn, dev, repeat=1):
  from torch.autograd import DeviceType  # pylint: disable=import-outside-toplevel
  from torch.profiler import ProfilerActivity, profile  # pylint: disable=import-outside-toplevel
  torch.cuda.synchronize(dev)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(repeat):
      fn()
    torch.cuda.synchronize(dev)
  # (the profiler also reports `Optimizer.step#...` ranges as device events:
  # they are spans over the kernels below them, not launches)
  return [e for e in prof.events() if e.device_type == DeviceType.CUDA
          and not e.name.lower().startswith(('memcpy', 'memset', 'optimizer.'))]


def count_launches(dev):
  for name, (forms, _) in (('ppo_22_tensors', _ppo_forms(dev)),
                           ('sac_19_tensors_12_targets', _sac_forms(dev))):
    res = {'measure': 'launches_per_step', 'case': name}
    for form, fn in forms.items():
      fn()
      kernels = _kernels(fn, dev, repeat=4)
      res[form] = len(kernels) / 4
      res[form + '_device_us'] = round(sum(e.device_time for e in kernels) / 4, 1)
      res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:8]
    print(json.dumps(res), flush=True)


def _timed(fn, dev):
  torch.cuda.synchronize(dev)
  t = time.perf_counter()
  r = fn()
  torch.cuda.synchronize(dev)
  return time.perf_counter() - t, r


def _ppo_learners(dev, parent):
  env = envs.create('ant', episode_length=1000, batch_size=ANT['num_envs'], device=dev)
  forms = {'parent': {}} if parent else {'fused_adam': dict(fused_adam=True),
                                         'torch_adam': dict(fused_adam=False)}
  out = {}
  for form, kw in forms.items():
    out[form] = ppo.Learner(env, device=dev, seed=0, fused_mlp=True, fused_head=True, **ANT, **kw)
    out[form].reset(np.array([0, 1], np.uint32))
  return out


def bench_ppo(dev, steps, parent):
  learners = _ppo_learners(dev, parent)

  def update(form):
    learner = learners[form]
    data = learner.collect()
    learner.update_normalizer(data)
    t, metrics = _timed(lambda: learner.update(data), dev)
    return t, float(metrics['total_loss'])
  for form in learners:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  n = ANT['num_updates_per_batch'] * ANT['num_minibatches']
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT, 'fused_mlp': True, 'fused_head': True,
         'unit': 'ms', 'steps': steps, 'adam_steps': n}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['torch_over_fused'] = round(res['torch_adam']['median'] / res['fused_adam']['median'], 2)
  print(json.dumps(res), flush=True)


def _sac_learners(dev, parent):
  env = envs.create('ant', episode_length=1000, batch_size=SAC['num_envs'], device=dev)
  forms = {'parent': {}} if parent else {'fused_adam': dict(fused_adam=True),
                                         'torch_adam': dict(fused_adam=False)}
  out = {}
  for form, kw in forms.items():
    L = sac.Learner(env, SAC['num_envs'], batch_size=SAC['batch_size'],
                    grad_updates_per_step=SAC['updates'], max_replay_size=1 << 20,
                    normalize_observations=True, seed=0, fused_mlp=True,
                    network_factory=sac_networks.make_sac_networks, device=dev, **kw)
    L.reset(wrappers.split_key(np.array([0, 0], np.uint32))[0])
    for _ in range(4):
      L.get_experience()
    out[form] = L
  return out


def bench_sac(dev, steps, parent):
  learners = _sac_learners(dev, parent)

  def update(form):
    L = learners[form]
    L.get_experience()
    sample = L.buffer.sample()
    t, metrics = _timed(lambda: L.update(sample), dev)
    return t, float(metrics['critic_loss'])
  for form in learners:
    update(form)
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  res = {'measure': 'sac_gradient_updates', 'env': 'ant', **SAC, 'hidden': [256, 256],
         'fused_mlp': True, 'unit': 'ms', 'steps': steps}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / SAC['updates'], 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    res['torch_over_fused'] = round(res['torch_adam']['median'] / res['fused_adam']['median'], 2)
  print(json.dumps(res), flush=True)


OWNERS = ('network kernels', 'head kernels', 'optimiser', 'other torch')


def _owner(name):
  n = name.lower()
  if 'ppo_head' in n:
    return 'head kernels'
  if 'mlp_' in n:
    return 'network kernels'
  if 'multi_tensor' in n or 'adam' in n:
    return 'optimiser'
  return 'other torch'


def _split(kernels, n):
  res = {}
  for owner in OWNERS:
    own = [e for e in kernels if _owner(e.name) == owner]
    res[owner] = [round(len(own) / n, 1), round(sum(e.device_time for e in own) / n, 1)]
  res['all'] = [round(len(kernels) / n, 1), round(sum(e.device_time for e in kernels) / n, 1)]
  return res


def split_updates(dev):
  """(the SAC target loop's launches are elementwise torch kernels and count
  under 'other torch' in the torch form)"""
  n = ANT['num_updates_per_batch'] * ANT['num_minibatches']
  for form, learner in _ppo_learners(dev, False).items():
    data = learner.collect()
    learner.update_normalizer(data)
    learner.update(data)  # warm-up; the second update is profiled
    kernels = _kernels(lambda: learner.update(data), dev)  # pylint: disable=cell-var-from-loop
    print(json.dumps({'measure': 'ppo_update_split', 'form': form, 'adam_steps': n,
                      'unit': 'per Adam step: launches, device us', **_split(kernels, n)}),
          flush=True)
  for form, L in _sac_learners(dev, False).items():
    L.get_experience()
    sample = L.buffer.sample()
    L.update(sample)
    kernels = _kernels(lambda: L.update(sample), dev)  # pylint: disable=cell-var-from-loop
    print(json.dumps({'measure': 'sac_update_split', 'form': form, 'gradient_steps': SAC['updates'],
                      'unit': 'per gradient step: launches, device us',
                      **_split(kernels, SAC['updates'])}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parts', default='step,launches,ppo,sac,split')
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--calls', type=int, default=100)
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--parent', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('optim_bench needs a GPU: a CPU run gives no time')
  dev = torch.device('cuda', 0)
  parts = a.parts.split(',')
  if a.parent:
    parts = [p for p in parts if p in ('ppo', 'sac')]
  if 'step' in parts:
    bench_step(dev, a.runs, a.calls)
  if 'launches' in parts:
    count_launches(dev)
  if 'ppo' in parts:
    bench_ppo(dev, a.steps, a.parent)
  if 'sac' in parts:
    bench_sac(dev, a.steps, a.parent)
  if 'split' in parts:
    split_updates(dev)


if __name__ == '__main__':
  main()
