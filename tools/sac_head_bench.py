"""SAC loss head timings on one GPU (a tool, not a test; `bench.py` is untouched).

  head      the three gradients of one SAC step at Ant's sizes (B 256 and 512,
            O 87, A 8, C 2, (256, 256), `fused_mlp` on): `sac_losses` and
            autograd against `sac_head.gradients`. The networks run in both
            forms (the chained losses cannot be taken without them), so the
            launches are counted by owner with `torch.profiler` in a run of its
            own; the times are microseconds per call, median (min .. max) of
            `--runs` regions of `--calls` calls, forms alternating.
  sac       the 64 gradient updates of one Ant training step at 4,096 envs,
            batch 256, (256, 256), `fused_mlp` and `fused_adam` on, `fused_head`
            on and off on two learners, alternating, `--steps` steps each.
  split     one such update phase of each form under `torch.profiler`: the
            kernels' count and device time by owner per gradient step, and the
            names of what is left under 'other torch' in the fused form.
  `--parent` runs sac without naming `fused_head` at all, so the same file
  measures a tree from before the keyword existed; `--root` names the tree
  whose package is imported (default: this file's).

Prints one JSON line per measurement.

    python tools/sac_head_bench.py [--parts head,sac,split] [--runs 7] [--calls 50]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

SAC = dict(num_envs=4096, batch_size=256, updates=64)
ANT_OBS, ANT_ACT = 87, 8
OWNERS = ('network kernels', 'head kernels', 'optimiser', 'other torch')


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


def _kernels(fn, dev, repeat=1):
  from torch.autograd import DeviceType  # pylint: disable=import-outside-toplevel
  from torch.profiler import ProfilerActivity, profile  # pylint: disable=import-outside-toplevel
  torch.cuda.synchronize(dev)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(repeat):
      fn()
    torch.cuda.synchronize(dev)
  return [e for e in prof.events() if e.device_type == DeviceType.CUDA
          and not e.name.lower().startswith(('memcpy', 'memset', 'optimizer.'))]


def _owner(name):
  n = name.lower()
  if 'sac_head' in n:
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


def bench_head(dev, runs, calls):
  from brax_amd.training import sac, sac_head  # pylint: disable=import-outside-toplevel
  for B in (256, 512):
    ts = sac.init_training_state(ANT_OBS, ANT_ACT, seed=0, device=dev)
    r = lambda *s: torch.randn(s, device=dev)  # noqa: E731
    trans = {'observation': r(B, ANT_OBS), 'action': torch.tanh(r(B, ANT_ACT)), 'reward': r(B),
             'discount': torch.ones(B, device=dev), 'next_observation': r(B, ANT_OBS),
             'truncation': torch.zeros(B, device=dev)}
    normalizer = (r(ANT_OBS), 0.5 + torch.rand(ANT_OBS, device=dev))
    eps = (r(B, ANT_ACT), r(B, ANT_ACT), r(B, ANT_ACT))
    args = (ts, normalizer, trans, eps, 30.0, 0.997, True)
    forms = {'chained': lambda: sac._chained_gradients(*args),  # pylint: disable=protected-access
             'fused': lambda: sac_head.gradients(*args)}
    times = {k: [] for k in forms}
    for fn in forms.values():
      region(fn, calls, dev)  # warm-up
    for _ in range(runs):
      for k, fn in forms.items():
        times[k].append(region(fn, calls, dev))
    res = {'measure': 'sac_gradients', 'B': B, 'O': ANT_OBS, 'A': ANT_ACT, 'C': 2,
           'hidden': [256, 256], 'fused_mlp': True, 'unit': 'us per call', 'runs': runs,
           'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
    print(json.dumps(res), flush=True)
    for form, fn in forms.items():
      kernels = _kernels(fn, dev, repeat=4)
      print(json.dumps({'measure': 'sac_gradients_launches', 'B': B, 'form': form,
                        'unit': 'per call: launches, device us', **_split(kernels, 4)}), flush=True)


def _learners(dev, parent):
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  from brax_amd.envs import wrappers  # pylint: disable=import-outside-toplevel
  from brax_amd.training import sac, sac_networks  # pylint: disable=import-outside-toplevel
  env = envs.create('ant', episode_length=1000, batch_size=SAC['num_envs'], device=dev)
  forms = {'parent': {}} if parent else {'fused_head': dict(fused_head=True),
                                         'chained_head': dict(fused_head=False)}
  out = {}
  for form, kw in forms.items():
    L = sac.Learner(env, SAC['num_envs'], batch_size=SAC['batch_size'],
                    grad_updates_per_step=SAC['updates'], max_replay_size=1 << 20,
                    learning_rate=6e-4, discounting=0.997, reward_scaling=30.0,
                    normalize_observations=True, seed=0, fused_mlp=True, fused_adam=True,
                    network_factory=sac_networks.make_sac_networks, device=dev, **kw)
    L.reset(wrappers.split_key(np.array([0, 0], np.uint32))[0])
    for _ in range(4):
      L.get_experience()
    out[form] = L
  return out


def bench_sac(dev, steps, parent):
  learners = _learners(dev, parent)

  def update(form):
    L = learners[form]
    L.get_experience()
    sample = L.buffer.sample()
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    metrics = L.update(sample)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, float(metrics['critic_loss'])
  for form in learners:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  res = {'measure': 'sac_gradient_updates', 'env': 'ant', **SAC, 'hidden': [256, 256],
         'fused_mlp': True, 'fused_adam': True, 'unit': 'ms', 'steps': steps}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / SAC['updates'], 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained_head']['median'] / res['fused_head']['median'], 2)
  print(json.dumps(res), flush=True)


def split_updates(dev):
  for form, L in _learners(dev, False).items():
    L.get_experience()
    sample = L.buffer.sample()
    L.update(sample)  # warm-up; the second update is profiled
    kernels = _kernels(lambda: L.update(sample), dev)  # pylint: disable=cell-var-from-loop
    res = {'measure': 'sac_update_split', 'form': form, 'gradient_steps': SAC['updates'],
           'unit': 'per gradient step: launches, device us', **_split(kernels, SAC['updates'])}
    if form == 'fused_head':
      other = collections.Counter(e.name[:70] for e in kernels if _owner(e.name) == 'other torch')
      res['other_torch_per_step'] = {k: round(v / SAC['updates'], 2) for k, v in other.most_common()}
      head = collections.Counter(e.name[:50] for e in kernels if _owner(e.name) == 'head kernels')
      res['head_kernels_per_step'] = {k: round(v / SAC['updates'], 2) for k, v in head.items()}
    print(json.dumps(res), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parts', default='head,sac,split')
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--calls', type=int, default=50)
  ap.add_argument('--steps', type=int, default=5)
  ap.add_argument('--parent', action='store_true')
  ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  a = ap.parse_args()
  sys.path.insert(0, os.path.abspath(a.root))
  if not torch.cuda.is_available():
    sys.exit('sac_head_bench needs a GPU: a CPU run gives no time')
  dev = torch.device('cuda', 0)
  parts = a.parts.split(',')
  if a.parent:
    parts = [p for p in parts if p == 'sac']
  if 'head' in parts:
    bench_head(dev, a.runs, a.calls)
  if 'sac' in parts:
    bench_sac(dev, a.steps, a.parent)
  if 'split' in parts:
    split_updates(dev)


if __name__ == '__main__':
  main()
