"""What the `*_bench.py` tools share: one timing method, one copy of each
benchmarked setup and one way to point a tool at a tree.

The tools import this module as a sibling (a script's directory is on
`sys.path`). It imports `torch` but never `brax_amd` at module level:
`use_tree` has to run first, so that `--root` decides whose package is
measured. Everything that touches `brax_amd` imports it inside the function.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

TOOLS_TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The Ant setups the README quotes and every learner tool measures.
ANT_OBS, ANT_ACT = 87, 8
ANT_PPO = dict(num_envs=2048, unroll_length=5, batch_size=1024, num_minibatches=32,
               num_updates_per_batch=8, learning_rate=3e-4, entropy_cost=1e-2, discounting=0.97,
               reward_scaling=10.0, normalize_observations=True)
SAC_ANT = dict(num_envs=4096, batch_size=256, updates=64)


# ---- timing ----------------------------------------------------------------


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


def timed(fn, dev):
  """(seconds, result) of one call, a synchronise on either side."""
  torch.cuda.synchronize(dev)
  t = time.perf_counter()
  r = fn()
  torch.cuda.synchronize(dev)
  return time.perf_counter() - t, r


def alternate(forms, runs, calls, dev, warmup_calls=None):
  """Seconds per call of each form: one warm-up region per form (of `calls`
  calls unless `warmup_calls` says otherwise), then `runs` rounds over the
  forms in dict order, so that a drift of the machine lands on all of them."""
  times = {k: [] for k in forms}
  for fn in forms.values():
    region(fn, calls if warmup_calls is None else warmup_calls, dev)  # warm-up
  for _ in range(runs):
    for k, fn in forms.items():
      times[k].append(region(fn, calls, dev))
  return times


def regions(fn, n, calls, dev, warmup=0):
  """Seconds per call of `n` regions of `calls` calls of one function, after
  `warmup` untimed calls (the rollout tools' loop: the state carries over)."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize(dev)
  return [region(fn, calls, dev) for _ in range(n)]


# ---- the profiler's view ---------------------------------------------------


def device_kernels(fn, dev, repeat=1, skip=('memcpy', 'memset', 'optimizer.')):
  """The kernel launches of `repeat` calls as `torch.profiler` device events,
  those whose lower-cased name starts with one of `skip` left out."""
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
          and not e.name.lower().startswith(skip)]


def owner_of(name, owners):
  """`owners` is ((substring or substrings, owner), ..., fall-through owner);
  a lower-cased kernel name goes to the first entry it matches."""
  n = name.lower()
  for needles, owner in owners[:-1]:
    if any(s in n for s in ((needles,) if isinstance(needles, str) else needles)):
      return owner
  return owners[-1]


def split_by_owner(kernels, n, owners):
  """{owner: [launches / n, device us / n]}, the owners in the table's order."""
  res = {}
  for owner in [o for _, o in owners[:-1]] + [owners[-1]]:
    own = [e for e in kernels if owner_of(e.name, owners) == owner]
    res[owner] = [round(len(own) / n, 1), round(sum(e.device_time for e in own) / n, 1)]
  return res


def all_kernels(kernels, n):
  return [round(len(kernels) / n, 1), round(sum(e.device_time for e in kernels) / n, 1)]


# ---- a tool's frame --------------------------------------------------------


def emit(record):
  print(json.dumps(record), flush=True)


def require_gpu(tool):
  if not torch.cuda.is_available():
    sys.exit(f'{tool} needs a GPU: a CPU run gives no time')


def use_tree(root):
  """Put `root` first on `sys.path`, so that `brax_amd` comes from that tree."""
  if 'brax_amd' in sys.modules:
    raise RuntimeError('use_tree after brax_amd was imported: the tree is already chosen')
  sys.path.insert(0, os.path.abspath(root))


def tool_args(doc, runs=None, calls=None, steps=None, parts=None):
  """The parser a tool starts from; it adds its own arguments and hands the
  parser to `start`. `--root` always; `--runs`, `--calls` and `--steps` where
  the tool has a default for them; `--parts` and `--parent` where it has parts."""
  ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
  for name, default in (('--runs', runs), ('--calls', calls), ('--steps', steps)):
    if default is not None:
      ap.add_argument(name, type=int, default=default)
  if parts is not None:
    ap.add_argument('--parts', default=parts)
    ap.add_argument('--parent', action='store_true',
                    help='only the parts an older tree has, its newer keyword not named')
  ap.add_argument('--root', default=TOOLS_TREE,
                  help="the tree whose brax_amd is measured (default: this file's)")
  return ap


def start(tool, ap):
  """(arguments, device) once the GPU is there and the tree is chosen."""
  a = ap.parse_args()
  require_gpu(tool)
  use_tree(a.root)
  return a, torch.device('cuda', 0)


def parts_of(a, in_parent):
  parts = a.parts.split(',')
  return [p for p in parts if p in in_parent] if a.parent else parts


# ---- the learners over the setups ------------------------------------------


def ant_env(dev, num_envs):
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  return envs.create('ant', episode_length=1000, batch_size=num_envs, device=dev)


def ppo_learner(dev, env=None, **switches):
  """A reset PPO learner at `ANT_PPO`; `switches` are the `fused_*` keywords
  (an older tree is measured by naming none it does not have)."""
  from brax_amd.training import ppo  # pylint: disable=import-outside-toplevel
  env = env or ant_env(dev, ANT_PPO['num_envs'])
  learner = ppo.Learner(env, device=dev, seed=0, **ANT_PPO, **switches)
  learner.reset(np.array([0, 1], np.uint32))
  return learner


def sac_learner(dev, env=None, prefill=4, **overrides):
  """A reset SAC learner at `SAC_ANT` after `prefill` experience steps;
  `overrides` are `sac.Learner` keywords: the `fused_*` switches and whatever
  one tool sets differently from the others."""
  from brax_amd.envs import wrappers  # pylint: disable=import-outside-toplevel
  from brax_amd.training import sac  # pylint: disable=import-outside-toplevel
  env = env or ant_env(dev, SAC_ANT['num_envs'])
  kw = dict(num_envs=SAC_ANT['num_envs'], batch_size=SAC_ANT['batch_size'],
            grad_updates_per_step=SAC_ANT['updates'], max_replay_size=1 << 20,
            normalize_observations=True, seed=0, device=dev)
  kw.update(overrides)
  L = sac.Learner(env, **kw)
  L.reset(wrappers.split_key(np.array([0, 0], np.uint32))[0])
  for _ in range(prefill):
    L.get_experience()
  return L
