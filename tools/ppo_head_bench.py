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
import functools

import torch

from measure import (ANT_PPO, alternate, device_kernels, emit, parts_of, ppo_learner, split_by_owner,
                     spread, start, timed, tool_args)

SHAPE = (5, 1024, 8)
OWNERS = (('ppo_head', 'head kernels'), ('mlp_', 'network kernels'), ('compute_gae', 'gae kernel'),
          (('multi_tensor', 'adam'), 'adam'), 'other torch')


def _forms(dev):
  from brax_amd.training import ppo_head  # pylint: disable=import-outside-toplevel
  from brax_amd.training.losses import Transition  # pylint: disable=import-outside-toplevel
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
  times = alternate(_forms(dev), runs, calls, dev)
  res = {'measure': 'ppo_head_forward_backward', 'shape_T_B_A': list(SHAPE),
         'unit': 'us per iteration', 'runs': runs, 'calls_per_region': calls}
  res.update({k: spread(v, 1e6) for k, v in times.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  emit(res)


def count_launches(dev):
  res = {'measure': 'launches_per_iteration', 'shape_T_B_A': list(SHAPE)}
  for form, fn in _forms(dev).items():
    fn()
    kernels = device_kernels(fn, dev, repeat=4)
    res[form] = len(kernels) / 4
    res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:12]
  emit(res)


def bench_ppo(dev, steps, parent):
  learner = ppo_learner(dev, fused_mlp=True)
  forms = ('parent',) if parent else ('fused_head', 'chained_head')

  def update(form):
    if not parent:
      learner.fused_head = form == 'fused_head'
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
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT_PPO, 'fused_mlp': True, 'unit': 'ms',
         'steps': steps, 'adam_steps': n}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained_head']['median'] / res['fused_head']['median'], 2)
  emit(res)


def split_update(dev):
  learner = ppo_learner(dev, fused_mlp=True)
  n = ANT_PPO['num_updates_per_batch'] * ANT_PPO['num_minibatches']
  for form in (True, False):
    learner.fused_head = form
    data = learner.collect()
    learner.update_normalizer(data)
    learner.update(data)  # warm-up; the second update is profiled
    # (this tool has always kept the `Optimizer.step#` spans: they match 'adam', so that row
    # is torch's seven launches plus one span, and its time counts the seven twice)
    kernels = device_kernels(lambda: learner.update(data), dev,  # pylint: disable=cell-var-from-loop
                             skip=('memcpy', 'memset'))
    res = {'measure': 'ppo_update_split', 'fused_head': form, 'adam_steps': n,
           'unit': 'per Adam step: launches, device us', **split_by_owner(kernels, n, OWNERS)}
    emit(res)


def main():
  a, dev = start('ppo_head_bench', tool_args(__doc__, runs=7, calls=100, steps=3,
                                             parts='head,launches,ppo,split'))
  parts = parts_of(a, in_parent=('ppo',))
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
