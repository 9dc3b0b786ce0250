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
import functools

import torch

from measure import (ANT_PPO, SAC_ANT, alternate, device_kernels, emit, parts_of, ppo_learner,
                     sac_learner, spread, start, timed, tool_args)

NETS = (('ppo value', (87,) + (256,) * 5 + (1,), 6144, 'swish'),
        ('ppo policy', (87,) + (32,) * 4 + (16,), 5120, 'swish'),
        ('sac critic', (95, 256, 256, 1), 512, 'relu'))


def _forms(sizes, rows, activation, dev):
  from brax_amd.training import networks  # pylint: disable=import-outside-toplevel
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
    times = alternate(forms, runs, calls, dev)
    flop = 6 * rows * sum(i * o for i, o in zip(sizes[:-1], sizes[1:]))
    res = {'measure': 'mlp_forward_backward', 'net': name, 'sizes': list(sizes), 'rows': rows,
           'activation': activation, 'unit': 'us per iteration', 'runs': runs,
           'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
    res['fused_TFLOP_per_s'] = round(flop / res['fused']['median'] / 1e6, 2)
    emit(res)


def count_launches(dev):
  for name, sizes, rows, activation in NETS:
    res = {'measure': 'launches_per_iteration', 'net': name}
    for form, fn in _forms(sizes, rows, activation, dev).items():
      fn()
      kernels = device_kernels(fn, dev, repeat=4)
      res[form] = len(kernels) / 4
      res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:12]
    emit(res)


def bench_ppo(dev, steps, parent):
  learner = ppo_learner(dev)
  forms = ('parent',) if parent else ('fused', 'chained')

  def update(form):
    if not parent:
      learner.fused_mlp = form == 'fused'
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
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT_PPO, 'unit': 'ms', 'steps': steps,
         'adam_steps': n}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  emit(res)


def bench_sac(dev, steps, parent):
  L = sac_learner(dev)
  forms = ('parent',) if parent else ('fused', 'chained')

  def update(form):
    if not parent:
      L.fused_mlp = form == 'fused'
    L.get_experience()
    sample = L.buffer.sample()
    t, metrics = timed(lambda: L.update(sample), dev)
    return t, float(metrics['critic_loss'])
  for form in forms:
    update(form)
  rec = {form: [] for form in forms}
  for _ in range(steps):
    for form in forms:
      rec[form].append(update(form))
  updates = SAC_ANT['updates']
  res = {'measure': 'sac_gradient_updates', 'env': 'ant', 'num_envs': SAC_ANT['num_envs'],
         'batch_size': SAC_ANT['batch_size'], 'grad_updates_per_step': updates,
         'hidden': [256, 256], 'unit': 'ms', 'steps': steps}
  for form in forms:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / updates, 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  emit(res)


def main():
  a, dev = start('mlp_bench', tool_args(__doc__, runs=7, calls=100, steps=3,
                                        parts='mlp,launches,ppo,sac'))
  parts = parts_of(a, in_parent=('ppo', 'sac'))
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
