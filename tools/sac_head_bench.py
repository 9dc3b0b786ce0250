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
  group     the same 64 updates with every switch on (`fused_mlp`, `fused_adam`,
            `fused_head`), `fused_group` on and off on two learners,
            alternating; with `--parent` one learner with the three older
            switches on and `fused_group` not named.
  `--parent` runs sac without naming `fused_head` at all, so the same file
  measures a tree from before the keyword existed; `--root` names the tree
  whose package is imported (default: this file's).

Prints one JSON line per measurement.

    python tools/sac_head_bench.py [--parts head,sac,split,group] [--runs 7] [--calls 50]
"""
import collections

import torch

from measure import (ANT_ACT, ANT_OBS, SAC_ANT, all_kernels, alternate, ant_env, device_kernels, emit,
                     owner_of, parts_of, sac_learner, split_by_owner, spread, start, timed, tool_args)

OWNERS = (('sac_head', 'head kernels'), ('mlp_', 'network kernels'),
          (('multi_tensor', 'adam'), 'optimiser'), 'other torch')


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
    times = alternate(forms, runs, calls, dev)
    res = {'measure': 'sac_gradients', 'B': B, 'O': ANT_OBS, 'A': ANT_ACT, 'C': 2,
           'hidden': [256, 256], 'fused_mlp': True, 'unit': 'us per call', 'runs': runs,
           'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
    emit(res)
    for form, fn in forms.items():
      kernels = device_kernels(fn, dev, repeat=4)
      emit({'measure': 'sac_gradients_launches', 'B': B, 'form': form,
            'unit': 'per call: launches, device us', **split_by_owner(kernels, 4, OWNERS),
            'all': all_kernels(kernels, 4)})


HEAD_FORMS = {'fused_head': dict(fused_head=True), 'chained_head': dict(fused_head=False)}
GROUP_FORMS = {'grouped': dict(fused_head=True, fused_group=True),
               'ungrouped': dict(fused_head=True, fused_group=False)}


def _learners(dev, parent, forms=None, parent_form=None):
  """(this tool alone sets the learning rate, the discount and the reward
  scale of the README's SAC run; the others leave `sac.Learner`'s defaults)"""
  env = ant_env(dev, SAC_ANT['num_envs'])
  forms = {'parent': parent_form or {}} if parent else (forms or HEAD_FORMS)
  return {form: sac_learner(dev, env, learning_rate=6e-4, discounting=0.997, reward_scaling=30.0,
                            fused_mlp=True, fused_adam=True, **kw)
          for form, kw in forms.items()}


def bench_sac(dev, steps, parent, forms=None, parent_form=None, measure='sac_gradient_updates'):
  learners = _learners(dev, parent, forms, parent_form)

  def update(form):
    L = learners[form]
    L.get_experience()
    sample = L.buffer.sample()
    t, metrics = timed(lambda: L.update(sample), dev)
    return t, float(metrics['critic_loss'])
  for form in learners:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  res = {'measure': measure, 'env': 'ant', **SAC_ANT, 'hidden': [256, 256],
         'fused_mlp': True, 'fused_adam': True, 'unit': 'ms', 'steps': steps}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / SAC_ANT['updates'], 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    fast, slow = list(learners)
    name = 'chained_over_fused' if forms is None else f'{slow}_over_{fast}'
    res[name] = round(res[slow]['median'] / res[fast]['median'], 2)
  emit(res)


def split_updates(dev):
  n = SAC_ANT['updates']
  for form, L in _learners(dev, False).items():
    L.get_experience()
    sample = L.buffer.sample()
    L.update(sample)  # warm-up; the second update is profiled
    kernels = device_kernels(lambda: L.update(sample), dev)  # pylint: disable=cell-var-from-loop
    res = {'measure': 'sac_update_split', 'form': form, 'gradient_steps': n,
           'unit': 'per gradient step: launches, device us',
           **split_by_owner(kernels, n, OWNERS), 'all': all_kernels(kernels, n)}
    if form == 'fused_head':
      names = lambda owner, width: collections.Counter(  # noqa: E731
          e.name[:width] for e in kernels if owner_of(e.name, OWNERS) == owner)
      res['other_torch_per_step'] = {k: round(v / n, 2)
                                     for k, v in names('other torch', 70).most_common()}
      res['head_kernels_per_step'] = {k: round(v / n, 2)
                                      for k, v in names('head kernels', 50).items()}
    emit(res)


def main():
  a, dev = start('sac_head_bench', tool_args(__doc__, runs=7, calls=50, steps=5,
                                             parts='head,sac,split'))
  parts = parts_of(a, in_parent=('sac', 'group'))
  if 'head' in parts:
    bench_head(dev, a.runs, a.calls)
  if 'sac' in parts:
    bench_sac(dev, a.steps, a.parent)
  if 'split' in parts:
    split_updates(dev)
  if 'group' in parts:
    bench_sac(dev, a.steps, a.parent, GROUP_FORMS, dict(fused_head=True),
              'sac_gradient_updates_grouped')


if __name__ == '__main__':
  main()
