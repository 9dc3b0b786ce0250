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
import torch

from measure import (ANT_ACT, ANT_OBS, ANT_PPO, SAC_ANT, all_kernels, alternate, ant_env,
                     device_kernels, emit, parts_of, ppo_learner, sac_learner, split_by_owner,
                     spread, start, timed, tool_args)

TAU = 0.005
# (SAC's loss heads are named `sac_head` and count under 'other torch' here)
OWNERS = (('ppo_head', 'head kernels'), ('mlp_', 'network kernels'),
          (('multi_tensor', 'adam'), 'optimiser'), 'other torch')


def _ppo_forms(dev):
  from brax_amd.training import networks, optim  # pylint: disable=import-outside-toplevel
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
  from brax_amd.training import networks, optim, sac_networks  # pylint: disable=import-outside-toplevel

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
    times = alternate(forms, runs, calls, dev)
    res = {'measure': 'optimiser_step', 'case': name, 'parameters': n, 'unit': 'us per step',
           'runs': runs, 'calls_per_region': calls}
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['torch_over_fused'] = round(res['torch']['median'] / res['fused']['median'], 2)
    emit(res)


def count_launches(dev):
  for name, (forms, _) in (('ppo_22_tensors', _ppo_forms(dev)),
                           ('sac_19_tensors_12_targets', _sac_forms(dev))):
    res = {'measure': 'launches_per_step', 'case': name}
    for form, fn in forms.items():
      fn()
      kernels = device_kernels(fn, dev, repeat=4)
      res[form] = len(kernels) / 4
      res[form + '_device_us'] = round(sum(e.device_time for e in kernels) / 4, 1)
      res[form + '_kernels'] = sorted({e.name[:60] for e in kernels})[:8]
    emit(res)


def _adam_forms(parent):
  return {'parent': {}} if parent else {'fused_adam': dict(fused_adam=True),
                                        'torch_adam': dict(fused_adam=False)}


def _ppo_learners(dev, parent):
  env = ant_env(dev, ANT_PPO['num_envs'])
  return {form: ppo_learner(dev, env, fused_mlp=True, fused_head=True, **kw)
          for form, kw in _adam_forms(parent).items()}


def bench_ppo(dev, steps, parent):
  learners = _ppo_learners(dev, parent)

  def update(form):
    learner = learners[form]
    data = learner.collect()
    learner.update_normalizer(data)
    t, metrics = timed(lambda: learner.update(data), dev)
    return t, float(metrics['total_loss'])
  for form in learners:
    update(form)  # warm-up: code objects, the allocator, Adam's state
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  n = ANT_PPO['num_updates_per_batch'] * ANT_PPO['num_minibatches']
  res = {'measure': 'ppo_update_phase', 'env': 'ant', **ANT_PPO, 'fused_mlp': True, 'fused_head': True,
         'unit': 'ms', 'steps': steps, 'adam_steps': n}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_adam_step'] = round(res[form]['median'] / n, 3)
    res[form + '_last_total_loss'] = rec[form][-1][1]
  if not parent:
    res['torch_over_fused'] = round(res['torch_adam']['median'] / res['fused_adam']['median'], 2)
  emit(res)


def _sac_learners(dev, parent):
  env = ant_env(dev, SAC_ANT['num_envs'])
  return {form: sac_learner(dev, env, fused_mlp=True, **kw)
          for form, kw in _adam_forms(parent).items()}


def bench_sac(dev, steps, parent):
  learners = _sac_learners(dev, parent)

  def update(form):
    L = learners[form]
    L.get_experience()
    sample = L.buffer.sample()
    t, metrics = timed(lambda: L.update(sample), dev)
    return t, float(metrics['critic_loss'])
  for form in learners:
    update(form)
  rec = {form: [] for form in learners}
  for _ in range(steps):
    for form in learners:
      rec[form].append(update(form))
  res = {'measure': 'sac_gradient_updates', 'env': 'ant', **SAC_ANT, 'hidden': [256, 256],
         'fused_mlp': True, 'unit': 'ms', 'steps': steps}
  for form in learners:
    res[form] = spread([t for t, _ in rec[form]], 1e3)
    res[form + '_ms_per_update'] = round(res[form]['median'] / SAC_ANT['updates'], 3)
    res[form + '_last_critic_loss'] = rec[form][-1][1]
  if not parent:
    res['torch_over_fused'] = round(res['torch_adam']['median'] / res['fused_adam']['median'], 2)
  emit(res)


def split_updates(dev):
  """(the SAC target loop's launches are elementwise torch kernels and count
  under 'other torch' in the torch form)"""
  n = ANT_PPO['num_updates_per_batch'] * ANT_PPO['num_minibatches']
  for form, learner in _ppo_learners(dev, False).items():
    data = learner.collect()
    learner.update_normalizer(data)
    learner.update(data)  # warm-up; the second update is profiled
    kernels = device_kernels(lambda: learner.update(data), dev)  # pylint: disable=cell-var-from-loop
    emit({'measure': 'ppo_update_split', 'form': form, 'adam_steps': n,
          'unit': 'per Adam step: launches, device us', **split_by_owner(kernels, n, OWNERS),
          'all': all_kernels(kernels, n)})
  for form, L in _sac_learners(dev, False).items():
    L.get_experience()
    sample = L.buffer.sample()
    L.update(sample)
    kernels = device_kernels(lambda: L.update(sample), dev)  # pylint: disable=cell-var-from-loop
    emit({'measure': 'sac_update_split', 'form': form, 'gradient_steps': SAC_ANT['updates'],
          'unit': 'per gradient step: launches, device us',
          **split_by_owner(kernels, SAC_ANT['updates'], OWNERS),
          'all': all_kernels(kernels, SAC_ANT['updates'])})


def main():
  a, dev = start('optim_bench', tool_args(__doc__, runs=7, calls=100, steps=3,
                                          parts='step,launches,ppo,sac,split'))
  parts = parts_of(a, in_parent=('ppo', 'sac'))
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
