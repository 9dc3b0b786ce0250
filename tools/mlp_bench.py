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
  `--group` measures the group launches instead (`fused_mlp.mlp_group`: several
  networks in one forward and two backward launches) against the same members
  through `fused_mlp` one by one (the single entry points), both under
  autograd as the learners run them, alternating, with their launch counts: the SAC critic group (six evaluations of 95 -> 256 -> 256 -> 1 at
  256 rows forward, four of them backward: dW / db for two, dx for two) and
  the PPO group (policy at 5,120 rows, value at 6,144, bootstrap value at
  1,024 forward; policy and value backward).
  `--parent` runs ppo and sac without naming `fused_mlp` at all, so the same
  file measures a tree from before the keyword existed.

Prints one JSON line per measurement.

    python tools/mlp_bench.py [--parts mlp,launches,ppo,sac] [--runs 7] [--calls 100] [--steps 3]
    python tools/mlp_bench.py --group [--runs 7] [--calls 100]
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


# a group: (name, activation, networks {name: sizes}, members (network, x, rows, backward)):
# backward is None (forward only), 'params' (dW / db) or 'dx'
GROUPS = (
    ('sac critics', 'relu', {'q1': (95, 256, 256, 1), 'q2': (95, 256, 256, 1),
                             't1': (95, 256, 256, 1), 't2': (95, 256, 256, 1)},
     (('q1', 'cur', 256, 'params'), ('q2', 'cur', 256, 'params'), ('t1', 'next', 256, None),
      ('t2', 'next', 256, None), ('q1', 'pi', 256, 'dx'), ('q2', 'pi', 256, 'dx'))),
    ('ppo', 'swish', {'policy': (87,) + (32,) * 4 + (16,), 'value': (87,) + (256,) * 5 + (1,)},
     (('policy', 'obs5120', 5120, 'params'), ('value', 'obs6144', 6144, 'params'),
      ('value', 'boot', 1024, None))),
)


def _group_forms(activation, nets, members, dev):
  """Both forms as the learners run them, through autograd: `mlp_group` and one
  `autograd.grad` for the group, against `fused_mlp` (`bx_mlp_forward` /
  `bx_mlp_backward`) and one `autograd.grad` per member."""
  from brax_amd.training import fused_mlp, networks  # pylint: disable=import-outside-toplevel
  g = torch.Generator().manual_seed(len(members))
  layers = {k: networks.make_layers(s, g, device=dev) for k, s in nets.items()}
  xs, table, dys, leaves = {}, [], [], []
  for net, x, rows, backward in members:
    key = (x, net if backward == 'dx' else None)  # a leaf of its own per dx: no sum
    if key not in xs:
      xs[key] = torch.randn((rows, nets[net][0]), generator=g).to(dev).requires_grad_(backward == 'dx')
    # (only what a member's backward pass is for requires a gradient)
    own = layers[net] if backward == 'params' else networks.detached(layers[net])
    table.append((own, xs[key], activation))
    dys.append(torch.randn((rows, nets[net][-1]), generator=g).to(dev))
    leaves.append(networks.parameters(own) if backward == 'params' else
                  [xs[key]] if backward == 'dx' else [])
  back = [k for k, m in enumerate(members) if m[3]]

  def grouped():
    ys = fused_mlp.mlp_group(table, fused=True)
    return torch.autograd.grad([ys[k] for k in back], [t for k in back for t in leaves[k]],
                               grad_outputs=[dys[k] for k in back])

  def singly():
    out = []
    for k, (own, x, act) in enumerate(table):
      y = fused_mlp.fused_mlp(own, x, act, fused=True)
      if leaves[k]:
        out.append(torch.autograd.grad(y, leaves[k], grad_outputs=dys[k]))
    return out
  return {'grouped': grouped, 'singly': singly}


def bench_groups(dev, runs, calls):
  for name, activation, nets, members in GROUPS:
    forms = _group_forms(activation, nets, members, dev)
    res = {'measure': 'mlp_group_forward_backward', 'group': name,
           'members': [list(m) for m in members], 'unit': 'us per iteration', 'runs': runs,
           'calls_per_region': calls}
    times = alternate(forms, runs, calls, dev)
    res.update({k: spread(v, 1e6) for k, v in times.items()})
    res['singly_over_grouped'] = round(res['singly']['median'] / res['grouped']['median'], 2)
    for form, fn in forms.items():
      kernels = [e for e in device_kernels(fn, dev, repeat=4) if 'mlp_' in e.name]
      res[form + '_launches'] = len(kernels) / 4
      res[form + '_device_us'] = round(sum(e.device_time for e in kernels) / 4, 1)
    emit(res)


def main():
  ap = tool_args(__doc__, runs=7, calls=100, steps=3, parts='mlp,launches,ppo,sac')
  ap.add_argument('--group', action='store_true', help='the group launches against single ones')
  a, dev = start('mlp_bench', ap)
  if a.group:
    bench_groups(dev, a.runs, a.calls)
    return
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
