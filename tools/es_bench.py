"""ES / ARS trainer timings on one GPU (a tool, not a test; `bench.py` is
untouched).

  (a) `PolicyPopulation.perturb_` and `weighted_noise_sum`, fused (one
      `bx_population_perturb` launch; `bx_population_delta`'s one or two) against
      chained (the same results through a materialised `(P, n_params)` noise
      array and float64 torch expressions) on the same device buffers: Ant with
      ES's default network (6,512 parameters) at a population of 4,096, and
      Ant with ARS's matrix (704 parameters, the bias frozen) at 60 directions,
      20 of them weighted. A timed region is `--calls` back-to-back calls
      ending in a device synchronise; the figure is microseconds per call,
      median (min .. max) of `--runs` regions after a warm-up, the two forms
      alternating.
  (b) one ES epoch on Ant at that population, episode length 1,000, split into
      its phases, each ending in a synchronise; perturb and delta with the
      fused and the chained forms, alternating, median (min .. max) of
      `--epochs` epochs.
  `--learn`: a short ARS run and a short ES run on `inverted_pendulum`, the
      evaluation reward at every evaluation.

Prints one JSON line per measurement.

    python tools/es_bench.py [--runs 7] [--calls 50] [--epochs 3] [--learn]
"""
import time

import torch

from measure import ANT_ACT, ANT_OBS, alternate, emit, spread, start, timed, tool_args


def bench_kernels(dev, agent, P, runs, calls):
  from brax_amd.envs.policy import MLPPolicy  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.population import PolicyPopulation  # pylint: disable=import-outside-toplevel
  from brax_amd.training import ars, es  # pylint: disable=import-outside-toplevel
  if agent == 'es':
    layers = es.make_es_networks(ANT_OBS, ANT_ACT, seed=0, device=dev)
    policy = MLPPolicy([(w.detach(), b.detach()) for w, b in layers], activation='relu', device=dev)
    frozen, sigma = None, 0.1
    w = torch.randn((P,), generator=torch.Generator().manual_seed(P)).to(dev)
  else:
    policy = MLPPolicy(ars.make_policy_network(ANT_OBS, ANT_ACT, device=dev), head='identity',
                       device=dev)
    frozen = torch.cat([torch.zeros(ANT_OBS * ANT_ACT), torch.ones(ANT_ACT)]).to(dev, torch.uint8)
    sigma = 0.025
    w = torch.randn((P,), generator=torch.Generator().manual_seed(P))
    w[torch.randperm(P, generator=torch.Generator().manual_seed(1))[P // 3:]] = 0.
    w = w.to(dev)
  pop, ref = PolicyPopulation(policy, 2 * P), PolicyPopulation(policy, 2 * P)
  ws = pop.delta_workspace()
  n = pop.n_params
  pop.perturb_(sigma, 1, 0, frozen=frozen, fused=True)
  ref.perturb_(sigma, 1, 0, frozen=frozen, fused=False)
  same = torch.equal(pop.rows.view(torch.int32), ref.rows.view(torch.int32))
  a = pop.weighted_noise_sum(w, 1, 0, frozen=frozen, fused=True, workspace=ws)
  b = pop.weighted_noise_sum(w, 1, 0, frozen=frozen, fused=False)
  head = {'agent': agent, 'env': 'ant', 'directions': P, 'n_params': n, 'unit': 'us per call',
          'runs': runs, 'calls_per_region': calls}
  t = alternate({'fused': lambda: pop.perturb_(sigma, 1, 0, frozen=frozen, fused=True),
                 'chained': lambda: ref.perturb_(sigma, 1, 0, frozen=frozen, fused=False)},
                runs, calls, dev, warmup_calls=max(calls // 4, 1))
  res = {'measure': 'perturb', **head, 'bit_identical': same,
         # what the fused form moves: theta once per direction (cached) and the rows
         'fused_bytes_written': 2 * P * n * 4}
  res.update({k: spread(v, 1e6) for k, v in t.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  res['fused_store_GB_per_s'] = round(res['fused_bytes_written'] / res['fused']['median'] / 1e3, 1)
  emit(res)
  t = alternate({'fused': lambda: pop.weighted_noise_sum(w, 1, 0, frozen=frozen, fused=True,
                                                         workspace=ws),
                 'chained': lambda: pop.weighted_noise_sum(w, 1, 0, frozen=frozen, fused=False)},
                runs, calls, dev, warmup_calls=max(calls // 4, 1))
  res = {'measure': 'weighted_noise_sum', **head,
         'nonzero_weights': int((w != 0).sum()),
         'max_abs_difference': float((a.double() - b.double()).abs().max()),
         'max_abs_value': float(b.abs().max())}
  res.update({k: spread(v, 1e6) for k, v in t.items()})
  res['chained_over_fused'] = round(res['chained']['median'] / res['fused']['median'], 2)
  emit(res)


def bench_epoch(dev, P, epochs):
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  from brax_amd.envs import wrappers  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.population import population_rollout, population_supported  # pylint: disable=import-outside-toplevel
  from brax_amd.training import es  # pylint: disable=import-outside-toplevel
  env = envs.create('ant', episode_length=1000, batch_size=2 * P, device=dev)
  L = es.Learner(env, population_size=P, episode_length=1000,
                 fitness_shaping=es.FitnessShaping.CENTERED_RANK, normalize_observations=True,
                 seed=0, device=dev)
  why = population_supported(env, L.population)
  key = [L._key]  # pylint: disable=protected-access

  def phases(fused):
    out = {}
    key[0], reset_key = wrappers.split_key(key[0])
    out['reset'], state = timed(lambda: env.reset(reset_key), dev)
    out['perturb'], _ = timed(lambda: L.population.perturb_(
        L.perturbation_std, L.param_seed, L.param_offset, fused=fused), dev)
    out['episodes'], (_, res) = timed(lambda: population_rollout(
        env, state, L.population, 1000, seed=L.action_seed, offset=L.action_offset), dev)
    out['normaliser'], _ = timed(lambda: L.normalizer.update_from_moments(res), dev)
    out['weights'], w = timed(
        lambda: es.es_weights(res.scores, L.fitness_shaping, L.center_fitness), dev)
    out['delta'], delta = timed(lambda: L.population.weighted_noise_sum(
        w, L.param_seed, L.param_offset, fused=fused,
        workspace=L._workspace if fused is not False else None), dev)  # pylint: disable=protected-access

    def update():
      L.theta.grad = L.gradient(delta)
      L.optimizer.step()
      L.publish()
    out['update'], _ = timed(update, dev)
    L.param_offset += 2 * P * L.population.n_params
    L.action_offset += 1000 * 2 * 2 * P * env.action_size
    out['env_steps'] = int(res.obs_count.double().sum().item())
    return out
  phases(None), phases(False)  # warm-up
  rec = {None: [], False: []}
  for _ in range(epochs):
    for fused in (None, False):
      rec[fused].append(phases(fused))
  both = rec[None] + rec[False]
  res = {'measure': 'es_epoch', 'env': 'ant', 'population_size': P, 'n_params': L.population.n_params,
         'episode_length': 1000, 'unit': 'ms', 'epochs': epochs,
         'episodes_in_one_launch': why is None, 'chained_reason': why}
  for name in ('reset', 'episodes', 'normaliser', 'weights', 'update'):
    res[name] = spread([r[name] for r in both], 1e3)
  for name in ('perturb', 'delta'):
    res[name + '_fused'] = spread([r[name] for r in rec[None]], 1e3)
    res[name + '_chained'] = spread([r[name] for r in rec[False]], 1e3)
  res['env_steps_per_epoch'] = spread([r['env_steps'] for r in both], 1, 0)
  total = lambda recs: [sum(v for k, v in r.items() if k != 'env_steps') for r in recs]  # noqa: E731
  res['epoch_fused'] = spread(total(rec[None]), 1e3)
  res['epoch_chained'] = spread(total(rec[False]), 1e3)
  emit(res)


def learn(dev, agent, num_timesteps, num_evals):
  from brax_amd.training import ars, es  # pylint: disable=import-outside-toplevel
  curve = []

  def progress(step, m):
    curve.append({'env_steps': step, 'eval/episode_reward': round(float(m['eval/episode_reward']), 2),
                  'eval/avg_episode_length': round(float(m['eval/avg_episode_length']), 1)})
    emit({'measure': 'learn_progress', 'agent': agent, **curve[-1]})
  t = time.perf_counter()
  if agent == 'ars':
    cfg = dict(number_of_directions=60, top_directions=20, step_size=0.015,
               exploration_noise_std=0.025, normalize_observations=True)
    _, _, metrics = ars.train('inverted_pendulum', num_timesteps=num_timesteps,
                              episode_length=1000, num_eval_envs=128, seed=1, num_evals=num_evals,
                              device=dev, progress_fn=progress, **cfg)
  else:
    cfg = dict(population_size=128, learning_rate=1e-2, perturbation_std=0.1,
               normalize_observations=True)
    _, _, metrics = es.train('inverted_pendulum', num_timesteps=num_timesteps, episode_length=1000,
                             num_eval_envs=128, seed=1, num_evals=num_evals, device=dev,
                             progress_fn=progress,
                             fitness_shaping=es.FitnessShaping.CENTERED_RANK, **cfg)
    cfg['fitness_shaping'] = 'centered_rank'
  emit({'measure': 'learn', 'agent': agent, 'env': 'inverted_pendulum', **cfg,
        'num_timesteps': num_timesteps, 'wall_s': round(time.perf_counter() - t, 1),
        'training/sps': round(float(metrics['training/sps'])), 'curve': curve})


def main():
  ap = tool_args(__doc__, runs=7, calls=50)
  ap.add_argument('--epochs', type=int, default=3)
  ap.add_argument('--learn', action='store_true')
  ap.add_argument('--learn-timesteps', type=int, default=2_000_000)
  ap.add_argument('--learn-evals', type=int, default=6)
  ap.add_argument('--skip-epoch', action='store_true')
  a, dev = start('es_bench', ap)
  bench_kernels(dev, 'es', 4096, a.runs, a.calls)
  bench_kernels(dev, 'ars', 60, a.runs, a.calls)
  if not a.skip_epoch:
    bench_epoch(dev, 4096, a.epochs)
  if a.learn:
    for agent in ('ars', 'es'):
      learn(dev, agent, a.learn_timesteps, a.learn_evals)


if __name__ == '__main__':
  main()
