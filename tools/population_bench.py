"""Population-evaluation timings: Ant, episode length 1,000, auto-reset,
4,096 members (P = 2,048 antithetic directions), for two nets: ES's default
((32,) * 4 relu, NormalTanh head, stochastic; 6,512 parameters per member) and
ARS's linear policy (87 x 8 plus a zero bias row, identity head; 704).

Three loops over one evaluation (1,000 policy steps of every env from one
reset state), each the median (min .. max) of `--runs` whole evaluations
after a warm-up, with the peak of `torch.cuda.max_memory_allocated` over the
timed runs:

  (a) `population_rollout`, fused: one launch, env e reading row e (and, with
      `--ab`, the same launch with the rows read from global memory / staged
      as the plan would not, where the plan leaves a choice);
  (b) `eval_rollout` with ONE shared policy of the same shape: the evaluation
      kernel without per-member weights, the floor (an identity head goes to
      the population kernel with stride 0);
  (c) `population_rollout(fused=False)`: the chained path (per step a batched
      `torch.bmm` forward, `env.step`, the recurrences in torch).

Prints one JSON line per net (microseconds per env step of the whole batch).

    python tools/population_bench.py [--members 4096] [--runs 5] [--ab]
"""
import math

import numpy as np
import torch

from eval_bench import EP, evaluation
from measure import emit, start, tool_args


def net(env, dev, which):
  from brax_amd.envs.policy import MLPPolicy  # pylint: disable=import-outside-toplevel
  O, A = env.observation_size, env.action_size
  g = torch.Generator(device='cpu').manual_seed(0)
  if which == 'ars_linear':
    w = (torch.rand((O, A), generator=g) * 2 - 1) * math.sqrt(3.0 / O)
    return MLPPolicy([(w, torch.zeros(A))], head='identity', device=dev,
                     obs_mean=torch.zeros(O), obs_std=torch.ones(O))
  sizes = (O, 32, 32, 32, 32, 2 * A)
  layers = [((torch.rand((i, o), generator=g) * 2 - 1) * math.sqrt(3.0 / i), torch.zeros(o))
            for i, o in zip(sizes[:-1], sizes[1:])]
  return MLPPolicy(layers, activation='relu', device=dev, obs_mean=torch.zeros(O),
                   obs_std=torch.ones(O))


def main():
  ap = tool_args(__doc__, runs=5)
  ap.add_argument('--members', type=int, default=4096)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--ab', action='store_true')
  ap.add_argument('--nets', nargs='+', default=['es_default', 'ars_linear'])
  a, dev = start('population_bench', ap)
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.evaluator import eval_rollout  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.population import PolicyPopulation, population_rollout  # pylint: disable=import-outside-toplevel
  B = a.members
  eval_env = envs.create('ant', batch_size=B, episode_length=EP, auto_reset=True,
                         eval_metrics=True, device=dev)
  st0 = eval_env.reset(np.array([0, 1], np.uint32))
  for which in a.nets:
    policy = net(eval_env, dev, which)
    pp = PolicyPopulation(policy, B).perturb_(0.02, seed=1)
    res = {'env': 'ant', 'net': which, 'members': B, 'n_params': pp.n_params,
           'episode_length': EP, 'runs': a.runs, 'unit': 'us per env step (whole batch)'}

    def record(name, run):
      res[name] = evaluation(run, a.runs, a.warmup, dev)

    _, r = population_rollout(eval_env, st0, pp, k=EP, fused=True)
    res['staged'] = r.staged
    res['mean_episode_steps'] = round(float(r.episode_steps.mean()), 1)
    record('a_population_fused', lambda: population_rollout(eval_env, st0, pp, k=EP, fused=True))
    if a.ab:
      record('a_rows_from_global', lambda: population_rollout(eval_env, st0, pp, k=EP, fused=True, stage=False))
      record('a_no_moments', lambda: population_rollout(eval_env, st0, pp, k=EP, fused=True, moments=False))
      record('a_shared_row', lambda: population_rollout(eval_env, st0, policy, k=EP, fused=True))
    record('b_eval_shared_policy', lambda: eval_rollout(eval_env, st0, k=EP, policy=policy, fused=True))
    record('c_population_chained', lambda: population_rollout(eval_env, st0, pp, k=EP, fused=False))
    ra = res['a_population_fused']['median']
    res['a_over_b'] = round(ra / res['b_eval_shared_policy']['median'], 3)
    res['a_over_c'] = round(ra / res['c_population_chained']['median'], 4)
    emit(res)


if __name__ == '__main__':
  main()
