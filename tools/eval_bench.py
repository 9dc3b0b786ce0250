"""Whole-evaluation timings: Ant, episode length 1,000, auto-reset, the
default PPO policy ((32,) * 4 swish, NormalTanh head, normalised
observations), deterministic, at 128 and at 4,096 envs.

Three loops over one evaluation (1,000 policy steps of every env from one
reset state), each the median (min .. max) of `--runs` whole evaluations
after a warm-up, with the peak of `torch.cuda.max_memory_allocated` over the
timed runs:

  (a) the one-launch evaluation: `eval_rollout` (and `Evaluator.run_evaluation`
      around it, which adds the reset and the host-side metric dict);
  (b) the best path without it: `policy_rollout` on the unwrapped env in
      K = 50 chunks, the `EvalWrapper` recurrences applied to each chunk in
      torch (vectorised over the chunk: the flags by a cumulative product);
  (c) `policy_rollout` on the eval env itself, which takes the chained path
      (per step: the torch MLP forward, `env.step`, the wrapper's tensor ops).

Prints one JSON line per batch size (microseconds per env step of the whole
batch).

    python tools/eval_bench.py [--envs 128 4096] [--runs 5]
"""
import numpy as np
import torch

from measure import emit, regions, spread, start, tool_args
from policy_rollout_bench import ppo_policy

EP = 1000


def evaluation(run, runs, warmup, dev):
  """One loop's entry: us per env step over `runs` whole evaluations after the
  warm-up, and the peak allocation of the timed runs alone."""
  for _ in range(warmup):
    run()
  torch.cuda.synchronize(dev)
  torch.cuda.reset_peak_memory_stats()
  entry = spread(regions(run, runs, 1, dev), 1e6 / EP, 3)
  entry['peak_MiB'] = round(torch.cuda.max_memory_allocated() / 2**20, 1)
  return entry


def chunked(policy_rollout, env, st0, policy, K):
  """(b): the trajectory kernel in K-step chunks, EvalWrapper's sums per chunk."""
  B = st0.obs.shape[0]
  dev = st0.obs.device
  M = len(env.unwrapped.metric_keys)
  sums = torch.zeros((M + 1, B), device=dev)
  active = torch.ones(B, device=dev)
  ep_steps = torch.zeros(B, device=dev)
  st = st0
  for _ in range(EP // K):
    st, tr, _ = policy_rollout(env, st, policy, K, fused=True)
    # active before each step of the chunk: the incoming flag times the
    # running product of the earlier steps' (1 - done)
    keep = torch.cumprod(1 - tr.done, 0)
    before = active * torch.cat([torch.ones_like(keep[:1]), keep[:-1]])
    sums[:M] += (tr.metrics * before[:, :, None]).sum(0).T
    sums[M] += (tr.reward * before).sum(0)
    # (the counter of the last step the first episode was active at)
    ep_steps = torch.maximum(ep_steps, (tr.steps * before).amax(0))
    active = active * keep[-1]
  return sums, active, ep_steps


def main():
  ap = tool_args(__doc__, runs=5)
  ap.add_argument('--envs', type=int, nargs='+', default=[128, 4096])
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--k', type=int, default=50)
  a, dev = start('eval_bench', ap)
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.evaluator import Evaluator, eval_rollout  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.policy import policy_rollout  # pylint: disable=import-outside-toplevel
  for B in a.envs:
    eval_env = envs.create('ant', batch_size=B, episode_length=EP, auto_reset=True,
                           eval_metrics=True, device=dev)
    policy = ppo_policy(eval_env, dev, deterministic=True)
    st0 = eval_env.reset(np.array([0, 1], np.uint32))
    res = {'env': 'ant', 'envs': B, 'episode_length': EP, 'runs': a.runs,
           'unit': 'us per env step (whole batch)'}

    def record(name, run):
      res[name] = evaluation(run, a.runs, a.warmup, dev)

    ev = Evaluator(eval_env, policy, num_eval_envs=B, episode_length=EP, fused=True)
    record('a_run_evaluation', ev.run_evaluation)
    record('a_eval_rollout', lambda: eval_rollout(eval_env, st0, k=EP, policy=policy, fused=True))
    record('b_chunked_trajectory', lambda: chunked(policy_rollout, eval_env.env, st0, policy, a.k))
    record('c_chained_eval_env', lambda: policy_rollout(eval_env, st0, policy, EP))
    rb = res['b_chunked_trajectory']['median']
    for k in ('a_run_evaluation', 'a_eval_rollout', 'c_chained_eval_env'):
      res[k]['over_b'] = round(res[k]['median'] / rb, 3)
    emit(res)


if __name__ == '__main__':
  main()
