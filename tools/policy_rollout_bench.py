"""Closed-loop rollout timings: Ant, 4,096 envs, episode length 1,000,
auto-reset, K = 50 steps per launch, the default PPO policy ((32,) * 4 swish,
NormalTanh head, normalised observations).

Three loops, each the median of `--regions` timed regions of `--reps`
K-step chunks after a warm-up, the state carried from chunk to chunk:

  (a) RolloutRunner: the open-loop kernel with in-kernel uniform draws;
  (b) fused policy_rollout, stochastic and deterministic;
  (c) what a user has without (b): a torch MLP forward + env.step per step,
      eager and under one captured graph of K steps.

Prints one JSON line (microseconds per env step of the whole batch).

    python tools/policy_rollout_bench.py [--envs 4096] [--k 50]
"""
import math

import numpy as np
import torch

from measure import emit, regions, spread, start, tool_args


def ppo_policy(env, dev, deterministic=False, seed=0):
  from brax_amd.envs.policy import MLPPolicy  # pylint: disable=import-outside-toplevel
  g = torch.Generator(device='cpu').manual_seed(seed)
  sizes = (env.observation_size, 32, 32, 32, 32, 2 * env.action_size)
  layers = []
  for i, o in zip(sizes[:-1], sizes[1:]):
    lim = math.sqrt(3.0 / i)
    layers.append(((torch.rand((i, o), generator=g) * 2 - 1) * lim, torch.zeros(o)))
  O = env.observation_size
  return MLPPolicy(layers, obs_mean=torch.rand((O,), generator=g) - 0.5,
                   obs_std=torch.rand((O,), generator=g) + 0.5, deterministic=deterministic,
                   device=dev)


def main():
  ap = tool_args(__doc__)
  ap.add_argument('--envs', type=int, default=4096)
  ap.add_argument('--k', type=int, default=50)
  ap.add_argument('--regions', type=int, default=7)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  a, dev = start('policy_rollout_bench', ap)
  from brax_amd import envs  # pylint: disable=import-outside-toplevel
  from brax_amd.base import PackedQP, packed_buffer  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.policy import PolicyExtras, policy_rollout  # pylint: disable=import-outside-toplevel
  from brax_amd.envs.rollout import RolloutRunner, chain_options  # pylint: disable=import-outside-toplevel
  B, K = a.envs, a.k
  env = envs.create('ant', batch_size=B, episode_length=1000, auto_reset=True, device=dev)
  A = env.action_size
  res = {'env': 'ant', 'envs': B, 'k': K, 'regions': a.regions, 'reps': a.reps,
         'unit': 'us per env step (whole batch)'}

  def record(name, chunk):
    res[name] = spread(regions(chunk, a.regions, a.reps, dev, a.warmup), 1e6 / K, 3)

  # (a) open-loop, in-kernel uniform draws
  runner = RolloutRunner(env, env.reset(np.array([0, 1], np.uint32)), K, seed=1)
  record('a_rollout_runner', runner.run)

  # (b) fused policy + env
  for name, det in (('b_fused_stochastic', False), ('b_fused_deterministic', True)):
    policy = ppo_policy(env, dev, det)
    st = env.reset(np.array([0, 1], np.uint32))
    u = chain_options(env)[0]
    block = B * (u.sys.num_bodies * 16 + u.obs_size + 4 + len(u.metric_keys))
    bufs = [torch.empty((K * block,), dtype=torch.float32, device=dev) for _ in range(2)]
    ex = PolicyExtras(action=torch.empty((K, B, A), device=dev),
                      raw_action=torch.empty((K, B, A), device=dev),
                      log_prob=torch.empty((K, B), device=dev))
    box = {'st': st, 'c': 0}

    def chunk(policy=policy, bufs=bufs, ex=ex, box=box):
      c = box['c']
      box['st'], _, _ = policy_rollout(env, box['st'], policy, K, seed=1, offset=c * K * 2 * B * A,
                                       fused=True, out=bufs[c & 1], extras=ex)
      box['c'] = c + 1
    record(name, chunk)

  # (c) unfused: torch forward + env.step per step
  policy = ppo_policy(env, dev)
  box = {'st': env.reset(np.array([0, 1], np.uint32))}

  def steps(st):
    for _ in range(K):
      act, _, _, _ = policy.forward(st.obs, torch.randn((B, A), device=dev))
      st = env.step(st, act)
    return st

  def eager(box=box):
    box['st'] = steps(box['st'])
  record('c_unfused_eager', eager)

  try:
    st = env.reset(np.array([0, 1], np.uint32))
    qp = packed_buffer(st.qp).clone()
    statics = {'obs': st.obs.clone(), 'done': st.done.clone(),
               'steps': st.info['steps'].clone()}
    info = dict(st.info)
    info['steps'] = statics['steps']
    st_in = st.replace(qp=PackedQP(qp), obs=statics['obs'], done=statics['done'], info=info)

    def body():
      out = steps(st_in)
      qp.copy_(packed_buffer(out.qp))
      statics['obs'].copy_(out.obs)
      statics['done'].copy_(out.done)
      statics['steps'].copy_(out.info['steps'])
    with torch.cuda.device(dev):
      side = torch.cuda.Stream(dev)
      side.wait_stream(torch.cuda.current_stream(dev))
      with torch.cuda.stream(side):
        body()
      torch.cuda.current_stream(dev).wait_stream(side)
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        body()
      torch.cuda.current_stream(dev).synchronize()
    record('c_unfused_graph', graph.replay)
  except Exception as e:  # pylint: disable=broad-except
    res['c_unfused_graph'] = {'error': f'{type(e).__name__}: {e}'}

  ra = res['a_rollout_runner']['median']
  for k in ('b_fused_stochastic', 'b_fused_deterministic', 'c_unfused_eager', 'c_unfused_graph'):
    if 'median' in res.get(k, {}):
      res[k]['over_a'] = round(res[k]['median'] / ra, 3)
  emit(res)


if __name__ == '__main__':
  main()
