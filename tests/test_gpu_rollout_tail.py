"""The Ant rollout kernel's per-step tail on running addresses
(`env_step_body`'s RT: the output block's base, the recorded actions' base and
the draw counter advance once per step; the observation's elements go to
per-lane offsets formed once per launch), at the smallest shapes that reach
what the addressing can get wrong.

A ragged batch (B = 6: one full wave's four envs and a half-empty second
workgroup), `episode_length` 5 so AutoReset's select runs inside the longer
launches, `bx_env_rollout_random` launches through `RolloutRunner`. Every
output array of every step must be bit-equal to `env.step` chained over
`bx_uniform_slabs` draws with the same seed, offset and step stride. The
runner's buffers are replaced by ones pre-filled with a guard pattern, so the
words a launch must not touch (past the last env's last step, the other
buffer's earlier steps, the records' pad words, past the recorded actions) are
compared against the pattern on the host.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, EP = 6, 5
SEED, OFFSET = 11, 777
GUARD = 4096       # words after each guarded buffer
PAT = 0x7FC0DEAD   # a NaN no kernel computes


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _pattern(n, dev):
  return torch.full((n,), PAT, dtype=torch.int32, device=dev).view(torch.float32)


def _is_pattern(t):
  return bool(torch.all(t.contiguous().view(torch.int32) == PAT))


def _env(dev, xy):
  from brax_amd import envs
  return envs.create('ant', batch_size=B, episode_length=EP, auto_reset=True, device=dev,
                     exclude_current_positions_from_observation=not xy)


def _guarded_runner(env, st0, K, stride):
  """A RolloutRunner whose trajectory and action buffers sit in pattern-filled
  allocations with GUARD words behind them (the start state copied over, as
  the constructor placed it)."""
  from brax_amd.envs.rollout import RolloutRunner
  r = RolloutRunner(env, st0, K, seed=SEED, offset=OFFSET, step_stride=stride)
  assert r.draw  # one bx_env_rollout_random launch per run
  blk = r._lay.block
  big = _pattern(2 * K * blk + GUARD, r.device)
  new = big[:2 * K * blk].view(2, K * blk)
  lay = r._lay
  # the start state into buffer 0's last step, so the first launch writes
  # buffer 1, the one the guard words follow
  old_last = lay.step_views(r._out[1].view(K, blk)[K - 1])
  new_last = lay.step_views(new[0].view(K, blk)[K - 1])
  for i in (0, 3, 4):  # qp, done, steps: what the first launch reads
    new_last[i].copy_(old_last[i])
  r._out, r._cur = new, 0
  acts = _pattern(K * B * r.A + GUARD, r.device)
  r._acts = acts[:K * B * r.A].view(K, B, r.A)
  return r, big, acts


def _chain(env, st, dev, n, first, stride):
  """n chained env.step calls on bx_uniform_slabs' draws for steps first ..
  first + n - 1: the actions and each step's State."""
  from brax_amd import _native
  A = env.action_size
  acts = torch.empty((n, B, A), dtype=torch.float32, device=dev)
  _native.check(_native.lib().bx_uniform_slabs(
      C.c_void_p(acts.data_ptr()), B * A, n, SEED, OFFSET + first * stride, stride, None, 0,
      -1.0, 1.0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
  out = []
  for t in range(n):
    st = env.step(st, acts[t])
    out.append(st)
  return acts, out


def _equal(tr, t, st):
  q = torch.cat([st.qp.pos, st.qp.rot, st.qp.vel, st.qp.ang], -1)
  assert torch.equal(tr.qp[t][..., :13], q), ('qp', t)
  assert torch.equal(tr.obs[t], st.obs), ('obs', t)
  assert torch.equal(tr.reward[t], st.reward), ('reward', t)
  assert torch.equal(tr.done[t], st.done), ('done', t)
  assert torch.equal(tr.steps[t], st.info['steps']), ('steps', t)
  assert torch.equal(tr.truncation[t], st.info['truncation']), ('truncation', t)
  assert len(tr.metric_keys) == 10
  for i, k in enumerate(tr.metric_keys):
    assert torch.equal(tr.metrics[t][:, i], st.metrics[k]), (k, t)


@pytest.mark.parametrize('xy', [False, True])
@pytest.mark.parametrize('K', [1, 2, 7])
def test_ragged_batch_one_launch(dev, K, xy):
  """K = 1 (a single step), 2 (the first advance), 7 (neither a power of two
  nor a divisor of anything; the episodes end at step 5), with the torso's
  x, y in the observation (x = 2) and without (x = 0)."""
  env = _env(dev, xy)
  assert env.observation_size == (89 if xy else 87)
  st0 = env.reset(np.array([5, 3], np.uint32))
  stride = 3 * B * env.action_size  # not the dense B * A
  r, big, abuf = _guarded_runner(env, st0, K, stride)
  blk = r._lay.block
  r.run()
  tr = r.trajectory()
  acts, ref = _chain(env, st0, dev, K, 0, stride)
  torch.cuda.synchronize()
  assert torch.equal(r.actions(), acts)
  for t in range(K):
    _equal(tr, t, ref[t])
  if K > EP:
    assert float(tr.done.sum()) > 0  # AutoReset's select ran inside the launch
  # what the launch must not have touched: the words behind the last env's
  # last step and behind the recorded actions, the source buffer's steps
  # before its last, the records' three pad words
  assert _is_pattern(big[2 * K * blk:]) and _is_pattern(abuf[K * B * r.A:])
  assert _is_pattern(big[:(K - 1) * blk])
  assert _is_pattern(tr.qp[..., 13:])


def test_second_launch_reads_first_in_place(dev):
  """Two launches of K = 3 from one runner (the second reads the first's last
  step in place and writes the other buffer) equal one chained run of 6."""
  K = 3
  env = _env(dev, False)
  st0 = env.reset(np.array([8, 1], np.uint32))
  stride = B * env.action_size
  r, big, abuf = _guarded_runner(env, st0, K, stride)
  blk = r._lay.block
  acts, ref = _chain(env, st0, dev, 2 * K, 0, stride)
  r.run()
  first = [v.clone() for v in r._lay.views(r._out[1], K)]
  a0 = r.actions().clone()
  torch.cuda.synchronize()
  # (the first launch wrote buffer 1 and left buffer 0's first K - 1 steps alone)
  assert _is_pattern(big[2 * K * blk:]) and _is_pattern(big[:(K - 1) * blk])
  r.run()
  tr = r.trajectory()
  torch.cuda.synchronize()
  assert torch.equal(a0, acts[:K]) and torch.equal(r.actions(), acts[K:])
  from brax_amd.envs.rollout import trajectory
  tr0 = trajectory(r._u, first, None)
  for t in range(K):
    _equal(tr0, t, ref[t])
    _equal(tr, t, ref[K + t])
  assert float(tr.done.sum()) > 0  # step 5 of 6 ends the episodes
  # the second launch wrote buffer 0 and nothing behind it: the first
  # launch's trajectory, which follows it, is as it was, and so are the guards
  assert _is_pattern(big[2 * K * blk:]) and _is_pattern(abuf[K * B * r.A:])
  for a, b in zip(first, r._lay.views(r._out[1], K)):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
  fin = r.state()
  assert torch.equal(fin.obs, ref[-1].obs) and torch.equal(fin.qp.pos, ref[-1].qp.pos)
