"""What surrounds every packed env launch, once: the output block's layout,
the inputs a launch reads from a `State`, the K-step call itself with its
arguments by name (`launch`, `refusal`), and the `State` it returns.

`bx_env_step_packed` and the K-step entry points built on it (`rollout`,
`policy_rollout`, `eval_rollout`, `population_rollout`, `RolloutRunner`) write
one block of float32 words per step (`bx_capi_env.cpp`, `env_step_packed`):

    qp (B, N, 16) | obs (B, O) | reward, done, steps, truncation (B,) each |
    metrics (B, M)

`Layout` is that block on the Python side; nothing else in the package spells
its sizes or offsets.
"""
import ctypes as C
import itertools

import torch

from brax_amd import _native
from brax_amd.base import PackedQP
from brax_amd.envs.env import State, _f32, _Metrics
from brax_amd.system import _stream

FIELDS = ('qp', 'obs', 'reward', 'done', 'steps', 'truncation', 'metrics')


class Layout:
  """The output block of one step of B envs with N bodies, O observations and
  M metrics. `sizes` are the fields' words in `FIELDS` order, `offset[field]`
  the word a field starts at, `block` the words of a whole step."""

  __slots__ = ('B', 'N', 'O', 'M', 'sizes', 'offset', 'block')

  def __init__(self, B, N, O, M):
    self.B, self.N, self.O, self.M = B, N, O, M
    self.sizes = (B * N * 16, B * O, B, B, B, B, B * M)
    self.offset = dict(zip(FIELDS, itertools.accumulate((0,) + self.sizes)))
    self.block = B * (N * 16 + O + 4 + M)

  def out_buffer(self, out, K, dev):
    """The flat buffer K blocks are written to: `out` checked, or a new one."""
    n = K * self.block
    if out is None:
      return torch.empty((n,), dtype=torch.float32, device=dev)
    if (out.numel() < n or out.dtype != torch.float32 or not out.is_contiguous()
        or out.device != dev):
      raise ValueError(f'out must hold {n} contiguous float32 on {dev}')
    return out

  def step_views(self, blk):
    """One block (`block` words) as its fields' views, in `FIELDS` order:
    (B, N, 16), (B, O), four (B,), (B, M)."""
    q, obs, reward, done, steps, trunc, met = torch.split(blk, self.sizes)
    return (q.view(self.B, self.N, 16), obs.view(self.B, self.O), reward, done, steps, trunc,
            met.view(self.B, self.M))

  def views(self, out, K):
    """The first K blocks of `out` as views with a leading step axis:
    (K, B, N, 16), (K, B, O), four (K, B), (K, B, M)."""
    B = self.B
    q, obs, reward, done, steps, trunc, met = torch.split(
        out[:K * self.block].view(K, self.block), self.sizes, dim=1)
    return (q.view(K, B, self.N, 16), obs.view(K, B, self.O), reward, done, steps, trunc,
            met.view(K, B, self.M))


def layout(u, B):
  """The `Layout` of B envs of the kernel env `u` (built once per batch size)."""
  cache = u.__dict__.setdefault('_layouts', {})
  lay = cache.get(B)
  if lay is None:
    lay = cache[B] = Layout(B, u.sys.num_bodies, u.obs_size, len(u.metric_keys))
  return lay


def step_inputs(u, opts, state, B):
  """What a launch of the kernel env `u` under the wrapper options `opts`
  reads from `state` besides the QP: (the `bx_env_params`, done, steps or
  None, the per-env streams or None), each a contiguous device tensor."""
  dev = u.sys.device
  info = state.info
  auto = bool(opts.get('auto_reset'))
  first_qp = info.get('first_qp') if auto else None
  first_obs = info.get('first_obs') if auto else None
  if auto and (first_qp is None or first_obs is None):
    raise ValueError('AutoResetWrapper state lacks first_qp / first_obs')
  p = u._cached_params(opts, first_qp, first_obs)  # pylint: disable=protected-access
  done_in = _f32(state.done, dev)
  steps_in = info.get('steps')
  if steps_in is not None:
    steps_in = _f32(steps_in, dev)
  rng_in = info.get('rng')
  if rng_in is None and getattr(u, 'needs_rng', False):
    rng_in = torch.zeros((B,), dtype=torch.int32, device=dev)  # a state built by hand
  return p, done_in, steps_in, rng_in


def obs_input(u, state, B):
  """`state.obs` as the (B, O) device rows a policy kernel reads first."""
  obs_in = _f32(state.obs, u.sys.device)
  if tuple(obs_in.shape) != (B, u.obs_size):
    raise ValueError(f'state.obs {tuple(obs_in.shape)} != ({B}, {u.obs_size})')
  return obs_in


def final_state(u, p, state, step, rng_out, info=None, eval_metrics=None):
  """The `State` after a launch that started from `state`: `step` are the
  last block's `Layout.step_views`, `rng_out` the streams it wrote (or None).
  What the launch does not rewrite is carried over from `state`.

  `info`: the input info to carry instead of `state.info` (the population
  rollout's, without 'eval_metrics'). `eval_metrics`: the evaluation's new
  `EvalMetrics`; with it 'reward' joins the metrics, as `EvalWrapper.step`
  has it."""
  q, obs, reward, done, steps, trunc, met = step
  info = dict(state.info if info is None else info)
  if p.episode_length > 0:
    info['steps'] = steps
    info['truncation'] = trunc
  if rng_out is not None:
    info['rng'] = rng_out
  keys = u.metric_keys
  m_in = state.metrics
  extra = m_in.carried(keys) if type(m_in) is _Metrics else {
      k: v for k, v in m_in.items() if k not in keys}
  if eval_metrics is not None:
    info['eval_metrics'] = eval_metrics
    extra = dict(extra, reward=reward)
  return State(qp=PackedQP(q), obs=obs, reward=reward, done=done,
               metrics=_Metrics(met, keys, extra), info=info)


def actions_input(actions, B, A, dev):
  """Given actions as the (K, B, A) float32 device tensor a launch reads
  (any strides with a unit last-axis stride)."""
  act = actions
  if type(act) is not torch.Tensor or act.dtype != torch.float32 or act.device != dev:
    act = torch.as_tensor(act, dtype=torch.float32, device=dev)
  if act.dim() != 3 or act.shape[1] != B or act.shape[2] != A:
    raise ValueError(f'actions {tuple(act.shape)} != (K, {B}, {A})')
  return act if act.stride(-1) == 1 else act.contiguous()


def output_buffer(name, t, shape, dev):
  """A caller's buffer `t` for a launch to write: contiguous float32 `shape`
  on `dev`, or ValueError."""
  if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
      or t.device != dev):
    raise ValueError(f'{name} must be contiguous float32 {shape} on {dev}')
  return t


def launch(u, entry, inputs, qbuf, K, out, every_step, **named):
  """One K-step launch of the entry point `entry` on the caller's stream, its
  result checked. What the K-step entry points share goes in by name from
  `inputs` (what `step_inputs` returned), `qbuf` and `out`; `named` are the
  entry point's own arguments (a tensor stands for its address; the ones left
  out are NULL or 0). Returns the target envs' streams the launch wrote, or
  None for a state without them: (K, B) with `every_step`, else (B,)."""
  p, done_in, steps_in, rng_in = inputs
  dev, B = u.sys.device, qbuf.shape[0]
  rng_out = (torch.empty((K, B) if every_step else (B,), dtype=torch.int32, device=dev)
             if rng_in is not None else None)
  def addresses(**tensors):
    return {k: v.data_ptr() if isinstance(v, torch.Tensor) else v for k, v in tensors.items()}
  _native.check(getattr(_native.lib(), entry)(*_native.args(
      entry, sys=u.sys._h, env=C.byref(p), n_envs=B, n_steps=K,  # pylint: disable=protected-access
      stream=_stream(dev.index), **addresses(
          qp_in=qbuf, done_in=done_in, steps_in=steps_in, rng_in=rng_in, out=out,
          rng_out=rng_out, **named))))
  return rng_out


def refusal(u, opts, entry, **named):
  """None when the library's entry point `entry` takes the kernel env `u`
  under `opts` with the arguments `named` (a zero-step call, so argument
  checks only and no launch), else the library's reason."""
  p = u._params(opts, None, None)  # pylint: disable=protected-access
  p.auto_reset = 0
  lib = _native.lib()
  rc = getattr(lib, entry)(*_native.args(entry, sys=u.sys._h, env=C.byref(p), **named))  # pylint: disable=protected-access
  return None if rc == 0 else lib.bx_last_error().decode()
