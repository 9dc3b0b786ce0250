"""Open-loop rollouts: K `Env.step`s in ONE kernel launch.

The reference collects trajectories by scanning `env.step` under `jit`
(`brax/training/acting.py:53-77`, `generate_unroll`: `jax.lax.scan` of
`actor_step`); when the actions are known up front (random-action rollouts,
replayed action sequences, the reference notebook's benchmark loop) the scan
is open-loop. `rollout(env, state, actions)` runs that scan through
`bx_env_rollout_packed`: one launch steps every env K times, the state held on
chip between steps, and writes every step's complete output (state, obs,
reward, done, episode counters, metrics, the target envs' streams) to HBM -
bit for bit the outputs of K chained `env.step` calls
(`tests/test_gpu_rollout.py`).
"""
import ctypes as C
import dataclasses
from typing import Any, Optional, Tuple

import torch

from brax_amd import _native
from brax_amd.base import pack_qp
from brax_amd.envs import packed
from brax_amd.envs.env import PhysicsEnv, State, Wrapper
from brax_amd.envs.graph import _Captured
from brax_amd.system import _stream


@dataclasses.dataclass(frozen=True)
class Trajectory:
  """Every step of a rollout, leading axis K (steps) then B (envs):
  qp (K, B, N, 16) packed (pos 0:3, rot 3:7, vel 7:10, ang 10:13), obs
  (K, B, O), reward / done / steps / truncation (K, B), metrics (K, B, M)
  with `metric_keys` naming the columns, rng (K, B) for the target envs."""
  qp: Any
  obs: Any
  reward: Any
  done: Any
  steps: Any
  truncation: Any
  metrics: Any
  metric_keys: Tuple[str, ...]
  rng: Optional[Any] = None


def chain_options(env):
  """The PhysicsEnv under a wrapper chain and the options the fused kernel
  applies for it: EpisodeWrapper (episode_length, action_repeat),
  AutoResetWrapper (auto_reset); Vector / Vmap wrappers pass through.
  Other wrappers have no fused form: NotImplementedError."""
  from brax_amd.envs import wrappers  # pylint: disable=import-outside-toplevel
  opts = {}
  w = env
  while isinstance(w, Wrapper):
    if isinstance(w, wrappers.EpisodeWrapper):
      opts['episode_length'] = w.episode_length
      opts['action_repeat'] = w.action_repeat
    elif isinstance(w, wrappers.AutoResetWrapper):
      opts['auto_reset'] = True
    elif not isinstance(w, (wrappers.VectorWrapper, wrappers.VmapWrapper)):
      raise NotImplementedError(f'{type(w).__name__} has no fused rollout')
    w = w.env
  if not isinstance(w, PhysicsEnv):
    raise NotImplementedError(f'{type(w).__name__} is not a kernel env')
  return w, opts


def trajectory(u, views, rng) -> Trajectory:
  """The Trajectory over `Layout.views` of the kernel env `u`'s K blocks."""
  q, obs, reward, done, steps, trunc, met = views
  return Trajectory(qp=q, obs=obs, reward=reward, done=done, steps=steps, truncation=trunc,
                    metrics=met, metric_keys=tuple(u.metric_keys), rng=rng)


def rollout(env, state: State, actions, out: Optional[torch.Tensor] = None
            ) -> Tuple[State, Trajectory]:
  """K consecutive `env.step(state, actions[t])` in one launch.

  Args:
    env: an env from `brax_amd.envs.create` (Episode / AutoReset / Vector
      wrappers over a kernel env).
    state: the state to start from (a batch of B envs).
    actions: (K, B, A) float32 on the env's device (any strides with a
      unit last-axis stride).
    out: optional flat float32 buffer of K blocks (`packed.Layout.block`
      floats each) for the trajectory (reused across calls by graph captures).
  Returns:
    (the state after the K-th step, the Trajectory of all K steps); the
    state's tensors are views into the trajectory's last step.
  """
  u, opts = chain_options(env)
  dev = u.sys.device
  qbuf = pack_qp(state.qp, dev)
  B = qbuf.shape[0]
  act = packed.actions_input(actions, B, u.action_size, dev)
  K = act.shape[0]
  inputs = packed.step_inputs(u, opts, state, B)
  lay = packed.layout(u, B)
  out = lay.out_buffer(out, K, dev)
  rng_out = packed.launch(u, 'bx_env_rollout_packed', inputs, qbuf, K, out, True, act=act,
                          act_stride=act.stride(1), act_step_stride=act.stride(0),
                          act_width=act.shape[2])
  views = lay.views(out, K)
  final = packed.final_state(u, inputs[0], state, tuple(v[K - 1] for v in views),
                             None if rng_out is None else rng_out[K - 1])
  return final, trajectory(u, views, rng_out)


class RolloutGraph(_Captured):
  """`rollout` of K steps with on-device action draws, captured as one HIP
  graph: per replay ONE `bx_uniform_slabs` launch draws the K action slabs
  (slab t at `offset + (r * K + t) * step_stride`, the eager loop's
  `bx_uniform` offsets, as `StepGraph` draws them), ONE
  `bx_env_rollout_packed` launch steps every env K times, and the K-th state
  is fed back into the graph's static inputs. `hook(traj)` (device work
  only) is recorded after the rollout, e.g. the episodic (reward, done) sum
  over the K steps. `replay()` returns (state after the K-th step,
  trajectory), valid until the next replay."""

  def __init__(self, env, state: State, k: int, seed: int = 1, offset: int = 0,
               step_stride: Optional[int] = None, lo: float = -1.0, hi: float = 1.0,
               hook=None):
    if k < 1:
      raise ValueError(f'k must be >= 1, got {k}')
    u, _ = chain_options(env)
    dev = u.sys.device
    self.env, self.k, self.device = env, int(k), dev
    B = self._static_inputs(u, state)
    A = env.action_size
    stride = B * A if step_stride is None else int(step_stride)
    self._acts = torch.empty((self.k, B, A), dtype=torch.float32, device=dev)
    self._out = packed.layout(u, B).out_buffer(None, self.k, dev)
    lib = _native.lib()

    def body(hook=hook):
      _native.check(lib.bx_uniform_slabs(
          C.c_void_p(self._acts.data_ptr()), B * A, self.k, seed, offset, stride,
          C.c_void_p(self._epoch.data_ptr()), self.k * stride, lo, hi, _stream(dev.index)))
      st, tr = rollout(env, self._in, self._acts, out=self._out)
      if hook is not None:
        hook(tr)
      self._feed_back(st)
      return st, tr

    self._res = self._capture(body)

  def replay(self):
    """Steps every env K steps forward; returns (state, trajectory)."""
    self.graph.replay()
    return self._res


class RolloutRunner:
  """Back-to-back open-loop rollouts of K steps with on-device action draws,
  launched directly: per `run()` ONE `bx_env_rollout_random` launch that
  draws each step's actions inside the kernel (the K slabs at the eager
  loop's `bx_uniform` offsets: chunk c's slab t at `offset + (c * K + t) *
  step_stride`, recorded in `actions()`) and steps every env K times; for a
  system whose staged action row is narrower than the env's action (`draw`
  False), one `bx_uniform_slabs` launch and one `bx_env_rollout_packed`
  launch instead. Two trajectory buffers alternate: chunk c reads its input
  state from chunk c - 1's last step in place (no copies); one C call of host
  time per run, on the caller's current stream. `hook(traj)` runs after each
  rollout (device work, e.g. the episodic sums). `state()` is the state after
  the last run."""

  def __init__(self, env, state: State, k: int, seed: int = 1, offset: int = 0,
               step_stride: Optional[int] = None, lo: float = -1.0, hi: float = 1.0,
               hook=None):
    if k < 1:
      raise ValueError(f'k must be >= 1, got {k}')
    u, opts = chain_options(env)
    dev = u.sys.device
    self.env, self.k, self.device, self.hook = env, int(k), dev, hook
    self._u = u
    qbuf = pack_qp(state.qp, dev)
    B, A = qbuf.shape[0], env.action_size
    self.B, self.A = B, A
    self.seed, self.offset, self.lo, self.hi = seed, int(offset), float(lo), float(hi)
    self.stride = B * A if step_stride is None else int(step_stride)
    self._start = state  # (it also keeps the auto-reset first state of `_p` alive)
    self._p, done_in, steps_in, rng_in = packed.step_inputs(u, opts, state, B)
    self._has_steps = self._p.episode_length > 0
    self._lay = packed.layout(u, B)
    self._out = torch.empty((2, self.k * self._lay.block), dtype=torch.float32, device=dev)
    self._rng = (torch.zeros((2, self.k, B), dtype=torch.int32, device=dev)
                 if rng_in is not None else None)
    self._acts = torch.empty((self.k, B, A), dtype=torch.float32, device=dev)
    # the starting state goes into buffer 1's last step: chunk 0 reads it there
    q, _, _, done, steps, _, _ = self._last(1)
    q.copy_(qbuf)
    done.copy_(done_in)
    if steps_in is not None:
      steps.copy_(steps_in)
    else:
      steps.zero_()
    if rng_in is not None:
      self._rng[1, self.k - 1].copy_(rng_in)
    self._c = 0
    self._cur = 1  # the buffer holding the latest trajectory
    self._lib = _native.lib()
    # one-launch draws when the system stages the whole action row (probed
    # with a zero-step call: argument checks only)
    self.draw = self._lib.bx_env_rollout_random(*_native.args(
        'bx_env_rollout_random', sys=u.sys._h, env=C.byref(self._p), n_envs=B,  # pylint: disable=protected-access
        act_width=A, hi=1.0)) == 0
    # the launch's C arguments per buffer parity, built once (run() then
    # passes ctypes objects straight through: the host half of a launch is
    # on the critical path of a short timed region)
    self._args = {}
    self._stream_key = None

  def _last(self, i):
    """The views of buffer i's last step."""
    return self._lay.step_views(self._out[i].view(self.k, self._lay.block)[self.k - 1])

  def _launch_args(self, src, stream):
    """(the arguments before the draw offset, the ones after it) of the
    launch that reads buffer `src` and writes the other, on `stream`."""
    dst = 1 - src
    K, B, lay = self.k, self.B, self._lay
    base = self._out[src].data_ptr() + 4 * (K - 1) * lay.block  # the last step's qp
    done_in = base + 4 * lay.offset['done']
    steps_in = base + 4 * lay.offset['steps'] if self._has_steps else None
    rng_in = None if self._rng is None else self._rng[src, K - 1].data_ptr()
    rng_out = None if self._rng is None else self._rng[dst].data_ptr()
    vp = C.c_void_p
    h = self._u.sys._h  # pylint: disable=protected-access
    if self.draw:
      pre = (h, C.byref(self._p), C.c_int64(B), C.c_int32(K), vp(base), vp(done_in),
             vp(steps_in), vp(rng_in), C.c_uint64(self.seed))
      post = (C.c_uint64(self.stride), C.c_float(self.lo), C.c_float(self.hi),
              C.c_int64(self.A), vp(self._acts.data_ptr()), vp(self._out[dst].data_ptr()),
              vp(rng_out), stream)
    else:
      pre = (vp(self._acts.data_ptr()), C.c_int64(B * self.A), C.c_int64(K),
             C.c_uint64(self.seed))
      post = ((C.c_uint64(self.stride), None, C.c_uint64(0), C.c_float(self.lo),
               C.c_float(self.hi), stream),
              (h, C.byref(self._p), C.c_int64(B), C.c_int32(K), vp(base), vp(done_in),
               vp(steps_in), vp(rng_in), vp(self._acts.data_ptr()), C.c_int64(self.A),
               C.c_int64(B * self.A), C.c_int64(self.A), vp(self._out[dst].data_ptr()),
               vp(rng_out), stream))
    return pre, post

  def run(self):
    """Draws the next K action slabs and steps every env K steps."""
    src = self._cur
    stream = _stream(self.device.index)
    if stream.value != self._stream_key:  # the caller's current stream moved
      self._args = {}
      self._stream_key = stream.value
    a = self._args.get(src)
    if a is None:
      a = self._args[src] = self._launch_args(src, stream)
    pre, post = a
    off = C.c_uint64(self.offset + self._c * self.k * self.stride)
    if self.draw:
      _native.check(self._lib.bx_env_rollout_random(*pre, off, *post))
    else:
      _native.check(self._lib.bx_uniform_slabs(*pre, off, *post[0]))
      _native.check(self._lib.bx_env_rollout_packed(*post[1]))
    self._cur = 1 - src
    self._c += 1
    if self.hook is not None:
      self.hook(self.trajectory())

  def actions(self):
    """The last run's (K, B, A) actions."""
    return self._acts

  def trajectory(self) -> Trajectory:
    return trajectory(self._u, self._lay.views(self._out[self._cur], self.k),
                      None if self._rng is None else self._rng[self._cur])

  def state(self) -> State:
    """The state after the last run (views of the current trajectory)."""
    return packed.final_state(
        self._u, self._p, self._start, self._last(self._cur),
        None if self._rng is None else self._rng[self._cur, self.k - 1])
