"""Closed-loop rollouts: an MLP policy evaluated inside the K-step kernel.

The reference collects experience by scanning `policy(obs, key) -> action`
then `env.step` (`brax/training/acting.py:30-73`, `actor_step` /
`generate_unroll`). `policy_rollout(env, state, policy, k)` is the acting half
of that scan in ONE launch (`bx_env_rollout_policy`): each step's action row
is the policy's, computed on chip from the observation the previous step
wrote, with the default PPO head (`ppo/networks.py:62-88`: `networks.MLP`,
`NormalTanhDistribution`, `make_inference_fn`). The learner (losses, GAE,
the PPO loop) is `brax_amd.training`.

`MLPPolicy` owns one packed float32 parameter buffer on the device; the
kernel reads it at launch, so `load_` (in place, same address) or a replayed
graph sees new weights. `MLPPolicy.forward` is the plain torch restatement
(float32 or float64 as its inputs), the chained path's policy and the tests'
reference.
"""
import ctypes as C
import dataclasses
import math
from typing import Any, Optional, Tuple

import torch

from brax_amd import _native, abi
from brax_amd.base import pack_qp
from brax_amd.envs import packed
from brax_amd.envs.env import State, _f32
from brax_amd.envs.rollout import Trajectory, chain_options, trajectory
from brax_amd.fused import use_kernel
from brax_amd.system import _stream

_ACTIVATIONS = {
    'swish': torch.nn.functional.silu,
    'relu': torch.relu,
    'tanh': torch.tanh,
}


def head_scale(s, min_std):
  """The NormalTanh head's scale from its parameter half."""
  return torch.nn.functional.softplus(s) + min_std


def tanh_log_det(raw):
  """log |d tanh(x) / dx| (`TanhBijector.forward_log_det_jacobian`)."""
  return 2.0 * (math.log(2.0) - raw - torch.nn.functional.softplus(-2.0 * raw))


def normal_tanh_log_prob(loc, scale, raw):
  """Per action: log N(raw; loc, scale) minus the tanh log-det. One copy of
  the formulae for `MLPPolicy.forward` and the learner (`brax_amd.training`),
  so the log-prob a loss recomputes is the one the rollout recorded."""
  z = (raw - loc) / scale
  return -0.5 * z * z - 0.5 * math.log(2 * math.pi) - torch.log(scale) - tanh_log_det(raw)


@dataclasses.dataclass(frozen=True)
class PolicyExtras:
  """What the policy did at every step: action and raw_action (K, B, A)
  (action = tanh(raw_action)), log_prob (K, B) of raw_action under the head's
  Normal minus the tanh log-det (deterministic: evaluated at the mode)."""
  action: Any
  raw_action: Any
  log_prob: Any


def normal_tanh_head(policy, logits, eps=None):
  """`policy`'s NormalTanh head over its last layer's output: (action, raw,
  loc, scale) with raw = loc + scale * eps and action = tanh(raw); `eps` is
  zeros when None or when the policy is deterministic, scale ones when the
  head has no scale half."""
  if policy._loc_only():  # pylint: disable=protected-access
    loc, scale = logits, torch.ones_like(logits)
  else:
    loc, s = torch.chunk(logits, 2, dim=-1)
    scale = head_scale(s, policy.min_std)
  if policy.deterministic or eps is None:
    eps = torch.zeros_like(loc)
  raw = loc + scale * eps.to(logits.dtype)
  return torch.tanh(raw), raw, loc, scale


class MLPPolicy:
  """An MLP with a NormalTanh head over one packed device buffer.

  Args:
    layers: [(W (in, out), b (out,)), ...] in flax's kernel layout; the last
      layer is 2 * action_size wide (loc | scale parameter), or action_size
      with `deterministic`.
    activation: 'swish', 'relu' or 'tanh' (hidden layers).
    obs_mean, obs_std: optional (obs_size,) normalisation, x = (obs - mean) / std.
    min_std: the scale's floor, scale = softplus(s) + min_std.
    deterministic: act at the mode (raw = loc).
    head: 'normal_tanh' (above) or 'identity': action = raw = the last
      layer's output, `action_size` wide, no tanh, no scale half, no noise
      (ARS's `obs @ W`; a zero bias expresses a bias-free matrix). The
      evaluation and population kernels take it; the trajectory kernel of
      `policy_rollout` does not.
  """

  def __init__(self, layers, activation='swish', obs_mean=None, obs_std=None, min_std=1e-3,
               deterministic=False, device=None, head='normal_tanh'):
    if activation not in _ACTIVATIONS:
      raise ValueError(f'activation {activation!r} not in {sorted(_ACTIVATIONS)}')
    if head not in abi.HEADS:
      raise ValueError(f'head {head!r} not in {sorted(abi.HEADS)}')
    self.head = head
    if (obs_mean is None) != (obs_std is None):
      raise ValueError('obs_mean and obs_std go together')
    self.device = torch.device('cpu' if device is None else device)
    self.activation = activation
    self.min_std = float(min_std)
    self.deterministic = bool(deterministic)
    layers = self._checked(layers)
    self.sizes = [(w.shape[0], w.shape[1]) for w, _ in layers]
    self.obs_size = self.sizes[0][0]
    self.params = torch.empty((sum((i + 1) * o for i, o in self.sizes),), dtype=torch.float32,
                              device=self.device)
    self.load_(layers)
    self.obs_mean = self.obs_std = None
    if obs_mean is not None:
      self.obs_mean = torch.as_tensor(obs_mean, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
      self.obs_std = torch.as_tensor(obs_std, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
      if self.obs_mean.numel() != self.obs_size or self.obs_std.numel() != self.obs_size:
        raise ValueError(f'obs_mean / obs_std must hold {self.obs_size} values')

  @staticmethod
  def _checked(layers):
    out = []
    for w, b in layers:
      w = torch.as_tensor(w, dtype=torch.float32)
      b = torch.as_tensor(b, dtype=torch.float32)
      if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[1]:
        raise ValueError(f'layer shapes {tuple(w.shape)}, {tuple(b.shape)}: want (in, out), (out,)')
      if out and out[-1][0].shape[1] != w.shape[0]:
        raise ValueError(f'layer input {w.shape[0]} != previous output {out[-1][0].shape[1]}')
      out.append((w, b))
    if not out:
      raise ValueError('no layers')
    return out

  @classmethod
  def from_flax_params(cls, params, **kwargs):
    """From the nested dict `brax.io.model` pickles: {'params': {'hidden_0':
    {'kernel', 'bias'}, 'hidden_1': ...}} of array-likes (layers in index
    order; the outer 'params' level is optional)."""
    tree = params.get('params', params) if hasattr(params, 'get') else None
    if not hasattr(tree, 'items') or not tree:
      raise ValueError("expected {'params': {'hidden_0': {'kernel', 'bias'}, ...}}")
    named = []
    for name, leaf in tree.items():
      head, _, idx = str(name).rpartition('_')
      if not head or not idx.isdigit() or not hasattr(leaf, 'keys') or set(leaf.keys()) != {'kernel', 'bias'}:
        raise ValueError(f'layer {name!r}: want <name>_<index> holding kernel and bias')
      named.append((int(idx), leaf))
    named.sort(key=lambda x: x[0])
    if [i for i, _ in named] != list(range(len(named))):
      raise ValueError('layer indices must be 0..n-1')
    return cls([(leaf['kernel'], leaf['bias']) for _, leaf in named], **kwargs)

  def load_(self, layers):
    """New weights into the same buffer (same address, same shapes)."""
    layers = self._checked(layers)
    if hasattr(self, 'sizes') and [(w.shape[0], w.shape[1]) for w, _ in layers] != self.sizes:
      raise ValueError('load_ keeps the layer shapes')
    flat = torch.cat([torch.cat([w.reshape(-1), b]) for w, b in layers])
    self.params.copy_(flat)
    return self

  def layers(self, dtype=torch.float32):
    """The packed buffer unpacked: [(W (in, out), b (out,)), ...]."""
    out, o = [], 0
    for i, n in self.sizes:
      w = self.params[o:o + i * n].view(i, n)
      b = self.params[o + i * n:o + (i + 1) * n]
      out.append((w.to(dtype), b.to(dtype)))
      o += (i + 1) * n
    return out

  @property
  def action_size(self):
    last = self.sizes[-1][1]
    if self.head == 'identity':
      return last
    return last // 2 if last % 2 == 0 and not self._loc_only() else last

  def _loc_only(self):
    """True when the head has no scale half (set by `for_actions`)."""
    return getattr(self, '_a', None) == self.sizes[-1][1]

  def for_actions(self, a):
    """Checks the head against an env's action size; a deterministic policy
    may be `a` wide (no scale half)."""
    last = self.sizes[-1][1]
    if self.head == 'identity':
      if last != a:
        raise ValueError(f'the last layer is {last} wide: the identity head wants {a}')
      self._a = a
    elif last == 2 * a:
      self._a = None
    elif last == a and self.deterministic:
      self._a = a
    else:
      raise ValueError(f'the last layer is {last} wide: want {2 * a}'
                       + (f' or {a}' if self.deterministic else ''))
    return self

  def forward(self, obs, eps=None):
    """(action, raw, log_prob, logits) of a batch of observations, in the
    dtype of `obs`; `eps` (…, A) is the standard-normal noise (ignored when
    deterministic; zeros when None)."""
    dt = obs.dtype
    x = obs
    if self.obs_mean is not None:
      x = (x - self.obs_mean.to(x.device, dt)) / self.obs_std.to(x.device, dt)
    ls = self.layers(dt)
    fn = _ACTIVATIONS[self.activation]
    for k, (w, b) in enumerate(ls):
      x = x @ w.to(x.device) + b.to(x.device)
      if k + 1 < len(ls):
        x = fn(x)
    logits = x
    if self.head == 'identity':
      return logits, logits, torch.zeros(logits.shape[:-1], dtype=dt, device=logits.device), logits
    action, raw, loc, scale = normal_tanh_head(self, logits, eps)
    return action, raw, normal_tanh_log_prob(loc, scale, raw).sum(-1), logits

  def descriptor(self, action_size):
    """The `bx_policy` struct over this policy's buffers (they must outlive
    the calls that read it)."""
    self.for_actions(action_size)
    if len(self.sizes) > abi.POLICY_MAX_LAYERS:
      raise NotImplementedError(f'more than {abi.POLICY_MAX_LAYERS} layers')
    p = abi.BxPolicy()
    p.params = self.params.data_ptr()
    p.n_layers = len(self.sizes)
    for k, (_, n) in enumerate(self.sizes):
      p.width[k] = n
    p.activation = abi.POLICY_ACTIVATIONS[self.activation]
    p.obs_mean = None if self.obs_mean is None else self.obs_mean.data_ptr()
    p.obs_std = None if self.obs_std is None else self.obs_std.data_ptr()
    p.min_std = self.min_std
    p.deterministic = int(self.deterministic)
    p.action_size = int(action_size)
    return p


def normal_slabs(out, slab_n, n_slabs, seed, offset, slab_stride):
  """Fills `out` with the fused kernel's noise: out[s * slab_n + j] =
  N(seed, offset + s * slab_stride + 2 j) (`bx_normal_slabs`)."""
  _native.check(_native.lib().bx_normal_slabs(
      C.c_void_p(out.data_ptr()), slab_n, n_slabs, seed, offset, slab_stride, None, 0,
      _stream(out.device.index)))
  return out


def _packed(state, dev):
  """`pack_qp` of a state's QP (the GPU tests read final states through it)."""
  return pack_qp(state.qp, dev)


def step_noise(policy, K, B, A, seed, offset, stride, dev):
  """The chained paths' eps, step by step: yields K times one (B, A) buffer,
  refilled for step t by one `bx_normal_slabs` launch at `offset + t *
  stride`; zeros for a deterministic policy or an identity head (no draws)."""
  eps = torch.zeros((B, A), dtype=torch.float32, device=dev)
  draws = not policy.deterministic and policy.head == 'normal_tanh'
  for t in range(K):
    if draws:
      normal_slabs(eps, B * A, 1, seed, offset + t * stride, 0)
    yield eps


def _extras(extras, K, B, A, dev):
  if extras is None:
    return PolicyExtras(action=torch.empty((K, B, A), dtype=torch.float32, device=dev),
                        raw_action=torch.empty((K, B, A), dtype=torch.float32, device=dev),
                        log_prob=torch.empty((K, B), dtype=torch.float32, device=dev))
  for t, shape in ((extras.action, (K, B, A)), (extras.raw_action, (K, B, A)),
                   (extras.log_prob, (K, B))):
    packed.output_buffer('extras', t, shape, dev)
  return extras


def fused_supported(env, policy, trajectory: bool = True) -> Optional[str]:
  """None when `bx_env_rollout_policy` takes this env and policy, else the
  library's reason (a zero-step call: argument checks only, no launch).
  `trajectory=False` makes only the checks every policy kernel shares (the
  evaluation and population kernels probe their own entry points after it)."""
  try:
    u, opts = chain_options(env)
  except NotImplementedError as e:
    return str(e)
  if trajectory and policy.head != 'normal_tanh':
    return f'the trajectory kernel has no {policy.head} head'
  try:
    desc = policy.descriptor(u.action_size)
  except (ValueError, NotImplementedError) as e:
    return str(e)
  if policy.params.device != u.sys.device:
    return f'the policy lives on {policy.params.device}, the env on {u.sys.device}'
  if policy.obs_size != u.obs_size:
    return f'the policy reads {policy.obs_size} observations, the env writes {u.obs_size}'
  if not trajectory:
    return None
  return packed.refusal(u, opts, 'bx_env_rollout_policy', policy=C.byref(desc))


def policy_rollout(env, state: State, policy: MLPPolicy, k: int, seed: int = 0, offset: int = 0,
                   step_stride: Optional[int] = None, fused: Optional[bool] = None,
                   out: Optional[torch.Tensor] = None, extras: Optional[PolicyExtras] = None
                   ) -> Tuple[State, Trajectory, PolicyExtras]:
  """K closed-loop steps: action_t = policy(obs_t, eps_t), state_{t+1} =
  env.step(state_t, action_t), with obs_0 = state.obs.

  eps of step t, env e, action a is N(seed, offset + t * step_stride +
  (e * A + a) * 2) (`step_stride` defaults to 2 * B * A), whatever the path.

  Args:
    fused: None takes the one-launch kernel where the env kind and the
      policy's shape allow it, else the chained path (per step: one
      `bx_normal_slabs` launch, `policy.forward`, `env.step`); True raises
      NotImplementedError where the kernel refuses; False forces the chained
      path (every env).
    out: optional flat float32 trajectory buffer, as `rollout`'s (fused path).
    extras: optional preallocated PolicyExtras to write into (with `out`, the
      fused call allocates nothing and can be graph-captured).
  Returns:
    (the state after the K-th step, the Trajectory, the PolicyExtras).
  """
  if k < 1:
    raise ValueError(f'k must be >= 1, got {k}')
  if not use_kernel(fused, 'policy rollout', lambda: fused_supported(env, policy)):
    return _chained(env, state, policy, int(k), seed, offset, step_stride)
  u, opts = chain_options(env)
  dev = u.sys.device
  qbuf = pack_qp(state.qp, dev)
  B, A, K = qbuf.shape[0], u.action_size, int(k)
  stride = 2 * B * A if step_stride is None else int(step_stride)
  inputs = packed.step_inputs(u, opts, state, B)
  obs_in = packed.obs_input(u, state, B)
  lay = packed.layout(u, B)
  out = lay.out_buffer(out, K, dev)
  ex = _extras(extras, K, B, A, dev)
  desc = policy.descriptor(A)
  rng_out = packed.launch(u, 'bx_env_rollout_policy', inputs, qbuf, K, out, True, obs_in=obs_in,
                          policy=C.byref(desc), seed=seed, offset=offset, step_stride=stride,
                          act_out=ex.action, raw_out=ex.raw_action, logp_out=ex.log_prob)
  views = lay.views(out, K)
  final = packed.final_state(u, inputs[0], state, tuple(v[K - 1] for v in views),
                             None if rng_out is None else rng_out[K - 1])
  return final, trajectory(u, views, rng_out), ex


def _chained(env, state, policy, K, seed, offset, step_stride):
  """The same loop through `env.step`: any env, any wrapper chain."""
  dev = torch.device(state.obs.device)
  B, A = state.obs.shape[0], env.action_size
  policy.for_actions(A)
  stride = 2 * B * A if step_stride is None else int(step_stride)
  acts, raws, lps, steps = [], [], [], []
  for eps in step_noise(policy, K, B, A, seed, offset, stride, dev):
    a, r, lp, _ = policy.forward(state.obs.to(torch.float32), eps)
    state = env.step(state, a)
    acts.append(a)
    raws.append(r)
    lps.append(lp)
    steps.append(state)
  zeros = torch.zeros((B,), dtype=torch.float32, device=dev)

  try:
    keys = tuple(chain_options(env)[0].metric_keys)
  except NotImplementedError:
    keys = tuple(sorted(state.metrics.keys()))
  met = (torch.stack([torch.stack([_f32(s.metrics[kk], dev) for kk in keys], -1) for s in steps])
         if keys else torch.zeros((K, B, 0), dtype=torch.float32, device=dev))
  rng = (torch.stack([s.info['rng'] for s in steps]) if steps[-1].info.get('rng') is not None
         else None)
  traj = Trajectory(
      qp=torch.stack([pack_qp(s.qp, dev) for s in steps]), obs=torch.stack([s.obs for s in steps]),
      reward=torch.stack([_f32(s.reward, dev) for s in steps]),
      done=torch.stack([_f32(s.done, dev) for s in steps]),
      steps=torch.stack([_f32(s.info.get('steps', zeros), dev) for s in steps]),
      truncation=torch.stack([_f32(s.info.get('truncation', zeros), dev) for s in steps]),
      metrics=met, metric_keys=keys, rng=rng)
  ex = PolicyExtras(action=torch.stack(acts), raw_action=torch.stack(raws),
                    log_prob=torch.stack(lps))
  return state, traj, ex
