"""One episode per perturbed policy in ONE launch: the env-side half of the
reference's evolution agents.

ES (`brax/training/agents/es/train.py:136-164`) and ARS
(`training/agents/ars/train.py:106-130`) evaluate `2 x population` perturbed
copies of one policy, env i running copy i for a whole episode, and keep two
things: `cumulative_reward += (reward - reward_shift) * active` with `active
*= 1 - done`, and the per-step `(obs, active)` pairs for
`running_statistics.update(..., weights=active)`. `population_rollout` is that
`run_episode` through `bx_env_eval_population`: env e reads its own parameter
row, the sums and the observation moments stay on chip, and the launch writes
one state block, `M + 3` floats and `2 O + 1` moment words per env, whatever K
is. The optimiser halves (fitness shaping, top directions, Adam) are
`brax_amd.training.es` and `brax_amd.training.ars`.

`PolicyPopulation` owns the `(n_members, stride)` parameter rows and writes
the perturbations from the counter RNG, so the update regenerates the noise
instead of keeping it: `perturb_` (`bx_population_perturb`) and
`weighted_noise_sum` (`bx_population_delta`) draw eps on chip and touch only
the rows and the `(n_params,)` sum; `noise` materialises it for the chained
forms. `update_running_statistics` finishes the normaliser's update from the
on-chip moments.
"""
import copy
import ctypes as C
import dataclasses
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from brax_amd import _native, abi
from brax_amd.base import pack_qp
from brax_amd.envs import packed, wrappers
from brax_amd.envs.env import State, _f32
from brax_amd.envs.policy import (_ACTIVATIONS, MLPPolicy, fused_supported, normal_slabs,
                                  normal_tanh_head, step_noise)
from brax_amd.envs.rollout import chain_options
from brax_amd.fused import use_kernel
from brax_amd.system import _stream


class PolicyPopulation:
  """`n_members` parameter rows of one `MLPPolicy` shape in one device buffer.

  `rows` is `(n_members, stride)` float32, `stride` the policy's `n_params`
  rounded up to 4 floats (each row 16-byte aligned, `MLPPolicy.params`'
  layout); the policy's own buffer is theta, the point the rows perturb.
  """

  def __init__(self, policy: MLPPolicy, n_members: int):
    if int(n_members) < 1:
      raise ValueError(f'n_members must be >= 1, got {n_members}')
    self.policy = policy
    self.n_members = int(n_members)
    self.n_params = policy.params.numel()
    self.stride = (self.n_params + 3) & ~3
    self.rows = torch.zeros((self.n_members, self.stride), dtype=torch.float32,
                            device=policy.params.device)
    self.rows[:, :self.n_params] = policy.params

  def set_(self, rows):
    """Explicit rows, `(n_members, n_params)`, into the same buffer."""
    rows = torch.as_tensor(rows, dtype=torch.float32)
    if tuple(rows.shape) != (self.n_members, self.n_params):
      raise ValueError(f'rows {tuple(rows.shape)} != ({self.n_members}, {self.n_params})')
    self.rows[:, :self.n_params].copy_(rows)
    return self

  def _directions(self, antithetic):
    if not antithetic:
      return self.n_members
    if self.n_members % 2:
      raise ValueError(f'antithetic perturbations need an even n_members, got {self.n_members}')
    return self.n_members // 2

  def noise(self, seed: int, offset: int = 0, antithetic: bool = True):
    """The eps of `perturb_(sigma, seed, offset, antithetic)`, regenerated:
    `(P, n_params)` float32, eps[p, j] = N(seed, offset + 2 (p * n_params +
    j)) of `bx_normal_slabs`."""
    P = self._directions(antithetic)
    eps = torch.empty((P, self.n_params), dtype=torch.float32, device=self.rows.device)
    normal_slabs(eps, P * self.n_params, 1, int(seed), int(offset), 0)
    return eps

  def _frozen(self, frozen):
    """`frozen` as (n_params,) uint8 on the rows' device (None stays None)."""
    if frozen is None:
      return None
    f = torch.as_tensor(frozen)
    if f.numel() != self.n_params:
      raise ValueError(f'frozen holds {f.numel()} flags, the policy {self.n_params} parameters')
    return (f.reshape(-1) != 0).to(self.rows.device, torch.uint8).contiguous()

  def _fused(self, fused, what):
    if fused is None:
      return self.rows.is_cuda
    if fused and not self.rows.is_cuda:
      raise NotImplementedError(f'no fused {what}: the rows live on {self.rows.device}')
    return bool(fused)

  def perturb_(self, sigma: float, seed: int, offset: int = 0, antithetic: bool = True,
               frozen=None, fused: Optional[bool] = None):
    """Rows 0..P-1 = theta + sigma eps and, antithetic, rows P..2P-1 = theta -
    sigma eps (the reference's `add_noise` and concatenate; otherwise all n
    rows take theta + sigma eps), each one float32 rounding of the float64
    expression.

    `frozen` (n_params,) marks parameters every row takes from theta
    unperturbed (their counters are skipped). `fused`: None writes device rows
    with one `bx_population_perturb` launch, which regenerates eps on chip and
    touches only the rows, and takes the torch expression below otherwise;
    False forces the torch expression (the same bits); True raises
    NotImplementedError for rows off the device."""
    P = self._directions(antithetic)
    frozen = self._frozen(frozen)
    if self._fused(fused, 'perturbation'):
      theta = self.policy.params
      if theta.device != self.rows.device or theta.dtype != torch.float32 or not theta.is_contiguous():
        raise ValueError(f'the policy buffer must be contiguous float32 on {self.rows.device}')
      _native.check(_native.lib().bx_population_perturb(
          self.rows.data_ptr(), theta.data_ptr(), P, self.n_params, self.stride, float(sigma),
          int(seed), int(offset), int(bool(antithetic)),
          None if frozen is None else frozen.data_ptr(), _stream(self.rows.device.index)))
      return self
    step = float(sigma) * self.noise(seed, offset, antithetic).to(torch.float64)
    theta = self.policy.params.to(torch.float64)
    keep = None if frozen is None else frozen.bool()
    halves = [(slice(0, P), theta + step)]
    if antithetic:
      halves.append((slice(P, None), theta - step))
    for rows, value in halves:
      value = value.to(torch.float32)
      if keep is not None:
        value = torch.where(keep, self.policy.params, value)
      self.rows[rows, :self.n_params] = value
    return self

  def delta_workspace(self, antithetic: bool = True):
    """A workspace `weighted_noise_sum` takes, for a caller that sums every
    epoch: the library states the size, this allocates it."""
    P = self._directions(antithetic)
    need = C.c_int64(0)
    _native.check(_native.lib().bx_population_delta(None, None, P, self.n_params, 0, 0, None, None,
                                                    C.byref(need), None))
    return torch.empty((max(need.value // 8, 1),), dtype=torch.float64, device=self.rows.device)

  def weighted_noise_sum(self, weights, seed: int, offset: int = 0, antithetic: bool = True,
                         frozen=None, fused: Optional[bool] = None, workspace=None):
    """sum_p weights[p] eps[p] over the P directions of `perturb_(sigma, seed,
    offset, antithetic)`: `(n_params,)` float32, the float64 sum rounded once;
    zeros where `frozen`.

    `fused`: None takes `bx_population_delta` for device rows (eps regenerated
    on chip, a fixed summation order: the same bits from run to run), else the
    chained form `(weights.double()[:, None] * noise.double()).sum(0).float()`
    over `noise()`; False forces the chained form; True raises
    NotImplementedError for rows off the device. `workspace`: a contiguous
    float64 device tensor of at least `delta_workspace()`'s size to hold the
    kernel's partials (None: allocated per call)."""
    P = self._directions(antithetic)
    dev = self.rows.device
    w = torch.as_tensor(weights).to(dev, torch.float32).reshape(-1).contiguous()
    if w.numel() != P:
      raise ValueError(f'{w.numel()} weights for {P} directions')
    frozen = self._frozen(frozen)
    if not self._fused(fused, 'weighted noise sum'):
      s = (w.double()[:, None] * self.noise(seed, offset, antithetic).double()).sum(0).float()
      return s if frozen is None else torch.where(frozen.bool(), torch.zeros_like(s), s)
    if workspace is None:
      workspace = self.delta_workspace(antithetic)
    if (workspace.device != dev or workspace.dtype != torch.float64
        or not workspace.is_contiguous()):
      raise ValueError(f'workspace must be contiguous float64 on {dev}')
    out = torch.empty((self.n_params,), dtype=torch.float32, device=dev)
    size = C.c_int64(workspace.numel() * 8)
    _native.check(_native.lib().bx_population_delta(
        out.data_ptr(), w.data_ptr(), P, self.n_params, int(seed), int(offset),
        None if frozen is None else frozen.data_ptr(), workspace.data_ptr(), C.byref(size),
        _stream(dev.index)))
    return out

  def member(self, i: int) -> MLPPolicy:
    """An `MLPPolicy` over row i (a view: it sees later `set_` / `perturb_`)."""
    if not 0 <= int(i) < self.n_members:
      raise IndexError(f'member {i} of {self.n_members}')
    m = copy.copy(self.policy)
    m.params = self.rows[int(i), :self.n_params]
    return m


@dataclasses.dataclass(frozen=True)
class PopulationResult:
  """What `run_episode` keeps, per env: `scores` (B,) the shifted reward sum,
  `active`, `episode_steps`, `metric_sums` {key: (B,)} (`EvalWrapper`'s), and
  the observation moments `obs_s1`, `obs_s2` (B, O), `obs_count` (B,) (None
  with `moments=False`). `eval_buf` (M + 3, B) and `mom_buf` (B, 2 O + 1) are
  the launch's buffers (the fields above are views of them); `staged` tells
  whether each env's row was copied to LDS (None on the chained path)."""
  scores: Any
  active: Any
  episode_steps: Any
  metric_sums: Dict[str, Any]
  obs_s1: Any
  obs_s2: Any
  obs_count: Any
  metric_keys: Tuple[str, ...]
  eval_buf: Any
  mom_buf: Any
  staged: Optional[bool] = None


def _result(ev, mom, keys, O, staged=None):
  M = len(keys)
  return PopulationResult(
      scores=ev[M], active=ev[M + 1], episode_steps=ev[M + 2],
      metric_sums={k: ev[i] for i, k in enumerate(keys)},
      obs_s1=None if mom is None else mom[:, :O], obs_s2=None if mom is None else mom[:, O:2 * O],
      obs_count=None if mom is None else mom[:, 2 * O], metric_keys=tuple(keys), eval_buf=ev,
      mom_buf=mom, staged=staged)


def _split(population):
  """(policy, rows or None): an `MLPPolicy` is a population of one shared row."""
  if isinstance(population, PolicyPopulation):
    return population.policy, population
  if isinstance(population, MLPPolicy):
    return population, None
  raise ValueError(f'population must be a PolicyPopulation or an MLPPolicy, got {type(population).__name__}')


def _inner(env):
  return env.env if isinstance(env, wrappers.EvalWrapper) else env


def population_supported(env, population, param_stride: Optional[int] = None,
                         head: Optional[str] = None) -> Optional[str]:
  """None when `bx_env_eval_population` takes this env and population, else
  the library's reason (a zero-step call: argument checks only, no launch).
  `param_stride` / `head` override the population's (the library's refusals)."""
  policy, pop = _split(population)
  inner = _inner(env)
  why = fused_supported(inner, policy, trajectory=False)
  if why is not None:
    return why
  u, opts = chain_options(inner)
  desc = policy.descriptor(u.action_size)
  if pop is not None:
    desc.params = pop.rows.data_ptr()
  stride = (0 if pop is None else pop.stride) if param_stride is None else int(param_stride)
  arg = abi.BxPopulation(param_stride=stride,
                         head=abi.HEADS[policy.head] if head is None else abi.HEADS.get(head, -1))
  return packed.refusal(u, opts, 'bx_env_eval_population', policy=C.byref(desc),
                        pop=C.byref(arg))


def population_rollout(env, state: State, population, k: Optional[int] = None, seed: int = 0,
                       offset: int = 0, reward_shift: float = 0.0, moments: bool = True,
                       carry: Optional[PopulationResult] = None, fused: Optional[bool] = None,
                       stage: Optional[bool] = None, out: Optional[torch.Tensor] = None,
                       eval_out: Optional[torch.Tensor] = None,
                       mom_out: Optional[torch.Tensor] = None) -> Tuple[State, PopulationResult]:
  """K steps of a batch whose env e acts with member e of `population`.

  action_t[e] = member_e(obs_t[e], eps_t[e]) with `policy_rollout`'s noise
  (eps of step t, env e, action a = N(seed, offset + t * 2 B A + (e A + a) *
  2); an identity head draws none), then `env.step`; per env, in float32 and
  in this order, with a = active before the step and o the row the policy
  reads: S1 += a (o - mean), S2 += a (o - mean)^2, count += a (mean: the
  policy's `obs_mean`, or 0); after the step `EvalWrapper.step`'s recurrences
  with the reward sum taking `(reward - reward_shift) * active`.

  Args:
    env: a batched env (an `EvalWrapper` on top is looked through).
    population: a `PolicyPopulation` of B members, or an `MLPPolicy` (every
      env shares its row).
    k: the steps; None takes `episode_length // action_repeat` of the env's
      `EpisodeWrapper`.
    moments: False keeps no observation moments.
    carry: an earlier call's result to continue from (None: a fresh run).
    fused: None takes the kernel where the library allows it, else the chained
      path (a batched `torch.bmm` forward, `env.step`, the recurrences in
      torch); True raises NotImplementedError where the kernel refuses; False
      forces the chained path.
    stage: False reads the rows from global memory whatever the LDS budget
      (the same bits; None: the library's plan).
    out, eval_out, mom_out: optional buffers for the fused launch to write: a
      flat contiguous float32 of one block (`packed.Layout.block` floats), a
      contiguous float32 (M + 3, B) and a contiguous float32 (B, 2 O + 1); the
      result's tensors are views of them.
  Returns:
    (the state after the K-th step, the PopulationResult).
  """
  policy, pop = _split(population)
  inner = _inner(env)
  if k is None:
    w = inner
    while isinstance(w, wrappers.Wrapper) and not isinstance(w, wrappers.EpisodeWrapper):
      w = w.env
    if not isinstance(w, wrappers.EpisodeWrapper):
      raise ValueError('k=None needs an EpisodeWrapper in the chain')
    k = w.episode_length // w.action_repeat
  K = int(k)
  if K < 1:
    raise ValueError(f'k must be >= 1, got {k}')
  B = state.obs.shape[0]
  if pop is not None and pop.n_members != B:
    raise ValueError(f'the population holds {pop.n_members} members, the state {B} envs')
  if not use_kernel(fused, 'population rollout', lambda: population_supported(env, population)):
    return _chained(inner, state, policy, pop, K, seed, offset, reward_shift, moments, carry)
  u, opts = chain_options(inner)
  dev = u.sys.device
  qbuf = pack_qp(state.qp, dev)
  A = u.action_size
  inputs = packed.step_inputs(u, opts, state, B)
  keys = tuple(u.metric_keys)
  O, M = u.obs_size, len(keys)
  obs_in = packed.obs_input(u, state, B)
  ev, mom = _fresh(carry, keys, B, O, moments, dev)
  for name, buf, shape in (('eval_out', eval_out, (M + 3, B)), ('mom_out', mom_out, (B, 2 * O + 1))):
    if buf is not None:
      packed.output_buffer(name, buf, shape, dev)
  if eval_out is not None:
    ev = eval_out.copy_(ev)
  if mom_out is not None and mom is not None:
    mom = mom_out.copy_(mom)
  lay = packed.layout(u, B)
  out = lay.out_buffer(out, 1, dev)
  desc = policy.descriptor(A)
  if pop is not None:
    desc.params = pop.rows.data_ptr()
  mom_ptr = None if mom is None else mom.data_ptr()
  arg = abi.BxPopulation(param_stride=0 if pop is None else pop.stride, head=abi.HEADS[policy.head],
                         reward_shift=float(reward_shift), mom_in=mom_ptr, mom_out=mom_ptr,
                         flags=abi.POP_NO_STAGE if stage is False else 0)
  rng_out = packed.launch(u, 'bx_env_eval_population', inputs, qbuf, K, out, False, obs_in=obs_in,
                          policy=C.byref(desc), seed=int(seed), offset=int(offset),
                          step_stride=2 * B * A, eval_in=ev, eval_out=ev, pop=C.byref(arg))
  final = packed.final_state(
      u, inputs[0], state, lay.step_views(out[:lay.block]), rng_out,
      info={kk: v for kk, v in state.info.items() if kk != 'eval_metrics'})
  return final, _result(ev, mom, keys, O, bool(arg.staged))


def _fresh(carry, keys, B, O, moments, dev):
  """The launch's `(M + 3, B)` and `(B, 2 O + 1)` buffers: copies of the
  carried ones, or a fresh run's (zero sums, active 1)."""
  M = len(keys)
  if carry is not None:
    if tuple(carry.metric_keys) != tuple(keys) or tuple(carry.eval_buf.shape) != (M + 3, B):
      raise ValueError('carry does not come from this env and batch')
    if moments and carry.mom_buf is None:
      raise ValueError('carry holds no moments')
    ev = carry.eval_buf.to(dev, torch.float32).clone()
    mom = carry.mom_buf.to(dev, torch.float32).clone() if moments else None
    return ev, mom
  ev = torch.zeros((M + 3, B), dtype=torch.float32, device=dev)
  ev[M + 1] = 1.
  mom = torch.zeros((B, 2 * O + 1), dtype=torch.float32, device=dev) if moments else None
  return ev, mom


def forward_rows(policy: MLPPolicy, rows, obs, eps=None):
  """`policy.forward`'s action with env e's weights read from `rows[e]`
  (`(B, >= n_params)`; None: the policy's own row for every env): one
  `torch.bmm` per layer."""
  if rows is None:
    return policy.forward(obs, eps)[0]
  dt = obs.dtype
  x = obs
  if policy.obs_mean is not None:
    x = (x - policy.obs_mean.to(x.device, dt)) / policy.obs_std.to(x.device, dt)
  fn = _ACTIVATIONS[policy.activation]
  o = 0
  for l, (i, n) in enumerate(policy.sizes):
    w = rows[:, o:o + i * n].reshape(-1, i, n).to(x.device, dt)
    b = rows[:, o + i * n:o + (i + 1) * n].to(x.device, dt)
    x = torch.bmm(x[:, None, :], w)[:, 0] + b
    if l + 1 < len(policy.sizes):
      x = fn(x)
    o += (i + 1) * n
  return x if policy.head == 'identity' else normal_tanh_head(policy, x, eps)[0]


def _chained(env, state, policy, pop, K, seed, offset, reward_shift, moments, carry):
  """The same loop through `env.step`, the recurrences in the kernel's order:
  any env, any chain."""
  dev = torch.device(state.obs.device)
  B, A, O = state.obs.shape[0], env.action_size, state.obs.shape[1]
  policy.for_actions(A)
  try:
    keys = tuple(chain_options(env)[0].metric_keys)
  except NotImplementedError:
    keys = tuple(sorted(state.metrics.keys()))
  M = len(keys)
  ev, mom = _fresh(carry, keys, B, O, moments, dev)
  rows = None if pop is None else pop.rows
  shift = torch.tensor(float(reward_shift), dtype=torch.float32, device=dev)
  mean = None if policy.obs_mean is None else policy.obs_mean.to(dev)
  zeros = torch.zeros((B,), dtype=torch.float32, device=dev)
  for eps in step_noise(policy, K, B, A, int(seed), int(offset), 2 * B * A, dev):
    obs = state.obs.to(torch.float32)
    active = ev[M + 1].clone()
    if mom is not None:
      d = obs if mean is None else obs - mean
      mom[:, :O] += active[:, None] * d
      mom[:, O:2 * O] += active[:, None] * (d * d)
      mom[:, 2 * O] += active
    state = env.step(state, forward_rows(policy, rows, obs, eps))
    steps = _f32(state.info.get('steps', zeros), dev)
    ev[M + 2] = torch.where(active != 0, steps, ev[M + 2])
    for i, kk in enumerate(keys):
      ev[i] += _f32(state.metrics[kk], dev) * active
    ev[M] += (_f32(state.reward, dev) - shift) * active
    ev[M + 1] = active * (1 - _f32(state.done, dev))
  return state, _result(ev, mom, keys, O)


def update_running_statistics(mean, summed_variance, count, result, std_min: float = 1e-6,
                              std_max: float = 1e6):
  """`running_statistics.update` (`acme/running_statistics.py:156-173`) of the
  normaliser from a result's moments, in float64. The moments are centred on
  the old mean (the policy's `obs_mean`; zeros when it had none), so with
  u = sum S1 / count': mean' = mean + u, summed_variance' += sum S2 - u sum S1
  (= sum a (o - mean)(o - mean')), exactly the reference's update.

  `result`: a `PopulationResult`, or `(obs_s1, obs_s2, obs_count)`. Returns
  float64 numpy `(mean, summed_variance, count, std)`.
  """
  if isinstance(result, PopulationResult):
    result = (result.obs_s1, result.obs_s2, result.obs_count)
  s1, s2, n = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, np.float64)
               for x in result)
  mean = np.asarray(mean, np.float64)
  summed_variance = np.asarray(summed_variance, np.float64)
  S1 = s1.reshape(-1, mean.shape[-1]).sum(0)
  S2 = s2.reshape(-1, mean.shape[-1]).sum(0)
  step = float(n.sum())
  new_count = float(count) + step
  u = S1 / new_count
  new_mean = mean + u
  new_sv = summed_variance + (S2 - u * S1)
  # (the summed variance can get negative by rounding: the std clamps it)
  std = np.clip(np.sqrt(np.maximum(new_sv, 0.) / new_count), std_min, std_max)
  return new_mean, new_sv, new_count, std
