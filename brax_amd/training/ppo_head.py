"""The PPO loss head: from the networks' outputs to the loss, in two launches.

`ppo_head` is the part of `losses.ppo_loss` after the three network
evaluations: the NormalTanh log-prob of the recorded actions, the GAE targets,
the advantage normalisation, the clipped surrogate, the value loss and the
entropy term. As chained torch (`_chained`, the lines `ppo_loss` has always
run) it is a few dozen elementwise and reduction launches forward and as many
backward on `(T, B, A)` arrays of a few tens of thousands of floats.

The fused form is `bx_ppo_head` (`include/brax_amd.h`): the loss, its three
parts and the gradients in `logits` and `baseline` come out of one call of two
launches, the GAE scan included (so `compute_gae`'s `fused` is not consulted).
It is a `torch.autograd.Function` over `(logits, baseline)` whose backward
scales the saved gradients by the incoming one. `bootstrap_value` gets no
gradient in either form: `compute_gae` detaches it.
"""
import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from brax_amd import _native, abi
from brax_amd.envs.policy import head_scale, normal_tanh_log_prob, tanh_log_det
from brax_amd.fused import use_kernel
from brax_amd.system import launch
from brax_amd.training.gae import compute_gae

METRICS = ('total_loss', 'policy_loss', 'v_loss', 'entropy_loss')


class Metrics(dict):
  """The four-key metrics dict; the fused form also hands out the four values
  as one detached `(4,)` tensor in `METRICS`' order (`vector`, else None)."""
  vector = None


_SEQS = ('reward', 'discount', 'truncation', 'log_prob')


def entropy(loc, scale, eps):
  """`ParametricDistribution.entropy` (`training/distribution.py:83-91`): the
  Normal's entropy plus the tanh log-det at the sample loc + scale * eps,
  summed over the actions."""
  normal = 0.5 + (0.5 * math.log(2.0 * math.pi) + torch.log(scale))
  return (normal + tanh_log_det(loc + scale * eps)).sum(-1)


def _chained(logits, baseline, bootstrap_value, data, eps, entropy_cost, discounting,
             reward_scaling, gae_lambda, clipping_epsilon, normalize_advantage, min_std, fused_gae,
             gae=None):
  loc, s = torch.chunk(logits, 2, dim=-1)
  scale = head_scale(s, min_std)
  target_log_probs = normal_tanh_log_prob(loc, scale, data.raw_action).sum(-1)
  # termination = (1 - discount) * (1 - truncation): compute_gae forms the
  # product from done = 1 - discount; the reward scaling is folded in as well
  vs, advantages = (gae or compute_gae)(
      truncation=data.truncation, termination=1 - data.discount, rewards=data.reward,
      values=baseline, bootstrap_value=bootstrap_value, lambda_=gae_lambda,
      discount=discounting, reward_scaling=reward_scaling, fused=fused_gae)
  if normalize_advantage:
    advantages = (advantages - advantages.mean()) / (advantages.std(unbiased=False) + 1e-8)
  rho_s = torch.exp(target_log_probs - data.log_prob)
  surrogate_loss1 = rho_s * advantages
  surrogate_loss2 = torch.clamp(rho_s, 1 - clipping_epsilon, 1 + clipping_epsilon) * advantages
  policy_loss = -torch.mean(torch.minimum(surrogate_loss1, surrogate_loss2))
  v_error = vs - baseline
  v_loss = torch.mean(v_error * v_error) * 0.5 * 0.5
  entropy_loss = entropy_cost * -torch.mean(entropy(loc, scale, eps.to(loc.dtype)))
  total_loss = policy_loss + v_loss + entropy_loss
  return total_loss, {'total_loss': total_loss, 'policy_loss': policy_loss, 'v_loss': v_loss,
                      'entropy_loss': entropy_loss}


def fused_supported(logits, baseline, bootstrap_value, data, eps) -> Optional[str]:
  """None when `bx_ppo_head` takes these tensors, else why not."""
  if logits.dim() != 3 or logits.shape[-1] % 2 or logits.shape[-1] < 2:
    return f'logits {tuple(logits.shape)} are not (T, B, 2 A)'
  T, B, A = logits.shape[0], logits.shape[1], logits.shape[2] // 2
  if T < 1:
    return 'no time step'
  named = [('logits', logits, (T, B, 2 * A)), ('baseline', baseline, (T, B)),
           ('bootstrap_value', bootstrap_value, (B,)), ('raw_action', data.raw_action, (T, B, A)),
           ('eps', eps, (T, B, A))] + [(n, getattr(data, n), (T, B)) for n in _SEQS]
  for name, t, shape in named:
    if tuple(t.shape) != shape:
      return f'{name} {tuple(t.shape)} is not {shape}'
  for name, t, _ in named:
    if t.dtype != torch.float32:
      return f'{name}: {t.dtype} is not float32'
  for name, t, shape in named:
    if len(shape) == 3 and shape[-1] > 1 and t.stride(-1) != 1:
      return f'{name} has inner stride {t.stride(-1)}, not 1'
  if T * B > 2 ** 31:
    return f'{T * B} rows, the kernels take 2^31'
  # (the device last, so the reasons above can be read off CPU tensors too)
  for name, t, _ in named:
    if not t.is_cuda:
      return f'{name} is a CPU tensor'
    if t.device != logits.device:
      return f'tensors on {logits.device} and {t.device}'
  return None


def _seq(t):
  return abi.BxSeq(t.data_ptr(), t.stride(0), t.stride(1))


def _rows(t):
  """A (T, B, W) tensor with unit stride along W (W == 1: any stride will do)."""
  return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


def head_call(logits, baseline, bootstrap_value, data, eps, entropy_cost, discounting,
              reward_scaling, gae_lambda, clipping_epsilon, normalize_advantage, min_std,
              want_gae=False, out=None, workspace=None):
  """One `bx_ppo_head` call on detached float32 device tensors.

  Returns `(losses (4,), dlogits (T, B, 2A), dbaseline (T, B), vs, advantages)`,
  the last two None unless `want_gae`. `out` may hold preallocated tensors
  under those five names (any layout the header allows), `workspace` a float32
  tensor of at least `workspace_floats(T, B)` elements, 16-byte aligned."""
  dev = logits.device
  T, B, A = logits.shape[0], logits.shape[1], logits.shape[2] // 2
  out = dict(out or {})
  new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
  losses = out.get('losses', None)
  losses = new(4) if losses is None else losses
  dlogits = out['dlogits'] if 'dlogits' in out else new(T, B, 2 * A)
  dbaseline = out['dbaseline'] if 'dbaseline' in out else new(T, B)
  vs = out.get('vs', new(T, B) if want_gae else None)
  adv = out.get('advantages', new(T, B) if want_gae else None)
  if B == 0:
    losses.fill_(float('nan'))  # the chained form's means over nothing
    return losses, dlogits, dbaseline, vs, adv
  if workspace is None:
    workspace = new(workspace_floats(T, B))
  nbytes = C.c_int64(workspace.numel() * 4)
  # (held until the launches are queued: three may be fresh tensors)
  held = (_rows(logits), baseline, _rows(data.raw_action), _rows(eps), data.log_prob, data.reward,
          1 - data.discount, data.truncation, dlogits, dbaseline)
  seqs = [_seq(t) for t in held]
  opt = [None if t is None else _seq(t) for t in (vs, adv)]
  boot = bootstrap_value.contiguous()
  launch(dev, 'bx_ppo_head',
         T, B, A, C.byref(seqs[0]), C.byref(seqs[1]), boot.data_ptr(), C.byref(seqs[2]),
         C.byref(seqs[3]), C.byref(seqs[4]), C.byref(seqs[5]), C.byref(seqs[6]), C.byref(seqs[7]),
         reward_scaling, discounting, gae_lambda, clipping_epsilon, entropy_cost, min_std,
         int(bool(normalize_advantage)), losses.data_ptr(), C.byref(seqs[8]), C.byref(seqs[9]),
         None if opt[0] is None else C.byref(opt[0]), None if opt[1] is None else C.byref(opt[1]),
         workspace.data_ptr(), C.byref(nbytes))
  del held
  return losses, dlogits, dbaseline, vs, adv


def workspace_floats(T: int, B: int) -> int:
  """The workspace `bx_ppo_head` asks for at (T, B), in float32 elements."""
  nbytes = C.c_int64(0)
  _native.check(_native.lib().bx_ppo_head(
      T, B, 1, *[None] * 9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, *[None] * 6, C.byref(nbytes), None))
  return (nbytes.value + 3) // 4


class _FusedHead(torch.autograd.Function):
  """`(logits, baseline, bootstrap_value, data, eps, hyper)` -> losses (4,):
  total, policy, v, entropy. Differentiable in `logits` and `baseline` through
  element 0 alone (the other three are returned detached by `ppo_head`)."""

  @staticmethod
  def forward(ctx, logits, baseline, bootstrap_value, data, eps, hyper):
    d = lambda t: t.detach()  # noqa: E731
    losses, dlogits, dbaseline, _, _ = head_call(
        d(logits), d(baseline), d(bootstrap_value), data, d(eps), **hyper)
    ctx.save_for_backward(dlogits, dbaseline)
    return losses

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, dlosses):
    dlogits, dbaseline = ctx.saved_tensors
    need = ctx.needs_input_grad
    g = dlosses[0]
    return (dlogits * g if need[0] else None, dbaseline * g if need[1] else None,
            None, None, None, None)


def ppo_head(logits, baseline, bootstrap_value, data, eps, entropy_cost: float = 1e-4,
             discounting: float = 0.9, reward_scaling: float = 1.0, gae_lambda: float = 0.95,
             clipping_epsilon: float = 0.3, normalize_advantage: bool = True,
             min_std: float = 1e-3, fused: Optional[bool] = None,
             fused_gae: Optional[bool] = None, gae=None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
  """`(total_loss, metrics)` from the networks' outputs, time first.

  Args:
    logits: `(T, B, 2A)`, the policy network's output.
    baseline: `(T, B)`, the value network's; bootstrap_value: `(B,)`, its
      value of the observation after the last step.
    data: a `losses.Transition` whose leading dimensions are `[T, B]` (views
      of `[B, T]` arrays pass without a copy); `raw_action`, `log_prob`,
      `reward`, `discount` and `truncation` are read.
    eps: `(T, B, A)` standard-normal draws for the entropy term's sample.
    fused: None takes `bx_ppo_head` where `fused_supported` has no objection,
      else the chained form; True raises NotImplementedError where the kernel
      does not apply; False is the chained form.
    fused_gae: the chained form's `compute_gae(fused=...)`; the kernel runs its
      own scan and does not read it.
    gae: the chained form's GAE function (default `gae.compute_gae`).
  Returns:
    the total loss and `{'total_loss', 'policy_loss', 'v_loss',
    'entropy_loss'}`; in the fused form only the total carries a gradient.
  """
  hyper = dict(entropy_cost=entropy_cost, discounting=discounting, reward_scaling=reward_scaling,
               gae_lambda=gae_lambda, clipping_epsilon=clipping_epsilon,
               normalize_advantage=normalize_advantage, min_std=min_std)
  if use_kernel(fused, 'ppo_head',
                lambda: fused_supported(logits, baseline, bootstrap_value, data, eps)):
    # (detached here as compute_gae detaches it: the network that produced
    # it then has no backward pass to run on a zero gradient)
    losses = _FusedHead.apply(logits, baseline, bootstrap_value.detach(), data, eps, hyper)
    total, parts = losses[0], losses.detach()
    metrics = Metrics(total_loss=total, policy_loss=parts[1], v_loss=parts[2],
                      entropy_loss=parts[3])
    metrics.vector = parts
    return total, metrics
  return _chained(logits, baseline, bootstrap_value, data, eps, fused_gae=fused_gae,
                  gae=gae, **hyper)
