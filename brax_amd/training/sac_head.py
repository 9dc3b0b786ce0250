"""The SAC loss heads: a gradient step's three losses between the networks,
in four launches.

`sac.sgd_step`'s chained form builds the alpha, critic and actor losses as
torch expressions (`sac_losses`) and lets autograd walk them: the NormalTanh
sample three times, two observation normalisations, `cat`, `min`, the means and
their elementwise backward, some 150 small launches. `gradients` is the same
three gradients over `bx_sac_head_*` (`include/brax_amd.h`):

1. `prep`: the critics' inputs `X_cur = [n(obs) | action]`, `X_next =
   [n(next_obs) | .]`, `X_pi = [n(obs) | .]`; the policy reads the column
   slices `X_pi[:, :O]` and `X_next[:, :O]` in place;
2. the policy on `X_pi[:, :O]` (once: the alpha and the actor loss differ in
   `eps` alone) and on `X_next[:, :O]`;
3. `sample`: the three jobs' actions (into the `X` buffers) and log-probs;
4. `Q(X_cur)`, `Qtarget(X_next)`, and `Q` with detached layers on `X_pi`;
5. `losses`: the Bellman target, the gradients in the critics' outputs and in
   the actor's log-prob;
6. the critics' backward passes (`dW` from `X_cur`, `dx` from `X_pi`);
7. `sample_backward`: `dlogits`, and the three losses and `dlog_alpha` from
   the partial sums `losses` left;
8. the policy's backward pass.

The networks go through `networks.mlp(..., fused_mlp)` as in the chained form.
With `fused_group` step 4's six critic evaluations are one forward launch and
step 6's four backward passes two (`fused_mlp.group_forward` /
`group_backward`): each member's bits are the ungrouped call's.
"""
import ctypes as C
from typing import Optional

import torch

from brax_amd import _native, abi
from brax_amd.system import launch
from brax_amd.training import fused_mlp as fused_mlp_lib
from brax_amd.training import sac_losses
from brax_amd.training.networks import detached, mlp, parameters
from brax_amd.training.sac_networks import ACTIVATION

METRICS = ('critic_loss', 'actor_loss', 'alpha_loss')
_FLAGS = ('reward', 'discount', 'truncation')


class Metrics(dict):
  """The losses' metrics dict; the fused form also hands out the three values
  as one detached `(3,)` tensor in `METRICS`' order (`vector`, else None)."""
  vector = None


def fused_supported(ts, normalizer, transitions, eps) -> Optional[str]:
  """None when `bx_sac_head_*` take this step's tensors, else why not."""
  obs = transitions['observation']
  if obs.dim() != 2:
    return f'observation {tuple(obs.shape)} is not (B, O)'
  B, O = obs.shape
  if len(eps) != 3:
    return f'{len(eps)} eps tensors, not 3'
  A = eps[0].shape[-1]
  named = [('observation', obs, (B, O)), ('next_observation', transitions['next_observation'], (B, O)),
           ('action', transitions['action'], (B, A))]
  named += [(f'eps[{k}]', e, (B, A)) for k, e in enumerate(eps)]
  if normalizer is not None:
    named += [('mean', normalizer[0], (O,)), ('std', normalizer[1], (O,))]
  for name, t, shape in named:
    if tuple(t.shape) != shape:
      return f'{name} {tuple(t.shape)} is not {shape}'
  flags = [(n, transitions[n]) for n in _FLAGS]
  for name, t in flags:
    if tuple(t.shape) not in ((B,), (B, 1)):
      return f'{name} {tuple(t.shape)} is not ({B},) or ({B}, 1)'
  if O < 1 or A < 1:
    return f'no observation or action ({O}, {A})'
  C_ = len(ts.q_layers)
  if not 1 <= C_ <= abi.SAC_MAX_CRITICS or len(ts.target_q_layers) != C_:
    return f'{C_} critics, the kernels take 1..{abi.SAC_MAX_CRITICS}'
  tensors = [(n, t) for n, t, _ in named] + flags + [('log_alpha', ts.log_alpha)]
  tensors += [('a network parameter', p) for p in
              parameters(ts.policy_layers, *ts.q_layers, *ts.target_q_layers)]
  for name, t in tensors:
    if t.dtype != torch.float32:
      return f'{name}: {t.dtype} is not float32'
  for name, t, shape in named:
    if shape[-1] > 1 and t.stride(-1) != 1:
      return f'{name} has inner stride {t.stride(-1)}, not 1'
  for name, t, shape in named:
    if len(shape) == 2 and B > 1 and t.stride(0) < shape[1]:
      return f'{name} has row stride {t.stride(0)} below its width {shape[1]}'
  if B > 2 ** 31:
    return f'{B} rows, the kernels take 2^31'
  # (the device last, so the reasons above can be read off CPU tensors too)
  for name, t in tensors:
    if not t.is_cuda:
      return f'{name} is a CPU tensor'
    if t.device != obs.device:
      return f'tensors on {obs.device} and {t.device}'
  return None


def _pitch(t):
  """The row pitch of a (B, W) tensor with unit inner stride (one row: W)."""
  return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def workspace_floats(B: int) -> int:
  """The workspace `bx_sac_head_losses` and `_sample_backward` ask for at B
  rows, in float32 elements."""
  nbytes = C.c_int64(0)
  _native.check(_native.lib().bx_sac_head_losses(
      B, 1, None, None, None, None, None, 0, None, 0, None, 0, None, 0.0, 0.0, 0.0, None, None,
      C.byref(nbytes), None))
  return (nbytes.value + 3) // 4


def prep_call(obs, next_obs, action, normalizer, x_cur, x_next, x_pi):
  """`bx_sac_head_prep`: fills the three `(B, O + A)` buffers (one pitch)."""
  B, O = obs.shape
  A = action.shape[1]
  if B == 0:
    return
  assert _pitch(x_cur) == _pitch(x_next) == _pitch(x_pi)
  mean, std = (None, None) if normalizer is None else (normalizer[0].contiguous(),
                                                       normalizer[1].contiguous())
  launch(obs.device, 'bx_sac_head_prep',
         B, O, A, obs.data_ptr(), _pitch(obs), next_obs.data_ptr(), _pitch(next_obs),
         action.data_ptr(), _pitch(action), None if mean is None else mean.data_ptr(),
         None if std is None else std.data_ptr(), x_cur.data_ptr(), x_next.data_ptr(),
         x_pi.data_ptr(), _pitch(x_cur))


def sample_call(jobs, min_std=sac_losses.MIN_STD):
  """`bx_sac_head_sample`: `jobs` is up to three `(logits (B, 2A), eps (B, A),
  action out (B, A) or None, log_prob out (B,))`, one launch for all."""
  logits = jobs[0][0]
  B, A = logits.shape[0], logits.shape[1] // 2
  if B == 0:
    return
  table = (abi.BxSacSampleJob * len(jobs))()
  for j, (lg, eps, action, log_prob) in zip(table, jobs):
    j.logits, j.logits_pitch = lg.data_ptr(), _pitch(lg)
    j.eps, j.eps_pitch = eps.data_ptr(), _pitch(eps)
    if action is not None:
      j.action, j.action_pitch = action.data_ptr(), _pitch(action)
    j.log_prob = log_prob.data_ptr()
  launch(logits.device, 'bx_sac_head_sample', B, A, table, len(jobs), min_std)


def _flag(t):
  return t.data_ptr(), t.stride(0)


def losses_call(log_probs, q_old, next_q, q_pi, reward, discount, truncation, log_alpha,
                reward_scaling, discounting, target_entropy, dq_old, dq_pi, g_lp, workspace):
  """`bx_sac_head_losses`: `log_probs` is the alpha, critic and actor jobs'
  `(B,)`; `q_old`, `next_q`, `q_pi`, `dq_old` and `dq_pi` are C contiguous
  `(B,)` or `(B, 1)` tensors each. The losses themselves come out of
  `sample_backward_call` on the same workspace."""
  B, n = log_probs[0].shape[0], len(q_old)
  if B == 0:
    return
  q = abi.BxSacQ()
  for name, ts_ in (('q_old', q_old), ('next_q', next_q), ('q_pi', q_pi), ('dq_old', dq_old),
                    ('dq_pi', dq_pi)):
    for c, t in enumerate(ts_):
      assert t.is_contiguous() and t.numel() == B
      getattr(q, name)[c] = t.data_ptr()
  nbytes = C.c_int64(workspace.numel() * 4)
  launch(g_lp.device, 'bx_sac_head_losses',
         B, n, log_probs[0].data_ptr(), log_probs[1].data_ptr(), log_probs[2].data_ptr(),
         C.byref(q), *_flag(reward), *_flag(discount), *_flag(truncation), log_alpha.data_ptr(),
         reward_scaling, discounting, target_entropy, g_lp.data_ptr(), workspace.data_ptr(),
         C.byref(nbytes))


def sample_backward_call(logits, eps, g_lp, dactions, dlogits, losses, dlog_alpha, workspace,
                         min_std=sac_losses.MIN_STD):
  """`bx_sac_head_sample_backward`: `dactions` is C `(B, A)` tensors (column
  slices of the critics' input gradients pass without a copy); writes `dlogits
  (B, 2A)`, `losses (3,)` and the 0-d `dlog_alpha`."""
  B, A = eps.shape
  if B == 0:
    return
  da = abi.BxSacDaction()
  for c, t in enumerate(dactions):
    da.ptr[c], da.pitch[c] = t.data_ptr(), _pitch(t)
  nbytes = C.c_int64(workspace.numel() * 4)
  launch(logits.device, 'bx_sac_head_sample_backward',
         B, A, len(dactions), logits.data_ptr(), _pitch(logits), eps.data_ptr(), _pitch(eps),
         g_lp.data_ptr(), C.byref(da), min_std, dlogits.data_ptr(), _pitch(dlogits),
         losses.data_ptr(), dlog_alpha.data_ptr(), workspace.data_ptr(), C.byref(nbytes))


_BUFFERS = {}


def _buffers(dev, B, O, A, n):
  """The step's buffers, allocated once per (device, B, O, A, C)."""
  key = (dev, B, O, A, n)
  if key not in _BUFFERS:
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    _BUFFERS[key] = dict(
        x_cur=new(B, O + A), x_next=new(B, O + A), x_pi=new(B, O + A),
        log_probs=[new(B) for _ in range(3)], dq_old=[new(B, 1) for _ in range(n)],
        dq_pi=[new(B, 1) for _ in range(n)], g_lp=new(B), dlogits=new(B, 2 * A),
        workspace=new(max(workspace_floats(B), 4)))
  return _BUFFERS[key]


def _unit_rows(t):
  return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


def gradients(ts, normalizer, transitions, eps, reward_scaling: float = 1.0,
              discounting: float = 0.9, fused_mlp=False, fused_group=False):
  """The three gradients of one SAC step through the kernels.

  Args as `sac.sgd_step`'s; the tensors must pass `fused_supported`.
  Returns:
    `(a_grads, c_grads, p_grads, metrics)`: the gradients in `[log_alpha]`, in
    `q_parameters(ts.q_layers)` and in `parameters(ts.policy_layers)`, and a
    `Metrics` of critic_loss, actor_loss and alpha_loss.
  """
  obs, next_obs, action = (transitions[k] for k in ('observation', 'next_observation', 'action'))
  eps_alpha, eps_critic, eps_actor = eps
  dev = obs.device
  B, O = obs.shape
  A, n = action.shape[1], len(ts.q_layers)
  buf = _buffers(dev, B, O, A, n)
  x_cur, x_next = buf['x_cur'], buf['x_next']
  # (a leaf over the buffer's storage: the critics' input gradient is taken in it)
  x_pi = buf['x_pi'].detach().requires_grad_()
  out = torch.empty((4,), dtype=torch.float32, device=dev)  # the step's own: it is handed out
  losses, dlog_alpha = out[:3], out[3]
  if B == 0:
    out.fill_(float('nan'))  # the chained form's means over nothing
  prep_call(obs, next_obs, action, normalizer, x_cur, x_next, buf['x_pi'])
  policy_params = parameters(ts.policy_layers)
  logits = mlp(ts.policy_layers, buf['x_pi'][:, :O], ACTIVATION, fused_mlp)
  with torch.no_grad():
    next_logits = mlp(ts.policy_layers, x_next[:, :O], ACTIVATION, fused_mlp)
  lg = _unit_rows(logits.detach())
  sample_call([(lg, eps_alpha, None, buf['log_probs'][0]),
               (_unit_rows(next_logits), eps_critic, x_next[:, O:], buf['log_probs'][1]),
               (lg, eps_actor, buf['x_pi'][:, O:], buf['log_probs'][2])])
  # the critics' evaluations: Q on X_cur, Qtarget on X_next, Q on X_pi
  evals = [(c, x) for cs, x in ((ts.q_layers, x_cur), (ts.target_q_layers, x_next),
                                (ts.q_layers, buf['x_pi'])) for c in cs]
  group = fused_mlp_lib.use_group(fused_group, fused_mlp, evals, ACTIVATION)
  if group:
    members = [(parameters(detached(c)), x, ACTIVATION) for c, x in evals]
    ys, saveds = fused_mlp_lib.group_forward(members, [True] * n + [False] * n + [True] * n)
    q_old, next_q, q_pi = ys[:n], ys[n:2 * n], ys[2 * n:]
  else:
    q_old = [mlp(c, x_cur, ACTIVATION, fused_mlp) for c in ts.q_layers]
    with torch.no_grad():
      next_q = [mlp(c, x_next, ACTIVATION, fused_mlp) for c in ts.target_q_layers]
    q_pi = [mlp(detached(c), x_pi, ACTIVATION, fused_mlp) for c in ts.q_layers]
  flat = lambda ts_: [t.detach().contiguous() for t in ts_]  # noqa: E731
  losses_call(buf['log_probs'], flat(q_old), flat(next_q), flat(q_pi), transitions['reward'],
              transitions['discount'], transitions['truncation'], ts.log_alpha.detach(),
              reward_scaling, discounting, sac_losses.target_entropy(A), buf['dq_old'],
              buf['dq_pi'], buf['g_lp'], buf['workspace'])
  c_grads = []
  if group:
    # dW / db from X_cur and dx from X_pi; the target critics take no part
    on = members[:n] + members[2 * n:]
    dxs, grads = fused_mlp_lib.group_backward(
        on, saveds[:n] + saveds[2 * n:], buf['dq_old'] + buf['dq_pi'], [False] * n + [True] * n,
        [[True] * len(m[0]) for m in on[:n]] + [[False] * len(m[0]) for m in on[n:]])
    for g in grads[:n]:
      c_grads += g
    dx = dxs[n:]
  else:
    for c, q in zip(range(n), q_old):
      c_grads += torch.autograd.grad(q, parameters(ts.q_layers[c]), grad_outputs=buf['dq_old'][c])
    dx = [_unit_rows(torch.autograd.grad(q, x_pi, grad_outputs=buf['dq_pi'][c])[0])
          for c, q in enumerate(q_pi)]
  sample_backward_call(lg, eps_actor, buf['g_lp'], [d[:, O:] for d in dx], buf['dlogits'], losses,
                       dlog_alpha, buf['workspace'])
  p_grads = torch.autograd.grad(logits, policy_params, grad_outputs=buf['dlogits'])
  metrics = Metrics(critic_loss=losses[0], actor_loss=losses[1], alpha_loss=losses[2])
  metrics.vector = losses
  return (dlog_alpha,), tuple(c_grads), tuple(p_grads), metrics
