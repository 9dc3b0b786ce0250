"""The PPO loss head without a GPU: the ABI mirror of `bx_ppo_head`, its
refusals (host pointers: a launch would fault), `fused_supported`'s reasons,
and the chained form's bits (`ppo_head(fused=False)` is `ppo_loss`'s tail)."""
import ctypes as C

import pytest
import torch

from brax_amd import _native, abi
from brax_amd.training import networks
from brax_amd.training import ppo_head as ph
from brax_amd.training.losses import Transition, normalize, ppo_loss


def test_header_abi_and_exports():
  # (bx_ppo_head's names and types against the header: tests/test_abi.py)
  # additive: the version stays
  assert abi.ABI_VERSION == 14 and _native.lib().bx_abi_version() == 14


def _call(lib, p, T=3, B=5, A=2, nb=None, ws=None, **null):
  """bx_ppo_head on host memory `p`; a keyword names an argument to pass as
  NULL ('x') or as a bx_seq with a null ptr ('x_ptr')."""
  seq = lambda name: (None if name in null else  # noqa: E731
                      C.byref(abi.BxSeq(None if name + '_ptr' in null else p, B, 1)))
  ptr = lambda name: None if name in null else p  # noqa: E731
  return lib.bx_ppo_head(
      T, B, A, seq('logits'), seq('baseline'), ptr('bootstrap'), seq('raw_action'), seq('eps'),
      seq('log_prob'), seq('reward'), seq('done'), seq('truncation'), 1.0, 0.9, 0.95, 0.3, 1e-4,
      1e-3, 1, ptr('losses'), seq('dlogits'), seq('dbaseline'), seq('vs'), seq('advantages'),
      p if ws is None else ws, None if 'workspace_bytes' in null else C.byref(nb), None)


def test_refusals_before_any_launch():
  """Every refusal sets bx_last_error and returns before a device call (the
  pointers here are host memory: a launch would fault)."""
  lib = _native.lib()
  buf = (C.c_float * 64)()
  p = C.addressof(buf)
  big = C.c_int64(1 << 30)
  cases = [(dict(workspace_bytes=1), b'null'), (dict(T=0), b'n_steps must be >= 1'),
           (dict(A=0), b'n_actions must be >= 1'), (dict(B=-1), b'negative n_envs'),
           (dict(A=(1 << 20) + 1), b'too many actions'),
           (dict(T=1 << 16, B=(1 << 15) + 1), b'too many rows'),
           (dict(bootstrap=1), b'null'), (dict(losses=1), b'null'),
           (dict(ws=p + 4), b'workspace not 16-byte aligned')]
  for name in ('logits', 'baseline', 'raw_action', 'eps', 'log_prob', 'reward', 'done',
               'truncation', 'dlogits', 'dbaseline'):
    cases += [({name: 1}, b'null'), ({name + '_ptr': 1}, b'null')]
  for kw, word in cases:
    assert _call(lib, p, nb=big, **kw) != 0 and word in lib.bx_last_error(), (kw, lib.bx_last_error())
  # (3, 5): 8 (4 + 1) + 8 * 15 = 160 bytes
  assert _call(lib, p, nb=C.c_int64(159)) != 0
  assert b'workspace of 159 bytes, 160 needed' in lib.bx_last_error()
  # a zero stride on an output
  z = abi.BxSeq(p, 0, 1)
  ok = lambda: C.byref(abi.BxSeq(p, 5, 1))  # noqa: E731
  assert lib.bx_ppo_head(3, 5, 2, ok(), ok(), p, ok(), ok(), ok(), ok(), ok(), ok(), 1.0, 0.9, 0.95,
                         0.3, 1e-4, 1e-3, 1, p, ok(), C.byref(z), None, None, p, C.byref(big),
                         None) != 0
  assert b'zero stride on an output' in lib.bx_last_error()
  # no envs: a successful no-op, whatever the pointers
  assert _call(lib, p, B=0, nb=big, logits=1, dlogits=1, losses=1) == 0
  # the size query
  for (T, B), want in (((3, 5), 160), ((1, 1), 48), ((5, 1024), 8 * (16 + 20) + 8 * 5120),
                       ((2, 257), 8 * (8 + 3) + 8 * 514), ((4, 0), 0)):
    q = C.c_int64(-1)
    assert _call(lib, p, T=T, B=B, nb=q, ws=0, logits=1) == 0
    assert q.value == (want + 15) // 16 * 16, (T, B)
  assert ph.workspace_floats(3, 5) == 40


def _case(T=4, B=6, A=3, O=7, seed=0, dtype=torch.float32):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(s, generator=g).to(dtype)  # noqa: E731
  flags = lambda p: (torch.rand((B, T), generator=g) < p).to(dtype)  # noqa: E731
  data = Transition(observation=r(B, T, O), action=r(B, T, A), reward=r(B, T),
                    discount=1 - flags(0.2), next_observation=r(B, T, O), truncation=flags(0.2),
                    raw_action=r(B, T, A), log_prob=-2 * A + r(B, T))
  return data, r(B, T, A)


def test_fused_supported_names_the_reason():
  T, B, A = 4, 6, 3
  data, eps = _case(T, B, A)
  data, eps = data.map(lambda x: x.transpose(0, 1)), eps.transpose(0, 1)
  logits, baseline, boot = torch.zeros((T, B, 2 * A)), torch.zeros((T, B)), torch.zeros((B,))
  why = lambda **kw: ph.fused_supported(**{**dict(logits=logits, baseline=baseline,  # noqa: E731
                                                  bootstrap_value=boot, data=data, eps=eps), **kw})
  assert why() == 'logits is a CPU tensor'
  assert 'not (T, B, 2 A)' in why(logits=torch.zeros((T, B, 5)))
  assert 'not (T, B, 2 A)' in why(logits=torch.zeros((T * B, 6)))
  assert 'no time step' in why(logits=torch.zeros((0, B, 6)))
  assert 'baseline (6, 4) is not (4, 6)' in why(baseline=torch.zeros((B, T)))
  assert 'bootstrap_value (4,) is not (6,)' in why(bootstrap_value=torch.zeros((T,)))
  assert 'eps (4, 6, 2) is not (4, 6, 3)' in why(eps=torch.zeros((T, B, 2)))
  assert 'torch.float64 is not float32' in why(baseline=baseline.double())
  assert 'reward: torch.float64' in why(data=Transition(**{**vars(data), 'reward': data.reward.double()}))
  assert 'eps has inner stride 2' in why(eps=torch.zeros((T, B, 2 * A))[..., ::2])
  with pytest.raises(NotImplementedError, match='no fused ppo_head: logits is a CPU tensor'):
    ph.ppo_head(logits, baseline, boot, data, eps, fused=True)
  # None falls back to the chained form
  a = ph.ppo_head(logits, baseline, boot, data, eps, fused=None)
  b = ph.ppo_head(logits, baseline, boot, data, eps, fused=False)
  assert torch.equal(a[0], b[0]) and sorted(a[1]) == sorted(ph.METRICS)


def _loss_and_grads(fn, policy, value):
  params = networks.parameters(policy, value)
  loss, metrics = fn()
  grads = torch.autograd.grad(loss, params)
  return [loss.detach()] + [metrics[k].detach() for k in ph.METRICS] + list(grads)


@pytest.mark.parametrize('normalize_advantage', [True, False])
def test_chained_head_is_ppo_loss_bit_for_bit(normalize_advantage):
  T, B, A, O = 4, 6, 3, 7
  data, eps = _case(T, B, A, O, seed=3)
  policy, value = networks.make_ppo_networks(O, A, policy_hidden_layer_sizes=(8, 8),
                                             value_hidden_layer_sizes=(16,), seed=2)
  mean_std = (torch.full((O,), 0.1), torch.full((O,), 1.5))
  hyper = dict(entropy_cost=1e-2, discounting=0.97, reward_scaling=0.5, gae_lambda=0.9,
               clipping_epsilon=0.2, normalize_advantage=normalize_advantage)

  def head():
    d, e = data.map(lambda x: x.transpose(0, 1)), eps.transpose(0, 1)
    obs = normalize(d.observation, mean_std)
    logits = networks.mlp(policy, obs)
    baseline = networks.mlp(value, obs).squeeze(-1)
    boot = networks.mlp(value, normalize(d.next_observation[-1], mean_std)).squeeze(-1)
    return ph.ppo_head(logits, baseline, boot, d, e, fused=False, fused_gae=False, **hyper)
  want = _loss_and_grads(lambda: ppo_loss(policy, value, mean_std, data, eps, fused=False, **hyper),
                         policy, value)
  off = _loss_and_grads(lambda: ppo_loss(policy, value, mean_std, data, eps, fused=False,
                                         fused_head=False, **hyper), policy, value)
  got = _loss_and_grads(head, policy, value)
  for g, o, w in zip(got, off, want):
    assert torch.equal(g, w) and torch.equal(o, w)


def test_learner_takes_the_keyword():
  import inspect
  from brax_amd.training import ppo
  for fn in (ppo.train, ppo.Learner.__init__, ppo_loss):
    assert inspect.signature(fn).parameters['fused_head'].default is False
