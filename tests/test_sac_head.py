"""The SAC loss heads without a GPU: the ABI mirror of `bx_sac_head_*`, their
refusals text for text (every check runs before the first HIP call; the
"device pointers" are arbitrary aligned integers, never dereferenced), the
size query against `sac_head_launch.h`'s formula, `fused_supported`'s reasons,
the three-way `fused_head` switch on CPU tensors, and the sample's closed-form
backward pass against autograd in float64."""
import ctypes as C
import functools
import inspect
import os

import pytest
import torch

from brax_amd import _native, abi
from brax_amd.envs.policy import head_scale, normal_tanh_log_prob
from brax_amd.training import sac, sac_head, sac_networks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bx_sac_head_prep', 'bx_sac_head_sample', 'bx_sac_head_losses',
         'bx_sac_head_sample_backward')
P = 0x7f0000001000  # a "device pointer": non-null, 4 KiB aligned
T31 = 1 << 31


def test_header_abi_and_exports():
  # (names, types and the macros against the header: tests/test_abi.py)
  assert abi.SAC_MAX_CRITICS == 4 and abi.SAC_MAX_JOBS == 3
  # additive: the version stays
  assert abi.ABI_VERSION == 14 and _native.lib().bx_abi_version() == 14


def wsb(n=1 << 20):
  return C.pointer(C.c_int64(n))


def prep(**kw):
  a = dict(n_rows=4, n_obs=3, n_actions=2, obs=P, obs_pitch=3, next_obs=P, next_obs_pitch=3,
           action=P, action_pitch=2, mean=P, std=P, x_cur=P, x_next=P, x_pi=P, x_pitch=5)
  a.update(kw)
  return tuple(a.values()) + (None,)


def jobs(n=3, **kw):
  t = (abi.BxSacSampleJob * 3)()
  for j in t:
    j.logits, j.logits_pitch, j.eps, j.eps_pitch, j.action, j.action_pitch, j.log_prob = (
        P, 4, P, 2, P, 2, P)
  for k, v in kw.items():
    setattr(t[n - 1], k, v)
  return t


def smp(n_rows=4, n_actions=2, table=None, n_jobs=3):
  return (n_rows, n_actions, jobs() if table is None else table, n_jobs, 1e-3, None)


def critics(n=2, **kw):
  q = abi.BxSacQ()
  for name in ('q_old', 'next_q', 'q_pi', 'dq_old', 'dq_pi'):
    for c in range(n):
      getattr(q, name)[c] = P
  for k, (c, v) in kw.items():
    getattr(q, k)[c] = v
  return q


def los(**kw):
  a = dict(n_rows=300, n_critics=2, lp_alpha=P, lp_next=P, lp_pi=P, q=critics(), reward=P,
           reward_stride=1, discount=P, discount_stride=1, truncation=P, truncation_stride=1,
           log_alpha=P, reward_scaling=1.0, discounting=0.99, target_entropy=-1.0, g_lp=P,
           workspace=P, workspace_bytes=wsb())
  a.update(kw)
  return tuple(a.values()) + (None,)


def dact(n=2, **kw):
  d = abi.BxSacDaction()
  for c in range(n):
    d.ptr[c], d.pitch[c] = P, 2
  for k, (c, v) in kw.items():
    getattr(d, k)[c] = v
  return d


def bwd(**kw):
  a = dict(n_rows=300, n_actions=2, n_critics=2, logits=P, logits_pitch=4, eps=P, eps_pitch=2,
           g_lp=P, da=dact(), min_std=1e-3, dlogits=P, dlogits_pitch=4, losses=P, dlog_alpha=P,
           workspace=P, workspace_bytes=wsb())
  a.update(kw)
  return tuple(a.values()) + (None,)


# (entry point, arguments, bx_last_error())
REFUSALS = [
    ('bx_sac_head_prep', prep(n_rows=-1), 'negative n_rows'),
    ('bx_sac_head_prep', prep(n_rows=T31 + 1), 'too many rows for one launch'),
    ('bx_sac_head_prep', prep(n_obs=0), 'n_obs must be >= 1'),
    ('bx_sac_head_prep', prep(n_obs=(1 << 20) + 1), 'too many observations'),
    ('bx_sac_head_prep', prep(n_actions=0), 'n_actions must be >= 1'),
    ('bx_sac_head_prep', prep(n_actions=(1 << 20) + 1), 'too many actions'),
    ('bx_sac_head_prep', prep(obs=None), 'null argument'),
    ('bx_sac_head_prep', prep(next_obs=None), 'null argument'),
    ('bx_sac_head_prep', prep(action=None), 'null argument'),
    ('bx_sac_head_prep', prep(x_cur=None), 'null argument'),
    ('bx_sac_head_prep', prep(x_next=None), 'null argument'),
    ('bx_sac_head_prep', prep(x_pi=None), 'null argument'),
    ('bx_sac_head_prep', prep(mean=None), 'one of mean and std is null'),
    ('bx_sac_head_prep', prep(std=None), 'one of mean and std is null'),
    ('bx_sac_head_prep', prep(obs_pitch=2), 'obs_pitch 2 below the row width 3'),
    ('bx_sac_head_prep', prep(next_obs_pitch=0), 'next_obs_pitch 0 below the row width 3'),
    ('bx_sac_head_prep', prep(action_pitch=1), 'action_pitch 1 below the row width 2'),
    ('bx_sac_head_prep', prep(x_pitch=4), 'x_pitch 4 below the row width 5'),
    ('bx_sac_head_sample', smp(n_rows=-1), 'negative n_rows'),
    ('bx_sac_head_sample', smp(n_rows=T31 + 1), 'too many rows for one launch'),
    ('bx_sac_head_sample', smp(n_actions=0), 'n_actions must be >= 1'),
    ('bx_sac_head_sample', smp(n_jobs=0), 'n_jobs 0 outside 1..3'),
    ('bx_sac_head_sample', smp(n_jobs=4), 'n_jobs 4 outside 1..3'),
    ('bx_sac_head_sample', (4, 2, None, 3, 1e-3, None), 'null argument'),
    ('bx_sac_head_sample', smp(table=jobs(1, logits=None)), 'job 0: null logits, eps or log_prob'),
    ('bx_sac_head_sample', smp(table=jobs(2, eps=None)), 'job 1: null logits, eps or log_prob'),
    ('bx_sac_head_sample', smp(table=jobs(3, log_prob=None)), 'job 2: null logits, eps or log_prob'),
    ('bx_sac_head_sample', smp(table=jobs(1, logits_pitch=3)), 'logits_pitch 3 below the row width 4'),
    ('bx_sac_head_sample', smp(table=jobs(2, eps_pitch=1)), 'eps_pitch 1 below the row width 2'),
    ('bx_sac_head_sample', smp(table=jobs(3, action_pitch=1)), 'action_pitch 1 below the row width 2'),
    ('bx_sac_head_losses', los(workspace_bytes=None), 'null argument'),
    ('bx_sac_head_losses', los(n_rows=-1), 'negative n_rows'),
    ('bx_sac_head_losses', los(n_rows=T31 + 1), 'too many rows for one launch'),
    ('bx_sac_head_losses', los(n_critics=0), 'n_critics 0 outside 1..4'),
    ('bx_sac_head_losses', los(n_critics=5), 'n_critics 5 outside 1..4'),
    ('bx_sac_head_losses', los(lp_alpha=None), 'null argument'),
    ('bx_sac_head_losses', los(lp_next=None), 'null argument'),
    ('bx_sac_head_losses', los(lp_pi=None), 'null argument'),
    ('bx_sac_head_losses', los(q=None), 'null argument'),
    ('bx_sac_head_losses', los(reward=None), 'null argument'),
    ('bx_sac_head_losses', los(discount=None), 'null argument'),
    ('bx_sac_head_losses', los(truncation=None), 'null argument'),
    ('bx_sac_head_losses', los(log_alpha=None), 'null argument'),
    ('bx_sac_head_losses', los(g_lp=None), 'null argument'),
    ('bx_sac_head_losses', los(q=critics(q_pi=(1, None))), 'critic 1: null pointer'),
    ('bx_sac_head_losses', los(q=critics(dq_old=(0, None))), 'critic 0: null pointer'),
    ('bx_sac_head_losses', los(n_critics=3), 'critic 2: null pointer'),
    ('bx_sac_head_losses', los(workspace_bytes=wsb(47)), 'workspace of 47 bytes, 48 needed'),
    ('bx_sac_head_losses', los(workspace=P + 8), 'workspace not 16-byte aligned'),
    ('bx_sac_head_sample_backward', bwd(workspace_bytes=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(n_rows=-1), 'negative n_rows'),
    ('bx_sac_head_sample_backward', bwd(n_rows=T31 + 1), 'too many rows for one launch'),
    ('bx_sac_head_sample_backward', bwd(n_actions=0), 'n_actions must be >= 1'),
    ('bx_sac_head_sample_backward', bwd(n_critics=5), 'n_critics 5 outside 1..4'),
    ('bx_sac_head_sample_backward', bwd(logits=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(eps=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(g_lp=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(da=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(dlogits=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(losses=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(dlog_alpha=None), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(logits_pitch=3), 'logits_pitch 3 below the row width 4'),
    ('bx_sac_head_sample_backward', bwd(eps_pitch=1), 'eps_pitch 1 below the row width 2'),
    ('bx_sac_head_sample_backward', bwd(dlogits_pitch=2), 'dlogits_pitch 2 below the row width 4'),
    ('bx_sac_head_sample_backward', bwd(da=dact(ptr=(1, None))), 'critic 1: null pointer'),
    ('bx_sac_head_sample_backward', bwd(da=dact(pitch=(0, 1))), 'daction pitch 1 below the row width 2'),
    ('bx_sac_head_sample_backward', bwd(workspace_bytes=wsb(16)), 'workspace of 16 bytes, 48 needed'),
    ('bx_sac_head_sample_backward', bwd(workspace=P + 4), 'workspace not 16-byte aligned'),
    # two faults at once: the first check in the order wins
    ('bx_sac_head_prep', prep(n_rows=-1, n_obs=0), 'negative n_rows'),
    ('bx_sac_head_prep', prep(obs=None, obs_pitch=2), 'null argument'),
    ('bx_sac_head_sample', smp(n_actions=0, n_jobs=4), 'n_actions must be >= 1'),
    ('bx_sac_head_losses', los(n_critics=5, workspace=None), 'n_critics 5 outside 1..4'),
    ('bx_sac_head_losses', los(reward=None, workspace=P + 8), 'null argument'),
    ('bx_sac_head_sample_backward', bwd(workspace=P + 4, workspace_bytes=wsb(16)),
     'workspace of 16 bytes, 48 needed'),
]

# rc 0 and no error: no rows, whatever the pointers
ZERO_WORK = [
    ('bx_sac_head_prep', prep(n_rows=0, obs=None, x_cur=None, x_pitch=0)),
    ('bx_sac_head_sample', (0, 2, None, 3, 1e-3, None)),
    ('bx_sac_head_losses', los(n_rows=0, lp_alpha=None, q=None, workspace_bytes=wsb(0))),
    ('bx_sac_head_sample_backward', bwd(n_rows=0, logits=None, da=None, workspace_bytes=wsb(0))),
]


def _call(name, args):
  lib = _native.lib()
  # a refusal must set the text itself: start from another one
  assert lib.bx_system_set_single(None, 0) == 1 and lib.bx_last_error() == b'null system'
  return getattr(lib, name)(*args), lib.bx_last_error().decode()


def _ids(rows):
  return [f'{i}-{r[0]}' for i, r in enumerate(rows)]


@pytest.mark.parametrize('name,args,message', REFUSALS, ids=_ids(REFUSALS))
def test_refusal(name, args, message):
  assert _call(name, args) == (1, message)


@pytest.mark.parametrize('name,args', ZERO_WORK, ids=_ids(ZERO_WORK))
def test_zero_rows_return_ok(name, args):
  assert _call(name, args) == (0, 'null system')  # (the error text is left alone)


def test_size_query():
  """`sac_head_workspace_bytes`: SAC_HEAD_PART doubles per workgroup of
  SAC_HEAD_BLOCK rows, rounded up to 16 bytes; both entry points agree, and
  the query comes before the null checks."""
  src = open(os.path.join(ROOT, 'brax_amd', 'csrc', 'sac_head_launch.h')).read()
  assert f'SAC_HEAD_BLOCK = {abi.SAC_HEAD_BLOCK};' in src
  assert f'SAC_HEAD_PART = {abi.SAC_HEAD_PART};' in src
  for B in (0, 1, 255, 256, 257, 512, 513, 100000, T31):
    groups = -(-B // abi.SAC_HEAD_BLOCK)
    want = (8 * abi.SAC_HEAD_PART * groups + 15) // 16 * 16
    for name, args in (('bx_sac_head_losses', los), ('bx_sac_head_sample_backward', bwd)):
      b = wsb(-1)
      kw = dict(lp_alpha=None) if args is los else dict(logits=None)
      assert _call(name, args(n_rows=B, workspace=None, workspace_bytes=b, **kw))[0] == 0
      assert b.contents.value == want, (name, B)
  assert sac_head.workspace_floats(300) == 12


# ---- fused_supported and the switch -------------------------------------------------------------

def _case(B=6, O=5, A=3, seed=0, dtype=torch.float32, n_critics=2, fused_adam=False):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(s, generator=g).to(dtype)  # noqa: E731
  flags = lambda p: (torch.rand((B,), generator=g) < p).to(dtype)  # noqa: E731
  factory = functools.partial(sac_networks.make_sac_networks, hidden_layer_sizes=(8, 8),
                              n_critics=n_critics)
  ts = sac.init_training_state(O, A, 1e-2, factory, seed + 1, dtype=dtype, fused_adam=fused_adam)
  trans = {'observation': r(B, O), 'action': torch.tanh(r(B, A)), 'reward': r(B),
           'discount': 1 - flags(0.2), 'next_observation': r(B, O), 'truncation': flags(0.2)}
  normalizer = (r(O), 0.5 + 1.5 * torch.rand((O,), generator=g).to(dtype))
  return ts, normalizer, trans, (r(B, A), r(B, A), r(B, A))


def test_fused_supported_names_the_reason():
  ts, normalizer, trans, eps = _case()
  why = sac_head.fused_supported
  assert why(ts, normalizer, trans, eps) == 'observation is a CPU tensor'
  assert why(ts, None, trans, eps) == 'observation is a CPU tensor'
  t64 = {**trans, 'reward': trans['reward'].double()}
  assert why(ts, normalizer, t64, eps) == 'reward: torch.float64 is not float32'
  ts64 = _case(dtype=torch.float64)[0]
  assert 'float64 is not float32' in why(ts64, normalizer, trans, eps)
  wide = torch.zeros((6, 6))
  assert why(ts, normalizer, trans, (eps[0], wide[:, ::2], eps[2])) == 'eps[1] has inner stride 2, not 1'
  assert why(ts, normalizer, {**trans, 'observation': torch.zeros((6, 10))[:, ::2]}, eps) == \
      'observation has inner stride 2, not 1'
  assert why(ts, normalizer, {**trans, 'next_observation': torch.zeros((6, 4))}, eps) == \
      'next_observation (6, 4) is not (6, 5)'
  assert why(ts, normalizer, {**trans, 'action': torch.zeros((5, 3))}, eps) == \
      'action (5, 3) is not (6, 3)'
  assert why(ts, normalizer, {**trans, 'discount': torch.zeros((6, 2))}, eps) == \
      'discount (6, 2) is not (6,) or (6, 1)'
  assert why(ts, (normalizer[0], torch.ones((4,))), trans, eps) == 'std (4,) is not (5,)'
  assert why(ts, normalizer, {**trans, 'observation': torch.zeros((6,))}, eps) == \
      'observation (6,) is not (B, O)'
  assert why(_case(n_critics=5)[0], normalizer, trans, eps) == '5 critics, the kernels take 1..4'


def _state(ts):
  return [t.detach().clone() for t in
          [ts.log_alpha] + sac_networks.q_parameters(ts.q_layers)
          + sac_networks.q_parameters(ts.target_q_layers)
          + sac_networks.q_parameters([ts.policy_layers])]


def test_the_switch_on_cpu_tensors():
  """True refuses with the reason; None falls back to the chained step's bits
  (two training states from one seed)."""
  for fn in (sac.sgd_step, sac.Learner.__init__, sac.train):
    assert inspect.signature(fn).parameters['fused_head'].default is False
  ts, normalizer, trans, eps = _case()
  with pytest.raises(NotImplementedError, match='no fused sac head: observation is a CPU tensor'):
    sac.sgd_step(ts, normalizer, trans, eps, fused_head=True)
  assert ts.gradient_steps == 0
  a, b = _case()[0], _case()[0]
  for _ in range(2):
    ma = sac.sgd_step(a, normalizer, trans, eps, reward_scaling=3.0, discounting=0.95,
                      fused_head=None)
    mb = sac.sgd_step(b, normalizer, trans, eps, reward_scaling=3.0, discounting=0.95,
                      fused_head=False)
    assert list(ma) == list(mb) == ['critic_loss', 'actor_loss', 'alpha_loss', 'alpha']
    for k in ma:
      assert torch.equal(ma[k], mb[k]), k
  for x, y in zip(_state(a), _state(b)):
    assert torch.equal(x, y)
  assert not torch.equal(_state(a)[0], _state(_case()[0])[0])


# ---- the closed-form backward -------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2])
def test_closed_form_sample_backward_equals_autograd(seed):
  """u = g 2 tanh(raw) + da (1 - tanh(raw)^2); dloc = u; dscale = u eps - g /
  scale; ds = dscale sigmoid(s): autograd's gradient of sum(g lp) + sum(da
  tanh(raw)) in float64, to 1e-12 relative."""
  B, A, min_std = 7, 5, 1e-3
  g_ = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(s, generator=g_, dtype=torch.float64)  # noqa: E731
  logits, eps, g, da = r(B, 2 * A).requires_grad_(), r(B, A), r(B), r(B, A)
  loc, s = torch.chunk(logits, 2, dim=-1)
  scale = head_scale(s, min_std)
  raw = loc + scale * eps
  lp = normal_tanh_log_prob(loc, scale, raw).sum(-1)
  want, = torch.autograd.grad((g * lp).sum() + (da * torch.tanh(raw)).sum(), logits)
  with torch.no_grad():
    th = torch.tanh(raw)
    u = g[:, None] * 2 * th + da * (1 - th * th)
    dscale = u * eps - g[:, None] / scale
    got = torch.cat([u, dscale * torch.sigmoid(s)], dim=-1)
  assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
