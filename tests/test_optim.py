"""The fused optimiser step without a GPU: the ABI mirror, the refusals (all
made before any device call, so host pointers will do), `reference_step`
against a numpy restatement, `supported`'s reasons and the arena's layout."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from brax_amd import _native, abi
from brax_amd.training import FusedAdam, optim


def test_header_abi_and_exports():
  # (names, types and BX_OPT_MAX_TENSORS against the header: tests/test_abi.py)
  nbytes = C.c_int32(0)
  assert _native.lib().bx_opt_sizes(C.byref(nbytes)) == 0
  assert nbytes.value == C.sizeof(abi.BxOptTensor) == 56
  # additive: the version stays
  assert abi.ABI_VERSION == 14 and _native.lib().bx_abi_version() == 14


def _table(sizes, target=False):
  """A table over host arrays (never dereferenced: every call here returns
  before a device call) and the arrays that keep the pointers alive."""
  keep, table = [], (abi.BxOptTensor * len(sizes))()
  for e, n in zip(table, sizes):
    arrays = [np.zeros(max(n, 1), np.float32) for _ in range(5)]
    keep.append(arrays)
    e.p, e.g, e.m, e.v = (a.ctypes.data for a in arrays[:4])
    e.target = arrays[4].ctypes.data if target else None
    e.n, e.lr, e.tau = n, 1e-3, 0.005
  return table, keep


def _refused(match, table, n, step=1, beta1=0.9, beta2=0.999, eps=1e-8):
  lib = _native.lib()
  rc = lib.bx_adam_step(table, n, step, beta1, beta2, eps, None)
  msg = lib.bx_last_error().decode()
  assert rc != 0 and re.search(match, msg), (rc, msg)


def test_refusals_come_before_any_device_call():
  table, keep = _table([4, 1])
  _refused('null', None, 2)
  _refused('n_tensors', table, 0)
  _refused('n_tensors', table, 33)
  _refused('step', table, 2, step=0)
  _refused('step', table, 2, step=-3)
  for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=math.nan)):
    _refused('beta1', table, 2, **kw)
  for kw in (dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=math.nan)):
    _refused('beta2', table, 2, **kw)
  _refused('eps', table, 2, eps=-1e-8)
  _refused('eps', table, 2, eps=math.nan)
  table[1].n = -1
  _refused('negative n', table, 2)
  for field in ('p', 'g', 'm', 'v'):
    table, keep = _table([4, 1])
    setattr(table[1], field, None)
    _refused('null p, g, m or v', table, 2)
    # ... but not on an empty tensor, and a table of empty tensors launches nothing
    table[0].n = table[1].n = 0
    assert _native.lib().bx_adam_step(table, 2, 1, 0.9, 0.999, 1e-8, None) == 0
  del keep


def _numpy_step(p, g, m, v, step, lr, beta1, beta2, eps, target=None, tau=0.0):
  m = m + (g - m) * (1 - beta1)
  v = v * beta2 + g * g * (1 - beta2)
  denom = np.sqrt(v) / math.sqrt(1 - beta2 ** step) + eps
  p = p - (lr / (1 - beta1 ** step)) * (m / denom)
  if target is not None:
    target = target * (1 - tau) + p * tau
  return p, m, v, target


def test_reference_step_equals_a_numpy_restatement():
  rng = np.random.default_rng(0)
  shapes, lrs, taus = [(), (3,), (5, 7)], [3e-4, 1e-2, 1e-3], [0.0, 0.005, 0.0]
  betas, eps = (0.9, 0.999), 1e-8
  p = [rng.standard_normal(s) for s in shapes]
  m, v = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
  t = [None, rng.standard_normal(shapes[1]), None]
  tp, tm, tv = ([torch.tensor(x, dtype=torch.float64) for x in xs] for xs in (p, m, v))
  tt = [None if x is None else torch.tensor(x, dtype=torch.float64) for x in t]
  for step in (1, 2, 3):
    g = [rng.standard_normal(s) for s in shapes]
    optim.reference_step(tp, [torch.tensor(x, dtype=torch.float64) for x in g], tm, tv, step, lrs,
                         betas, eps, targets=tt, tau=taus)
    for k in range(3):
      p[k], m[k], v[k], t[k] = _numpy_step(p[k], g[k], m[k], v[k], step, lrs[k], *betas, eps,
                                           t[k], taus[k])
      for got, want in ((tp[k], p[k]), (tm[k], m[k]), (tv[k], v[k]), (tt[k], t[k])):
        if want is not None:
          np.testing.assert_allclose(got.numpy(), want, rtol=1e-14, atol=0)
  # one step of torch's own Adam from the same state lands on the same values
  q = torch.tensor(p[2], dtype=torch.float64, requires_grad=True)
  ref = [torch.tensor(p[2], dtype=torch.float64)], [torch.zeros(shapes[2], dtype=torch.float64)], \
      [torch.zeros(shapes[2], dtype=torch.float64)]
  adam = torch.optim.Adam([q], lr=1e-3, eps=eps)
  g = torch.tensor(rng.standard_normal(shapes[2]))
  q.grad = g.clone()
  adam.step()
  optim.reference_step(ref[0], [g], ref[1], ref[2], 1, 1e-3, betas, eps)
  np.testing.assert_allclose(ref[0][0].numpy(), q.detach().numpy(), rtol=1e-12, atol=0)


def test_supported_gives_its_reasons_on_cpu_tensors():
  ok = [torch.zeros(4, 3), torch.zeros(3)]
  assert optim.supported([dict(params=ok, lr=1e-3)], device=False) is None
  assert 'float64 is not float32' in optim.supported([dict(params=[ok[0].double()], lr=1e-3)])
  assert 'not contiguous' in optim.supported([dict(params=[ok[0].t()], lr=1e-3)])
  why = optim.supported([dict(params=ok, lr=1e-3, targets=[torch.zeros(4, 3), torch.zeros(4)],
                              tau=0.1)])
  assert 'target 1 (4,) is not shaped as its param (3,)' in why
  assert 'is a CPU tensor' in optim.supported([dict(params=ok, lr=1e-3)])
  with pytest.raises(NotImplementedError, match='float64'):
    FusedAdam([dict(params=[ok[0].double()], lr=1e-3)])
  from brax_amd.training import ppo, sac
  with pytest.raises(NotImplementedError, match='CPU tensor'):
    ppo.make_optimizer(ok, 1e-3, fused_adam=True)
  assert isinstance(ppo.make_optimizer(ok, 1e-3, fused_adam=None), torch.optim.Adam)
  with pytest.raises(NotImplementedError, match='CPU tensor'):
    sac.init_training_state(5, 2, fused_adam=True)
  ts = sac.init_training_state(5, 2, fused_adam=None)
  assert ts.fused_optimizer is None and ts.q_optimizer is not None


def test_arena_slices_are_aligned_and_disjoint():
  sizes = (1, 3, 5, 1024)
  params = [torch.zeros(n) for n in sizes] + [torch.zeros(())]
  opt = FusedAdam([dict(params=params[:2], lr=1e-3), dict(params=params[2:], lr=1e-2)])
  assert opt.lrs == [1e-3, 1e-3, 1e-2, 1e-2, 1e-2] and opt.step_count == 0
  for arena in (opt.exp_avg, opt.exp_avg_sq):
    spans = []
    for i, p in enumerate(params):
      s = arena(i)
      assert s.shape == p.shape and s.dtype == torch.float32 and s.is_contiguous()
      assert s.data_ptr() % 16 == 0 and not bool(s.any())
      spans.append((s.data_ptr(), s.data_ptr() + 4 * s.numel()))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
  assert opt.exp_avg(0).data_ptr() != opt.exp_avg_sq(0).data_ptr()
  # a slice is a view: a write through it lands in the arena
  opt.exp_avg(3).fill_(1.0)
  assert float(opt._m.sum()) == 1024  # pylint: disable=protected-access
  with pytest.raises(_native.NativeError):
    opt.step([torch.zeros_like(p) for p in params])  # no CPU fallback
