"""`_native.args` and the two callers that name arguments, `packed.refusal` and
`packed.launch`, without a GPU: for each zero-step probe and each K-step
launch of `brax_amd.envs`, the tuple that reaches the library equals the
positional tuple the call site spelled out before the arguments had names,
written here as literals. The library is a stub that records its arguments."""
import ctypes as C

import pytest
import torch

from brax_amd import _native, abi
from brax_amd.envs import packed

H = C.c_void_p(0x5150)  # the system handle
STREAM = C.c_void_p(0x57)
B, K, A = 3, 4, 2


class _Recorder:
  """Stands for the loaded library: every entry point records its arguments
  and succeeds."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, entry):
    assert entry in abi.ARGS, entry
    return lambda *a: self.calls.append((entry, a)) or 0


class _Env:
  """What `packed.refusal` / `packed.launch` read of a kernel env."""

  class sys:  # pylint: disable=invalid-name
    _h = H
    device = torch.device('cpu')

  def __init__(self):
    self.params = abi.BxEnvParams()

  def _params(self, opts, first_qp, first_obs):
    assert (first_qp, first_obs) == (None, None)
    return self.params


@pytest.fixture
def lib(monkeypatch):
  rec = _Recorder()
  monkeypatch.setattr(_native, 'lib', lambda: rec)
  monkeypatch.setattr(packed, '_stream', lambda index: STREAM)
  return rec


def _plain(args):
  """`byref(x)` compares by identity of x; everything else as it is."""
  return tuple(('byref', id(a._obj)) if type(a).__name__ == 'CArgObject' else a for a in args)


def ref(x):
  return ('byref', id(x))


def test_args_fills_the_unnamed_and_refuses_the_unknown():
  assert _native.args('bx_abi_version') == ()
  assert _native.args('bx_uniform', n=5, hi=1.0) == (None, 5, 0, 0, 0, 1.0, None)
  # an explicit None or 0 is kept as given
  assert _native.args('bx_system_set_single', sys=None, on=0) == (None, 0)
  with pytest.raises(TypeError, match='steps'):
    _native.args('bx_uniform', steps=1)
  with pytest.raises(TypeError):
    _native.args('bx_uniform', **{'n': 1}, n=2)  # pylint: disable=repeated-keyword
  with pytest.raises(KeyError):
    _native.args('bx_no_such_entry')
  # every entry point, nothing named: NULL for pointers, 0 for scalars
  for entry, sig in abi.ARGS.items():
    got = _native.args(entry)
    assert len(got) == len(sig)
    for v, (_, t) in zip(got, sig):
      assert v == (0 if t in (C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double)
                   else None), entry


def test_the_six_probes(lib):
  u, desc, pop = _Env(), abi.BxPolicy(), abi.BxPopulation()
  head = (H, ref(u.params))
  nul5 = (None,) * 5
  # policy.fused_supported
  assert packed.refusal(u, {}, 'bx_env_rollout_policy', policy=C.byref(desc)) is None
  # evaluator.eval_supported: given actions, an identity head, a NormalTanh head
  packed.refusal(u, {}, 'bx_env_eval_packed', act_width=A)
  packed.refusal(u, {}, 'bx_env_eval_population', policy=C.byref(desc), pop=C.byref(pop))
  packed.refusal(u, {}, 'bx_env_eval_policy', policy=C.byref(desc))
  # population.population_supported (the same entry point, its own structs)
  desc2, pop2 = abi.BxPolicy(), abi.BxPopulation(param_stride=8)
  packed.refusal(u, {}, 'bx_env_eval_population', policy=C.byref(desc2), pop=C.byref(pop2))
  want = [
      ('bx_env_rollout_policy', head + (0, 0) + nul5 + (ref(desc), 0, 0, 0, None, None, None,
                                                         None, None, None)),
      ('bx_env_eval_packed', head + (0, 0) + nul5 + (0, 0, A, None, None, None, None, None)),
      ('bx_env_eval_population', head + (0, 0) + nul5 + (ref(desc), 0, 0, 0, None, None, None, None,
                                                          ref(pop), None)),
      ('bx_env_eval_policy', head + (0, 0) + nul5 + (ref(desc), 0, 0, 0, None, None, None, None,
                                                      None)),
      ('bx_env_eval_population', head + (0, 0) + nul5 + (ref(desc2), 0, 0, 0, None, None, None,
                                                          None, ref(pop2), None)),
  ]
  assert [(e, _plain(a)) for e, a in lib.calls] == want
  assert u.params.auto_reset == 0
  # RolloutRunner.__init__: its own params and batch size, not `refusal`'s
  p = abi.BxEnvParams()
  got = _native.args('bx_env_rollout_random', sys=H, env=C.byref(p), n_envs=B, act_width=A, hi=1.0)
  assert _plain(got) == (H, ref(p), B, 0, None, None, None, None, 0, 0, 0, 0.0, 1.0, A, None, None,
                         None, None)


def _tensors(with_streams):
  f = lambda *shape: torch.zeros(shape, dtype=torch.float32)  # noqa: E731
  p = abi.BxEnvParams()
  steps, rng = (f(B), torch.zeros((B,), dtype=torch.int32)) if with_streams else (None, None)
  return (p, f(B), steps, rng), f(B, 5, 16), f(7)


def _ptr(t):
  return None if t is None else t.data_ptr()


@pytest.mark.parametrize('with_streams', [False, True])
def test_the_six_launches(lib, with_streams):
  u = _Env()
  inputs, qbuf, out = _tensors(with_streams)
  p, done, steps, rng = inputs
  pre = (H, ref(p), B, K, qbuf.data_ptr())
  state = (done.data_ptr(), _ptr(steps), _ptr(rng))
  act = torch.zeros((K, B, 2 * A), dtype=torch.float32)[:, :, :A]  # strided: (2 B A, 2 A, 1)
  obs, ev = torch.zeros((B, 6)), torch.zeros((5, B))
  ea, er, el = torch.zeros((K, B, A)), torch.zeros((K, B, A)), torch.zeros((K, B))
  desc, pop = abi.BxPolicy(), abi.BxPopulation()
  seed, offset, stride = 11, 22, 2 * B * A

  def check(rng_out, every_step, want):
    assert (rng_out is None) == (rng is None)
    if rng_out is not None:
      assert tuple(rng_out.shape) == ((K, B) if every_step else (B,))
      assert rng_out.dtype == torch.int32
    entry, got = lib.calls.pop()
    assert not lib.calls
    assert _plain(got) == tuple(_ptr(rng_out) if w == 'rng_out' else w for w in want), entry

  # rollout
  r = packed.launch(u, 'bx_env_rollout_packed', inputs, qbuf, K, out, True, act=act,
                    act_stride=act.stride(1), act_step_stride=act.stride(0), act_width=act.shape[2])
  check(r, True, pre + state + (act.data_ptr(), 2 * A, 2 * B * A, A, out.data_ptr(), 'rng_out',
                                STREAM))
  # policy_rollout
  r = packed.launch(u, 'bx_env_rollout_policy', inputs, qbuf, K, out, True, obs_in=obs,
                    policy=C.byref(desc), seed=seed, offset=offset, step_stride=stride,
                    act_out=ea, raw_out=er, logp_out=el)
  check(r, True, pre + (obs.data_ptr(),) + state + (
      ref(desc), seed, offset, stride, ea.data_ptr(), er.data_ptr(), el.data_ptr(), out.data_ptr(),
      'rng_out', STREAM))
  # eval_rollout: an identity head, a NormalTanh head, given actions
  closed = dict(obs_in=obs, policy=C.byref(desc), seed=seed, offset=offset, step_stride=stride)
  r = packed.launch(u, 'bx_env_eval_population', inputs, qbuf, K, out, False, eval_in=ev,
                    eval_out=ev, pop=C.byref(pop), **closed)
  check(r, False, pre + (obs.data_ptr(),) + state + (
      ref(desc), seed, offset, stride, ev.data_ptr(), out.data_ptr(), ev.data_ptr(), 'rng_out',
      ref(pop), STREAM))
  r = packed.launch(u, 'bx_env_eval_policy', inputs, qbuf, K, out, False, eval_in=ev, eval_out=ev,
                    **closed)
  check(r, False, pre + (obs.data_ptr(),) + state + (
      ref(desc), seed, offset, stride, ev.data_ptr(), out.data_ptr(), ev.data_ptr(), 'rng_out',
      STREAM))
  r = packed.launch(u, 'bx_env_eval_packed', inputs, qbuf, K, out, False, eval_in=ev, eval_out=ev,
                    act=act, act_stride=act.stride(1), act_step_stride=act.stride(0), act_width=A)
  check(r, False, pre + state + (act.data_ptr(), 2 * A, 2 * B * A, A, ev.data_ptr(),
                                 out.data_ptr(), ev.data_ptr(), 'rng_out', STREAM))
  # population_rollout
  r = packed.launch(u, 'bx_env_eval_population', inputs, qbuf, K, out, False, obs_in=obs,
                    policy=C.byref(desc), seed=int(seed), offset=int(offset),
                    step_stride=2 * B * A, eval_in=ev, eval_out=ev, pop=C.byref(pop))
  check(r, False, pre + (obs.data_ptr(),) + state + (
      ref(desc), seed, offset, 2 * B * A, ev.data_ptr(), out.data_ptr(), ev.data_ptr(), 'rng_out',
      ref(pop), STREAM))
  # a shared argument named twice is refused, not overridden
  with pytest.raises(TypeError):
    packed.launch(u, 'bx_env_eval_policy', inputs, qbuf, K, out, False, qp_in=qbuf)


def test_the_two_shared_checks_keep_their_texts():
  dev = torch.device('cpu')
  with pytest.raises(ValueError, match=r'^actions \(4, 2, 2\) != \(K, 3, 2\)$'):
    packed.actions_input(torch.zeros((4, 2, 2)), 3, 2, dev)
  act = torch.zeros((4, 3, 4))[:, :, :2]
  assert packed.actions_input(act, 3, 2, dev) is act  # a unit last stride passes as it is
  assert packed.actions_input(act.transpose(1, 2), 2, 3, dev).is_contiguous()
  with pytest.raises(ValueError, match=r'^eval_out must be contiguous float32 \(5, 3\) on cpu$'):
    packed.output_buffer('eval_out', torch.zeros((3, 5)), (5, 3), dev)
  with pytest.raises(ValueError, match=r'^extras must be contiguous float32 \(4, 3, 2\) on cpu$'):
    packed.output_buffer('extras', torch.zeros((4, 3, 2), dtype=torch.float64), (4, 3, 2), dev)
  t = torch.zeros((5, 3))
  assert packed.output_buffer('mom_out', t, (5, 3), dev) is t
