"""The refusals of the C ABI's entry points that take no system handle, pinned
text for text: every check in them runs before the first HIP call, so no GPU
is needed and nothing here passes validation and reaches a launch. One row per
refusal (entry point, arguments, exact bx_last_error() text; the return code
is 1); then the zero-work returns, the three workspace size queries, and rows
with two faults at once, where the first check in the order wins. Device
pointers are arbitrary non-null aligned integers: never dereferenced."""
import ctypes as C

import pytest

from brax_amd import _native
from brax_amd import abi

P = 0x7f0000001000  # a "device pointer": non-null, 4 KiB aligned
Q = P + (1 << 30)  # another, far from the first


def seq(ptr=P, ts=8, es=1):
  return abi.BxSeq(ptr, ts, es)


def fields(widths=(3, 1), ptr=P, n=None):
  f = abi.BxFields()
  f.n_fields = len(widths) if n is None else n
  for k, w in enumerate(widths):
    f.ptr[k], f.width[k], f.row_stride[k] = ptr, w, w
  return f


def mlp(ins=(3, 4), outs=(4, 2), act=0, n=None, w=P, b=P):
  m = abi.BxMlp()
  m.n_layers = len(outs) if n is None else n
  m.activation = act
  for l, (i, o) in enumerate(zip(ins, outs)):
    m.__getattribute__('in')[l], m.out[l], m.w[l], m.b[l] = i, o, w, b
  return m


def tensors(*specs):
  """specs: (n, p) per tensor; g, m, v are P."""
  t = (abi.BxOptTensor * len(specs))()
  for k, (n, p) in enumerate(specs):
    t[k].p, t[k].g, t[k].m, t[k].v, t[k].n, t[k].lr = p, P, P, P, n, 1e-3
  return t


def wsb(n=0):
  return C.pointer(C.c_int64(n))


def gae(**kw):
  a = dict(n_steps=2, n_envs=2, reward=seq(), done=seq(), truncation=seq(), values=seq(),
           bootstrap=P, vs=seq(), advantages=seq())
  a.update(kw)
  return tuple(a[k] for k in ('n_steps', 'n_envs', 'reward', 'done', 'truncation', 'values',
                              'bootstrap', 'vs', 'advantages')) + (1.0, 0.99, 0.95, None)


def ppo(**kw):
  a = dict(n_steps=2, n_envs=2, n_actions=3, logits=seq(), baseline=seq(), bootstrap=P,
           raw_action=seq(), eps=seq(), log_prob=seq(), reward=seq(), done=seq(),
           truncation=seq(), reward_scaling=1.0, discount=0.99, lam=0.95, clipping_epsilon=0.3,
           entropy_cost=1e-2, min_std=1e-3, normalize_advantage=1, losses=P, dlogits=seq(),
           dbaseline=seq(), vs=seq(), advantages=seq(), workspace=P, workspace_bytes=wsb(1 << 20))
  a.update(kw)
  return tuple(a.values()) + (None,)


def pert(rows=P, theta=Q, nd=4, npar=8, stride=8):
  return (rows, theta, nd, npar, stride, 0.1, 1, 0, 1, None, None)


def delta(out=P, weights=Q, nd=64, npar=10, ws=P, bytes_=wsb(1 << 20)):
  return (out, weights, nd, npar, 1, 0, None, ws, bytes_, None)


def ins(data=P, cap=4, row=4, pos=0, n=2, f=None):
  return (data, cap, row, pos, n, fields() if f is None else f, None)


def smp(data=P, cap=4, row=4, pos=0, size=4, n=2, f=None):
  return (data, cap, row, pos, size, n, 1, 0, fields() if f is None else f, None, None)


def fwd(net=None, rows=4, x=P, xs=3, y=P):
  return (mlp() if net is None else net, rows, x, xs, y, P, None)


def bwd(net=None, rows=10, x=P, xs=3, saved=P, dy=P, ws=P, bytes_=None):
  return (mlp() if net is None else net, rows, x, xs, saved, dy, P, None, ws,
          wsb(1 << 20) if bytes_ is None else bytes_, None)


def adam(t=None, n=None, step=1, b1=0.9, b2=0.999, eps=1e-8):
  t = tensors((4, P)) if t is None else t
  return (t, len(t) if n is None else n, step, b1, b2, eps, None)


def slabs(out=P, slab_n=4, n_slabs=2):
  return (out, slab_n, n_slabs, 1, 0, 0, None, 0)


NULL_SEQ = C.POINTER(abi.BxSeq)()
T40, T31 = 1 << 40, 1 << 31

# (entry point, arguments, bx_last_error())
REFUSALS = [
    ('bx_uniform', (P, -1, 1, 0, -1.0, 1.0, None), 'negative size'),
    ('bx_uniform', (P, T40 + 1, 1, 0, -1.0, 1.0, None), 'too many elements for one draw'),
    ('bx_uniform', (None, 4, 1, 0, -1.0, 1.0, None), 'null output'),
    ('bx_uniform_epoch', (P, 4, 1, 0, None, 0, -1.0, 1.0, None), 'null epoch counter'),
    ('bx_uniform_epoch', (None, 4, 1, 0, P, 0, -1.0, 1.0, None), 'null output'),
    ('bx_uniform_slabs', slabs(slab_n=-1) + (-1.0, 1.0, None), 'negative size'),
    ('bx_uniform_slabs', slabs(n_slabs=-1) + (-1.0, 1.0, None), 'negative size'),
    ('bx_uniform_slabs', slabs(slab_n=1 << 62, n_slabs=4) + (-1.0, 1.0, None),
     'too many elements for one draw'),
    ('bx_uniform_slabs', slabs(slab_n=1 << 21, n_slabs=1 << 20) + (-1.0, 1.0, None),
     'too many elements for one draw'),
    ('bx_uniform_slabs', slabs(out=None) + (-1.0, 1.0, None), 'null output'),
    ('bx_normal_slabs', slabs(slab_n=-1) + (None,), 'negative size'),
    ('bx_normal_slabs', slabs(n_slabs=-1) + (None,), 'negative size'),
    ('bx_normal_slabs', slabs(slab_n=1 << 62, n_slabs=4) + (None,), 'too many elements for one draw'),
    ('bx_normal_slabs', slabs(slab_n=1 << 21, n_slabs=1 << 20) + (None,),
     'too many elements for one draw'),
    ('bx_normal_slabs', slabs(out=None) + (None,), 'null output'),
    # bx_compute_gae
    ('bx_compute_gae', gae(reward=NULL_SEQ), 'null argument'),
    ('bx_compute_gae', gae(advantages=NULL_SEQ), 'null argument'),
    ('bx_compute_gae', gae(n_steps=0), 'n_steps must be >= 1'),
    ('bx_compute_gae', gae(n_envs=-1), 'negative n_envs'),
    ('bx_compute_gae', gae(n_envs=T31 + 1), 'too many envs for one launch'),
    ('bx_compute_gae', gae(done=seq(ptr=None)), 'null argument'),
    ('bx_compute_gae', gae(bootstrap=None), 'null argument'),
    ('bx_compute_gae', gae(vs=seq(ts=0)), 'zero stride on an output'),
    ('bx_compute_gae', gae(advantages=seq(es=0)), 'zero stride on an output'),
    # bx_population_perturb
    ('bx_population_perturb', pert(rows=None), 'null argument'),
    ('bx_population_perturb', pert(theta=None), 'null argument'),
    ('bx_population_perturb', pert(nd=0), 'n_directions must be >= 1'),
    ('bx_population_perturb', pert(npar=0), 'n_params must be >= 1'),
    ('bx_population_perturb', pert(stride=7), 'stride below n_params'),
    ('bx_population_perturb', pert(nd=2, npar=T40, stride=T40), 'too many samples for one launch'),
    ('bx_population_perturb', pert(nd=2, npar=1, stride=1 << 41), 'stride too large'),
    ('bx_population_perturb', pert(rows=P, theta=P + 16), 'rows overlap theta'),
    # bx_population_delta
    ('bx_population_delta', delta(bytes_=None), 'null argument'),
    ('bx_population_delta', delta(nd=0), 'n_directions must be >= 1'),
    ('bx_population_delta', delta(npar=0), 'n_params must be >= 1'),
    ('bx_population_delta', delta(nd=2, npar=T40), 'too many samples for one launch'),
    ('bx_population_delta', delta(out=None), 'null argument'),
    ('bx_population_delta', delta(weights=None), 'null argument'),
    ('bx_population_delta', delta(bytes_=wsb(8)), 'workspace of 8 bytes, 80 needed'),
    ('bx_population_delta', delta(ws=P + 4), 'workspace not 8-byte aligned'),
    ('bx_population_delta', delta(nd=65536 * 64, npar=1), 'too many directions for one launch'),
    # bx_replay_insert / bx_replay_sample (replay_args)
    ('bx_replay_insert', ins(n=-1), 'negative n_rows'),
    ('bx_replay_insert', ins(data=None), 'null argument'),
    ('bx_replay_insert', (P, 4, 4, 0, 2, None, None), 'null argument'),
    ('bx_replay_insert', ins(f=fields(n=9)), 'n_fields 9 outside 0..8'),
    ('bx_replay_insert', ins(f=fields(n=-1)), 'n_fields -1 outside 0..8'),
    ('bx_replay_insert', ins(cap=0), 'capacity must be >= 1'),
    ('bx_replay_insert', ins(row=-1), 'row_words outside 0..2^24'),
    ('bx_replay_insert', ins(row=(1 << 24) + 1), 'row_words outside 0..2^24'),
    ('bx_replay_insert', ins(cap=T40, row=2), 'ring too large'),
    ('bx_replay_insert', ins(pos=4), 'position outside the ring'),
    ('bx_replay_insert', ins(pos=-1), 'position outside the ring'),
    ('bx_replay_insert', ins(f=fields((5, -1))), 'field width outside 0..2^24'),
    ('bx_replay_insert', ins(f=fields((2, 1))), 'field widths sum to 3, row_words is 4'),
    ('bx_replay_insert', ins(f=fields(ptr=None)), 'null field pointer'),
    ('bx_replay_insert', ins(n=5), 'n_rows 5 above the capacity 4'),
    ('bx_replay_sample', smp(n=-1), 'negative n_samples'),
    ('bx_replay_sample', smp(data=None), 'null argument'),
    ('bx_replay_sample', smp(pos=4), 'position outside the ring'),
    ('bx_replay_sample', smp(f=fields((2, 1))), 'field widths sum to 3, row_words is 4'),
    ('bx_replay_sample', smp(size=0), 'size 0 outside 1..4'),
    ('bx_replay_sample', smp(size=5), 'size 5 outside 1..4'),
    # bx_mlp_* (mlp_args)
    ('bx_mlp_sizes', (None, C.pointer(C.c_int32())), 'null argument'),
    ('bx_mlp_sizes', (C.pointer(C.c_int32()), None), 'null argument'),
    ('bx_mlp_forward', (None, 4, P, 3, P, P, None), 'null argument'),
    ('bx_mlp_forward', fwd(mlp(n=0)), 'n_layers 0 outside 1..8'),
    ('bx_mlp_forward', fwd(mlp(n=9)), 'n_layers 9 outside 1..8'),
    ('bx_mlp_forward', fwd(mlp(act=7)), 'unknown activation 7'),
    ('bx_mlp_forward', fwd(mlp(act=-1)), 'unknown activation -1'),
    ('bx_mlp_forward', fwd(rows=-1), 'negative rows'),
    ('bx_mlp_forward', fwd(rows=T31 + 1), 'too many rows for one launch'),
    ('bx_mlp_forward', fwd(mlp(outs=(0, 2))), 'layer 0: width 0 outside 1..256'),
    ('bx_mlp_forward', fwd(mlp(outs=(4, 257))), 'layer 1: width 257 outside 1..256'),
    ('bx_mlp_forward', fwd(mlp(ins=(0, 4))), 'input width 0 outside 1..1024'),
    ('bx_mlp_forward', fwd(mlp(ins=(1025, 4)), xs=1025), 'input width 1025 outside 1..1024'),
    ('bx_mlp_forward', fwd(mlp(ins=(3, 5))), 'layer 1: in 5 != the previous out 4'),
    ('bx_mlp_forward', fwd(mlp(w=None)), 'null weight or bias'),
    ('bx_mlp_forward', fwd(mlp(b=None)), 'null weight or bias'),
    ('bx_mlp_forward', fwd(xs=2), 'x_stride 2 below the input width 3'),
    ('bx_mlp_forward', fwd(x=None), 'null argument'),
    ('bx_mlp_forward', fwd(y=None), 'null argument'),
    ('bx_mlp_backward', bwd()[:9] + (None, None), 'null argument'),
    ('bx_mlp_backward', bwd(mlp(act=3)), 'unknown activation 3'),
    ('bx_mlp_backward', bwd(xs=2), 'x_stride 2 below the input width 3'),
    ('bx_mlp_backward', bwd(x=None), 'null argument'),
    ('bx_mlp_backward', bwd(dy=None), 'null argument'),
    ('bx_mlp_backward', bwd(saved=None), 'null saved with hidden layers'),
    ('bx_mlp_backward', bwd(bytes_=wsb(16)), 'workspace of 16 bytes, 160 needed'),
    ('bx_mlp_backward', bwd(ws=P + 8), 'workspace not 16-byte aligned'),
    # bx_ppo_head
    ('bx_ppo_head', ppo(workspace_bytes=None), 'null argument'),
    ('bx_ppo_head', ppo(n_steps=0), 'n_steps must be >= 1'),
    ('bx_ppo_head', ppo(n_actions=0), 'n_actions must be >= 1'),
    ('bx_ppo_head', ppo(n_envs=-1), 'negative n_envs'),
    ('bx_ppo_head', ppo(n_actions=(1 << 20) + 1), 'too many actions'),
    ('bx_ppo_head', ppo(n_steps=T31 + 1), 'too many rows for one launch'),
    ('bx_ppo_head', ppo(n_envs=T31 + 1), 'too many rows for one launch'),
    ('bx_ppo_head', ppo(n_steps=1 << 16, n_envs=1 << 16), 'too many rows for one launch'),
    ('bx_ppo_head', ppo(logits=NULL_SEQ), 'null argument'),
    ('bx_ppo_head', ppo(truncation=seq(ptr=None)), 'null argument'),
    ('bx_ppo_head', ppo(bootstrap=None), 'null argument'),
    ('bx_ppo_head', ppo(losses=None), 'null argument'),
    ('bx_ppo_head', ppo(dlogits=NULL_SEQ), 'null argument'),
    ('bx_ppo_head', ppo(dbaseline=seq(ptr=None)), 'null argument'),
    ('bx_ppo_head', ppo(dlogits=seq(ts=0)), 'zero stride on an output'),
    ('bx_ppo_head', ppo(dbaseline=seq(es=0)), 'zero stride on an output'),
    ('bx_ppo_head', ppo(vs=seq(ts=0)), 'zero stride on an output'),
    ('bx_ppo_head', ppo(advantages=seq(es=0)), 'zero stride on an output'),
    ('bx_ppo_head', ppo(workspace_bytes=wsb(16)), 'workspace of 16 bytes, 80 needed'),
    ('bx_ppo_head', ppo(workspace=P + 8), 'workspace not 16-byte aligned'),
    # bx_opt_sizes / bx_adam_step (opt_check_scalars)
    ('bx_opt_sizes', (None,), 'null argument'),
    ('bx_adam_step', (None, 1, 1, 0.9, 0.999, 1e-8, None), 'null tensor table'),
    ('bx_adam_step', adam(n=0), 'n_tensors 0 outside 1..32'),
    ('bx_adam_step', adam(n=33), 'n_tensors 33 outside 1..32'),
    ('bx_adam_step', adam(step=0), 'step must be >= 1 (the count after this step)'),
    ('bx_adam_step', adam(b1=1.0), 'beta1 outside [0, 1)'),
    ('bx_adam_step', adam(b1=-0.1), 'beta1 outside [0, 1)'),
    ('bx_adam_step', adam(b1=float('nan')), 'beta1 outside [0, 1)'),
    ('bx_adam_step', adam(b2=1.0), 'beta2 outside [0, 1)'),
    ('bx_adam_step', adam(b2=float('nan')), 'beta2 outside [0, 1)'),
    ('bx_adam_step', adam(eps=-1e-8), 'negative eps'),
    ('bx_adam_step', adam(eps=float('nan')), 'negative eps'),
    ('bx_adam_step', adam(tensors((-1, P))), 'tensor 0: negative n'),
    ('bx_adam_step', adam(tensors((4, P), (4, None))), 'tensor 1: null p, g, m or v'),
    ('bx_adam_step', adam(tensors((4, P), (1 << 42, P))), 'too many elements for one launch'),
    # bx_system_plan / bx_system_blob (host only)
    ('bx_system_plan', (None, None, C.pointer(C.c_int32()), C.pointer(C.c_int32()),
                        C.pointer(C.c_int32())), 'null argument'),
    ('bx_system_blob', (None, None, None, 0, C.pointer(C.c_int64()), (C.c_int32 * 8)()),
     'null argument'),
]

# two faults at once: the first check in the order wins
ORDER = [
    ('bx_uniform_slabs', slabs(out=None, slab_n=-1) + (-1.0, 1.0, None), 'negative size'),
    ('bx_normal_slabs', slabs(out=None, slab_n=1 << 62, n_slabs=4) + (None,),
     'too many elements for one draw'),
    ('bx_uniform_epoch', (None, 4, 1, 0, None, 0, -1.0, 1.0, None), 'null epoch counter'),
    ('bx_compute_gae', gae(n_steps=0, n_envs=-1), 'n_steps must be >= 1'),
    ('bx_compute_gae', gae(n_steps=0, reward=NULL_SEQ), 'null argument'),
    ('bx_compute_gae', gae(n_envs=-1, done=seq(ptr=None)), 'negative n_envs'),
    ('bx_compute_gae', gae(vs=seq(ptr=None, ts=0)), 'null argument'),
    ('bx_population_perturb', pert(nd=0, npar=0), 'n_directions must be >= 1'),
    ('bx_population_perturb', pert(stride=7, theta=P), 'stride below n_params'),
    ('bx_population_delta', delta(out=None, bytes_=wsb(8)), 'null argument'),
    ('bx_population_delta', delta(ws=P + 4, bytes_=wsb(8)), 'workspace of 8 bytes, 80 needed'),
    ('bx_population_delta', delta(nd=65536 * 64, npar=1, ws=P + 4), 'workspace not 8-byte aligned'),
    ('bx_replay_insert', ins(n=-1, data=None), 'negative n_rows'),
    ('bx_replay_insert', ins(n=5, pos=4), 'position outside the ring'),
    ('bx_replay_insert', ins(cap=0, f=fields(n=9)), 'n_fields 9 outside 0..8'),
    ('bx_replay_insert', ins(f=fields((2, 1), ptr=None)), 'field widths sum to 3, row_words is 4'),
    ('bx_replay_sample', smp(n=-1, data=None), 'negative n_samples'),
    ('bx_replay_sample', smp(size=0, pos=4), 'position outside the ring'),
    ('bx_mlp_forward', fwd(mlp(act=7, n=0)), 'n_layers 0 outside 1..8'),
    ('bx_mlp_forward', fwd(mlp(act=7), rows=-1), 'unknown activation 7'),
    ('bx_mlp_forward', fwd(xs=2, x=None), 'x_stride 2 below the input width 3'),
    # (the size query comes after mlp_args: a null workspace does not hide its refusals)
    ('bx_mlp_backward', bwd(mlp(act=7), ws=None), 'unknown activation 7'),
    ('bx_mlp_backward', bwd(saved=None, bytes_=wsb(16)), 'null saved with hidden layers'),
    ('bx_mlp_backward', bwd(ws=P + 8, bytes_=wsb(16)), 'workspace of 16 bytes, 160 needed'),
    ('bx_ppo_head', ppo(n_steps=0, logits=NULL_SEQ), 'n_steps must be >= 1'),
    ('bx_ppo_head', ppo(n_actions=0, n_envs=-1), 'n_actions must be >= 1'),
    ('bx_ppo_head', ppo(n_steps=0, workspace=None), 'n_steps must be >= 1'),
    ('bx_ppo_head', ppo(logits=NULL_SEQ, dlogits=seq(ts=0)), 'null argument'),
    ('bx_ppo_head', ppo(dlogits=seq(ts=0), workspace_bytes=wsb(16)), 'zero stride on an output'),
    ('bx_ppo_head', ppo(workspace=P + 8, workspace_bytes=wsb(16)),
     'workspace of 16 bytes, 80 needed'),
    ('bx_adam_step', adam(n=0, step=0), 'n_tensors 0 outside 1..32'),
    ('bx_adam_step', adam(step=0, b1=1.0), 'step must be >= 1 (the count after this step)'),
    ('bx_adam_step', adam(b1=1.0, b2=1.0), 'beta1 outside [0, 1)'),
    ('bx_adam_step', adam(tensors((-1, P)), eps=-1.0), 'negative eps'),
    ('bx_adam_step', adam(tensors((4, None), (-1, P))), 'tensor 0: null p, g, m or v'),
]

# rc 0 and no error: nothing to do (the buffers may be null)
ZERO_WORK = [
    ('bx_uniform', (None, 0, 1, 0, -1.0, 1.0, None)),
    ('bx_uniform_epoch', (None, 0, 1, 0, None, 0, -1.0, 1.0, None)),
    ('bx_uniform_slabs', slabs(out=None, slab_n=0) + (-1.0, 1.0, None)),
    ('bx_uniform_slabs', slabs(out=None, n_slabs=0) + (-1.0, 1.0, None)),
    ('bx_normal_slabs', slabs(out=None, slab_n=0) + (None,)),
    ('bx_normal_slabs', slabs(out=None, n_slabs=0) + (None,)),
    ('bx_compute_gae', gae(n_envs=0, reward=seq(ptr=None), vs=seq(ptr=None, ts=0), bootstrap=None)),
    ('bx_replay_insert', ins(n=0, data=None, cap=0)),
    ('bx_replay_sample', smp(n=0, data=None, cap=0)),
    ('bx_mlp_forward', fwd(rows=0, x=None, y=None)),
    ('bx_mlp_backward', bwd(rows=0, x=None, dy=None, saved=None, bytes_=wsb(0))),
    ('bx_ppo_head', ppo(n_envs=0, logits=NULL_SEQ, bootstrap=None, workspace_bytes=wsb(0))),
    ('bx_adam_step', adam(tensors((0, None), (0, None)))),
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


@pytest.mark.parametrize('name,args,message', ORDER, ids=_ids(ORDER))
def test_first_fault_wins(name, args, message):
  assert _call(name, args) == (1, message)


@pytest.mark.parametrize('name,args', ZERO_WORK, ids=_ids(ZERO_WORK))
def test_zero_work_returns_ok(name, args):
  assert _call(name, args) == (0, 'null system')  # (the error text is left alone)


def test_population_delta_size_query():
  # ceil(n_directions / 64) chunks x n_params doubles
  for nd, npar, want in ((1, 1, 8), (64, 10, 80), (65, 10, 160), (1000, 37, 4736)):
    b = wsb(-1)
    assert _call('bx_population_delta', delta(out=None, weights=None, nd=nd, npar=npar, ws=None,
                                              bytes_=b))[0] == 0
    assert b.contents.value == want, (nd, npar)


def test_mlp_backward_size_query():
  # max(16, 4 x rows x the hidden widths' sum); rows == 0 still answers
  for net, rows, want in ((mlp((3,), (2,)), 10, 16), (mlp(), 10, 160), (mlp(), 0, 16),
                          (mlp((5, 7, 9), (7, 9, 2)), 33, 2112)):
    b = wsb(-1)
    assert _call('bx_mlp_backward', bwd(net, rows=rows, xs=8, x=None, dy=None, saved=None,
                                        ws=None, bytes_=b))[0] == 0
    assert b.contents.value == want, rows


def test_ppo_head_size_query():
  # the query comes before the null checks and the empty batch
  for T, B, want in ((2, 2, 80), (5, 300, 12112), (3, 0, 0)):
    b = wsb(-1)
    assert _call('bx_ppo_head', ppo(n_steps=T, n_envs=B, logits=NULL_SEQ, bootstrap=None,
                                    workspace=None, workspace_bytes=b))[0] == 0
    assert b.contents.value == want, (T, B)


def test_struct_sizes():
  a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
  assert _call('bx_mlp_sizes', (C.byref(a), C.byref(b)))[0] == 0
  assert _call('bx_opt_sizes', (C.byref(c),))[0] == 0
  assert (a.value, b.value, c.value) == (C.sizeof(abi.BxMlp), C.sizeof(abi.BxMlpGrads),
                                         C.sizeof(abi.BxOptTensor))


def test_system_blob_capacity():
  from tests.helpers import compiled
  _, d, rd, meta = compiled('ant')
  cd, keep = abi.make_desc(d)
  crd, keep_r = abi.make_reset_desc(rd, meta['num_joint_dof'])
  n, plan = C.c_int64(), (C.c_int32 * 8)()
  words = (C.c_uint32 * 4)()
  head = (C.byref(cd), C.byref(crd))
  assert _call('bx_system_blob', head + (None, 0, C.byref(n), plan))[0] == 0 and n.value > 4
  assert _call('bx_system_blob', head + (words, 4, C.byref(n), plan)) == (
      1, f'blob capacity 4 < {n.value} words')
  assert _call('bx_system_blob', head + (None, 0, None, plan)) == (1, 'null argument')
  assert _call('bx_system_blob', head + (None, 0, C.byref(n), None)) == (1, 'null argument')
  m = C.c_int32()
  for k in range(3):  # bx_system_plan: each null output
    outs = [C.byref(m)] * 3
    outs[k] = None
    assert _call('bx_system_plan', head + tuple(outs)) == (1, 'null argument')
  del keep, keep_r
