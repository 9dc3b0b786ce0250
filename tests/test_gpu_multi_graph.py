"""A captured MULTI step, and the overflow buffer's lifetime under it.

`bx_system_step` on a MULTI system owns one piece of mutable device memory:
`movf`, each env's slice of the penetrating contacts past the first MCBUF =
128 of a collision pass. A graph captured at one batch has the buffer's
address in its kernel arguments, so the address has to stay valid for as long
as the System lives, whatever batches are stepped later: growth to a larger
`n_envs` makes a new allocation and keeps the superseded ones until
`bx_system_destroy`, and a capture at a batch never stepped is refused (a
capture cannot allocate).

The scene is `tests.helpers.piled_mountain4` with all pairs at `substeps = 2`,
as tests/test_gpu_multi_overflow.py: one step lists 184-186 penetrating rows
per env (the float64 oracle's counts are pinned on the CPU there), so the
captured launch really writes the buffer and reads it back. 3 and 8 envs, env
e on row e of the 16-env actions.

Every comparison is `torch.equal` between runs of the same kernel on the same
inputs (state `pos` / `rot` / `vel` / `ang`; with Info also `Info.contact`
`vel` / `ang` and `contact_penetration`): no tolerance anywhere. The capture
recipe is `brax_amd/envs/graph.py::_Captured._capture`: a warm-up on a side
stream, then `torch.cuda.graph(..., capture_error_mode='thread_local')` over
static inputs and outputs.
"""
import functools
import gc

import numpy as np
import pytest
import torch

from tests.helpers import config_for, piled_actions, piled_mountain4, set_variant

pytestmark = pytest.mark.gpu

MCBUF = 128  # pbd_layout.h: the listed contacts kept in LDS; the rest go to the overflow buffer
MOVF_W = 12  # pbd_layout.h: words per overflow record
VARIANTS = ['multi', 'multi256']
QP = ('pos', 'rot', 'vel', 'ang')
REFUSAL = 'step the batch once before capturing it'


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _piled():
  """(cfg, (N, 13) start state, two steps' (16, 32) actions). Read-only."""
  cfg, q0 = piled_mountain4(0, 2)
  return cfg, q0, piled_actions(16, 2)


@pytest.fixture
def piled(oracle_lib):
  del oracle_lib  # piled_mountain4 reads the default state off the built oracle
  return _piled()


def _system(cfg, dev, variant):
  import brax_amd
  from brax_amd import _native
  sys_ = brax_amd.System(cfg, device=dev)
  _native.check(set_variant(sys_, variant))
  return sys_


def _start(piled, n, dev):
  """The piled scene's inputs for n envs: the packed (n, N, 16) start state
  and the two steps' (n, 32) actions, on the device."""
  from brax_amd.base import packed_buffer, qp_from_numpy
  _, q0, acts = piled
  buf = packed_buffer(qp_from_numpy(np.repeat(q0[None], n, axis=0), dev))
  return buf, [torch.as_tensor(a[:n], dtype=torch.float32, device=dev).contiguous() for a in acts]


def _snap(qp, info):
  """Copies of a step's compared outputs, by name."""
  out = {f: getattr(qp, f).clone() for f in QP}
  if info is not None:
    out['contact_vel'] = info.contact.vel.clone()
    out['contact_ang'] = info.contact.ang.clone()
    out['contact_penetration'] = info.contact_penetration.clone()
  return out


def _assert_same(got, want, what):
  assert got.keys() == want.keys(), what
  for k in want:
    assert torch.equal(got[k], want[k]), (what, k)


def _rows(snap, lo, hi):
  return {k: v[lo:hi] for k, v in snap.items()}


def _eager(sys_, buf, act, info=True):
  """One uncaptured step from the packed state `buf`: (the output QP, the
  snapshot of its compared outputs)."""
  from brax_amd.base import packed_view
  qp, inf = sys_.step(packed_view(buf), act, info=info)
  torch.cuda.synchronize()
  return qp, _snap(qp, inf)


class _StepGraph:
  """One `System.step` captured over a static packed state and static
  actions; `replay` rewrites both, replays and snapshots the static outputs."""

  def __init__(self, sys_, buf, act, info=True, warm_up=True):
    from brax_amd.base import packed_view
    dev = sys_.device
    self.qp, self.act = buf.clone(), act.clone()

    def body():
      return sys_.step(packed_view(self.qp), self.act, info=info)

    with torch.cuda.device(dev):
      if warm_up:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
          body()
        torch.cuda.current_stream(dev).wait_stream(side)
      # the Systems that earlier tests dropped wait in reference cycles for the
      # cyclic collector, and their finaliser frees device memory: collected
      # here, never inside the capture, where the hipFree would invalidate it
      gc.collect()
      self.graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
        self.out = body()
      torch.cuda.current_stream(dev).synchronize()

  def replay(self, buf, act):
    # the 13 state words of each body; the packed rows' 3 pad words stay
    self.qp[..., :13].copy_(buf[..., :13])
    self.act.copy_(act)
    self.graph.replay()
    torch.cuda.synchronize()
    return _snap(*self.out)


def _refused_capture(sys_, buf, act):
  """Enters a capture and calls `step` in it with no warm-up (a warm-up would
  be the eager step that grows the buffer): the library refuses before any
  launch, and the context ends the (empty) capture on its way out."""
  from brax_amd import _native
  with pytest.raises(_native.NativeError, match=REFUSAL):
    _StepGraph(sys_, buf, act, warm_up=False)
  assert not torch.cuda.is_current_stream_capturing()


@functools.lru_cache(maxsize=None)
def _fresh(variant, n, dev):
  """Step 0 of the piled scene's first n envs on a System of its own, with
  Info: the snapshot. Computed once per (variant, n); read-only."""
  sys_ = _system(_piled()[0], dev, variant)
  buf, acts = _start(_piled(), n, dev)
  return _eager(sys_, buf, acts[0])[1]


def _penetrating(snap):
  return (snap['contact_penetration'] > 0).sum(-1).tolist()


CAPTURED = [('multi', True), ('multi', False), ('multi256', True), ('multi256', False),
            ('ant', True)]


@pytest.mark.parametrize('variant,info', CAPTURED,
                         ids=[f'{v}-{"info" if i else "noinfo"}' for v, i in CAPTURED])
def test_captured_step_replays_to_the_eager_bits(dev, piled, variant, info):
  """Two eager steps chained at B = 3 (the first allocates the overflow
  buffer), then one step captured from the same start state and replayed
  twice, the second replay from the first one's output with step 1's
  actions: both replays are the eager chain bit for bit, state and Info. On
  the piled scene the eager Info shows that an env listed more than MCBUF
  penetrating rows, so the captured launch went through the buffer. `ant` is
  the same through plain `System.step` on the SINGLE kernel, which has no
  such buffer (only `Env.step` is captured elsewhere)."""
  from brax_amd.base import pack_qp, packed_buffer
  B = 3
  if variant == 'ant':
    import brax_amd
    sys_ = brax_amd.System(config_for('ant'), device=dev)
    buf0 = pack_qp(sys_.default_qp(), dev)[None].repeat(B, 1, 1).contiguous()
    g = torch.Generator().manual_seed(3)
    acts = [(torch.rand((B, sys_.action_size), generator=g) * 2 - 1).to(dev) for _ in range(2)]
  else:
    sys_ = _system(piled[0], dev, variant)
    buf0, acts = _start(piled, B, dev)
  qp1, e1 = _eager(sys_, buf0, acts[0], info)
  _, e2 = _eager(sys_, packed_buffer(qp1), acts[1], info)
  for s in (e1, e2):
    for k, v in s.items():
      assert torch.isfinite(v).all(), k
  if variant != 'ant':  # (without Info: the same step's Info from a System of its own)
    n = _penetrating(e1 if info else _fresh(variant, B, dev))
    print(f'{variant}: device penetrating rows per env at B = 3: {n}')
    assert max(n) > MCBUF, n

  graph = _StepGraph(sys_, buf0, acts[0], info)
  r1 = graph.replay(buf0, acts[0])
  _assert_same(r1, e1, 'replay 1')
  r2 = graph.replay(packed_buffer(graph.out[0]).clone(), acts[1])
  _assert_same(r2, e2, 'replay 2')
  assert not torch.equal(r1['pos'], r2['pos'])  # the static inputs were read again


@pytest.mark.parametrize('variant', VARIANTS)
def test_growth_after_capture_leaves_the_graph_its_buffer(dev, piled, variant):
  """A graph captured at B = 3 holds the 3-env buffer's address. An
  uncaptured step at B = 8 on the same System then grows the buffer (a new
  allocation, the old one kept), and fresh torch tensors of more than the old
  buffer's size are allocated and filled, so a freed buffer would plausibly
  have been handed out again. The B = 3 graph still replays to its first
  replay's bits and the tensors keep their fill; the B = 8 result is a fresh
  System's and its rows 0-2 are the B = 3 rows (envs are independent); a
  second graph captured at B = 8 and the first, replayed alternately twice
  each, give their own eager bits every time."""
  sys_ = _system(piled[0], dev, variant)
  buf3, acts3 = _start(piled, 3, dev)
  buf8, acts8 = _start(piled, 8, dev)
  e3 = _eager(sys_, buf3, acts3[0])[1]
  assert max(_penetrating(e3)) > MCBUF
  g3 = _StepGraph(sys_, buf3, acts3[0])
  r3 = g3.replay(buf3, acts3[0])
  _assert_same(r3, e3, 'B = 3 replay before growth')

  e8 = _eager(sys_, buf8, acts8[0])[1]  # grows the buffer
  old_bytes = 3 * (sys_.num_rows - MCBUF) * MOVF_W * 4
  assert old_bytes > 0
  torch.cuda.empty_cache()
  fill = [torch.full((max(old_bytes, 1 << 20) // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
          for _ in range(8)]
  torch.cuda.synchronize()

  _assert_same(g3.replay(buf3, acts3[0]), r3, 'B = 3 replay after growth')
  for t in fill:
    assert bool((t == 0x5A5A5A5A).all())
  _assert_same(e8, _fresh(variant, 8, dev), 'B = 8 against a fresh System')
  _assert_same(_rows(e8, 0, 3), e3, 'B = 8 rows 0-2 against B = 3')

  g8 = _StepGraph(sys_, buf8, acts8[0])
  for i in range(2):
    _assert_same(g3.replay(buf3, acts3[0]), e3, f'B = 3 replay, round {i}')
    _assert_same(g8.replay(buf8, acts8[0]), e8, f'B = 8 replay, round {i}')
  for t in fill:
    assert bool((t == 0x5A5A5A5A).all())


@pytest.mark.parametrize('variant', VARIANTS)
def test_capture_before_the_first_step_is_refused_and_harmless(dev, piled, variant):
  """On a fresh System, `step` at B = 3 inside a capture raises the library's
  error (the buffer would have to be allocated), and once the context has
  closed the stream is not capturing: an eager B = 3 step on the same System
  gives a fresh System's bits. The same with a B = 3 graph in place and a
  captured call at B = 8: refused, the B = 3 graph still replays to its bits,
  and an eager B = 8 step afterwards gives a fresh System's bits. The refusal
  returns before any launch, so both aborted captures are empty."""
  sys_ = _system(piled[0], dev, variant)
  buf3, acts3 = _start(piled, 3, dev)
  buf8, acts8 = _start(piled, 8, dev)
  _refused_capture(sys_, buf3, acts3[0])
  e3 = _eager(sys_, buf3, acts3[0])[1]
  _assert_same(e3, _fresh(variant, 3, dev), 'B = 3 after the refused capture')

  g3 = _StepGraph(sys_, buf3, acts3[0])
  _assert_same(g3.replay(buf3, acts3[0]), e3, 'B = 3 replay')
  _refused_capture(sys_, buf8, acts8[0])
  _assert_same(g3.replay(buf3, acts3[0]), e3, 'B = 3 replay after the refused B = 8 capture')
  e8 = _eager(sys_, buf8, acts8[0])[1]
  _assert_same(e8, _fresh(variant, 8, dev), 'B = 8 after the refused capture')
  _assert_same(g3.replay(buf3, acts3[0]), e3, 'B = 3 replay after the B = 8 step')


@pytest.mark.parametrize('variant', VARIANTS)
def test_destroy_with_superseded_buffers(dev, piled, variant):
  """A System stepped at 3, 8, 16 and 3 envs holds one current and two
  superseded overflow buffers, and a graph captured at 3 holds the first.
  Dropping the graph and the System frees all three; a new System then steps
  3 envs to the first one's first bits. Nothing is asserted about addresses."""
  sys_ = _system(piled[0], dev, variant)
  first = None
  graph = None
  for n in (3, 8, 16, 3):
    buf, acts = _start(piled, n, dev)
    snap = _eager(sys_, buf, acts[0])[1]
    if first is None:
      first = snap
      graph = _StepGraph(sys_, buf, acts[0])
      _assert_same(graph.replay(buf, acts[0]), first, 'B = 3 replay')
    else:
      _assert_same(_rows(snap, 0, 3), first, f'rows 0-2 at B = {n}')
  del graph, sys_
  gc.collect()
  torch.cuda.synchronize()
  again = _system(piled[0], dev, variant)
  buf, acts = _start(piled, 3, dev)
  _assert_same(_eager(again, buf, acts[0])[1], first, 'a new System at B = 3')
