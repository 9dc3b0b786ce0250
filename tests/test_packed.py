"""The packed launches' host side (no GPU, no library): `packed.Layout`
against the block the C entry points document (per step: qp (B, N, 16) | obs
(B, O) | reward, done, steps, truncation (B,) each | metrics (B, M), float32
words), its `out` check, and `pack_qp`."""
import pytest
import torch

from brax_amd.base import QP, pack_qp, packed_view
from brax_amd.envs.packed import FIELDS, Layout

K, B, N, O = 3, 2, 2, 5
CPU = torch.device('cpu')


def _expected(M):
  """(block, {field: (word offset within a block, per-step shape)}), written
  out from the header's description."""
  shapes = {'qp': (B, N, 16), 'obs': (B, O), 'reward': (B,), 'done': (B,), 'steps': (B,),
            'truncation': (B,), 'metrics': (B, M)}
  offsets = {'qp': 0, 'obs': B * N * 16, 'reward': B * N * 16 + B * O,
             'done': B * N * 16 + B * O + B, 'steps': B * N * 16 + B * O + 2 * B,
             'truncation': B * N * 16 + B * O + 3 * B, 'metrics': B * N * 16 + B * O + 4 * B}
  block = B * N * 16 + B * O + 4 * B + B * M
  return block, {f: (offsets[f], shapes[f]) for f in FIELDS}


@pytest.mark.parametrize('M', [3, 0])
def test_layout_views_alias_the_buffer_at_the_documented_offsets(M):
  block, want = _expected(M)
  lay = Layout(B, N, O, M)
  assert lay.block == block
  assert lay.offset == {f: off for f, (off, _) in want.items()}
  # two spare words at the end: the views cover the first K blocks only
  buf = torch.arange(K * block + 2, dtype=torch.float32)
  views = lay.views(buf, K)
  assert len(views) == len(FIELDS)
  for f, v in zip(FIELDS, views):
    off, shape = want[f]
    assert tuple(v.shape) == (K,) + shape, f
    assert v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), f
    assert v.storage_offset() == off, f
    for t in range(K):  # step t's field is the contiguous run of its words
      n = v[t].numel()
      assert torch.equal(v[t].reshape(-1), buf[t * block + off:t * block + off + n]), (f, t)
  for t in (0, K - 1):
    step = lay.step_views(buf[t * block:(t + 1) * block])
    assert len(step) == len(FIELDS)
    for f, v, kv in zip(FIELDS, step, views):
      off, shape = want[f]
      assert tuple(v.shape) == shape, f
      assert v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), f
      assert v.storage_offset() == t * block + off, f
      assert v.is_contiguous() and torch.equal(v, kv[t]), f
  views[3][K - 1, 1] = -7.  # done of the last step's env 1, through the view
  assert buf[(K - 1) * block + want['done'][0] + 1] == -7.


def test_out_buffer_allocates_or_validates():
  lay = Layout(B, N, O, 3)
  n = K * lay.block
  new = lay.out_buffer(None, K, CPU)
  assert new.shape == (n,) and new.dtype == torch.float32 and new.is_contiguous()
  ok = torch.empty(n + 5)
  assert lay.out_buffer(ok, K, CPU) is ok
  msg = f'out must hold {n} contiguous float32 on cpu'
  for bad in (torch.empty(n - 1), torch.empty(2 * n)[::2], torch.empty(n, dtype=torch.float64)):
    with pytest.raises(ValueError) as e:
      lay.out_buffer(bad, K, CPU)
    assert str(e.value) == msg


def test_pack_qp():
  g = torch.Generator().manual_seed(0)
  f = [torch.randn((B, N, w), generator=g) for w in (3, 4, 3, 3)]
  buf = pack_qp(QP(*f), CPU)
  assert buf.shape == (B, N, 16) and buf.dtype == torch.float32 and buf.is_contiguous()
  assert torch.equal(buf[..., :13], torch.cat(f, -1))
  assert not buf[..., 13:].any()
  b = torch.randn((B, N, 16), generator=g)
  assert pack_qp(packed_view(b), CPU) is b
  # a QP of the buffer's own field views is recognised too
  assert pack_qp(QP(b[..., 0:3], b[..., 3:7], b[..., 7:10], b[..., 10:13]), CPU) is b
