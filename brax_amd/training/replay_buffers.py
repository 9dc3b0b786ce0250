"""The replay queue of the off-policy learner, on the device, ONE launch per
insert and per sample.

`UniformSamplingQueue` is the reference's
(`brax/training/replay_buffers.py:61-131`, `:190-215`): a FIFO of the last
`max_replay_size` rows, each row the flattened fields of one transition,
sampled uniformly with replacement. Two things differ, neither visible in what
a learner reads:

* `insert` wraps inside the batch instead of rolling. The reference rolls the
  whole `(max_replay_size, row)` array when a batch would run past the end
  (`:117-123`) and then writes it in one piece; here batch row r goes to ring
  row `(position + r) % capacity`. The physical placement then differs, the
  queue does not: after any sequence of inserts, `size` is the reference's and
  the age-ordered content `data[(position - size + i) % capacity]`, i <
  `size` (oldest first), equals the reference's
  `data[(current_position - current_size + i) % capacity]`
  (`tests/test_sac.py` holds the chained form to a numpy restatement of the
  reference's roll).
* `sample`'s indices are a pure function of `(seed, counter)`, like all of
  the project's noise, not of a generator's state: sample j of a call is ring
  row `(position - size + mulhi64(mix(seed, counter + j), size)) % capacity`
  with `mix` the counter RNG's 64-bit splitmix64 finaliser, and the call
  advances `counter` by `sample_batch_size`.

`fused=None` takes `bx_replay_insert` / `bx_replay_sample` for float32 device
data; the chained form (`fused=False`) builds the same rows and the same
indices from torch operations on any device and dtype, and is both the
fallback and the kernels' yardstick.
"""
import collections
import ctypes as C
from typing import Dict, Mapping, Optional

import torch

from brax_amd import abi
from brax_amd.fused import use_kernel
from brax_amd.system import launch

_M64 = (1 << 64) - 1


def transition_fields(observation_size: int, action_size: int) -> 'collections.OrderedDict[str, int]':
  """SAC's `Transition` in the reference's `ravel_pytree` order
  (`sac/train.py:185-196`): the row is 2 * O + A + 3 words."""
  return collections.OrderedDict([
      ('observation', int(observation_size)), ('action', int(action_size)), ('reward', 1),
      ('discount', 1), ('next_observation', int(observation_size)), ('truncation', 1)])


def _i64(x: int) -> int:
  """The int64 whose bits are the uint64 `x mod 2^64`."""
  x &= _M64
  return x - (1 << 64) if x >> 63 else x


def _lsr(z, s):
  """Logical right shift of int64 bit patterns."""
  return (z >> s) & ((1 << (64 - s)) - 1)


def mix64(seed: int, counters: torch.Tensor) -> torch.Tensor:
  """`mix(seed, i)` of int64 counters `i` (uint64 bit patterns): splitmix64's
  finaliser in torch's wrapping int64 arithmetic (`bx_mix.h`)."""
  z = counters + _i64(seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019)
  z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
  z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
  return z ^ _lsr(z, 31)


def mulhi64(z: torch.Tensor, n: int) -> torch.Tensor:
  """The high 64 bits of the unsigned 128-bit product `z * n`, `z` int64 bit
  patterns, 0 <= n < 2^63: 32-bit limbs, every partial sum below 2^64."""
  lo = (1 << 32) - 1
  zl, zh = z & lo, _lsr(z, 32)
  nl, nh = n & lo, n >> 32
  ll, lh, hl, hh = zl * nl, zl * nh, zh * nl, zh * nh
  mid = _lsr(ll, 32) + (lh & lo) + (hl & lo)
  return hh + _lsr(lh, 32) + _lsr(hl, 32) + _lsr(mid, 32)


def sample_rows(seed: int, offset: int, n: int, position: int, size: int, capacity: int,
                device=None) -> torch.Tensor:
  """The `n` ring rows `bx_replay_sample` draws at counter `offset`, int64."""
  j = torch.arange(n, dtype=torch.int64, device=device) + _i64(offset)  # wraps as uint64
  k = mulhi64(mix64(seed, j), size)
  return (k + (position - size)) % capacity


class UniformSamplingQueue:
  """See the module's text.

  Args:
    max_replay_size: the capacity in rows.
    fields: ordered mapping name -> width in words (`transition_fields`).
    sample_batch_size: rows per `sample`.
    seed: of the index draws.
    device, dtype: of `data` (the kernels take float32 on a GPU).
  Attributes:
    data: `(max_replay_size, row_words)`; position, size: host ints (batch
      sizes are static, so nothing needs a device control block); counter: the
      draw counter of the next `sample`.
  """

  def __init__(self, max_replay_size: int, fields: Mapping[str, int], sample_batch_size: int,
               seed: int = 0, device=None, dtype=torch.float32):
    if max_replay_size < 1:
      raise ValueError('max_replay_size must be >= 1')
    if len(fields) > abi.FIELDS_MAX:
      raise ValueError(f'more than {abi.FIELDS_MAX} fields')
    self.fields = collections.OrderedDict((k, int(v)) for k, v in fields.items())
    if any(v < 1 for v in self.fields.values()):
      raise ValueError('field widths must be >= 1')
    self.capacity = int(max_replay_size)
    self.row_words = sum(self.fields.values())
    self.sample_batch_size = int(sample_batch_size)
    self.seed = int(seed)
    self.data = torch.zeros((self.capacity, self.row_words), dtype=dtype, device=device)
    self.position = 0
    self.size = 0
    self.counter = 0

  # ---- shared ---------------------------------------------------------------------------------

  def _why_not_fused(self, tensors) -> Optional[str]:
    if self.data.dtype != torch.float32:
      return f'{self.data.dtype} data is not float32'
    if not self.data.is_cuda:
      return 'CPU data'
    for t in tensors:
      if t.dtype != torch.float32:
        return f'{t.dtype} is not float32'
      if t.device != self.data.device:
        return f'data on {self.data.device}, a field on {t.device}'
    return None

  def _rows(self, mapping, what) -> Dict[str, torch.Tensor]:
    """The mapping's tensors as (n, width) views, in field order."""
    if set(mapping.keys()) != set(self.fields):
      raise ValueError(f'{what} must hold exactly the fields {list(self.fields)}')
    out, n = {}, None
    for name, width in self.fields.items():
      t = mapping[name]
      if t.dim() == 1 and width == 1:
        t = t[:, None]
      if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f'{what}[{name!r}] {tuple(mapping[name].shape)}: want (n, {width})')
      n = t.shape[0] if n is None else n
      if t.shape[0] != n:
        raise ValueError(f'{what}: {name!r} has {t.shape[0]} rows, not {n}')
      out[name] = t
    return out

  def _descriptor(self, rows):
    """`bx_fields` over (n, width) float32 tensors whose words are adjacent."""
    f = abi.BxFields()
    f.n_fields = len(rows)
    for k, t in enumerate(rows):
      f.ptr[k] = t.data_ptr()
      f.width[k] = t.shape[1]
      f.row_stride[k] = t.stride(0)
    return f

  # ---- insert ---------------------------------------------------------------------------------

  def insert(self, batch: Mapping[str, torch.Tensor], fused: Optional[bool] = None):
    """Appends the batch's n rows; the oldest rows leave when the queue is
    full. `batch[name]` is `(n, width)`, or `(n,)` for a width of 1; column
    slices of wider tensors pass to the kernel without a copy.

    fused: None takes the kernel for float32 tensors on the data's GPU, else
      the chained form; True raises NotImplementedError where the kernel does
      not apply; False forces the chained form.
    """
    rows = self._rows(batch, 'batch')
    tensors = [t.detach() for t in rows.values()]
    n = tensors[0].shape[0]
    if n > self.capacity:
      raise ValueError('Trying to insert a batch of samples larger than the maximum replay '
                       f'size. num_samples: {n}, max replay size {self.capacity}')
    kernel = use_kernel(fused, 'insert', lambda: self._why_not_fused(tensors))
    if n == 0:
      return self
    if not kernel:
      flat = torch.cat([t.to(self.data.device, self.data.dtype) for t in tensors], dim=1)
      at = (torch.arange(n, dtype=torch.int64, device=self.data.device) + self.position) % self.capacity
      self.data.index_copy_(0, at, flat)
    else:
      tensors = [t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous() for t in tensors]
      src = self._descriptor(tensors)
      launch(self.data.device, 'bx_replay_insert', self.data.data_ptr(), self.capacity,
             self.row_words, self.position, n, C.byref(src))
    self.position = (self.position + n) % self.capacity
    self.size = min(self.size + n, self.capacity)
    return self

  # ---- sample ---------------------------------------------------------------------------------

  def sample(self, fused: Optional[bool] = None, out: Optional[Mapping[str, torch.Tensor]] = None,
             indices: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """`sample_batch_size` rows, uniform with replacement over the live rows,
    as a mapping name -> contiguous `(sample_batch_size, width)` tensor; the
    draw counter advances by `sample_batch_size`.

    fused: as `insert`'s.
    out: optional mapping of tensors to write (`(n, width)`, or `(n,)` for a
      width of 1; the kernel writes views whose words are adjacent in place).
    indices: optional `(sample_batch_size,)` int64 tensor on the data's
      device that receives the ring rows drawn.
    """
    if self.size < 1:
      raise ValueError('the replay queue is empty')
    n, dev = self.sample_batch_size, self.data.device
    if out is None:
      out = {k: torch.empty((n, w), dtype=self.data.dtype, device=dev)
             for k, w in self.fields.items()}
    rows = self._rows(out, 'out')
    tensors = list(rows.values())
    if tensors[0].shape[0] != n:
      raise ValueError(f'out must hold {n} rows')
    if indices is not None and (indices.dtype != torch.int64 or tuple(indices.shape) != (n,)
                                or indices.device != dev or not indices.is_contiguous()):
      raise ValueError(f'indices must be a contiguous int64 ({n},) tensor on {dev}')

    def why_not():
      why = self._why_not_fused(tensors)
      if why is None and any(t.stride(1) != 1 and t.shape[1] != 1 for t in tensors):
        why = 'an out field whose words are not adjacent'
      return why
    kernel = use_kernel(fused, 'sample', why_not)
    offset = self.counter & _M64
    self.counter = (self.counter + n) & _M64
    if n == 0:
      return dict(out)
    if not kernel:
      idx = sample_rows(self.seed, offset, n, self.position, self.size, self.capacity, dev)
      if indices is not None:
        indices.copy_(idx)
      flat = self.data.index_select(0, idx)
      for t, part in zip(tensors, torch.split(flat, list(self.fields.values()), dim=1)):
        t.copy_(part)
    else:
      dst = self._descriptor(tensors)
      launch(dev, 'bx_replay_sample', self.data.data_ptr(), self.capacity, self.row_words,
             self.position, self.size, n, self.seed & _M64, offset, C.byref(dst),
             None if indices is None else indices.data_ptr())
    return dict(out)
