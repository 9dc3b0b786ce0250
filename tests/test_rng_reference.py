"""The host restatement of the counter RNG (`tests.helpers.uniform01_ref` /
`normal_ref`) on its own: the GPU tests hold the device generator to it per
sample (tests/test_gpu_rng_reference.py), so the distribution is checked here,
once, on the reference.

The bounds are conditions, not measurements: the Kolmogorov-Smirnov distance
to the standard normal times sqrt(n) <= 1.36 (the 5 % critical value), the
lag-1 autocorrelation times sqrt(n) within 3 (three standard deviations of an
independent sequence's), max |x| below sqrt(2 * 24 ln 2) = 5.77 (the largest
value 1 - U = 2^-24 can give), every value finite.
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import counters, normal_ref, splitmix_bits, uniform01_ref

N = 1 << 20
PAIRS = [(7, 3), (9, 40), (5, 1000), (2**63 + 11, 2**33 + 7)]


def test_splitmix_known_answers():
  """Python-int splitmix64 (arbitrary precision, masked) against the numpy
  one, on counters that carry out of 32 and out of 64 bits."""
  m = (1 << 64) - 1

  def bits(seed, i):
    z = (seed * 0x9E3779B97F4A7C15 + i + 0x632BE59BD9B4E019) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return (z ^ (z >> 31)) >> 40
  for seed in (0, 1, 7, 2**63 + 5, m):
    for i in (0, 1, 2**32 - 1, 2**32, 2**40 + 1, m - 1, m):
      assert int(splitmix_bits(seed, np.array([i], np.uint64))[0]) == bits(seed, i), (seed, i)
  # counters() wraps and carries like the device's uint64 arithmetic
  c = counters(2**32 - 3, 8)
  assert [int(v) for v in c] == [2**32 - 3 + j for j in range(8)]
  c = counters(m - 1, 4, 2)
  assert [int(v) for v in c] == [(m - 1 + 2 * j) & m for j in range(4)]


@pytest.mark.parametrize('seed,offset', PAIRS)
def test_normal_reference_distribution(seed, offset):
  x = normal_ref(seed, counters(offset, N, 2))
  assert x.dtype == np.float64 and x.shape == (N,)
  assert np.isfinite(x).all()
  top = float(np.abs(x).max())
  assert top < math.sqrt(2 * 24 * math.log(2.0)), top
  s = np.sort(x)
  cdf = (0.5 * (1.0 + torch.erf(torch.from_numpy(s) / math.sqrt(2.0)))).numpy()
  k = np.arange(N, dtype=np.float64)
  ks = max(float(((k + 1) / N - cdf).max()), float((cdf - k / N).max()))
  d = x - x.mean()
  lag1 = float((d[:-1] * d[1:]).sum() / (d * d).sum())
  print(f'seed {seed} offset {offset}: mean {x.mean():.3e} std {x.std(ddof=1):.5f} '
        f'KS*sqrt(n) {ks * math.sqrt(N):.2f} |lag1|*sqrt(n) {abs(lag1) * math.sqrt(N):.2f} '
        f'max|x| {top:.3f}')
  assert ks * math.sqrt(N) <= 1.36
  assert abs(lag1) * math.sqrt(N) <= 3.0


@pytest.mark.parametrize('seed,offset', PAIRS)
def test_uniform_reference(seed, offset):
  u = uniform01_ref(seed, counters(offset, N, 2))
  assert u.dtype == np.float64
  assert (u >= 0.0).all() and (u < 1.0).all()
  assert abs(float(u.mean()) - 0.5) <= 4.0 / math.sqrt(12.0 * N)
  # 24-bit values: the float32 cast loses nothing
  assert np.array_equal(u.astype(np.float32).astype(np.float64), u)


def test_float32_reference_is_float32():
  """The yardstick of the GPU comparison: the same formula in float32."""
  idx = counters(3, 4096, 2)
  x32, x64 = normal_ref(7, idx, dtype=np.float32), normal_ref(7, idx)
  assert x32.dtype == np.float32
  err = float(np.abs(x32.astype(np.float64) - x64).max())
  # float32's share: the cosine's argument rounds twice below 2 pi (half-ulp
  # 2.4e-7 each) under r <= 5.77, plus a few ulp of a result below 5.77:
  # under 5e-6 in all
  print(f'float32 normal_ref against float64: {err:.3e}')
  assert 0.0 < err < 5e-6, err
