"""The device's counter RNG against its host restatement, sample by sample.

`bx_uniform` / `bx_uniform_slabs` / `bx_normal_slabs` and the fused policy
kernel's noise all come from `uniform_at` / `normal_at` (pbd_kernels.hip);
`tests.helpers.uniform01_ref` / `normal_ref` restate them in numpy from the
documented formulas (their distribution: tests/test_rng_reference.py). Seeds
and counters reach past 2^32 and 2^63, so a truncated or carry-less counter
shows.

Tolerances:
* [0, 1) uniforms: bit for bit ((z >> 40) * 2^-24 is exact in float32).
* [lo, hi) = [-1, 1): 2^-23 absolute against float64 lo + (hi - lo) u - at
  most two float32 roundings, of a product below 2 (half-ulp 2^-24) and of a
  sum in [-1, 1) (half-ulp at most 2^-25), contracted or not.
* normals: measured, by the policy tests' rule. The yardstick is `normal_ref`
  in float32 against float64 (largest absolute error over the batch); the
  device may be within 8 x that plus 1e-6 (fast log / cos, another rounding of
  2 pi u). Each figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import counters, normal_ref, uniform01_ref

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 2**63 + 5]
OFFSETS = [0, 2**32 - 3, 2**40 + 1]
PAIRS = [(7, 3), (9, 40), (5, 1000), (2**63 + 11, 2**33 + 7)]


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _stream(dev):
  from brax_amd.system import _stream as s
  return s(dev.index)


def _uniform(dev, n, seed, offset, lo, hi):
  from brax_amd import _native
  out = torch.full((n + 1,), -7.0, dtype=torch.float32, device=dev)
  _native.check(_native.lib().bx_uniform(C.c_void_p(out.data_ptr()), n, seed, offset, lo, hi,
                                         _stream(dev)))
  got = out.cpu().numpy()
  assert got[n] == -7.0, 'wrote past n'
  return got[:n]


def _uniform_slabs(dev, slab_n, n_slabs, seed, offset, stride, lo, hi):
  from brax_amd import _native
  out = torch.full((n_slabs * slab_n + 1,), -7.0, dtype=torch.float32, device=dev)
  _native.check(_native.lib().bx_uniform_slabs(C.c_void_p(out.data_ptr()), slab_n, n_slabs, seed,
                                               offset, stride, None, 0, lo, hi, _stream(dev)))
  got = out.cpu().numpy()
  assert got[-1] == -7.0, 'wrote past the slabs'
  return got[:-1].reshape(n_slabs, slab_n)


def _normal_slabs(dev, slab_n, n_slabs, seed, offset, stride, epoch=None, epoch_stride=0):
  from brax_amd import _native
  out = torch.full((n_slabs * slab_n + 1,), -7.0, dtype=torch.float32, device=dev)
  _native.check(_native.lib().bx_normal_slabs(
      C.c_void_p(out.data_ptr()), slab_n, n_slabs, seed, offset, stride,
      None if epoch is None else C.c_void_p(epoch.data_ptr()), epoch_stride, _stream(dev)))
  got = out.cpu().numpy()
  assert got[-1] == -7.0, 'wrote past the slabs'
  return got[:-1].reshape(n_slabs, slab_n)


def _slab_counters(offset, slab_n, n_slabs, stride, step):
  return np.stack([counters(offset + s * stride, slab_n, step) for s in range(n_slabs)])


def _normal_gate(got, seed, idx, label):
  """The measured rule; returns the device / yardstick ratio."""
  r64 = normal_ref(seed, idx)
  r32 = normal_ref(seed, idx, dtype=np.float32)
  assert got.dtype == np.float32 and got.shape == r64.shape
  assert np.isfinite(got).all()
  err = float(np.abs(got.astype(np.float64) - r64).max())
  yard = float(np.abs(r32.astype(np.float64) - r64).max())
  ratio = err / max(yard, 1e-30)
  print(f'{label}: device err {err:.3e}  float32 yardstick {yard:.3e}  ratio {ratio:.2f}')
  if not err <= 8 * yard + 1e-6:
    # which Box-Muller term carries it: the radius (counter i) or the cosine
    # (counter i + 1), each against the device's product
    k = int(np.argmax(np.abs(got.astype(np.float64) - r64)))
    i = idx.ravel()[k]
    u0, u1 = uniform01_ref(seed, i), uniform01_ref(seed, i + np.uint64(1))
    r, c = np.sqrt(-2.0 * np.log(1.0 - u0)), np.cos(2.0 * np.pi * u1)
    print(f'{label}: worst sample {k}: u0 {u0!r} u1 {u1!r} r {r!r} c {c!r} '
          f'device {got.ravel()[k]!r} reference {r64.ravel()[k]!r}')
  assert err <= 8 * yard + 1e-6, (label, err, yard)
  return ratio


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('seed', SEEDS)
def test_uniform01_bit_exact(dev, seed, offset):
  """C1: bx_uniform(0, 1) is the reference's 24-bit value, bit for bit (the
  run from 2^32 - 3 crosses 2^32)."""
  n = 4096
  got = _uniform(dev, n, seed, offset, 0.0, 1.0)
  ref = uniform01_ref(seed, counters(offset, n)).astype(np.float32)
  assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (
      seed, offset, int((got != ref).sum()), got[:4], ref[:4])


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('seed', SEEDS)
def test_uniform_range(dev, seed, offset):
  """C2: [lo, hi) = [-1, 1) within two float32 roundings of float64."""
  n = 4096
  got = _uniform(dev, n, seed, offset, -1.0, 1.0)
  ref = -1.0 + 2.0 * uniform01_ref(seed, counters(offset, n))
  err = float(np.abs(got.astype(np.float64) - ref).max())
  print(f'seed {seed} offset {offset}: |bx_uniform(-1, 1) - float64| max {err:.3e}')
  assert err <= 2.0**-23
  assert (got >= -1.0).all() and (got < 1.0).all()


@pytest.mark.parametrize('seed,offset', [(0, 0), (2**63 + 5, 2**32 - 3), (1, 2**40 + 1)])
def test_uniform_slabs_stride(dev, seed, offset):
  """C3: slab s at offset + s * stride + j with stride != slab_n (and past
  2^32)."""
  slab_n, n_slabs, stride = 100, 3, 2**32 + 1000
  got = _uniform_slabs(dev, slab_n, n_slabs, seed, offset, stride, -1.0, 1.0)
  ref = -1.0 + 2.0 * uniform01_ref(seed, _slab_counters(offset, slab_n, n_slabs, stride, 1))
  err = float(np.abs(got.astype(np.float64) - ref).max())
  print(f'seed {seed} offset {offset}: slabs err {err:.3e}')
  assert err <= 2.0**-23
  assert (got < 1.0).all()
  # and the unit range bit for bit
  got01 = _uniform_slabs(dev, slab_n, n_slabs, seed, offset, stride, 0.0, 1.0)
  ref01 = uniform01_ref(seed, _slab_counters(offset, slab_n, n_slabs, stride, 1)).astype(np.float32)
  assert np.array_equal(got01.view(np.uint32), ref01.view(np.uint32))


@pytest.mark.parametrize('seed,offset', PAIRS)
def test_normal_slabs_per_sample(dev, seed, offset):
  """C4: one slab of 2^16 normals at counters offset + 2 j."""
  n = 1 << 16
  got = _normal_slabs(dev, n, 1, seed, offset, 0)
  _normal_gate(got, seed, _slab_counters(offset, n, 1, 0, 2), f'normal {seed}/{offset}')


def test_normal_slabs_stride_and_epoch(dev):
  """C4: three slabs 2^32 + 2 slab_n apart, and the device-side epoch term
  (an int64 holding 5, epoch_stride 2^33) through the C entry."""
  n = 1 << 16
  seed, offset = PAIRS[3]
  stride = 2**32 + 2 * n
  got = _normal_slabs(dev, n, 3, seed, offset, stride)
  _normal_gate(got, seed, _slab_counters(offset, n, 3, stride, 2), 'normal 3 slabs')
  epoch = torch.tensor([5], dtype=torch.int64, device=dev)
  for sd, off in (PAIRS[0], PAIRS[3]):
    got = _normal_slabs(dev, n, 1, sd, off, 0, epoch, 2**33)
    _normal_gate(got, sd, _slab_counters(off + 5 * 2**33, n, 1, 0, 2), f'normal epoch {sd}/{off}')
    plain = _normal_slabs(dev, n, 1, sd, off + 5 * 2**33, 0)
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_fused_noise_at_64_bit_counters(dev):
  """C5: one Ant launch whose seed, offset and step stride need all 64 bits:
  the teacher-forced policy check with the noise of `normal_ref`, and with
  `normal_slabs`' at the same arguments."""
  from brax_amd.envs.policy import policy_rollout
  from tests.test_gpu_policy_rollout import _check_physics, _check_policy, _eps, _make, _policy
  B, K = 20, 3
  env, st0 = _make(dev, 'ant', B, 1000, 1)
  A = env.action_size
  policy = _policy(env, dev)
  seed, offset, stride = 2**63 + 11, 2**33 + 7, 2**32 + 2 * B * A
  _, tr, ex = policy_rollout(env, st0, policy, K, seed=seed, offset=offset, step_stride=stride,
                             fused=True)
  torch.cuda.synchronize()
  idx = _slab_counters(offset, B * A, K, stride, 2)
  ref64 = normal_ref(seed, idx).reshape(K, B, A)
  eps_ref = torch.from_numpy(ref64.astype(np.float32))
  _check_policy(policy, st0, tr, ex, eps_ref, 'ant/64-bit counters, normal_ref')
  eps_dev = _eps(dev, K, B, A, seed, offset, stride)
  _check_policy(policy, st0, tr, ex, eps_dev, 'ant/64-bit counters, normal_slabs')
  _normal_gate(eps_dev.cpu().numpy().reshape(K, B * A), seed, idx, 'normal_slabs at the launch')
  _check_physics(env, st0, tr, ex)
