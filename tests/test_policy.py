"""`brax_amd.envs.policy.MLPPolicy` on the CPU: parameter packing, the flax
dict walk, `forward` in float64 against hand-computed values of the head's
formulas (networks.MLP, NormalTanhDistribution, TanhBijector), and the ABI /
header declarations of the fused rollout."""
import math

import numpy as np
import pytest
import torch

from brax_amd import abi
from brax_amd.envs.policy import MLPPolicy


def _layers(sizes, seed=0):
  g = torch.Generator().manual_seed(seed)
  return [(torch.rand((i, o), generator=g) - 0.5, torch.rand((o,), generator=g) - 0.5)
          for i, o in zip(sizes[:-1], sizes[1:])]


def test_packing_round_trip():
  ls = _layers([5, 7, 3, 4])
  p = MLPPolicy(ls)
  assert p.params.numel() == 6 * 7 + 8 * 3 + 4 * 4 and p.params.dtype == torch.float32
  assert p.obs_size == 5 and p.sizes == [(5, 7), (7, 3), (3, 4)]
  # layer after layer: the kernel row-major, then the bias
  assert torch.equal(p.params[:35], ls[0][0].reshape(-1)) and torch.equal(p.params[35:42], ls[0][1])
  for (w, b), (w2, b2) in zip(ls, p.layers()):
    assert torch.equal(w, w2) and torch.equal(b, b2)
  # load_ writes in place: the same storage, the new values
  ptr = p.params.data_ptr()
  new = _layers([5, 7, 3, 4], seed=1)
  p.load_(new)
  assert p.params.data_ptr() == ptr
  assert torch.equal(p.layers()[2][0], new[2][0])
  with pytest.raises(ValueError):
    p.load_(_layers([5, 6, 3, 4]))
  with pytest.raises(ValueError):
    MLPPolicy([(torch.zeros(3, 4), torch.zeros(4)), (torch.zeros(5, 2), torch.zeros(2))])
  with pytest.raises(ValueError):
    MLPPolicy(ls, activation='gelu')
  with pytest.raises(ValueError):
    MLPPolicy(ls, obs_mean=torch.zeros(5))


def test_from_flax_params():
  ls = _layers([3, 4, 2])
  tree = {'params': {'hidden_1': {'kernel': ls[1][0].numpy(), 'bias': ls[1][1].numpy()},
                     'hidden_0': {'kernel': ls[0][0].tolist(), 'bias': ls[0][1].tolist()}}}
  p = MLPPolicy.from_flax_params(tree, activation='tanh')
  assert p.activation == 'tanh' and p.sizes == [(3, 4), (4, 2)]
  assert torch.equal(p.layers()[0][0], ls[0][0]) and torch.equal(p.layers()[1][1], ls[1][1])
  assert MLPPolicy.from_flax_params(tree['params']).sizes == p.sizes  # bare inner dict
  bad = {'params': {'hidden_0': {'kernel': np.zeros((3, 4)), 'bias': np.zeros(5)}}}
  with pytest.raises(ValueError):
    MLPPolicy.from_flax_params(bad)
  with pytest.raises(ValueError):  # the second layer's input is not the first's output
    MLPPolicy.from_flax_params({'params': {
        'hidden_0': {'kernel': np.zeros((3, 4)), 'bias': np.zeros(4)},
        'hidden_1': {'kernel': np.zeros((5, 2)), 'bias': np.zeros(2)}}})
  with pytest.raises(ValueError):
    MLPPolicy.from_flax_params({'params': {'hidden_0': {'kernel': np.zeros((3, 4))}}})
  with pytest.raises(ValueError):
    MLPPolicy.from_flax_params({'params': {'hidden_1': {'kernel': np.zeros((3, 4)),
                                                        'bias': np.zeros(4)}}})


def test_forward_float64_hand_values():
  # obs (2) -> hidden (2, swish) -> logits (2): one action, loc | scale parameter
  w0 = [[1.0, -2.0], [0.5, 0.25]]
  b0 = [0.0, 1.0]
  w1 = [[2.0, -1.0], [1.0, 3.0]]
  b1 = [-0.5, 0.25]
  p = MLPPolicy([(w0, b0), (w1, b1)], obs_mean=[1.0, 2.0], obs_std=[2.0, 4.0], min_std=1e-3)
  obs = torch.tensor([[3.0, -2.0]], dtype=torch.float64)
  eps = torch.tensor([[0.5]], dtype=torch.float64)
  action, raw, logp, logits = p.forward(obs, eps)
  assert action.dtype == torch.float64
  x = [(3.0 - 1.0) / 2.0, (-2.0 - 2.0) / 4.0]  # (1, -1)
  pre = [x[0] * 1.0 + x[1] * 0.5 + 0.0, x[0] * -2.0 + x[1] * 0.25 + 1.0]  # (0.5, -1.25)
  h = [v / (1.0 + math.exp(-v)) for v in pre]
  lg = [h[0] * 2.0 + h[1] * 1.0 - 0.5, h[0] * -1.0 + h[1] * 3.0 + 0.25]
  scale = math.log1p(math.exp(lg[1])) + 1e-3
  r = lg[0] + scale * 0.5
  lp = (-0.5 * 0.25 - 0.5 * math.log(2 * math.pi) - math.log(scale)
        - 2.0 * (math.log(2.0) - r - math.log1p(math.exp(-2.0 * r))))
  assert logits[0].tolist() == pytest.approx(lg, rel=1e-14)
  assert float(raw) == pytest.approx(r, rel=1e-14)
  assert float(action) == pytest.approx(math.tanh(r), rel=1e-14)
  assert float(logp) == pytest.approx(lp, rel=1e-13)
  # deterministic: raw = loc, whatever eps
  pd = MLPPolicy([(w0, b0), (w1, b1)], obs_mean=[1.0, 2.0], obs_std=[2.0, 4.0], deterministic=True)
  a2, r2, _, _ = pd.forward(obs, eps)
  assert float(r2) == pytest.approx(lg[0], rel=1e-14) and float(a2) == pytest.approx(math.tanh(lg[0]), rel=1e-14)


def _linear(loc, s, **kw):
  """A one-layer net whose logits are (loc, s) for the observation (1,)."""
  return MLPPolicy([([[loc, s]], [0.0, 0.0])], **kw)


def test_forward_scale_floor_and_tanh_log_det():
  one = torch.ones((1, 1), dtype=torch.float64)
  # softplus(-800) underflows to 0: the scale is min_std exactly
  p = _linear(0.25, -800.0, min_std=1e-3)
  _, raw, logp, _ = p.forward(one, torch.full((1, 1), 2.0, dtype=torch.float64))
  assert float(raw) == pytest.approx(0.25 + 1e-3 * 2.0, rel=1e-15)
  # raw = 0, eps = 0, scale = softplus(0) = ln 2 (min_std 0): the log-det is
  # 2 (ln 2 - 0 - softplus(0)) = 0, so log_prob = -ln sqrt(2 pi) - ln ln 2
  p = _linear(0.0, 0.0, min_std=0.0)
  a, raw, logp, _ = p.forward(one, torch.zeros((1, 1), dtype=torch.float64))
  assert float(raw) == 0.0 and float(a) == 0.0
  assert float(logp) == pytest.approx(-0.5 * math.log(2 * math.pi) - math.log(math.log(2.0)), rel=1e-14)
  # large |raw|: log(1 - tanh^2) -> 2 ln 2 - 2 |raw| (no overflow, no log(0))
  for r in (40.0, -40.0):
    p = _linear(r, 0.0, min_std=0.0)
    a, raw, logp, _ = p.forward(one, torch.zeros((1, 1), dtype=torch.float64))
    assert float(a) == math.copysign(1.0, r)
    want = -0.5 * math.log(2 * math.pi) - math.log(math.log(2.0)) - (2 * math.log(2.0) - 2 * abs(r))
    assert float(logp) == pytest.approx(want, rel=1e-13)
  # relu and tanh hidden layers
  for name, fn in (('relu', lambda v: max(v, 0.0)), ('tanh', math.tanh)):
    p = MLPPolicy([([[1.0, -1.0]], [0.5, 0.25]), ([[1.0, 0.0], [2.0, 0.0]], [0.0, 0.0])],
                  activation=name)
    _, _, _, lg = p.forward(one)
    assert float(lg[0, 0]) == pytest.approx(fn(1.5) + 2.0 * fn(-0.75), rel=1e-14)


def test_chained_rollout_on_the_torch_only_env():
  """Fast has no kernel form and a qp without a body axis: the chained path
  under Episode + AutoReset keeps every step's shapes (the AutoReset select
  masks each field at its own rank), and a finished episode restarts from the
  first state, each env for itself."""
  from brax_amd.envs import wrappers
  from brax_amd.envs.fast import Fast
  from brax_amd.envs.policy import fused_supported, policy_rollout
  B, K = 3, 5
  env = wrappers.AutoResetWrapper(wrappers.EpisodeWrapper(Fast(batch_size=B, device='cpu'), 2, 1))
  st0 = env.reset(np.array([1, 2], np.uint32))
  assert tuple(st0.obs.shape) == (B, 2)
  p = MLPPolicy([([[0.0, 0.0], [0.0, 0.0]], [1.0, 0.0])], deterministic=True)  # action tanh(1) > 0
  assert fused_supported(env, p)
  with pytest.raises(NotImplementedError):
    policy_rollout(env, st0, p, K, fused=True)
  final, tr, ex = policy_rollout(env, st0, p, K)
  assert tuple(tr.obs.shape) == (K, B, 2) and tuple(tr.qp.shape) == (K, B, 16)
  assert tuple(ex.action.shape) == (K, B, 1) and tuple(ex.log_prob.shape) == (K, B)
  assert tr.done.tolist() == [[0.0] * B, [1.0] * B, [0.0] * B, [1.0] * B, [0.0] * B]
  # vel += dt, pos += vel dt (dt 0.02) from the restored zero state
  dt = 0.02
  one, two = [dt * dt, dt], [0.0, 0.0]
  want = torch.tensor([[one] * B, [two] * B, [one] * B, [two] * B, [one] * B], dtype=torch.float32)
  assert torch.allclose(tr.obs, want, rtol=1e-6, atol=0.0)
  assert torch.equal(final.obs, tr.obs[-1])


def test_abi_version_and_header():
  # (the entry points, bx_policy and BX_POLICY_MAX_* against the header: tests/test_abi.py)
  assert abi.ABI_VERSION == 14
