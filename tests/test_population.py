"""Population evaluation without a GPU: the moments identity against the
reference's weighted `running_statistics.update`, `PolicyPopulation`'s rows,
the identity head, the chained path on the torch-only `fast` env and the ABI
mirror."""

import numpy as np
import pytest
import torch

from brax_amd import _native
from brax_amd import abi
from brax_amd.envs import population as pop_mod
from brax_amd.envs.policy import MLPPolicy
from brax_amd.envs.population import (PolicyPopulation, population_rollout,
                                      update_running_statistics)


def _reference_update(mean, sv, count, batch, weights, std_min=1e-6, std_max=1e6):
  """acme/running_statistics.py:132-190, restated in float64."""
  count = count + weights.sum()
  d_old = (batch - mean) * weights[..., None]
  mean = mean + d_old.sum(axis=(0, 1)) / count
  sv = sv + (d_old * (batch - mean)).sum(axis=(0, 1))
  std = np.clip(np.sqrt(np.maximum(sv, 0) / count), std_min, std_max)
  return mean, sv, count, std


@pytest.mark.parametrize('seed', [0, 1])
def test_moments_identity_equals_the_reference_update(seed):
  rng = np.random.default_rng(seed)
  K, B, O = 9, 5, 7
  obs = rng.normal(size=(K, B, O)) * rng.uniform(0.1, 30, O) + rng.normal(size=O) * 5
  w = (rng.uniform(size=(K, B)) < 0.6).astype(np.float64)
  w[:, 2] = 0.  # one env never active
  mean = rng.normal(size=O)
  sv = rng.uniform(0.5, 4, O) * 11
  count = 11.0
  d = obs - mean
  s1 = (w[..., None] * d).sum(0)  # (B, O), as the kernel keeps them per env
  s2 = (w[..., None] * d * d).sum(0)
  got = update_running_statistics(mean, sv, count, (s1, s2, w.sum(0)))
  want = _reference_update(mean, sv, count, obs, w)
  for g, r, name in zip(got, want, ('mean', 'summed_variance', 'count', 'std')):
    np.testing.assert_allclose(g, r, rtol=1e-12, atol=0, err_msg=name)
  # a second batch on the updated state, a custom clip
  got2 = update_running_statistics(got[0], got[1], got[2],
                                   ((w[..., None] * (obs - got[0])).sum(0),
                                    (w[..., None] * (obs - got[0]) ** 2).sum(0), w.sum(0)),
                                   std_min=2.0, std_max=3.0)
  want2 = _reference_update(want[0], want[1], want[2], obs, w, 2.0, 3.0)
  for g, r in zip(got2, want2):
    np.testing.assert_allclose(g, r, rtol=1e-12, atol=0)
  assert got2[3].min() >= 2.0 and got2[3].max() <= 3.0


def _net(obs=5, hidden=(4,), act=2, head='normal_tanh', seed=0, **kw):
  g = torch.Generator().manual_seed(seed)
  widths = [obs, *hidden, act if head == 'identity' else 2 * act]
  layers = [(torch.randn((i, o), generator=g) * 0.3, torch.randn((o,), generator=g) * 0.1)
            for i, o in zip(widths[:-1], widths[1:])]
  return MLPPolicy(layers, activation='relu', head=head, **kw)


def _fake_normal_slabs(out, slab_n, n_slabs, seed, offset, slab_stride):
  """A stand-in for the device noise: a pure function of (seed, offset, j)."""
  assert n_slabs == 1 and out.numel() == slab_n
  j = torch.arange(slab_n, dtype=torch.float64)
  out.copy_(torch.sin(j * 12.9898 + seed * 78.233 + offset * 0.37).mul(43758.5453).frac().mul(3).view(out.shape))
  return out


def test_perturb_and_noise_agree(monkeypatch):
  monkeypatch.setattr(pop_mod, 'normal_slabs', _fake_normal_slabs)
  policy = _net()
  theta = policy.params.clone()
  P = 3
  pp = PolicyPopulation(policy, 2 * P)
  assert tuple(pp.rows.shape) == (2 * P, pp.stride) and pp.stride % 4 == 0 and pp.stride >= pp.n_params
  assert torch.equal(pp.rows[:, :pp.n_params], theta.expand(2 * P, -1))  # starts at theta
  sigma = 0.1
  pp.perturb_(sigma, seed=5, offset=8)
  eps = pp.noise(5, 8)
  assert tuple(eps.shape) == (P, pp.n_params) and eps.dtype == torch.float32
  assert eps.abs().max() > 0
  plus = (theta.double() + sigma * eps.double()).float()
  minus = (theta.double() - sigma * eps.double()).float()
  assert torch.equal(pp.rows[:P, :pp.n_params], plus)
  assert torch.equal(pp.rows[P:, :pp.n_params], minus)
  assert not torch.equal(pp.noise(5, 9), eps) and not torch.equal(pp.noise(6, 8), eps)
  assert torch.equal(policy.params, theta)  # theta itself is not touched
  # not antithetic: every row its own direction
  pp.perturb_(sigma, seed=5, offset=8, antithetic=False)
  eps_all = pp.noise(5, 8, antithetic=False)
  assert tuple(eps_all.shape) == (2 * P, pp.n_params)
  assert torch.equal(pp.rows[:, :pp.n_params], (theta.double() + sigma * eps_all.double()).float())
  with pytest.raises(ValueError):
    PolicyPopulation(policy, 3).perturb_(sigma, seed=1)  # antithetic needs an even n


def test_set_member_and_shape_checks():
  policy = _net(obs=5, hidden=(3,), act=2)
  n = 4
  pp = PolicyPopulation(policy, n)
  rows = torch.randn((n, pp.n_params), generator=torch.Generator().manual_seed(1))
  assert pp.set_(rows) is pp
  assert torch.equal(pp.rows[:, :pp.n_params], rows)
  assert torch.equal(pp.rows[:, pp.n_params:], torch.zeros((n, pp.stride - pp.n_params)))
  m = pp.member(2)
  assert isinstance(m, MLPPolicy) and m.sizes == policy.sizes and m.head == policy.head
  assert m.params.data_ptr() == pp.rows[2].data_ptr() and m.params.data_ptr() % 16 == 0
  obs = torch.randn((6, 5), generator=torch.Generator().manual_seed(2))
  want = MLPPolicy([(w.clone(), b.clone()) for w, b in m.layers()], activation='relu').forward(obs)[0]
  assert torch.equal(m.forward(obs)[0], want)
  pp.rows[2] += 1  # a view: the member sees the buffer
  assert not torch.equal(m.forward(obs)[0], want)
  with pytest.raises(ValueError):
    pp.set_(rows[:, :-1])
  with pytest.raises(ValueError):
    pp.set_(rows[:-1])
  with pytest.raises(IndexError):
    pp.member(n)
  with pytest.raises(ValueError):
    PolicyPopulation(policy, 0)
  # the batched forward reads row e for env e
  from brax_amd.envs.population import forward_rows
  obs4 = obs[:n]
  got = forward_rows(policy, pp.rows, obs4)
  for e in range(n):
    torch.testing.assert_close(got[e], pp.member(e).forward(obs4[e:e + 1])[0][0], rtol=1e-6, atol=1e-6)


def test_identity_head_is_a_plain_affine_map():
  g = torch.Generator().manual_seed(4)
  W, b = torch.randn((7, 3), generator=g), torch.randn((3,), generator=g)
  p = MLPPolicy([(W, b)], head='identity')
  assert p.action_size == 3 and p.head == 'identity'
  obs = torch.randn((5, 7), generator=g)
  action, raw, logp, logits = p.forward(obs, eps=torch.ones((5, 3)))
  want = obs @ W + b
  assert torch.equal(action, want) and torch.equal(raw, want) and torch.equal(logits, want)
  assert torch.equal(logp, torch.zeros(5))
  p.for_actions(3)
  with pytest.raises(ValueError):
    p.for_actions(2)
  assert p.descriptor(3).width[0] == 3
  with pytest.raises(ValueError):
    MLPPolicy([(W, b)], head='softmax')
  # the default head is untouched
  q = MLPPolicy([(W, b)], deterministic=True).for_actions(3)
  assert q.head == 'normal_tanh' and torch.equal(q.forward(obs)[0], torch.tanh(want))
  # with a normaliser
  mean, std = torch.randn(7, generator=g), torch.rand(7, generator=g) + 0.5
  pn = MLPPolicy([(W, b)], head='identity', obs_mean=mean, obs_std=std)
  assert torch.equal(pn.forward(obs)[0], ((obs - mean) / std) @ W + b)


def _fast_env(B, ep):
  from brax_amd.envs import wrappers
  from brax_amd.envs.fast import Fast
  return wrappers.AutoResetWrapper(wrappers.EpisodeWrapper(Fast(batch_size=B, device='cpu'), ep, 1))


def test_population_rollout_on_fast_equals_a_hand_written_loop():
  B, ep, K, shift = 4, 3, 5, 0.125
  env = _fast_env(B, ep)
  mean, std = torch.tensor([0.01, -0.02]), torch.tensor([0.5, 2.0])
  policy = MLPPolicy([([[0.0], [0.0]], [0.0])], head='identity', obs_mean=mean, obs_std=std)
  pp = PolicyPopulation(policy, B)
  # members 0 and 2 push (positive action), 1 and 3 do not
  rows = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 3.0, 0.5], [0.0, 0.0, 0.0]])
  pp.set_(rows)
  st0 = env.reset(np.array([0, 3], np.uint32))
  with pytest.raises(NotImplementedError):
    population_rollout(env, st0, pp, k=K, fused=True)
  final, res = population_rollout(env, st0, pp, k=K, reward_shift=shift)
  assert res.staged is None and res.metric_keys == () and res.metric_sums == {}
  # by hand, in the kernel's order
  st = st0
  score = torch.zeros(B)
  active = torch.ones(B)
  esteps = torch.zeros(B)
  s1, s2, cnt = torch.zeros((B, 2)), torch.zeros((B, 2)), torch.zeros(B)
  for _ in range(K):
    d = st.obs - mean
    s1 += active[:, None] * d
    s2 += active[:, None] * (d * d)
    cnt += active
    x = (st.obs - mean) / std
    a = torch.stack([x[e] @ rows[e, :2] + rows[e, 2] for e in range(B)])[:, None]
    st = env.step(st, a)
    esteps = torch.where(active != 0, st.info['steps'], esteps)
    score += (st.reward - shift) * active
    active = active * (1 - st.done)
  assert torch.equal(res.scores, score) and torch.equal(res.active, active)
  assert torch.equal(res.episode_steps, esteps)
  assert torch.equal(res.obs_s1, s1) and torch.equal(res.obs_s2, s2) and torch.equal(res.obs_count, cnt)
  assert torch.equal(final.obs, st.obs) and torch.equal(final.done, st.done)
  assert active.tolist() == [0.0] * B and cnt.tolist() == [float(ep)] * B  # the episode ended inside the run
  assert score[0] > score[1] and score[1] == -shift * ep  # the pushers moved, the others paid the shift
  # k = None: the EpisodeWrapper's length; continuation through carry
  _, res_ep = population_rollout(env, st0, pp, reward_shift=shift)
  mid, r1 = population_rollout(env, st0, pp, k=2, reward_shift=shift)
  _, r2 = population_rollout(env, mid, pp, k=1, reward_shift=shift, carry=r1)
  for a_, b_ in ((res_ep.scores, r2.scores), (res_ep.obs_s1, r2.obs_s1), (res_ep.obs_s2, r2.obs_s2),
                 (res_ep.obs_count, r2.obs_count), (res_ep.active, r2.active)):
    assert torch.equal(a_, b_)
  # no moments; a shared policy (every env one row)
  _, r0 = population_rollout(env, st0, pp, k=K, moments=False)
  assert r0.obs_s1 is None and r0.obs_count is None and r0.mom_buf is None
  _, rs = population_rollout(env, st0, pp.member(0), k=K, reward_shift=shift)
  assert torch.equal(rs.scores, score[0].expand(B))
  with pytest.raises(ValueError):
    population_rollout(env, st0, PolicyPopulation(policy, B + 1), k=K)
  with pytest.raises(ValueError):
    population_rollout(env, st0, pp, k=0)


def test_policy_rollout_chains_an_identity_head():
  from brax_amd.envs import policy_rollout
  env = _fast_env(2, 3)
  policy = MLPPolicy([([[0.0], [0.0]], [1.0])], head='identity')
  st0 = env.reset(np.array([0, 3], np.uint32))
  with pytest.raises(NotImplementedError):
    policy_rollout(env, st0, policy, 2, fused=True)
  final, traj, ex = policy_rollout(env, st0, policy, 2)
  assert torch.equal(ex.action, torch.ones((2, 2, 1))) and torch.equal(ex.raw_action, ex.action)
  assert torch.equal(ex.log_prob, torch.zeros((2, 2)))


def test_header_abi_and_exports():
  # (the names, types and bx_population against the header: tests/test_abi.py)
  names = [n for n, _ in abi.ARGS['bx_env_eval_population']]
  # bx_env_eval_policy's arguments, the population struct before the stream
  pol = [n for n, _ in abi.ARGS['bx_env_eval_policy']]
  assert names == pol[:-1] + ['pop', 'stream']
  assert abi.ARGS['bx_env_eval_population'][-2][1]._type_ is abi.BxPopulation
  assert abi.ABI_VERSION == 14
  lib = _native.lib()
  assert lib.bx_abi_version() == 14
  # a null system fails with a message, no GPU touched
  rc = lib.bx_env_eval_population(None, None, 0, 0, None, None, None, None, None, None, 0, 0, 0, None,
                                  None, None, None, None, None)
  assert rc != 0 and b'null' in lib.bx_last_error()
