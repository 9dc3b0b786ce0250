"""`brax_amd.training.es` / `ars` without a GPU: the ABI mirror and the
refusals of `bx_population_perturb` / `bx_population_delta`, the workspace-size
query, and the optimiser halves (fitness shaping, ARS's ranks, weights and std,
both evaluation schedules) against arrays worked out by hand from the
reference's formulas (`training/agents/es/train.py:53-65, 238-246`,
`ars/train.py:87-88, 176-191`). Everything is float64, so rtol 1e-12: a few
float64 roundings."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from brax_amd import _native, abi
from brax_amd.training import ars, es
from tests.helpers import Header

RTOL = 1e-12

# length 6 (three directions) and 7, both with ties
X6 = [3., 1., 3., -2., 1., 5.]
X7 = [.5, -1., 2., 2., .5, 7., -3.]
# argsort(argsort(x)), stable: a tie ranks the lower index first
RANK6 = [3, 1, 4, 0, 2, 5]
RANK7 = [2, 1, 4, 5, 3, 6, 0]


def _close(got, want, atol=0.):
  assert got.dtype == torch.float64
  np.testing.assert_allclose(got.numpy(), np.asarray(want, np.float64), rtol=RTOL, atol=atol)


# ---- ABI ------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['bx_population_perturb', 'bx_population_delta'])
def test_header_abi_and_exports(name):
  # (names, types and BX_POPULATION_DELTA_CHUNK against the header: tests/test_abi.py)
  assert not any('bx_system' in ctype for ctype, _, _ in Header().functions[name][1])
  # additive: no ABI bump
  assert abi.ABI_VERSION == 14
  assert hasattr(_native.lib(), name)


def test_perturb_refusals():
  """Every refusal comes before any device call: host and null pointers."""
  lib = _native.lib()
  buf = (C.c_float * 64)()
  rows, theta = C.addressof(buf), C.addressof(buf) + 48 * 4
  call = lambda r, t, P, n, stride, anti=1: lib.bx_population_perturb(  # noqa: E731
      r, t, P, n, stride, 0.1, 0, 0, anti, None, None)
  for args, word in (((None, theta, 2, 5, 8), b'null'), ((rows, None, 2, 5, 8), b'null'),
                     ((rows, theta, 0, 5, 8), b'n_directions'),
                     ((rows, theta, -1, 5, 8), b'n_directions'),
                     ((rows, theta, 2, 0, 8), b'n_params'), ((rows, theta, 2, 5, 4), b'stride'),
                     # rows: 4 members x 8 floats; theta inside them, at their
                     # first word, and ending on their first word
                     ((rows, rows + 16 * 4, 2, 5, 8), b'overlap'),
                     ((rows, rows, 2, 5, 8), b'overlap'),
                     ((rows + 4 * 4, rows, 2, 5, 8), b'overlap'),
                     # the non-antithetic rows are half as long: theta at word
                     # 13 is past them, at word 12 (the last row's last) it is not
                     ((rows, rows + 12 * 4, 2, 5, 8, 0), b'overlap')):
    assert call(*args) != 0 and word in lib.bx_last_error(), (args[2:], lib.bx_last_error())


def test_delta_refusals_and_workspace_query():
  lib = _native.lib()
  buf = (C.c_float * 64)()
  ws = (C.c_double * 64)()
  out, w = C.addressof(buf), C.addressof(buf) + 32 * 4
  size = C.c_int64(0)
  call = lambda o, wt, P, n, wsp, sz: lib.bx_population_delta(  # noqa: E731
      o, wt, P, n, 0, 0, None, wsp, sz, None)
  chunk = abi.POPULATION_DELTA_CHUNK
  # the size query: a null workspace launches nothing, whatever the pointers
  for P, n, chunks in ((1, 1, 1), (chunk, 18, 1), (chunk + 1, 18, 2), (2 * chunk + 2, 323, 3),
                       (4096, 6000, 4096 // chunk)):
    size.value = -1
    assert call(None, None, P, n, None, C.byref(size)) == 0, lib.bx_last_error()
    assert size.value == 8 * n * chunks
  size.value = 8 * 64
  for args, word in (((out, w, 3, 5, C.addressof(ws), None), b'null'),
                     ((None, w, 3, 5, C.addressof(ws), C.byref(size)), b'null'),
                     ((out, None, 3, 5, C.addressof(ws), C.byref(size)), b'null'),
                     ((out, w, 0, 5, C.addressof(ws), C.byref(size)), b'n_directions'),
                     ((out, w, 3, 0, C.addressof(ws), C.byref(size)), b'n_params'),
                     ((out, w, 3, 0, None, C.byref(size)), b'n_params'),
                     ((out, w, 3, 5, C.addressof(ws) + 4, C.byref(size)), b'aligned')):
    assert call(*args) != 0 and word in lib.bx_last_error(), (args[2:4], lib.bx_last_error())
  size.value = 8 * 5 - 1  # one byte short of one chunk x 5 parameters
  assert call(out, w, 3, 5, C.addressof(ws), C.byref(size)) != 0
  assert b'workspace' in lib.bx_last_error() and b'40' in lib.bx_last_error()


# ---- ES: fitness shaping --------------------------------------------------------------------

def test_ranks_break_ties_by_index():
  assert es._ranks(torch.tensor(X6)).tolist() == RANK6  # pylint: disable=protected-access
  assert es._ranks(torch.tensor(X7)).tolist() == RANK7  # pylint: disable=protected-access


def test_centered_rank():
  _close(es.centered_rank(torch.tensor(X6, dtype=torch.float64)),
         [3 / 5 - .5, 1 / 5 - .5, 4 / 5 - .5, -.5, 2 / 5 - .5, .5])
  _close(es.centered_rank(torch.tensor(X7, dtype=torch.float64)),
         [2 / 6 - .5, 1 / 6 - .5, 4 / 6 - .5, 5 / 6 - .5, 3 / 6 - .5, .5, -.5])
  # float32 scores are shaped in float64
  assert es.FitnessShaping.CENTERED_RANK(torch.tensor(X6)).dtype == torch.float64


def test_wierstra():
  # len - rank = [3, 5, 2, 6, 4, 1]; u = max(0, log(6 / 2 + 1) - log(.))
  u6 = [math.log(4 / 3), 0., math.log(2.), 0., 0., math.log(4.)]
  s6 = math.log(4 / 3) + math.log(2.) + math.log(4.)
  _close(es.wierstra(torch.tensor(X6, dtype=torch.float64)), [u / s6 - 1 / 6 for u in u6])
  # len - rank = [5, 6, 3, 2, 4, 1, 7]; log(7 / 2 + 1) = log 4.5
  u7 = [0., 0., math.log(1.5), math.log(2.25), math.log(1.125), math.log(4.5), 0.]
  s7 = sum(u7)
  # 1.5 * 2.25 * 1.125 * 4.5 = 1.5^7, so the third entry is 1 / 7 - 1 / 7: a
  # difference that cancels is held to the same rtol of its operands, 1 / 7
  _close(es.wierstra(torch.tensor(X7, dtype=torch.float64)), [u / s7 - 1 / 7 for u in u7],
         atol=RTOL / 7)


def test_es_weights():
  x = torch.tensor(X6)  # float32, as the kernel's scores
  _close(es.es_weights(x), [3. - -2., 1. - 1., 3. - 5.])
  _close(es.es_weights(x, es.FitnessShaping.CENTERED_RANK), [.1 + .5, -.3 + .1, .3 - .5])
  u = [math.log(4 / 3), 0., math.log(2.), 0., 0., math.log(4.)]
  _close(es.es_weights(x, es.FitnessShaping.WIERSTRA),
         [(u[i] - u[i + 3]) / sum(u) for i in range(3)])
  # center_fitness: mean 11 / 6, population variance 49 / 6 - 121 / 36 = 173 / 36
  d = 1e-6 + math.sqrt(173.) / 6
  _close(es.es_weights(x, es.FitnessShaping.ORIGINAL, center_fitness=True),
         [((3 - 11 / 6) - (-2 - 11 / 6)) / d, ((1 - 11 / 6) - (1 - 11 / 6)) / d,
          ((3 - 11 / 6) - (5 - 11 / 6)) / d])
  # centred ranks: mean 0, variance (2 / 6) (.01 + .09 + .25) = 7 / 60
  d = 1e-6 + math.sqrt(7 / 60)
  _close(es.es_weights(x, es.FitnessShaping.CENTERED_RANK, center_fitness=True),
         [.6 / d, -.2 / d, -.2 / d])


# ---- ARS: ranks, weights, std ---------------------------------------------------------------

def test_ars_weights():
  # r+ = [3, 1, 3], r- = [-2, 1, 5]: max [3, 1, 5], ranks of -max [1, 2, 0]
  w, rw, std = ars.ars_weights(torch.tensor(X6), 2)
  _close(rw, [1., 0., 1.])
  _close(w, [5., 0., -2.])
  # selected scores 3, 3, -2, 5: mean 2.25, variance 26.75 / 4
  _close(std, math.sqrt(6.6875))
  # top_directions above the number of directions selects all of them
  w, rw, std = ars.ars_weights(torch.tensor(X6), 5)
  _close(rw, [1., 1., 1.])
  _close(w, [5., 0., -2.])
  _close(std, math.sqrt(173.) / 6)
  # seven directions, max [2, 3, 2, 2, 4, 4, 1]: ranks [3, 2, 4, 5, 0, 1, 6];
  # top 4 cuts the tie at 2 after the lowest index
  plus, minus = [2., 0., 2., -1., 4., 4., 1.], [1., 3., -5., 2., 0., 4., 1.]
  w, rw, std = ars.ars_weights(torch.tensor(plus + minus), 4)
  _close(rw, [1., 1., 0., 0., 1., 1., 0.])
  _close(w, [1., -3., 0., 0., 4., 0., 0.])
  # selected 2, 0, 4, 4, 1, 3, 0, 4: mean 2.25, squared deviations sum 21.5
  _close(std, math.sqrt(21.5 / 8))
  # one selected direction with equal scores: a zero std, passed on as it is
  w, rw, std = ars.ars_weights(torch.tensor([1., 0., 1., -1.]), 1)
  _close(rw, [1., 0.])
  assert std.item() == 0.0 and w.tolist() == [0., 0.]


# ---- the evaluation schedules ---------------------------------------------------------------

def test_es_eval_schedule():
  assert es.eval_schedule(1000, 1) == es.EvalSchedule(1, 1000, 1000)
  assert es.eval_schedule(1000, 2) == es.EvalSchedule(1, 1000, 1000)
  assert es.eval_schedule(1000, 4) == es.EvalSchedule(3, 333, 334)
  assert es.eval_schedule(100, 0) == es.EvalSchedule(1, 100, 100)


def test_ars_eval_schedule():
  assert ars.eval_schedule(100, 1) == ars.EvalSchedule(100, 100)
  assert ars.eval_schedule(1000, 3) == ars.EvalSchedule(333, 334)
  assert ars.eval_schedule(1000, 4) == ars.EvalSchedule(250, 250)


def test_train_signatures_follow_the_reference():
  import inspect
  d = {k: v.default for k, v in inspect.signature(es.train).parameters.items()}
  assert list(d)[:19] == [
      'environment', 'num_timesteps', 'episode_length', 'action_repeat', 'l2coeff',
      'max_devices_per_host', 'population_size', 'learning_rate', 'fitness_shaping',
      'num_eval_envs', 'perturbation_std', 'seed', 'normalize_observations', 'num_evals',
      'center_fitness', 'deterministic_eval', 'network_factory', 'progress_fn', 'eval_env']
  assert (d['num_timesteps'], d['episode_length'], d['l2coeff'], d['population_size'],
          d['learning_rate'], d['perturbation_std'], d['num_eval_envs']) == (100, 1000, 0, 128, 1e-3,
                                                                             .1, 128)
  assert d['fitness_shaping'] is es.FitnessShaping.ORIGINAL and 'device' in d
  d = {k: v.default for k, v in inspect.signature(ars.train).parameters.items()}
  assert list(d)[:16] == [
      'environment', 'num_timesteps', 'episode_length', 'action_repeat', 'max_devices_per_host',
      'number_of_directions', 'top_directions', 'step_size', 'num_eval_envs',
      'exploration_noise_std', 'seed', 'normalize_observations', 'num_evals', 'reward_shift',
      'network_factory', 'progress_fn']
  assert (d['number_of_directions'], d['top_directions'], d['step_size'],
          d['exploration_noise_std'], d['reward_shift']) == (60, 20, .015, .025, 0.)
  assert 'device' in d and 'eval_env' in d


# ---- PolicyPopulation off the device --------------------------------------------------------

def test_population_off_the_device_refuses_the_kernels():
  from brax_amd.envs.policy import MLPPolicy
  from brax_amd.envs.population import PolicyPopulation
  pol = MLPPolicy([(torch.zeros(5, 3), torch.zeros(3))], head='identity')
  pop = PolicyPopulation(pol, 6)
  with pytest.raises(NotImplementedError):
    pop.perturb_(.1, 0, fused=True)
  with pytest.raises(NotImplementedError):
    pop.weighted_noise_sum(torch.ones(3), 0, fused=True)
  with pytest.raises(ValueError):
    pop.weighted_noise_sum(torch.ones(4), 0, fused=False)
  with pytest.raises(ValueError):
    pop.perturb_(.1, 0, frozen=torch.zeros(17), fused=False)
