"""The two training loops of `brax_amd.training.driver` over a stub learner
and a stub evaluator: no GPU, no env."""
import itertools
import types

import pytest
import torch

from brax_amd.training import ars, driver, es


class _Policy:
  def __init__(self, name, log):
    self.name, self.log = name, log

  def load_(self, layers):
    self.log.append(('load', self.name, layers))


class _Evaluator:
  def __init__(self, log):
    self.log = log

  def run_evaluation(self, training_metrics=None):
    self.log.append('eval')
    return {'eval/runs': self.log.count('eval'), **training_metrics}


@pytest.fixture
def log(monkeypatch):
  out = []
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda dev=None: out.append('sync'))
  # a clock that advances one second per reading: every timed span is 1 s
  ticks = itertools.count()
  monkeypatch.setattr(driver, 'time', types.SimpleNamespace(time=lambda: float(next(ticks))))
  return out


# ---- the fixed schedule (PPO, SAC) --------------------------------------------------------------

STEPS_PER_EPOCH, ENV_STEPS = 2, 10


class _StepLearner:
  """`training_step` number i (from 1) reports the loss i and adds ENV_STEPS."""
  device = torch.device('cpu')

  def __init__(self, log):
    self.log, self.actor, self.env_steps, self.calls = log, _Policy('actor', log), 0, 0
    self.layers = [(torch.ones(2, 1, requires_grad=True), torch.zeros(1, requires_grad=True))]

  @property
  def params(self):
    return None, self.layers, 'value layers'

  def training_step(self):
    self.calls += 1
    self.env_steps += ENV_STEPS
    self.log.append('step')
    return {'loss': float(self.calls), 'size': self.calls}


def _run_epochs(log, num_evals, separate, prefill=True):
  learner = _StepLearner(log)
  eval_policy = _Policy('eval', log) if separate else learner.actor
  num_epochs = max(num_evals - 1, 1)
  calls = []
  metrics = driver.run_epochs(
      learner, eval_policy, _Evaluator(log), num_epochs, STEPS_PER_EPOCH,
      STEPS_PER_EPOCH * ENV_STEPS, num_epochs * STEPS_PER_EPOCH * ENV_STEPS, num_evals > 1,
      lambda n, m: calls.append((n, dict(m))),
      prefill=(lambda: log.append('prefill')) if prefill else None)
  assert metrics == calls[-1][1]
  return learner, num_epochs, calls


@pytest.mark.parametrize('num_evals', [1, 3])
def test_fixed_schedule(log, num_evals):
  learner, num_epochs, calls = _run_epochs(log, num_evals, separate=True)
  per_epoch = STEPS_PER_EPOCH * ENV_STEPS
  # the 0 entry only with an initial evaluation
  assert [n for n, _ in calls] == ([0] if num_evals > 1 else []) + [
      per_epoch * (e + 1) for e in range(num_epochs)]
  if num_evals > 1:
    assert calls[0][1] == {'eval/runs': 1}
  for e, (_, m) in enumerate(calls[-num_epochs:]):
    losses = [float(e * STEPS_PER_EPOCH + i + 1) for i in range(STEPS_PER_EPOCH)]
    assert m['training/loss'] == sum(losses) / STEPS_PER_EPOCH
    assert m['training/size'] == sum(losses) / STEPS_PER_EPOCH
    # (the prefill's second, then one per epoch)
    assert m['training/sps'] == per_epoch and m['training/walltime'] == e + 2
  # the prefill: once, after the initial evaluation, timed (a synchronise
  # follows it), before the first training step
  assert log.count('prefill') == 1
  at = log.index('prefill')
  assert log[:at] == (['eval'] if num_evals > 1 else []) and log[at + 1:at + 3] == ['sync', 'step']
  # then per epoch: the steps, one synchronise, the reload, the evaluation
  epoch = ['step'] * STEPS_PER_EPOCH + ['sync', 'load', 'eval']
  assert [x[0] if isinstance(x, tuple) else x for x in log[at + 2:]] == epoch * num_epochs
  loads = [x for x in log if isinstance(x, tuple)]
  assert all(name == 'eval' for _, name, _ in loads)
  for _, _, layers in loads:  # the learner's policy layers, detached
    assert len(layers) == 1 and not layers[0][0].requires_grad and not layers[0][1].requires_grad
    assert layers[0][0].data_ptr() == learner.layers[0][0].data_ptr()


def test_fixed_schedule_shared_actor_and_no_prefill(log):
  _, num_epochs, calls = _run_epochs(log, 3, separate=False, prefill=False)
  assert [n for n, _ in calls] == [0, 20, 40]
  # the shared actor is not reloaded; without a prefill nothing is timed
  # before the first step
  assert log == ['eval'] + (['step'] * STEPS_PER_EPOCH + ['sync', 'eval']) * num_epochs


def test_fixed_schedule_asserts_the_step_count(log):
  learner = _StepLearner(log)
  with pytest.raises(AssertionError):
    driver.run_epochs(learner, learner.actor, _Evaluator(log), 1, 1, ENV_STEPS, ENV_STEPS + 1,
                      False, lambda n, m: None)


# ---- the metric sums of the PPO and SAC updates -------------------------------------------------

def test_metric_sums_with_and_without_a_loss_vector():
  from brax_amd.training import sac_head
  names = sac_head.METRICS
  steps = [torch.tensor([1., 2., 3.]), torch.tensor([3., 4., 5.])]
  alphas = [torch.tensor(0.5), torch.tensor(1.5)]
  fused, chained = {}, {}
  for v, a in zip(steps, alphas):
    m = sac_head.Metrics(zip(names, v))
    m.vector = v
    m['alpha'] = a
    driver.add_metrics(fused, m)
    driver.add_metrics(chained, {**dict(zip(names, v.clone().requires_grad_())), 'alpha': a})
  # the vector is one entry (one addition per step), alpha another
  assert len(fused) == 2 and len(chained) == 4
  want = {'critic_loss': 2., 'actor_loss': 3., 'alpha_loss': 4., 'alpha': 1.}
  for sums in (fused, chained):
    got = driver.mean_metrics(sums, 2, names)
    assert list(got) == list(want)
    assert {k: float(v) for k, v in got.items()} == want
    assert not any(v.requires_grad for v in got.values())


# ---- epochs until num_timesteps (ES, ARS) -------------------------------------------------------

class _EpochLearner:
  """Every epoch adds 320 env steps (`tests/test_gpu_evolution.py`'s most)."""
  device = torch.device('cpu')
  num_envs, episode_length = 16, 20

  def __init__(self, log):
    self.log, self.policy, self.num_env_steps, self.steps = log, _Policy('actor', log), 0, []
    self.layers = 'layers'

  def epoch(self):
    self.num_env_steps += 320
    self.steps.append(self.num_env_steps)
    self.log.append('epoch')
    return {'metrics': {'params_norm': float(len(self.steps))}}


def _expected_calls(steps, first, between, initial):
  """The reference's loop over the recorded step counts: one evaluation after
  an epoch that reaches the next evaluation step."""
  calls, nxt = ([0] if initial else []), first
  for s in steps:
    if s >= nxt:
      calls.append(s)
      nxt += between
  return calls


@pytest.mark.parametrize('separate', [False, True])
def test_es_schedule(log, separate):
  learner, calls = _EpochLearner(log), []
  eval_policy = _Policy('eval', log) if separate else learner.policy
  sched = es.eval_schedule(641, 2)
  metrics = driver.run(learner, eval_policy, _Evaluator(log), 641, sched.first_eval_step,
                       sched.num_env_steps_between_evals, True,
                       lambda n, m: calls.append((n, dict(m))))
  assert learner.steps == [320, 640, 960]
  assert [n for n, _ in calls] == _expected_calls(learner.steps, 641, 641, True) == [0, 960]
  assert metrics == calls[-1][1] and metrics['training/params_norm'] == 3.0
  assert metrics['training/sps'] == 16 * 20 and metrics['training/walltime'] == 3
  reload = [('load', 'eval', 'layers')] if separate else []
  assert log == ['eval'] + ['epoch', 'sync'] * 3 + reload + ['eval']


def test_ars_schedule(log):
  learner, calls = _EpochLearner(log), []
  sched = ars.eval_schedule(641, 2)
  assert (sched.first_eval_step, sched.num_env_steps_between_evals) == (321, 320)
  driver.run(learner, learner.policy, _Evaluator(log), 641, sched.first_eval_step,
             sched.num_env_steps_between_evals, False, lambda n, m: calls.append((n, dict(m))))
  assert [n for n, _ in calls] == _expected_calls(learner.steps, 321, 320, False) == [640, 960]
  assert log == ['epoch', 'sync', 'epoch', 'sync', 'eval', 'epoch', 'sync', 'eval']
