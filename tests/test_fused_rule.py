"""The `fused` False / True / None rule (`brax_amd.fused.use_kernel`) and the
one optimiser choice built on it, without a GPU."""
import pytest
import torch

from brax_amd.fused import use_kernel
from brax_amd.training import optim


def _never():
  raise AssertionError('the support check ran')


def test_false_never_runs_the_support_check():
  assert use_kernel(False, 'x', _never) is False


def test_none_takes_the_kernel_where_it_applies():
  assert use_kernel(None, 'x', lambda: 'a reason') is False
  assert use_kernel(None, 'x', lambda: None) is True


def test_true_takes_the_kernel_or_raises_the_reason():
  assert use_kernel(True, 'x', lambda: None) is True
  with pytest.raises(NotImplementedError) as e:
    use_kernel(True, 'policy rollout', lambda: 'a CPU tensor')
  assert str(e.value) == 'no fused policy rollout: a CPU tensor'


def test_make_adam_on_cpu_tensors():
  groups = [dict(params=[torch.zeros(4, 3), torch.zeros(3)], lr=1e-3)]
  assert optim.make_adam(groups, None) is None  # torch's optimiser is to be used
  assert optim.make_adam(groups, False) is None
  with pytest.raises(NotImplementedError) as e:
    optim.make_adam(groups, True)
  assert str(e.value) == 'no fused Adam: group 0 param 0 is a CPU tensor'
