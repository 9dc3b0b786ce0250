"""The observation normaliser every trainer shares."""
import numpy as np
import torch

from brax_amd.envs.population import update_running_statistics


class RunningStatistics:
  """`running_statistics.RunningStatisticsState` for one observation vector:
  float64 on the host (`update_running_statistics`), with float32 device
  copies `mean_t` / `std_t` that are updated in place."""

  def __init__(self, size: int, device=None):
    self.mean = np.zeros(size)
    self.summed_variance = np.zeros(size)
    self.count = 0.0
    self.std = np.ones(size)
    self.mean_t = torch.zeros((size,), dtype=torch.float32, device=device)
    self.std_t = torch.ones((size,), dtype=torch.float32, device=device)

  def update(self, obs: torch.Tensor):
    """`running_statistics.update(state, obs)`, every row of `obs` (..., O)
    with weight 1: the sums centred on the old mean are taken on `obs`'s
    device in float64, the O-sized remainder on the host."""
    rows = obs.reshape(-1, obs.shape[-1])
    d = rows.double() - torch.as_tensor(self.mean, device=rows.device)
    self.mean, self.summed_variance, self.count, self.std = update_running_statistics(
        self.mean, self.summed_variance, self.count,
        (d.sum(0), (d * d).sum(0), np.array([rows.shape[0]], np.float64)))
    return self._publish()

  def update_from_moments(self, result):
    """The same update from a `PopulationResult`'s on-chip moments (each step
    weighted by the env's `active`), centred on `mean_t` as the acting policy
    read it."""
    self.mean, self.summed_variance, self.count, self.std = update_running_statistics(
        self.mean, self.summed_variance, self.count, result)
    return self._publish()

  def _publish(self):
    self.mean_t.copy_(torch.as_tensor(self.mean, dtype=torch.float32))
    self.std_t.copy_(torch.as_tensor(self.std, dtype=torch.float32))
    return self
