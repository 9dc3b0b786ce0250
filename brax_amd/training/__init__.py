"""The learner side (`brax/training`): PPO on the fused rollouts, ES and ARS
on the one-launch population episode, SAC on a device replay queue.

    from brax_amd.training import ars, es, ppo, sac
    make_policy, params, metrics = ppo.train('ant', num_timesteps=..., episode_length=1000, ...)
    make_policy, params, metrics = es.train('ant', num_timesteps=..., population_size=4096, ...)
    make_policy, params, metrics = ars.train('ant', num_timesteps=..., number_of_directions=60, ...)
    make_policy, params, metrics = sac.train('ant', num_timesteps=..., min_replay_size=8192, ...)
"""
from brax_amd.training import (ars, es, gae, losses, networks, optim, ppo, replay_buffers, sac,
                               sac_losses, sac_networks)
from brax_amd.training.gae import compute_gae
from brax_amd.training.losses import Transition, ppo_loss
from brax_amd.training.networks import make_ppo_networks, mlp
from brax_amd.training.optim import FusedAdam
from brax_amd.training.replay_buffers import UniformSamplingQueue, transition_fields
from brax_amd.training.sac_networks import make_sac_networks
# (the module, not its function of the same name: `training.fused_mlp.fused_mlp`)
from brax_amd.training import fused_mlp
from brax_amd.training.ppo import Learner, step_accounting, train, transitions
from brax_amd.training.running_statistics import RunningStatistics
