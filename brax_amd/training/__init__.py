"""The learner side (`brax/training`): PPO on the fused rollouts, ES and ARS
on the one-launch population episode.

    from brax_amd.training import ars, es, ppo
    make_policy, params, metrics = ppo.train('ant', num_timesteps=..., episode_length=1000, ...)
    make_policy, params, metrics = es.train('ant', num_timesteps=..., population_size=4096, ...)
    make_policy, params, metrics = ars.train('ant', num_timesteps=..., number_of_directions=60, ...)
"""
from brax_amd.training import ars, es, gae, losses, networks, ppo
from brax_amd.training.gae import compute_gae
from brax_amd.training.losses import Transition, ppo_loss
from brax_amd.training.networks import make_ppo_networks, mlp
from brax_amd.training.ppo import Learner, RunningStatistics, step_accounting, train, transitions
