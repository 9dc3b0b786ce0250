"""The learner side (`brax/training`): PPO on the fused rollouts.

    from brax_amd.training import ppo
    make_policy, params, metrics = ppo.train('ant', num_timesteps=..., episode_length=1000, ...)
"""
from brax_amd.training import gae, losses, networks, ppo
from brax_amd.training.gae import compute_gae
from brax_amd.training.losses import Transition, ppo_loss
from brax_amd.training.networks import make_ppo_networks, mlp
from brax_amd.training.ppo import Learner, RunningStatistics, step_accounting, train, transitions
