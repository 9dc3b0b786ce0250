"""The refusals of the C ABI's entry points that take a bx_system, pinned text
for text with the order of their checks. They need bx_system_create, so a
device, but every case is refused or is zero work before any kernel launch:
this file launches nothing. Two systems: 'ant' (SINGLE mode) and
'capsule_cull' (not SINGLE). Device pointers are arbitrary non-null aligned
integers, never dereferenced."""
import ctypes as C

import pytest
import torch

from brax_amd import _native
from brax_amd import abi
from brax_amd.system import System
from tests.helpers import compiled, config_for

pytestmark = pytest.mark.gpu

P = 0x7f0000001000  # a "device pointer": non-null, 4 KiB aligned
ANT, OBS, MET, ACT = 1, 27, 10, 8  # BX_ENV_ANT and its sizes on the ant system
NB = 4 * int(compiled('ant')[1]['n_bodies'])  # the smallest plane stride of 4 ant envs


@pytest.fixture(scope='module')
def systems():
  dev = torch.device('cuda', 0)
  return {'ant': System(config_for('ant'), device=dev),
          'cull': System(config_for('capsule_cull'), device=dev)}


def env(obs=OBS, met=MET, flags=0, **kw):
  p = abi.BxEnvParams()
  p.kind, p.obs_size, p.n_metrics, p.obs_flags, p.action_repeat = ANT, obs, met, flags, 1
  for k, v in kw.items():
    setattr(p, k, v)
  return p


def qp(ptr=P):
  q = abi.BxQP()
  for name in ('pos', 'rot', 'vel', 'ang'):
    f = getattr(q, name)
    f.ptr, f.env_stride, f.body_stride = ptr, 16 * 9, 16
  return q


def state(**kw):
  s = abi.BxEnvState()
  s.qp = qp()
  s.obs = s.reward = s.done = s.metrics = s.steps = s.truncation = s.rng = P
  for k, v in kw.items():
    setattr(s, k, v)
  return s


def policy(widths=(32, 16), params=P, act=0, n=None, mean=None, std=None, min_std=1e-3, det=0,
           A=ACT):
  p = abi.BxPolicy()
  p.params, p.n_layers, p.activation = params, len(widths) if n is None else n, act
  for l, w in enumerate(widths):
    p.width[l] = w
  p.obs_mean, p.obs_std, p.min_std, p.deterministic, p.action_size = mean, std, min_std, det, A
  return p


def population(stride=1424, head=0, mom_out=P, flags=0):
  p = abi.BxPopulation()
  p.param_stride, p.head, p.mom_out, p.flags, p.staged, p.lds_bytes = stride, head, mom_out, flags, -1, -1
  return p


def step(e=None, n=4, sin=None, sout=None, act=P, stride=ACT, width=ACT):
  return (e or env(), n, sin or state(), act, stride, width, sout or state(), None)


def step_packed(e=None, n=4, qp_in=P, done_in=P, act=P, width=ACT, out=P):
  return (e or env(), n, qp_in, done_in, P, None, act, ACT, width, out, None, None)


def rollout(e=None, n=4, k=2, qp_in=P, act=P, step_stride=32, width=ACT, out=P):
  return (e or env(), n, k, qp_in, P, P, None, act, ACT, step_stride, width, out, None, None)


def random(e=None, n=4, k=2, width=ACT):
  return (e or env(), n, k, P, P, P, None, 1, 0, 32, -1.0, 1.0, width, None, P, None, None)


def pol(e=None, n=4, k=2, obs_in=P, p=None):
  return (e or env(), n, k, P, obs_in, P, P, None, p, 1, 0, 64, None, None, None, P, None, None)


def evpol(e=None, n=4, k=2, obs_in=P, p=None, eval_out=P):
  return (e or env(), n, k, P, obs_in, P, P, None, p, 1, 0, 64, None, P, eval_out, None, None)


def evpop(e=None, n=4, k=2, obs_in=P, p=None, eval_out=P, pop=None):
  return evpol(e, n, k, obs_in, p, eval_out)[:-1] + (pop, None)


def evpacked(e=None, n=4, k=2, step_stride=32, eval_out=P):
  return (e or env(), n, k, P, P, P, None, P, ACT, step_stride, ACT, None, P, eval_out, None, None)


def reset(e=None, n=4, offset=0, noise=0.1, out=None):
  return (e or env(), n, 1, offset, None, noise, out or state(), None)


OBS_MSG = 'obs_size 28 != 27 for this env kind and system'
LAST_MSG = 'policy: the last layer is 2 x action_size wide (action_size when deterministic)'
DRAW_W = 'on-device draws stage the whole action row: act_width exceeds the row the system stages'
STRIDE_MSG = ('population: param_stride must be 0 or a multiple of 4 floats no smaller than '
              'n_params (1424)')
PLANE_MSG = 'plane stride must be >= N*n_envs and a multiple of 4'
N4_MSG = 'n_envs must be a positive multiple of 4'
NP = policy()  # (kept alive for the rows below)

# (system, entry point, arguments after the system, bx_last_error()); the rows
# of one entry point follow the order of its checks, and a row with two faults
# names the first
REFUSALS = [
    # check_env
    ('ant', 'bx_env_step', step(env(obs=28)), OBS_MSG),
    ('ant', 'bx_env_step', step(env(met=9)), 'n_metrics 9 != 10 for this env kind'),
    ('ant', 'bx_env_step', step(env(flags=2)), 'unknown obs_flags bits'),
    ('ant', 'bx_env_step', step(env(flags=2, obs=28)), 'unknown obs_flags bits'),
    ('ant', 'bx_env_step', step(env(obs=28, met=9)), OBS_MSG),
    # env_step_impl
    ('ant', 'bx_env_step', (None,) + step()[1:], 'null argument'),
    ('ant', 'bx_env_step', step()[:2] + (None,) + step()[3:], 'null argument'),
    ('ant', 'bx_env_step', step(env(obs=28), n=-1), OBS_MSG),
    ('ant', 'bx_env_step', step(n=-1, act=None), 'negative n_envs'),
    ('ant', 'bx_env_step', step(width=-1), 'negative action width or stride'),
    ('ant', 'bx_env_step', step(stride=-1), 'negative action width or stride'),
    ('ant', 'bx_env_step', step(act=None), 'null or empty action'),
    ('ant', 'bx_env_step', step(width=0), 'null or empty action'),
    ('ant', 'bx_env_step', step(act=None, sin=state(qp=qp(None))), 'null or empty action'),
    ('ant', 'bx_env_step', step(sin=state(qp=qp(None))), 'null qp field'),
    ('ant', 'bx_env_step', step(sout=state(qp=qp(None), obs=None)), 'null qp field'),
    ('ant', 'bx_env_step', step(sin=state(done=None)), 'null env buffer'),
    ('ant', 'bx_env_step', step(sout=state(obs=None)), 'null env buffer'),
    ('ant', 'bx_env_step', step(env(auto_reset=1), sout=state(reward=None)), 'null env buffer'),
    ('ant', 'bx_env_step', step(env(auto_reset=1)), 'auto_reset needs first_qp and first_obs'),
    ('ant', 'bx_env_step', step(env(auto_reset=1, first_qp=qp())),
     'auto_reset needs first_qp and first_obs'),
    ('ant', 'bx_env_step', step(env(auto_reset=1, episode_length=10), sout=state(steps=None)),
     'auto_reset needs first_qp and first_obs'),
    ('ant', 'bx_env_step', step(env(episode_length=10), sout=state(steps=None)),
     'episode wrapper needs steps and truncation buffers'),
    ('ant', 'bx_env_step', step(env(episode_length=10), sout=state(truncation=None)),
     'episode wrapper needs steps and truncation buffers'),
    # env_step_packed
    ('ant', 'bx_env_step_packed', (None,) + step_packed()[1:], 'null argument'),
    ('ant', 'bx_env_step_packed', step_packed(env(obs=28), n=-1), OBS_MSG),
    ('ant', 'bx_env_step_packed', step_packed(n=-1), 'negative n_envs'),
    ('ant', 'bx_env_step_packed', step_packed(qp_in=None), 'null argument'),
    ('ant', 'bx_env_step_packed', step_packed(out=None), 'null argument'),
    ('ant', 'bx_env_step_packed', step_packed(width=0), 'null or empty action'),
    ('ant', 'bx_env_step_packed', step_packed(done_in=None), 'null env buffer'),
    # bx_env_rollout_packed
    ('ant', 'bx_env_rollout_packed', rollout(env(obs=28), k=-1), 'negative n_steps'),
    ('ant', 'bx_env_rollout_packed', (None,) + rollout(k=0)[1:], 'null argument'),
    ('ant', 'bx_env_rollout_packed', rollout(env(obs=28), k=0), OBS_MSG),
    ('ant', 'bx_env_rollout_packed', rollout(step_stride=-1, qp_in=None),
     'negative action step stride'),
    ('ant', 'bx_env_rollout_packed', rollout(n=-1), 'negative n_envs'),
    ('ant', 'bx_env_rollout_packed', rollout(qp_in=None, act=None), 'null argument'),
    ('ant', 'bx_env_rollout_packed', rollout(act=None), 'null or empty action'),
    # bx_env_rollout_random, check_draw
    ('ant', 'bx_env_rollout_random', (None,) + random()[1:], 'null argument'),
    ('ant', 'bx_env_rollout_random', random(env(obs=28), k=-1), 'negative n_steps'),
    ('ant', 'bx_env_rollout_random', random(env(obs=28), k=0, width=0), OBS_MSG),
    ('ant', 'bx_env_rollout_random', random(k=0, width=0), 'on-device draws need act_width >= 1'),
    ('ant', 'bx_env_rollout_random', random(width=0), 'on-device draws need act_width >= 1'),
    ('ant', 'bx_env_rollout_random', random(width=ACT + 1), DRAW_W),
    ('ant', 'bx_env_rollout_random', random(k=0, width=ACT + 1), DRAW_W),
    ('ant', 'bx_env_rollout_random', random(n=-1), 'negative n_envs'),
    # policy_prelude, policy_plan
    ('ant', 'bx_env_rollout_policy', (None,) + pol(p=NP)[1:], 'null argument'),
    ('ant', 'bx_env_rollout_policy', pol(k=-1, p=None), 'negative n_steps'),
    ('ant', 'bx_env_rollout_policy', pol(env(obs=28), p=None), 'null policy'),
    ('ant', 'bx_env_rollout_policy', pol(env(obs=28), p=policy(A=0)), OBS_MSG),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(A=0, params=None)),
     'on-device draws need act_width >= 1'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(A=ACT + 1)), DRAW_W),
    ('cull', 'bx_env_rollout_policy', pol(env(obs=11), p=policy(A=1, params=None)),
     'the policy rollout needs a SINGLE-mode system'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(params=None)),
     'policy parameters: null or not 16-byte aligned'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(params=P + 4, n=0)),
     'policy parameters: null or not 16-byte aligned'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(n=0)), 'policy: 1..8 layers'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(n=9, act=3)), 'policy: 1..8 layers'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(act=3)), 'policy: unknown activation'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(act=-1, mean=P)), 'policy: unknown activation'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(mean=P)), 'policy: obs_mean and obs_std go together'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy(std=P, min_std=-1.0)),
     'policy: obs_mean and obs_std go together'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy((0, 16), min_std=-1.0)), 'policy: negative min_std'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy((0, 16))), 'policy: layer widths 1..128'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy((32, 129, 7))), 'policy: layer widths 1..128'),
    ('ant', 'bx_env_rollout_policy', pol(p=policy((32, 8))), LAST_MSG),
    ('ant', 'bx_env_rollout_policy', pol(p=policy((32, 12), det=1)), LAST_MSG),
    ('ant', 'bx_env_rollout_policy', pol(p=NP, obs_in=None), 'null obs_in'),
    # eval_plan and the evaluation entry points
    ('ant', 'bx_env_eval_policy', evpol(p=policy((32, 8))), LAST_MSG),
    ('cull', 'bx_env_eval_policy', evpol(env(obs=11), p=policy(A=1)),
     'the policy rollout needs a SINGLE-mode system'),
    ('ant', 'bx_env_eval_policy', evpol(p=NP, obs_in=None, eval_out=None), 'null obs_in'),
    ('ant', 'bx_env_eval_policy', evpol(p=NP, eval_out=None), 'null eval_out'),
    ('ant', 'bx_env_eval_packed', (None,) + evpacked()[1:], 'null argument'),
    ('ant', 'bx_env_eval_packed', evpacked(env(obs=28), k=-1), 'negative n_steps'),
    ('cull', 'bx_env_eval_packed', evpacked(env(obs=12)), 'obs_size 12 != 11 for this env kind and system'),
    ('cull', 'bx_env_eval_packed', evpacked(env(obs=11), k=0),
     'the evaluation kernels need a SINGLE-mode system'),
    ('ant', 'bx_env_eval_packed', evpacked(step_stride=-1, eval_out=None),
     'negative action step stride'),
    ('ant', 'bx_env_eval_packed', evpacked(eval_out=None), 'null eval_out'),
    # bx_env_eval_population
    ('ant', 'bx_env_eval_population', evpop(p=None, pop=None), 'null policy'),
    ('ant', 'bx_env_eval_population', evpop(env(obs=28), p=NP, pop=None), 'null population'),
    ('ant', 'bx_env_eval_population', evpop(env(obs=28), p=NP, pop=population(head=2)),
     'population: unknown head'),
    ('ant', 'bx_env_eval_population', evpop(p=NP, pop=population(head=1)),
     "population: the identity head's last layer is action_size wide"),
    ('ant', 'bx_env_eval_population', evpop(p=policy((32, 8)), pop=population()), LAST_MSG),
    ('cull', 'bx_env_eval_population', evpop(env(obs=11), p=policy(A=1), pop=population()),
     'the policy rollout needs a SINGLE-mode system'),
    ('ant', 'bx_env_eval_population', evpop(p=NP, pop=population(stride=1420)), STRIDE_MSG),
    ('ant', 'bx_env_eval_population', evpop(p=NP, pop=population(stride=1426), obs_in=None),
     STRIDE_MSG),
    ('ant', 'bx_env_eval_population', evpop(p=NP, pop=population(), obs_in=None, eval_out=None),
     'null obs_in'),
    ('ant', 'bx_env_eval_population', evpop(p=NP, pop=population(), eval_out=None), 'null eval_out'),
    # bx_env_reset
    ('ant', 'bx_env_reset', reset(env(obs=28), n=-1), OBS_MSG),
    ('ant', 'bx_env_reset', reset(n=-1, offset=-1), 'negative n_envs'),
    ('ant', 'bx_env_reset', reset(offset=-1, noise=-1.0), 'negative env_offset'),
    ('ant', 'bx_env_reset', reset(noise=-1.0, out=state(obs=None)), 'noise_scale must be >= 0'),
    ('ant', 'bx_env_reset', reset(out=state(obs=None, metrics=None)), 'null env buffer'),
    ('ant', 'bx_env_reset', reset(out=state(qp=qp(None))), 'null env buffer'),
    ('ant', 'bx_env_reset', reset(out=state(metrics=None)), 'null metrics buffer'),
    # bx_env_observe, bx_system_default_qp
    ('ant', 'bx_env_observe', (env(), 4, qp(), P, ACT, ACT, None, None), 'null argument'),
    ('ant', 'bx_env_observe', (env(obs=28), 4, qp(), P, ACT, -1, P, None), OBS_MSG),
    ('ant', 'bx_env_observe', (env(), -1, qp(), P, ACT, -1, P, None), 'negative action width or stride'),
    ('ant', 'bx_env_observe', (env(), -1, qp(), P, ACT, ACT, P, None), 'negative n_envs'),
    ('ant', 'bx_system_default_qp', (4, P, P, None, None), 'null argument'),
    ('ant', 'bx_system_default_qp', (-1, None, None, qp(), None), 'negative n_envs'),
    ('ant', 'bx_system_default_qp', (4, None, P, qp(), None), 'null joint arrays'),
    ('ant', 'bx_system_default_qp', (4, P, None, qp(), None), 'null joint arrays'),
    # the phase kernels
    ('ant', 'bx_phase', (0, 4, NB, None, P, None, 0, None), 'null argument'),
    ('ant', 'bx_phase', (3, 6, NB, P, P, None, 0, None), 'unknown phase'),
    ('ant', 'bx_phase', (0, 6, NB - 4, P, P, None, 0, None), N4_MSG),
    ('ant', 'bx_phase', (0, 0, NB, P, P, None, 0, None), N4_MSG),
    ('ant', 'bx_phase', (0, 4, NB - 4, P + 4, P, None, 0, None), PLANE_MSG),
    ('ant', 'bx_phase', (0, 4, NB + 2, P, P, None, 0, None), PLANE_MSG),
    ('ant', 'bx_phase', (1, 4, NB, P + 4, P, None, NB, None), 'bad aux planes'),
    ('ant', 'bx_phase', (1, 4, NB, P, P, P, NB - 4, None), 'bad aux planes'),
    ('ant', 'bx_phase', (2, 4, NB, P, P, P, NB + 2, None), 'bad aux planes'),
    ('ant', 'bx_phase', (0, 4, NB, P + 4, P, None, 0, None), 'SoA bases must be 16-byte aligned'),
    ('ant', 'bx_phase', (0, 4, NB, P, P + 8, None, 0, None), 'SoA bases must be 16-byte aligned'),
    ('ant', 'bx_phase', (1, 4, NB, P, P, P + 4, NB, None), 'SoA bases must be 16-byte aligned'),
    ('ant', 'bx_phase_capsule_plane', (4, NB, P, None, 1 << 20, None), 'null argument'),
    ('ant', 'bx_phase_capsule_plane', (6, NB - 4, P, P, 1 << 20, None), N4_MSG),
    ('ant', 'bx_phase_capsule_plane', (4, NB - 4, P, P, 2, None), PLANE_MSG),
    ('ant', 'bx_phase_capsule_plane', (4, NB, P + 4, P, 2, None), 'out plane stride must be >= R*n_envs'),
    ('ant', 'bx_phase_capsule_plane', (4, NB, P + 4, P, 1 << 20, None),
     'SoA bases must be 16-byte aligned'),
]

# rc 0 and no error: an empty batch or no steps, after the checks before it
ZERO_WORK = [
    ('ant', 'bx_env_step', step(n=0, sin=abi.BxEnvState(), sout=abi.BxEnvState(), act=None, width=0)),
    ('ant', 'bx_env_step_packed', step_packed(n=0, qp_in=None, out=None, act=None)),
    ('ant', 'bx_env_rollout_packed', rollout(k=0, n=-1, qp_in=None, step_stride=-1)),
    ('ant', 'bx_env_rollout_packed', rollout(n=0, qp_in=None, out=None)),
    ('ant', 'bx_env_rollout_random', random(k=0, n=-1)),
    ('ant', 'bx_env_rollout_random', random(n=0)),
    ('ant', 'bx_env_rollout_policy', pol(p=NP, k=0, n=-1, obs_in=None)),
    ('ant', 'bx_env_rollout_policy', pol(p=NP, n=0, obs_in=None)),
    ('ant', 'bx_env_eval_policy', evpol(p=NP, k=0, obs_in=None, eval_out=None)),
    ('ant', 'bx_env_eval_policy', evpol(p=NP, n=0, obs_in=None, eval_out=None)),
    ('ant', 'bx_env_eval_packed', evpacked(k=0, step_stride=-1, eval_out=None)),
    ('ant', 'bx_env_eval_packed', evpacked(n=0, eval_out=None)),
    ('ant', 'bx_env_reset', reset(n=0, offset=-1, noise=-1.0, out=abi.BxEnvState())),
    ('ant', 'bx_env_observe', (env(), 0, qp(None), None, 0, 0, P, None)),
    ('ant', 'bx_system_default_qp', (0, None, None, qp(None), None)),
]


def _call(systems, which, name, args):
  lib = _native.lib()
  # a refusal must set the text itself: start from another one
  assert lib.bx_system_set_single(None, 0) == 1 and lib.bx_last_error() == b'null system'
  args = tuple(C.byref(a) if isinstance(a, C.Structure) else a for a in args)
  return getattr(lib, name)(systems[which]._h, *args), lib.bx_last_error().decode()


def _ids(rows):
  return [f'{i}-{r[1]}' for i, r in enumerate(rows)]


def test_sizes_of_the_two_systems(systems):
  lib = _native.lib()
  for which, want in (('ant', (OBS, MET)), ('cull', (11, MET))):
    o, m = C.c_int32(), C.c_int32()
    e = env()
    assert lib.bx_env_sizes(systems[which]._h, C.byref(e), C.byref(o), C.byref(m)) == 0
    assert (o.value, m.value) == want
  assert System.plan(config_for('ant'))['mode'] == 1
  assert System.plan(config_for('capsule_cull'))['mode'] != 1
  assert 4 * systems['ant'].num_bodies == NB and systems['ant'].action_size == ACT


@pytest.mark.parametrize('which,name,args,message', REFUSALS, ids=_ids(REFUSALS))
def test_refusal(systems, which, name, args, message):
  assert _call(systems, which, name, args) == (1, message)


@pytest.mark.parametrize('which,name,args', ZERO_WORK, ids=_ids(ZERO_WORK))
def test_zero_work_returns_ok(systems, which, name, args):
  assert _call(systems, which, name, args) == (0, 'null system')  # (the error text is left alone)


# (policy widths, population, (staged, lds_bytes)): on ant's 18,432 bytes of
# step LDS at 4 envs per workgroup; the rows staged only where they fit 40 KiB
POP_LAYOUTS = [
    ((32, 16), dict(stride=1424), (0, 21184)),
    ((32, 16), dict(stride=0), (0, 26880)),
    ((32, 16), dict(stride=1424, flags=abi.POP_NO_STAGE, mom_out=None), (0, 20288)),
    ((16, 16), dict(stride=720), (1, 32576)),
]


@pytest.mark.parametrize('widths,kw,want', POP_LAYOUTS)
def test_population_layout_write_back(systems, widths, kw, want):
  """An accepted n_steps == 0 call writes the layout it would launch with."""
  pop = population(**kw)
  args = evpop(p=policy(widths), pop=pop, k=0, obs_in=None, eval_out=None)
  assert _call(systems, 'ant', 'bx_env_eval_population', args)[0] == 0
  print('population layout', widths, kw, (pop.staged, pop.lds_bytes))
  assert (pop.staged, pop.lds_bytes) == want


LANES_MSG = 'lanes must be 16, 32, 64, 128 or 256'
MODE_MSG = 'mode must be 0 (global), 1 (single), 2 (lds) or 3 (multi)'
SINGLE_MSG = 'system does not fit the single-item-per-lane kernel at that width'
MULTI_MSG = 'system does not fit the MULTI-mode kernel at that width (128 or 256 lanes)'
BLOCK_MSG = ('threads must be a multiple of the lanes per env, at most 64 (or the lanes per env '
             'past 64)')
PLAN_CALLS = [
    ('ant', 'bx_system_set_variant', (48, 4), LANES_MSG),
    ('ant', 'bx_system_set_variant', (0, 1), LANES_MSG),
    ('ant', 'bx_system_set_variant', (64, 4), MODE_MSG),
    ('ant', 'bx_system_set_variant', (64, -1), MODE_MSG),
    ('ant', 'bx_system_set_variant', (128, 1), SINGLE_MSG),
    ('ant', 'bx_system_set_variant', (64, 3), MULTI_MSG),
    ('cull', 'bx_system_set_variant', (64, 3), MULTI_MSG),
    ('ant', 'bx_system_set_block', (0,), BLOCK_MSG),
    ('ant', 'bx_system_set_block', (24,), BLOCK_MSG),
    ('ant', 'bx_system_set_block', (128,), BLOCK_MSG),
    ('cull', 'bx_system_set_block', (8,), BLOCK_MSG),
]


@pytest.mark.parametrize('which,name,args,message', PLAN_CALLS, ids=_ids(PLAN_CALLS))
def test_refused_plan_change_leaves_the_plan(systems, which, name, args, message):
  lib = _native.lib()
  h = systems[which]._h
  before = (lib.bx_system_lanes(h), lib.bx_system_env_lanes(h), lib.bx_system_lds_bytes(h))
  assert getattr(lib, name)(h, *args) == 1 and lib.bx_last_error().decode() == message
  assert (lib.bx_system_lanes(h), lib.bx_system_env_lanes(h), lib.bx_system_lds_bytes(h)) == before
  assert getattr(lib, name)(None, *args) == 1 and lib.bx_last_error() == b'null system'
