"""HIP path (through the C-ABI) vs the reference's golden vectors and the C
restatement. Needs an MI355X.

Parity gate, per env i and field, normwise
    max|Δ_i| <= tol_i * max(1, max|x_i|)   against the reference's float64 states:
  every field:             tol_i = max(1e-5, 2 * E32_i)
  Ant (the north-star config) pos/rot additionally <= 1e-5 flat
E32_i is the fp32 error envelope of Brax's OWN algorithm on the same sample:
the largest normwise error, vs the float64 reference, of the oracle's two
float32 builds (the reference algorithm executed in true fp32, plain and with
a*b+c contracted to FMA as XLA's jit does) over the exact inputs and copies
perturbed by fp32-ulp relative noise (x * (1 + U[-6e-8,6e-8]), SURVEY §8(c)'s
conditioning probe; 32 copies per build: 66 realisations per env). The HIP kernel must be as close to the
reference as fp32 rounding noise itself allows, within 2x. Velocities are
(pos - pos_prev)/h, so fp32 rounding is amplified ~1/h per substep, and the
contact masks (`penetration > 0`, `c < 0`, static-friction and sinking gates)
flip on rounding; a flat 1e-5 is not reachable for those by Brax itself.
"""
import os

import numpy as np
import pytest
import torch

from tests.conftest import golden
from tests.margins import record_exact, record_margin
from tests.helpers import (CAPSULES, MID, MID_ENV, N_PERTURB, NEAR_TOL, WIDE, Envelope, NN_MASKED,
                           SHORT_SCENES, ENVTRAJ_KERNEL, POINTS, QP_FIELDS, ROBOTS, SPRING_ENVS, SPRING_ROBOTS, XCOL, XY_ENVS, compiled, env_golden, env_kind,
                           golden_reset_qp, normwise, obs_flags, prep_oracle, reset_bodies,
                           sys_golden, teleported, without_teleported)

pytestmark = pytest.mark.gpu

ENV_TRAJ = ['ant', 'humanoid', 'halfcheetah', 'humanoidstandup'] + SPRING_ENVS
# the reference's long physics-test scenes (CAPSULES, box_ground / box_slide:
# 400-10,000 substeps per step, resting contacts at their gates) have an O(1)
# fp32 envelope, so a state gate there tests nothing: they stay KATs below,
# and their short-horizon twins (SHORT_SCENES) carry the trajectory gates
SYS_TRAJ = (['mountain1', 'mountain2', 'mountain4', 'mountain1nn', 'mountain4nn'] + ROBOTS + NN_MASKED
            + [p for p in POINTS if not p.startswith('box')] + SPRING_ROBOTS + XCOL + SHORT_SCENES)
POS_TOL = 1e-5


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


def _system(name, dev):
  import brax_amd
  from tests.helpers import config_for
  return brax_amd.System(config_for(name), device=dev)


def _qp_np(qp):
  return qp.numpy()


def _to_qp(a, dev):
  from brax_amd.base import qp_from_numpy
  return qp_from_numpy(a, dev)


# BX_PARITY_RECORD_ONLY=1 (diagnostic runs): record the per-env ratios of
# every gate without asserting them (the group bound is still asserted), so
# one run lists every env past its bound
RECORD_ONLY = os.environ.get('BX_PARITY_RECORD_ONLY') == '1'


def _dump_failure(field, got, ref, samples):
  """A per-env gate past its bound: the HIP output, the reference and Brax's
  fp32 realisations to gpurun_out/gate_fail_<test>_<field>.npz, for the
  offline search of the element and phase that carry the excess."""
  import re
  test = os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]
  name = re.sub(r'[^A-Za-z0-9_.-]+', '_', test.split('::')[-1]) + '_' + field
  runs = np.asarray([np.asarray(v) for v in (samples or [])])
  np.savez_compressed(os.path.join(out_dir(), f'gate_fail_{name}.npz'),
                      got=np.asarray(got), ref=np.asarray(ref), samples=runs)


def out_dir():
  """The directory the suite's recorded figures and dumps go to, created."""
  d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
  os.makedirs(d, exist_ok=True)
  return d


def _gate(got, ref, e32, field, split=True):
  """SURVEY 8(c)'s per-sample gate: env i's normwise error <= max(1e-5,
  2 x E32_i), E32_i the largest fp32 error of Brax's own algorithm over that
  env's 66 realisations (both oracle builds, exact and ulp-perturbed inputs).
  The envs are split: the well-conditioned ones (2 x E32_i <= 1e-2) take
  their own bound; the ill-conditioned ones (a contact flipping on rounding:
  Brax's own fp32 is off by > 5e-3 there) are gated on the NEAREST of Brax's
  fp32 realisations below, their envelope group recorded as
  `<field>:illcond` (role 'envelope'). Every gate records the distribution
  of HIP_i / bound_i over its envs (tests/margins.py). Without `split` (the
  reset lift's discontinuity: any env may flip), one group bound.
  (Until round 4 the well-conditioned bound was the group's largest E32,
  under which one env's large Brax error covered another's excess.)"""
  nw = normwise(got, ref)
  samples = getattr(e32, 'samples', None)
  e32 = np.broadcast_to(np.asarray(e32, np.float64), nw.shape)
  assert np.all(np.isfinite(got)), field
  ill = (2.0 * e32 > WIDE) if split else np.zeros(nw.shape, bool)
  worst = (0.0, POS_TOL)
  well = ~ill
  if well.any():
    group_tol = max(POS_TOL, 2.0 * float(e32[well].max()))
    tol_i = np.maximum(POS_TOL, 2.0 * e32) if split else np.full(nw.shape, group_tol)
    r = np.where(well, nw / tol_i, -1.0)
    k = int(np.argmax(r))
    m, tol = float(nw.flat[k]), float(tol_i.flat[k])
    record_margin(field, m, tol, n=int(well.sum()), ratios=r[well].ravel().tolist(),
                  gate='per_env' if split else 'group', group_tol=group_tol,
                  group_ratio=float(nw[well].max()) / group_tol)
    if split and samples is not None and len(samples) % 2 == 0:
      # the exact-input realisations: the first of each build's run list
      h = len(samples) // 2
      ex = np.broadcast_to(np.maximum(normwise(samples[0], ref), normwise(samples[h], ref)),
                           nw.shape)
      record_exact(field, (nw / np.maximum(POS_TOL, 2.0 * ex))[well].ravel().tolist())
    assert float(nw[well].max()) <= group_tol, f'{field}: group bound'
    if m > tol:
      _dump_failure(field, got, ref, samples)
    if not RECORD_ONLY:
      assert m <= tol, (f'{field}: env {k} normwise {m:.3e} > its bound {tol:.3e} '
                        f'({int((r > 1).sum())} of {int(well.sum())} envs past theirs)')
    worst = (m, tol)
  if ill.any():
    tol = max(POS_TOL, 2.0 * float(e32[ill].max()))
    m = float(nw[ill].max())
    # the ill-conditioned group's envelope bound (> 1e-2 by definition) is
    # Brax-vs-Brax branch distance; the binding gate for those envs is the
    # nearest-realisation one below
    record_margin(field + ':illcond', m, tol, n=int(ill.sum()), role='envelope')
    assert m <= tol, f'{field}:illcond: normwise {m:.3e} > tol {tol:.3e} ({int(ill.sum())} envs)'
    worst = max(worst, (m, tol))
    # an ill-conditioned env's branch (which contacts fire) is a coin toss
    # under fp32 rounding, so its gate is the distance to the NEAREST of
    # Brax's fp32 realisations (the envelope's runs): the HIP result must be
    # one of them up to rounding on its branch. The bound: twice the
    # realisations' own spread (for each, its distance to the nearest OTHER
    # one; the largest of those per env), floored at NEAR_TOL, capped at WIDE.
    assert samples is not None, f'{field}: an ill-conditioned gate needs the fp32 realisations'
    S = [np.asarray(v) for v in samples]
    near = np.broadcast_to(np.min([normwise(got, v) for v in S], axis=0), nw.shape)
    nn = np.zeros(nw.shape)
    for i, a in enumerate(S):
      d = np.full(nw.shape, np.inf)
      for j, b in enumerate(S):
        if i != j:
          d = np.minimum(d, np.broadcast_to(normwise(a, b), nw.shape))
      nn = np.maximum(nn, d)
    tol_e = np.clip(2.0 * nn, NEAR_TOL, WIDE)
    k = int(np.argmax(np.where(ill, near / tol_e, -1.0)))
    m, tol = float(near.flat[k]), float(tol_e.flat[k])
    record_margin(field + ':illcond_nearest', m, tol, n=int(ill.sum()), envelope_tol=float(2.0 * e32.flat[k]))
    assert m <= tol, f'{field}:illcond_nearest: {m:.3e} from the nearest fp32 realisation > tol {tol:.3e}'
  return worst


def _make_env(name, dev, **kw):
  from brax_amd import envs
  if name.endswith('_spring'):
    kw['legacy_spring'] = True
  if name.endswith('_xy'):
    kw['exclude_current_positions_from_observation'] = False
  return envs.get_environment(env_kind(name), device=dev, **kw)


class _E32(np.ndarray):
  """E32 per env, carrying the fp32 realisations it was taken over."""
  samples = None


def _env_err(vals, ref):
  e = np.asarray(np.max([normwise(v, ref) for v in vals], axis=0), np.float64).view(_E32)
  e.samples = vals
  return e


def _pattern_gate(pen, ref_pen, o_pen, e_all, rows, where):
  """The mid-episode fixtures' target rows: on every well-conditioned sample
  (2 x E32 <= WIDE on every field gated before, `e_all` the largest E32 per
  env) the HIP path's own `penetration > 0` equals the reference's, on the
  rows where the contact test is decided under fp32 rounding (every
  realisation of the envelope agrees with the reference). A kernel that
  skipped a row would otherwise pass whenever its impulse happened to be
  small. Returns the number of penetrating entries compared."""
  well = 2.0 * np.asarray(e_all) <= WIDE
  ref_on = ref_pen[:, rows] > 0
  decided = np.all([(o[:, rows] > 0) == ref_on for o in o_pen], axis=0) & well[:, None]
  got_on = pen[:, rows] > 0
  bad = decided & (got_on != ref_on)
  assert not bad.any(), (f'{where}: contact pattern differs from the reference at (env, target row) '
                         f'{[(int(b), int(rows[r])) for b, r in zip(*np.nonzero(bad))]}')
  return int((decided & ref_on).sum())


@pytest.mark.parametrize('name', ENV_TRAJ + SYS_TRAJ + [r + ':generic' for r in ROBOTS] + MID +
                         MID_ENV + ['mid_pusher:generic', 'mid_hopper:generic',
                                    'mid_walker2d:generic', 'mid_grasp:generic'])
def test_system_step_vs_golden(dev, oracle_lib, name):
  """One System.step from every recorded state against the reference: the
  next state, Info.contact, the contact rows' pos / normal / penetration.

  The fixtures of MID_ENV (`mid_grasp`) record an env whose step changes the
  state and the action before its System.step, so their System.step inputs
  are oracle/mid_states.py `pre_step` of the recorded ones (float64, on the
  host); the kernel, the envelope and the float64 oracle get the same arrays,
  and the float64 oracle's step of them is asserted to be the recorded one
  (1e-9), so a wrong input cannot pass as a kernel error or hide one. The
  recorded next state is the env's: on the samples whose target the env
  teleported after the step, that body's pos is taken out of the HIP output,
  the reference and every realisation alike (tests/helpers.py TELEPORTS)."""
  name, _, variant = name.partition(':')
  sys_ = _system(name, dev)
  if variant == 'generic':
    from brax_amd import _native
    _native.check(_native.lib().bx_system_set_single(sys_._h, 0))
  T = golden(sys_golden(name))
  compared = 0
  pre = None
  tbody, thit = None, None
  if name in MID_ENV:
    from oracle import mid_states
    meta = compiled(name)[3]
    o64 = prep_oracle(oracle_lib.Oracle(*compiled(name)[1:3], np.float64, safe_guard=False), name)
    tbody, thit = teleported(name, T)

    def pre(qp, act):
      # the system reads its own action_size columns; the palm's three past
      # them are spent by the move
      q, a = mid_states.pre_step(env_kind(name), meta, qp, act)
      return q, np.ascontiguousarray(a[:, :sys_.action_size])
  # 32 perturbed copies per build (N_PERTURB): the envelope is a max over samples, and 3 understate
  # it for small batches and for sums over discontinuous gates (legacy_spring
  # Info.contact sums an impulse pass per substep through `penetration > 0`,
  # `v_n < 0` and `|v_t| > 0.01`, colliders.py:290-293: E32 of HalfCheetah's
  # env 3 at t = 2 grows 5.6e-6 -> 1.08e-5 from 3 to 15 copies; one-env
  # scenes such as the height map likewise)
  env32 = Envelope(oracle_lib, name)
  for t in range(T['action'].shape[0]):
    q_in, a_in = (T['qp'][t], T['action'][t]) if pre is None else pre(T['qp'][t], T['action'][t])
    hit = None if thit is None else thit[t]
    qp_in = _to_qp(q_in, dev)
    act = torch.as_tensor(a_in, dtype=torch.float32, device=dev)
    out, info = sys_.step(qp_in, act)
    got = without_teleported(_qp_np(out), tbody, hit)
    ref = without_teleported(T['qp'][t + 1], tbody, hit)
    outs = env32.system(q_in, a_in)
    outs = [(without_teleported(o[0], tbody, hit), o[1]) for o in outs]
    if pre is not None:
      r64, i64 = o64.system_step(q_in, a_in)
      assert normwise(without_teleported(r64, tbody, hit), ref).max() <= 1e-9
      assert normwise(i64['contact'], T['info_contact'][t]).max() <= 1e-9
      assert normwise(i64['contact_penetration'], T['contact_penetration'][t]).max() <= 1e-9
    e_all = np.zeros(got.shape[0])  # the largest E32 per env over the gated fields
    for f, sl in QP_FIELDS.items():
      e32 = _env_err([o[0][..., sl] for o in outs], ref[..., sl])
      e_all = np.maximum(e_all, e32)
      _gate(got[..., sl], ref[..., sl], e32, f)
      if name == 'ant' and f in ('pos', 'rot'):
        assert normwise(got[..., sl], ref[..., sl]).max() <= POS_TOL, f
    ic = torch.cat([info.contact.vel, info.contact.ang], -1).cpu().numpy()
    e32 = _env_err([o[1]['contact'] for o in outs], T['info_contact'][t])
    e_all = np.maximum(e_all, e32)
    _gate(ic, T['info_contact'][t], e32, 'info_contact')
    if name.endswith('_spring'):
      # Info.joint (accumulated spring dp_j, system.py:362-364) vs the float64
      # restatement (the goldens do not record it)
      o64 = oracle_lib.Oracle(*compiled(name)[1:3], np.float64)
      rj = o64.system_step(T['qp'][t], T['action'][t])[1]['joint']
      ij = torch.cat([info.joint.vel, info.joint.ang], -1).cpu().numpy()
      _gate(ij, rj, _env_err([o[1]['joint'] for o in outs], rj), 'info_joint')
    pen = info.contact_penetration.cpu().numpy()
    if pen.size == 0:
      continue
    if 'contact_pos' in T:
      # Info.contact_pos / contact_normal (_get_contact_info, system.py:36-43)
      for k in ('contact_pos', 'contact_normal'):
        g = getattr(info, k).cpu().numpy()
        e32 = _env_err([o[1][k] for o in outs], T[k][t])
        e_all = np.maximum(e_all, e32)
        _gate(g, T[k][t], e32, k)
    ref_pen = T['contact_penetration'][t]
    o_pen = [o[1]['contact_penetration'] for o in outs]
    if 'row_target' in T:
      e_all = np.maximum(e_all, _env_err(o_pen, ref_pen))
      compared += _pattern_gate(pen, ref_pen, o_pen, e_all, T['row_target'], f'{name} step {t}')
    if (np.asarray(sys_.desc['col_cutoff']) > 0).any():
      # culled rows: top_k order, numpy ties arbitrary (see test_oracle)
      srt = lambda a: np.sort(np.maximum(a, 0), -1)  # noqa: E731
      pen, ref_pen, o_pen = srt(pen), srt(ref_pen), [srt(x) for x in o_pen]
    _gate(pen, ref_pen, _env_err(o_pen, ref_pen), 'pen')
  if 'row_target' in T:
    assert compared > 0, 'no decided, well-conditioned, penetrating target row was compared'


@pytest.mark.parametrize('name', ENV_TRAJ + XY_ENVS + ENVTRAJ_KERNEL +
                         ['ant:nojb', 'halfcheetah:nojb'] + MID + MID_ENV +
                         ['mid_halfcheetah:nojb'])
def test_env_step_vs_golden(dev, oracle_lib, name, monkeypatch):
  """One env step from every recorded state against the reference: obs, reward,
  done, metrics. On the mid-episode fixtures (`mid_*`: contact rows at work)
  the whole next state is gated too, pos / rot / vel / ang under the same
  per-env rule. `env.step` returns no Info, so the `penetration > 0` pattern
  cannot be compared here; it is compared in test_system_step_vs_golden
  (`_pattern_gate`), on the rows whose contact test is decided under fp32
  rounding rather than on every row of a well-conditioned sample (a row at
  zero margin flips in Brax's own fp32), and that gate asserts that it
  compared at least one penetrating row.

  The target envs teleport a hit target after the observation is taken
  (tests/helpers.py TELEPORTS): the reference draws the spot from its JAX key,
  the kernel from the env's counter stream, the oracle leaves the target
  where the physics did. On the (step, env) samples whose recorded `hits` is
  1 (`mid_grasp`: step 0, envs 4 and 8) the target's pos is therefore taken
  out of the `qp_pos` gate, in the kernel's output, the reference and every
  realisation alike; its rot / vel / ang and every other sample stay gated.
  There the kernel's spot is held to the teleport's contract instead
  (test_gpu_envs.py test_target_teleport_stream): x-y radius within
  [radius, radius + distance], Grasp's height in [0, 8), and every env's
  stream advanced by one. `hits` itself is asserted exactly: every fp32
  realisation agrees with the reference on it (tests/test_golden_coverage.py
  pins that on the CPU).

  Before this mask `mid_grasp` was left out of the list: `qp_pos` was 9.09e-1
  from the nearest fp32 realisation on one env (`qp_pos:illcond_nearest`
  against 1e-3). That was no rounding: the 66 realisations agree with each
  other to 1.7e-7 and sit 0.63 and 1.0 (normwise) from the reference's
  teleported target on envs 4 and 8, so the gate took a gap between the
  oracle's model and the reference's for an ill-conditioned sample and then
  measured the kernel's own random spot against the oracle's unmoved target.
  tests/test_golden_coverage.py now lists every such gap explicitly."""
  name, _, variant = name.partition(':')
  if variant == 'nojb':
    # the all-kinds kernel the Ant / HalfCheetah kinds fall back to when their
    # system does not allow the body copies of their own kernels (BX_NO_JB)
    monkeypatch.setenv('BX_NO_JB', '1')
  env = _make_env(name, dev)
  T = golden(env_golden(name))
  env32 = Envelope(oracle_lib, name)
  fl = obs_flags(name)
  O, M = T['obs'].shape[-1], T['metrics'].shape[-1]
  assert env.observation_size == O
  from brax_amd.envs.env import State
  tbody, thit = teleported(name, T)
  for t in range(T['action'].shape[0]):
    B = T['qp'].shape[1]
    info = {}
    if getattr(env, 'needs_rng', False):  # the target envs' streams, as a reset starts them
      from brax_amd.envs import tasks
      info['rng'] = tasks.rng_streams(0, 0, B, dev)
    st = State(qp=_to_qp(T['qp'][t], dev), obs=None,
               reward=torch.zeros(B, device=dev), done=torch.zeros(B, device=dev), info=info)
    act = torch.as_tensor(T['action'][t], dtype=torch.float32, device=dev)
    nst = env.step(st, act)
    outs = env32.env(env_kind(name), T['qp'][t], T['action'][t], O, M, fl, env.coef)
    _gate(nst.obs.cpu().numpy(), T['obs'][t + 1], _env_err([o[1] for o in outs], T['obs'][t + 1]),
          'obs')
    _gate(nst.reward.cpu().numpy()[:, None], T['reward'][t][:, None],
          _env_err([o[2][:, None] for o in outs], T['reward'][t][:, None]), 'reward')
    assert np.array_equal(nst.done.cpu().numpy(), T['done'][t])
    if 'row_target' in T:
      # the mid-episode fixtures: the env kernels write no Info (no
      # penetrations to compare patterns on), so the whole next state is gated
      # as well: a contact row the kernel skipped moves its bodies
      hit = None if thit is None else thit[t]
      raw = _qp_np(nst.qp)
      got = without_teleported(raw, tbody, hit)
      ref = without_teleported(T['qp'][t + 1], tbody, hit)
      qps = [without_teleported(o[0], tbody, hit) for o in outs]
      for f, sl in QP_FIELDS.items():
        _gate(got[..., sl], ref[..., sl], _env_err([q[..., sl] for q in qps], ref[..., sl]),
              'qp_' + f)
      if tbody is not None:
        # `hits` decides the teleport: exactly the reference's; a hit target's
        # spot: the teleport's contract, never the reference's draw
        k = list(env.metric_keys).index('hits')
        assert np.array_equal(nst.metrics['hits'].cpu().numpy(), T['metrics'][t][:, k])
        assert torch.equal(nst.info['rng'], info['rng'] + 1)
        c = env.coef
        radius, distance, height = ((c[4], c[5], None) if env_kind(name) == 'grasp'
                                    else (c[2], c[3], c[4]))
        spot = raw[hit, tbody, 0:3]
        r = np.linalg.norm(spot[:, :2], axis=-1)
        assert (r >= radius - 1e-4).all() and (r <= radius + distance + 1e-4).all(), r
        if height is None:
          assert (spot[:, 2] >= 0).all() and (spot[:, 2] < 8).all(), spot[:, 2]
        else:
          np.testing.assert_allclose(spot[:, 2], height, atol=1e-6)
    if env.metric_keys:
      met = np.stack([nst.metrics[k].cpu().numpy() for k in env.metric_keys], -1)
      _gate(met, T['metrics'][t], _env_err([o[4] for o in outs], T['metrics'][t]), 'metrics')


@pytest.mark.parametrize('name', ENV_TRAJ + XY_ENVS + ENVTRAJ_KERNEL)
def test_reset_vs_golden(dev, oracle_lib, name):
  """Reset = default_qp FK + lift + System.info (impulse contacts) + obs.

  The lift puts the lowest collider at exactly z = 0, so the contact test
  `penetration > 0` (colliders.py:297-299) is decided by rounding: Brax's own
  fp32 execution flips it on some envs (E32 ~ 2e-2 on Ant's contact-force obs).
  The gate is therefore relative to E32 for obs; the non-contact part of the
  observation and the state are held to 1e-5."""
  env = _make_env(name, dev)
  T = golden(env_golden(name))
  # the bodies the env's reset places (reacher target, pusher object) at the
  # golden's reset positions
  extra = {}
  placed = reset_bodies(name)
  if placed:
    bi = compiled(name)[3]['body_index']
    key = 'object' if name == 'pusher' else placed[0]
    extra = {'object_pos' if name == 'pusher' else 'target': T['qp'][0][:, bi[key], 0:3]}
  st = env.reset_from(torch.as_tensor(T['reset_qpos'], dtype=torch.float32, device=dev),
                      torch.as_tensor(T['reset_qvel'], dtype=torch.float32, device=dev), **extra)
  got = _qp_np(st.qp)
  for f, sl in QP_FIELDS.items():
    nw = normwise(got[..., sl], T['qp'][0][..., sl])
    assert nw.max() <= 1e-5, (f, nw.max())
  vc, d, rd, meta = compiled(name)
  o32 = oracle_lib.Oracle(d, rd, np.float32, safe_guard=True)
  q32 = golden_reset_qp(name, o32, T)
  B = q32.shape[0]
  obs32 = o32.env_obs(env_kind(name), q32, o32.system_info(q32), np.zeros((B, o32.A)),
                      T['obs'].shape[-1], obs_flags=obs_flags(name), coef=env.coef)
  obs = st.obs.cpu().numpy()
  _gate(obs, T['reset_obs'], normwise(obs32, T['reset_obs']), 'obs', split=False)
  n_state = (1 + 4 + 2 * meta['num_joint_dof'] + 6 + 2 * obs_flags(name)
             if env_kind(name) == 'ant' else obs.shape[-1])
  assert normwise(obs[:, :n_state], T['reset_obs'][:, :n_state]).max() <= 1e-5


@pytest.mark.parametrize('name', ['wrap_ant', 'wrap_ant_ar2'])
def test_wrapped_rollout_vs_golden(dev, oracle_lib, name):
  """Fused Episode+AutoReset (one launch per step) vs the reference's wrapped
  `envs.create('ant', episode_length=L, action_repeat=R, batch_size=8)`
  rollout: R = 1, and R = 2 (the kernel's `reps` loop: two env steps per
  launch, rewards summed, steps advanced by 2; wrappers.py:105-120)."""
  from brax_amd import envs
  from brax_amd.envs.env import State
  T = golden(name)
  ar = int(T['action_repeat']) if 'action_repeat' in T else 1
  env = envs.create('ant', episode_length=int(T['episode_length']), action_repeat=ar,
                    batch_size=8, device=dev)
  first_qp = _to_qp(T['first_qp'], dev)
  first_obs = torch.as_tensor(T['first_obs'], dtype=torch.float32, device=dev)
  st = State(qp=_to_qp(T['qp'][0], dev),
             obs=torch.as_tensor(T['obs'][0], dtype=torch.float32, device=dev),
             reward=torch.zeros(8, device=dev), done=torch.zeros(8, device=dev),
             metrics={}, info={'first_qp': first_qp, 'first_obs': first_obs,
                               'steps': torch.zeros(8, device=dev),
                               'truncation': torch.zeros(8, device=dev)})
  # action_repeat R runs R env steps per wrapped step: the fp32 envelope of
  # the R-step path (the oracle's float32 builds through R steps, then the
  # AutoReset select) sets the velocity gates
  from tests.helpers import compiled
  _, d, rd, _ = compiled('ant')
  os32 = [oracle_lib.Oracle(d, rd, np.float32, fma=f) for f in (False, True)]
  rng = np.random.default_rng(7)
  for t in range(T['action'].shape[0]):
    st = env.step(st, torch.as_tensor(T['action'][t], dtype=torch.float32, device=dev))
    got = _qp_np(st.qp)
    sel = T['done'][t + 1][:, None, None] != 0
    env32 = []
    for o in os32:
      for k in range(4):
        q = T['qp'][t] * (1 + (rng.uniform(-6e-8, 6e-8, T['qp'][t].shape) if k else 0))
        q = q.astype(np.float32)
        for _ in range(ar):
          q, ob, _, _, _ = o.env_step('ant', q, T['action'][t].astype(np.float32), 87, 10)
        env32.append((np.where(sel, T['first_qp'], q), np.where(sel[:, :, 0], T['first_obs'], ob)))
    # R > 1: the second env step starts from the first's fp32 state, whose
    # error (up to 2 x E32 of one step, not an ulp) the second step's
    # velocity projection amplifies by ~1/h: the velocity / observation gate
    # is the flat 1e-3 there; the fused loop itself is pinned bit for bit to
    # R chained launches (test_action_repeat_is_chained_steps)
    flat = 2e-4 if ar == 1 else 1e-3
    for f, sl in QP_FIELDS.items():
      e32 = max(normwise(x[0][..., sl], T['qp'][t + 1][..., sl]).max() for x in env32)
      tol = 1e-5 if f in ('pos', 'rot') and ar == 1 else max(2e-4 if f in ('pos', 'rot') else flat,
                                                              2 * e32)
      assert normwise(got[..., sl], T['qp'][t + 1][..., sl]).max() <= tol, (t, f)
    e32 = max(normwise(x[1], T['obs'][t + 1]).max() for x in env32)
    assert normwise(st.obs.cpu().numpy(), T['obs'][t + 1]).max() <= max(flat, 2 * e32)
    assert np.abs(st.reward.cpu().numpy() - T['reward'][t + 1]).max() <= 1e-4 * ar
    assert np.array_equal(st.done.cpu().numpy(), T['done'][t + 1])
    assert np.array_equal(st.info['steps'].cpu().numpy(), T['steps'][t + 1])
    assert np.array_equal(st.info['truncation'].cpu().numpy(), T['truncation'][t + 1])
  if ar > 1:  # EpisodeWrapper.sys: the config's dt and substeps scaled (wrappers.py:92-95)
    w = env
    while not isinstance(w, __import__('brax_amd.envs.wrappers', fromlist=['x']).EpisodeWrapper):
      w = w.env
    assert w.sys.config.dt == pytest.approx(ar * env.unwrapped.sys.config.dt)
    assert w.sys.config.substeps == ar * env.unwrapped.sys.config.substeps
    assert w.sys.num_bodies == env.unwrapped.sys.num_bodies


@pytest.mark.parametrize('name', ['ant', 'humanoid', 'fetch'])
def test_action_repeat_is_chained_steps(dev, name):
  """The fused kernel's action_repeat loop (EpisodeWrapper's scan,
  wrappers.py:105-120) is exactly R chained env steps: R = 3 in one launch
  gives the bits of three launches of R = 1 on the same action (state, obs,
  done, the target envs' stream), rewards summed in step order, steps + 3."""
  from brax_amd import envs
  B, R = 256, 3
  e3 = envs.create(name, batch_size=B, episode_length=1000, action_repeat=R, auto_reset=False,
                   device=dev)
  e1 = envs.create(name, batch_size=B, episode_length=1000, action_repeat=1, auto_reset=False,
                   device=dev)
  st = e1.reset(np.array([1, 2], np.uint32))
  g = torch.Generator(device='cpu').manual_seed(3)
  act = (torch.rand((B, e1.action_size), generator=g) * 2 - 1).to(dev)
  a = e3.step(st, act)
  b, rsum = st, 0
  for k in range(R):
    b = e1.step(b, act)
    rsum = b.reward if k == 0 else rsum + b.reward
  torch.cuda.synchronize()
  for f in ('pos', 'rot', 'vel', 'ang'):
    assert torch.equal(getattr(a.qp, f), getattr(b.qp, f)), f
  assert torch.equal(a.obs, b.obs) and torch.equal(a.done, b.done)
  assert torch.equal(a.reward, rsum)
  assert torch.equal(a.info['steps'], st.info['steps'] + R)
  if 'rng' in st.info:
    assert torch.equal(a.info['rng'], b.info['rng'])


def test_full_batch_properties(dev, oracle_lib):
  """B = 4096 (BASELINE configs[1]): determinism, batch independence, unit
  quaternions, and parity with the fp64 oracle on a sample of envs."""
  from brax_amd import envs
  env = envs.get_environment('ant', device=dev)
  B = 4096
  st = env.reset_batch(np.array([0, 1], np.uint32), B)
  g = torch.Generator(device='cpu').manual_seed(0)
  for _ in range(3):
    act = (torch.rand((B, 8), generator=g) * 2 - 1).to(dev)
    st = env.step(st, act)
  act = (torch.rand((B, 8), generator=g) * 2 - 1).to(dev)
  a = env.step(st, act)
  b = env.step(st, act)
  torch.cuda.synchronize()
  assert torch.equal(a.qp.pos, b.qp.pos) and torch.equal(a.obs, b.obs)
  # batch independence: the first 7 envs stepped alone give identical bits
  from brax_amd.envs.env import State
  small = State(qp=st.qp[:7], obs=st.obs[:7], reward=st.reward[:7], done=st.done[:7])
  c = env.step(small, act[:7])
  assert torch.equal(c.qp.pos, a.qp.pos[:7]) and torch.equal(c.obs, a.obs[:7])
  q = a.qp.rot
  assert torch.allclose(q.norm(dim=-1), torch.ones_like(q[..., 0]), atol=1e-5)
  assert torch.isfinite(a.obs).all()
  # parity vs the fp64 oracle on 256 sampled envs
  vc, d, rd, meta = compiled('ant')
  o64 = oracle_lib.Oracle(d, rd, np.float64, safe_guard=True)
  env32 = Envelope(oracle_lib, 'ant')
  idx = np.random.default_rng(0).choice(B, 256, replace=False)
  qp_in = st.qp.numpy()[idx]
  an = act.cpu().numpy()[idx].astype(np.float64)
  ref, _ = o64.system_step(qp_in, an)
  outs = env32.system(qp_in, an)
  got = a.qp.numpy()[idx]
  for f, sl in QP_FIELDS.items():
    _gate(got[..., sl], ref[..., sl], _env_err([o[0][..., sl] for o in outs], ref[..., sl]), f)


@pytest.mark.parametrize('name', ['humanoid', 'ant_spring', 'halfcheetah_spring'])
def test_full_batch_properties_other_envs(dev, oracle_lib, name):
  """The same full-batch properties for the spherical-joint kernel variant
  (Humanoid) and the legacy_spring item-loop kernel, at B = 4096."""
  env = _make_env(name, dev)
  B = 4096
  st = env.reset_batch(np.array([0, 3], np.uint32), B)
  g = torch.Generator(device='cpu').manual_seed(1)
  A = env.action_size
  for _ in range(2):
    st = env.step(st, (torch.rand((B, A), generator=g) * 2 - 1).to(dev))
  act = (torch.rand((B, A), generator=g) * 2 - 1).to(dev)
  a = env.step(st, act)
  b = env.step(st, act)
  torch.cuda.synchronize()
  assert torch.equal(a.qp.pos, b.qp.pos) and torch.equal(a.obs, b.obs)
  from brax_amd.envs.env import State
  small = State(qp=st.qp[:5], obs=st.obs[:5], reward=st.reward[:5], done=st.done[:5])
  c = env.step(small, act[:5])
  assert torch.equal(c.qp.pos, a.qp.pos[:5]) and torch.equal(c.obs, a.obs[:5])
  assert torch.isfinite(a.obs).all()
  vc, d, rd, meta = compiled(name)
  o64 = oracle_lib.Oracle(d, rd, np.float64, safe_guard=True)
  env32 = Envelope(oracle_lib, name)
  idx = np.random.default_rng(1).choice(B, 64, replace=False)
  qp_in = st.qp.numpy()[idx]
  an = act.cpu().numpy()[idx].astype(np.float64)
  ref, _ = o64.system_step(qp_in, an)
  outs = env32.system(qp_in, an)
  got = a.qp.numpy()[idx]
  for f, sl in QP_FIELDS.items():
    _gate(got[..., sl], ref[..., sl], _env_err([o[0][..., sl] for o in outs], ref[..., sl]), f)


@pytest.mark.parametrize('name', XCOL + ['capsule_cull', 'mountain1nn'])
def test_item_loop_batch_replicas(dev, name):
  """The item-loop kernels at a full batch: 1024 replicas of one golden state
  step to exactly the bits of that state stepped alone (no cross-env or
  batch-size dependence in the extended contact functions, culling or SAT)."""
  sys_ = _system(name, dev)
  T = golden('traj_' + name)
  q1 = T['qp'][0][:1]
  a1 = T['action'][0][:1]
  one, _ = sys_.step(_to_qp(q1, dev), torch.as_tensor(a1, dtype=torch.float32, device=dev))
  B = 1024
  many, _ = sys_.step(_to_qp(np.repeat(q1, B, axis=0), dev),
                      torch.as_tensor(np.repeat(a1, B, axis=0), dtype=torch.float32, device=dev))
  got, ref = _qp_np(many), _qp_np(one)
  assert np.array_equal(got, np.repeat(ref, B, axis=0))


def nn_cells_check(cells, ref_sel, sim, tol_rel=1e-5):
  """One env's NearNeighbors selection (one culled group) against the
  reference's top_k (colliders.py:84): `cells` the HIP path's selected flat
  cells in Info order, `ref_sel` the reference's top_k indices, `sim` the
  similarities it ranked (-(dist + dist_off): -inf for masked cells).
  Index work is bit-exact where the ranking is decided: a rank whose
  distance is separated from its neighbours by more than the fp32 envelope
  (tol_rel relative) holds exactly the reference's cell, the selected set is
  the reference's wherever the cutoff's distances are separated, and masked
  (-inf) cells follow jax.lax.top_k's lower-index order exactly; among
  near-ties the cell at each rank has the reference rank's distance. Returns
  the number of exact cell comparisons."""
  d = -np.asarray(sim, np.float64)
  k = len(ref_sel)
  assert len(cells) == k, (cells, ref_sel)
  fin = d[np.isfinite(d)]
  tol = tol_rel * max(1.0, float(np.abs(fin).max()) if fin.size else 1.0)
  ds = np.sort(d)
  exact = 0
  for i in range(k):
    dh, dr = d[cells[i]], d[ref_sel[i]]
    if np.isinf(dr) or np.isinf(dh):
      assert cells[i] == ref_sel[i], (i, cells, ref_sel)
      exact += 1
      continue
    assert abs(dh - dr) <= tol, (i, cells, ref_sel, dh, dr)
    lo = ds[i] - ds[i - 1] if i > 0 else np.inf
    hi = ds[i + 1] - ds[i] if i + 1 < ds.size else np.inf
    if lo > tol and hi > tol:
      assert cells[i] == ref_sel[i], (i, cells, ref_sel)
      exact += 1
  with np.errstate(invalid='ignore'):  # inf - inf: masked cells at the cutoff
    clear = k == ds.size or not ds[k] - ds[k - 1] <= tol
  if clear:
    assert set(cells) == set(ref_sel), (cells, ref_sel)
  return exact


@pytest.mark.parametrize('name,variant', [('mountain1nn', None), ('mountain1nn', 'itemloop'),
                                          ('mountain1nn', 'multi'), ('mountain4nn', None),
                                          ('mountain4nn', 'multi'), ('mountain4nn', 'multi256'),
                                          ('mountain4nn', 'itemloop'),
                                          ('capsule_cull_s', None),
                                          ('twin_cull', None), ('twin_cull', 'multi')])
def test_near_neighbors_cells_vs_reference(dev, name, variant):
  """NearNeighbors.update's top_k (colliders.py:71-85) is index work: the
  cells every step's contacts use (`Info.contact_cell`, the culled group's
  Info rows in top_k order) against the reference's own top_k indices
  recorded per step and env by oracle/gen_golden.py (`nn_cell`, `nn_sim`),
  on the kernel variants that cull (item loops, MULTI)."""
  from tests.helpers import set_variant
  sys_ = _system(name, dev)
  if variant is not None:
    rc = set_variant(sys_, variant)
    if rc != 0:
      pytest.skip(f'{name} does not fit the {variant} kernel')
  T = golden('traj_' + name)
  cut = [c for c in sys_.desc['col_cutoff'] if c > 0]
  assert len(cut) == 1  # one culled group in these scenes
  exact = 0
  for t in range(T['action'].shape[0]):
    _, info = sys_.step(_to_qp(T['qp'][t], dev),
                        torch.as_tensor(T['action'][t], dtype=torch.float32, device=dev))
    cells = info.contact_cell.cpu().numpy()
    for b in range(cells.shape[0]):
      sel = cells[b][cells[b] >= 0]
      exact += nn_cells_check(sel, T['nn_cell'][t][b], T['nn_sim'][t][b])
  assert exact > 0


def test_strided_views_match_packed(dev):
  """A QP of separate contiguous (B,N,3)/(B,N,4) tensors (the reference's own
  layout) steps to the same bits as the packed (B,N,16) layout."""
  from brax_amd.base import QP
  sys_ = _system('ant', dev)
  T = golden('traj_ant')
  packed = _to_qp(T['qp'][2], dev)
  split = QP(*(t.contiguous() for t in (packed.pos, packed.rot, packed.vel, packed.ang)))
  act = torch.as_tensor(T['action'][2], dtype=torch.float32, device=dev)
  a, _ = sys_.step(packed, act)
  b, _ = sys_.step(split, act)
  assert torch.equal(a.pos, b.pos) and torch.equal(a.ang, b.ang)


def test_unbatched_and_errors(dev):
  sys_ = _system('ant', dev)
  qp = sys_.default_qp()
  assert qp.pos.shape == (10, 3)
  out, info = sys_.step(qp, torch.zeros(8, device=dev))
  assert out.pos.shape == (10, 3) and info.contact.vel.shape == (10, 3)
  # a short action row clips like jp.take(mode='clip') (jumpy.py:151): index 7
  # reads element 6, so it equals the row padded with its last element
  a7 = torch.linspace(-1, 1, 7, device=dev)
  o7, _ = sys_.step(qp, a7)
  o8, _ = sys_.step(qp, torch.cat([a7, a7[-1:]]))
  assert torch.equal(o7.pos, o8.pos) and torch.equal(o7.ang, o8.ang)
  with pytest.raises(ValueError):  # batch mismatch
    qb = sys_.default_qp(joint_angle=torch.zeros(4, 8, device=dev),
                         joint_velocity=torch.zeros(4, 8, device=dev))
    sys_.step(qb, torch.zeros(3, 8, device=dev))


def test_capsule_capsule_kat(dev):
  """`colliders_test.py:100-115`: two parallel capsules (radius 0.05) at
  z = 0.15 and 0.2 penetrate by 0.05, contact at z = (0.15 + 0.2) / 2. With no
  gravity and a tiny dt the bodies do not move before contact generation."""
  import brax_amd
  cfg = """
    dt: 1e-6 substeps: 2 dynamics_mode: "pbd"
    bodies { name: "c1" mass: 1 inertia { x: 1 y: 1 z: 1 }
      colliders { capsule { radius: 0.05 length: 1.0 } rotation { y: 90 } } }
    bodies { name: "c2" mass: 1 inertia { x: 1 y: 1 z: 1 }
      colliders { capsule { radius: 0.05 length: 1.0 } rotation { y: 90 } } }
    defaults { qps { name: "c1" pos { z: 0.15 } } qps { name: "c2" pos { z: 0.2 } } }
  """
  s = brax_amd.System(cfg, device=dev)
  assert s.num_contacts == 1 and s.action_size == 0
  qp = s.default_qp()
  assert abs(float(qp.pos[1, 2]) - 0.2) < 1e-7
  _, info = s.step(qp, torch.zeros(0, device=dev))
  assert abs(float(info.contact_penetration[0]) - 0.05) < 1e-5
  np.testing.assert_allclose(info.contact_pos[0].cpu().numpy(), [0, 0, 0.175], atol=1e-5)


@pytest.mark.parametrize('kind', ['ground', 'capsule', 'cull'])
def test_capsule_scenes_kat(dev, kind):
  """The reference's CapsuleTest outcomes (`physics_test.py:330-361`, 2
  decimals): capsules come to rest on the ground and on each other, also
  with NearNeighbors culling at collider_cutoff = 1."""
  sys_ = _system('capsule_' + kind, dev)
  # default_qp(0 | 1) of the scene, as the reference built it
  qp = _to_qp(golden('traj_capsule_' + kind)['qp'][0][0], dev)
  qp, _ = sys_.step(qp, torch.zeros(0, device=dev))
  z = qp.pos[:, 2].cpu().numpy()
  if kind == 'ground':
    np.testing.assert_allclose(z[:4], [0.5, 0.25, 0.25, 0.25], atol=0.005)
  else:
    np.testing.assert_allclose(z[:2], [0.5, 1.25], atol=0.005)


@pytest.mark.parametrize('name', ['box_ground', 'box_slide', 'mesh_ground'])
def test_point_scenes_kat(dev, name):
  """Box corners / mesh vertices against the plane: the reference's BoxTest
  outcomes (`physics_test.py:67-83`, 2 decimals) and MeshTest's
  `test_mesh_hits_ground` (:392-408) on the inline hexagonal prism of
  oracle/scenes.py (half-height 0.1: it rests at z = 0.1). The starting
  state is `default_qp(default_index)` built on the device."""
  sys_ = _system(name, dev)
  di = 1 if name == 'box_slide' else 0
  qp = sys_.default_qp(di)
  q0 = golden('traj_' + name)['qp'][0][0]
  np.testing.assert_allclose(torch.cat([qp.pos, qp.rot, qp.vel, qp.ang], -1).cpu().numpy(),
                             q0, atol=1e-6)
  for _ in range(30 if name == 'mesh_ground' else 1):
    qp, info = sys_.step(qp, torch.zeros(0, device=dev))
  pos, vel = qp.pos[0].cpu().numpy(), qp.vel[0].cpu().numpy()
  if name == 'mesh_ground':
    assert abs(pos[2] - 0.1) < 0.005
    return
  assert abs(pos[2] - 0.5) < 0.005
  assert sys_.num_contacts == 8 and float(info.contact_penetration.max()) < 0.01
  if name == 'box_slide':
    assert 1 < pos[0] < 1.5 and abs(vel[0]) < 0.005


def test_culling_selects_nearest(dev, oracle_lib):
  """Ant Mountain(4) with collider_cutoff 36 (the published 9 per ant,
  `multiagent.ipynb`): same states as the float64 oracle's culled step, and
  no culled-out row acts."""
  import brax_amd
  from tests.helpers import config_for
  cfg = config_for('mountain4')
  cfg.collider_cutoff = 36
  sys_ = brax_amd.System(cfg, device=dev)
  assert sys_.num_contacts == 36 + 72
  qp = sys_.default_qp()
  B = 4
  from brax_amd.compiler import compile_reset
  vc, d, meta = brax_amd.compiler.compile_system(cfg)
  o = oracle_lib.Oracle(d, compile_reset(vc, meta['body_index']), np.float64)
  env32 = Envelope(oracle_lib, None, desc=(d, compile_reset(vc, meta['body_index'])))
  act = np.random.default_rng(5).uniform(-1, 1, (B, 32))
  qp_np = np.repeat(qp.numpy()[None], B, 0)
  for t in range(3):
    out, info = sys_.step(_to_qp(qp_np, dev), torch.as_tensor(act, dtype=torch.float32, device=dev))
    ref, rinfo = o.system_step(qp_np, act)
    outs = env32.system(qp_np, act)
    for f, sl in QP_FIELDS.items():
      e32 = _env_err([x[0][..., sl] for x in outs], ref[..., sl])
      _gate(out.numpy()[..., sl], ref[..., sl], e32, f)
    qp_np = ref


def _scene_system(text, dev):
  import brax_amd
  return brax_amd.System(text, device=dev)


def test_heightmap_kat(dev):
  """HeightMapTest (`physics_test.py:252-257`): the box falls onto the
  bottom-left quadrant of the height map and stays above z = 2."""
  from oracle import scenes
  sys_ = _scene_system(scenes.heightmap_config(), dev)
  qp = sys_.default_qp()
  qp, _ = sys_.step(qp, torch.zeros(0, device=dev))
  assert float(qp.pos[0, 2]) > 2.0


def test_clipped_plane_kat(dev):
  """CapsuleClippedPlaneTest (`physics_test.py:463-475`, 4 decimals): sphere 1
  rests on the clipped plane at z = 2, spheres 2 and 3 beside it on the
  ground."""
  from oracle import scenes
  sys_ = _scene_system(scenes.clipped_plane_config(), dev)
  qp, _ = sys_.step(sys_.default_qp(), torch.zeros(0, device=dev))
  np.testing.assert_allclose(qp.pos[:3, 2].cpu().numpy(), [2.5, 0.5, 0.5], atol=1.5e-4)


def test_box_capsule_kat(dev):
  """BoxCapsuleTest (`physics_test.py:207-225`, 2 decimals): boxes fall onto
  capsules and stay on them (unit and 10x mass), a capsule falls onto a frozen
  box. Its box-box (hull) pairs are far apart and never touch; the scene runs
  with them left out (oracle/scenes.py)."""
  from oracle import scenes
  sys_ = _scene_system(scenes.BOX_CAPSULE_NO_HULL_CONFIG, dev)
  qp = sys_.default_qp()
  for _ in range(30):
    qp, _ = sys_.step(qp, torch.zeros(0, device=dev))
  z = qp.pos[:, 2].cpu().numpy()
  assert abs(z[0] - 2.5) < 0.005 and abs(z[1] - 1.0) < 0.005
  assert z[2] >= 2.5 - 0.005 and abs(z[3] - 1.0) < 0.005
  assert abs(z[5] - 1.5) < 0.005


def test_mesh_capsule_kat(dev):
  """MeshTest's `test_mesh_hits_capsule` (`physics_test.py:409-423`) on the
  inline prism (half-height 0.1 at scale 0.1): the mesh comes to rest on the
  capsule (top at z = 0.4), not on the ground."""
  from oracle import scenes
  cfg = scenes.mesh_capsule_config().replace('z: 0.7 }', 'z: 1.5 }')
  sys_ = _scene_system(cfg, dev)
  qp = sys_.default_qp()
  for _ in range(30):
    qp, _ = sys_.step(qp, torch.zeros(0, device=dev))
  assert abs(float(qp.pos[0, 2]) - 0.5) < 0.01


def test_box_box_kat(dev):
  """BoxBoxTest (`physics_test.py:106-117`, 2 decimals): a box falls onto a
  box (hull-hull SAT contacts) and stays stacked, x-y unchanged."""
  from oracle import scenes
  sys_ = _scene_system(scenes.box_box_config(), dev)
  qp, _ = sys_.step(sys_.default_qp(), torch.zeros(0, device=dev))
  p = qp.pos.cpu().numpy()
  assert abs(p[0, 2] - 0.2) < 0.005 and abs(p[1, 2] - 0.5) < 0.005
  assert abs(p[1, 0] - 0.1) < 0.005 and abs(p[1, 1] - 1.0) < 0.005


def test_box_capsule_full_kat(dev):
  """BoxCapsuleTest as the reference runs it, its box-box hull pairs included
  (`physics_test.py:207-225`)."""
  from oracle import scenes
  sys_ = _scene_system(scenes.BOX_CAPSULE_TEST_CONFIG, dev)
  qp = sys_.default_qp()
  assert abs(float(qp.pos[0, 2]) - 3.5) < 0.005 and abs(float(qp.pos[2, 2]) - 3.5) < 0.005
  for _ in range(30):
    qp, _ = sys_.step(qp, torch.zeros(0, device=dev))
  z = qp.pos[:, 2].cpu().numpy()
  assert abs(z[0] - 2.5) < 0.005 and abs(z[1] - 1.0) < 0.005
  assert z[2] >= 2.5 - 0.005 and abs(z[3] - 1.0) < 0.005
  assert abs(z[5] - 1.5) < 0.005
