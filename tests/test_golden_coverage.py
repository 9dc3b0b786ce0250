"""What the committed goldens exercise, counted on the CPU.

The GPU parity gates (tests/test_gpu_parity.py) are only as strong as the
states under tests/golden/: a contact row that never penetrates in any
fixture has never been compared with the reference while it did anything.
This census reads the recorded reference arrays and the C oracle (never a
kernel) and keeps the gap closed:

* contact census: for every system of the env gates, over the union of the
  fixtures the GPU gates load for it, the (step, env) samples in which some
  row of each collider group penetrates;
* the per-row conditions the mid-episode fixtures (`mid_*`,
  oracle/mid_states.py) were recorded for, and the share of their active
  samples that is well conditioned under the gate's own fp32 envelope;
* joint-limit census: dofs past their limit at each gated sample's input;
* gate membership: every counted file is in the parameter list of the GPU
  gate it is credited to, read off the gate itself;
* model gaps: the float64 oracle's env step against every fixture the env
  gate loads, equal to 1e-9 but for an exact, explained list (the target
  envs' teleport), so that a large fp32 envelope in the gates can only mean
  rounding; and `mid_grasp`'s ill-conditioned samples once the teleported
  target is out: none on the state, one on Info.contact.

The table goes to golden_coverage.json in the suite's output directory
(tests/test_gpu_parity.py `out_dir`, beside parity_margins.json).
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, golden
from tests.helpers import (ENVTRAJ_KERNEL, MID, MID_ENV, ROBOTS, SPRING_ENVS, XY_ENVS, compiled, env_golden,
                           env_kind, sys_golden)

# tests/test_gpu_parity.py ENV_TRAJ (not imported at collection: that module
# needs torch only for its GPU tests, but its list is restated here so the
# census cannot silently follow a shrinking gate list)
ENV_TRAJ = ['ant', 'humanoid', 'halfcheetah', 'humanoidstandup'] + SPRING_ENVS
SYSTEMS = ENV_TRAJ + ENVTRAJ_KERNEL
MIN_SAMPLES = 8
# envelope copies per oracle build for the well-conditioned share: the GPU
# gates' own default (BX_ENVELOPE_N = 32). 5 fixtures x 2 steps x 8 envs x 66
# realisations of the C oracle take about a second.
ENVELOPE_N = 32


def credited(system):
  """(golden file, gate, the name the gate's parameter list has it under) of
  everything the census counts for `system`; gate 'env' is
  test_env_step_vs_golden, 'sys' test_system_step_vs_golden. A mid-episode
  file serves both."""
  out = [(env_golden(system), 'env', system)]
  if system in ROBOTS or system in ENV_TRAJ:
    out.append((sys_golden(system), 'sys', system))
  if system + '_xy' in XY_ENVS:
    out.append((env_golden(system + '_xy'), 'env', system + '_xy'))
  if 'mid_' + system in MID + MID_ENV:
    out += [('mid_' + system, 'env', 'mid_' + system), ('mid_' + system, 'sys', 'mid_' + system)]
  return out


def fixtures_of(system):
  """The golden files the GPU gates load for `system`."""
  return sorted({f for f, _, _ in credited(system)})


def test_env_traj_list_is_the_gates():
  from tests import test_gpu_parity
  assert ENV_TRAJ == test_gpu_parity.ENV_TRAJ


def gate_names(fn):
  """The golden names a GPU gate runs on the kernel it selects by itself: the
  `name` list of its own `pytest.mark.parametrize` without the forced-variant
  cases (`name:variant`), which come on top of a name and do not stand in
  for it."""
  (mark,) = [m for m in fn.pytestmark if m.name == 'parametrize']
  assert mark.args[0] == 'name'
  plain = {n for n in mark.args[1] if ':' not in n}
  lone = {n.partition(':')[0] for n in mark.args[1]} - plain
  assert not lone, f'{fn.__name__}: forced-variant cases of {sorted(lone)} without the plain name'
  return plain


def test_counted_fixtures_are_in_their_gates():
  """Every file `fixtures_of` credits to a system is loaded by the gate it is
  credited to, read off the gates' own parameter lists: the env-layer files
  by test_env_step_vs_golden, the System.step files by
  test_system_step_vs_golden, a mid-episode file by both (one file serves
  the two gates). A fixture dropped from a gate list fails here instead of
  still being counted."""
  from tests import test_gpu_parity
  names = {'env': gate_names(test_gpu_parity.test_env_step_vs_golden),
           'sys': gate_names(test_gpu_parity.test_system_step_vs_golden)}
  load = {'env': env_golden, 'sys': sys_golden}
  for system in SYSTEMS:
    for f, gate, name in credited(system):
      assert name in names[gate] and load[gate](name) == f, (
          f'{f} is counted for {system}, but the {gate} gate\'s list has no {name!r} to load it')
  for name in MID + MID_ENV:  # whether or not a system of the census claims them
    assert name in names['env'] and name in names['sys'], name


@pytest.fixture(scope='module')
def table(oracle_lib):
  from oracle import mid_states
  rows = {}
  for system in SYSTEMS:
    _, d, rd, _ = compiled(system)
    o64 = oracle_lib.Oracle(d, rd, np.float64)
    group = np.asarray(d['row_group'])
    entry = {'fixtures': {}, 'groups': {}, 'rows_never_active': None}
    active_rows = np.zeros(len(group), bool)
    per_group = {int(g): 0 for g in np.unique(group)}
    samples = 0
    for f in fixtures_of(system):
      T = golden(f)
      pen = T['contact_penetration'] > 0  # (T, B, R)
      steps, B = pen.shape[:2]
      samples += steps * B
      assert pen.shape[2] == len(group), (f, pen.shape)
      active_rows |= pen.any((0, 1))
      for g in per_group:
        per_group[g] += int(pen[..., group == g].any(-1).sum())
      lim = np.stack([mid_states.past_limit(o64, T['qp'][t], mid_states.LIMIT_MARGIN).sum((1, 2))
                      for t in range(steps)])
      entry['fixtures'][f] = {'samples': steps * B,
                              'samples_with_dof_past_limit': int((lim > 0).sum()),
                              'dofs_past_limit': int(lim.sum())}
    entry['samples'] = samples
    entry['groups'] = {str(g): n for g, n in per_group.items()}
    entry['rows_never_active'] = np.flatnonzero(~active_rows).tolist()
    rows[system] = entry
  for name in MID + MID_ENV:
    system = env_kind(name)
    T = golden(name)
    pen, well, dec, _ = mid_states.census(oracle_lib, system, T, n_perturb=ENVELOPE_N)
    tr = T['row_target']
    act = pen[..., tr].any(-1)
    rows[system]['mid'] = {
        'fixture': name, 'row_target': tr.tolist(),
        'target_rows_active': tr[pen[..., tr].any((0, 1))].tolist(),
        'target_rows_active_decided_well': tr[(pen[..., tr] & dec[..., tr]
                                               & well[..., None]).any((0, 1))].tolist(),
        'samples_per_target_row': pen[..., tr].sum((0, 1)).tolist(),
        'active_samples': int(act.sum()), 'active_well_conditioned': int((act & well).sum()),
        'envelope_n': ENVELOPE_N, 'comment': str(T['comment'])}
  from tests.test_gpu_parity import out_dir
  with open(os.path.join(out_dir(), 'golden_coverage.json'), 'w') as f:
    json.dump(rows, f, indent=1)
  print()
  print(f'{"system":28s} {"samples":>7s}  groups (active samples)  dofs past limit (samples)')
  for system, e in rows.items():
    jl = sum(x['samples_with_dof_past_limit'] for x in e['fixtures'].values())
    print(f'{system:28s} {e["samples"]:7d}  {e["groups"]}  {jl}')
  return rows


# The one exemption. halfcheetah_spring is in the census list (it is in
# ENV_TRAJ), its only fixture is traj_halfcheetah_spring (3 steps x 8 envs,
# from reset), and the mid-episode fixtures are not to be recorded for the
# spring variants of halfcheetah and humanoidstandup: the two requirements
# conflict for this one system. Its counts are pinned, not excused: plane
# group 0 on 7 of 24 samples, the feet's capsule-capsule group 1 on none. The
# test fails when either changes (a fixture closes it: drop the entry) and
# for every other system the bound holds without exception.
OPEN_GAPS = {('halfcheetah_spring', '0'): 7, ('halfcheetah_spring', '1'): 0}


@pytest.mark.parametrize('system', SYSTEMS)
def test_every_collider_group_is_exercised(table, system):
  e = table[system]
  need = min(MIN_SAMPLES, e['samples'])
  for g, n in e['groups'].items():
    if (system, g) in OPEN_GAPS:
      assert n == OPEN_GAPS[(system, g)] < need, (system, g, n)
      continue
    assert n >= need, (f'{system}: collider group {g} penetrates in {n} of {e["samples"]} '
                       f'gated samples ({sorted(e["fixtures"])})')


@pytest.mark.parametrize('name', MID)
def test_mid_fixture_shape_and_keys(name):
  """8 envs, 2 steps, the keys of the sibling fixture plus row_target."""
  T, S = golden(name), golden(env_golden(env_kind(name)))
  assert set(S.files) | {'row_target', 'comment'} == set(T.files)
  assert T['action'].shape[:2] == (2, 8) and T['qp'].shape[:2] == (3, 8)
  for k in S.files:
    assert T[k].shape[2:] == S[k].shape[2:] or T[k].ndim < 3, k
  assert np.all(np.isfinite(T['qp'])) and np.all(np.isfinite(T['obs']))
  assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < 1 << 20


def test_mid_row_conditions(table):
  m = {s: e['mid'] for s, e in table.items() if 'mid' in e}
  assert sorted('mid_' + s for s in m) == sorted(MID + MID_ENV)
  # Pusher: the two-way capsule-capsule rows 16..22; at least 4 distinct
  assert m['pusher']['row_target'] == list(range(16, 23))
  assert len(m['pusher']['target_rows_active']) >= 4
  # Hopper: both ground rows of the foot; Walker2d: both feet
  assert m['hopper']['target_rows_active'] == [6, 7]
  assert m['walker2d']['target_rows_active'] == [7, 13]
  # HalfCheetah: the feet's capsule-capsule row on at least 4 env-samples
  assert m['halfcheetah']['row_target'] == [16]
  assert m['halfcheetah']['samples_per_target_row'][0] >= 4
  # HumanoidStandup: at least 6 of the 15 rows no other fixture activates
  assert len(m['humanoidstandup']['row_target']) == 15
  assert len(m['humanoidstandup']['target_rows_active']) >= 6
  # Grasp: the Object - palm row (group 1) and the four Object - fingertip
  # rows (group 2); both groups are held to the bound above
  assert m['grasp']['row_target'] == [2, 3, 4, 5, 6]
  assert 2 in m['grasp']['target_rows_active'] and len(m['grasp']['target_rows_active']) >= 3
  for s, e in m.items():
    # the target rows are the rows no OTHER fixture of the system activates
    other = np.zeros(golden('mid_' + s)['contact_penetration'].shape[-1], bool)
    for f in fixtures_of(s):
      if f != 'mid_' + s:
        other |= (golden(f)['contact_penetration'] > 0).any((0, 1))
    assert not other[e['row_target']].any(), s
    # at least half of the samples with an active target row are well
    # conditioned (2 x E32 <= WIDE on every gated field, the oracle alone)
    assert e['active_samples'] > 0
    assert 2 * e['active_well_conditioned'] >= e['active_samples'], (s, e)
    # and the pattern assertion of the GPU gates has something to hold
    assert e['target_rows_active_decided_well'], s


@pytest.mark.parametrize('system', ['hopper', 'walker2d', 'halfcheetah', 'pusher'])
def test_mid_fixture_reaches_a_joint_limit(table, system):
  f = table[system]['fixtures']['mid_' + system]
  assert f['samples_with_dof_past_limit'] >= 1, f


# ---------------------------------------------------------------------------
# model gaps: where the float64 oracle and the recorded reference are not the
# same model. The GPU gates read a large fp32 envelope as ill-conditioning (a
# contact flipping on rounding) and fall back to the nearest fp32 realisation;
# that reading is only right where the float64 oracle itself reproduces the
# recorded arrays. Every place where it does not is listed here, with its
# cause, and the list is exact.
# ---------------------------------------------------------------------------
GAP_TOL = 1e-9  # normwise; float64 rounding order over a step's substeps (tests/test_oracle.py)
_TELEPORT = ('the env teleports a hit target after the observation is taken; the reference '
             'draws the spot from its JAX key and the oracle does not restate the teleport '
             '(tests/helpers.py TELEPORTS): the samples are exactly the recorded hits')
# (fixture, what: (array, field, body, ((step, env), ...)), why)
MODEL_GAPS = [
    ('mid_grasp', ('qp', 'pos', 'Target', ((0, 4), (0, 8))), _TELEPORT),
    ('envtraj_grasp', ('qp', 'pos', 'Target', tuple((0, e) for e in range(8))), _TELEPORT),
]
# Not a gap: with the safe-norm guard on (jumpy.py:183-189, the zero guard of
# the jit path: oracle.Oracle's default, and what oracle/mid_states.py scores
# candidates under) the float64 oracle is 1.97e-5 (qp) / 1.6e-5 (obs) from
# envtraj_ur5e on envs 0, 5, 6 at step 0 and env 6 at step 2, and 5.5e-7 from
# envtraj_pusher on env 4 at step 3: a norm whose components are all under
# 1e-8 is flushed to 0 there. The goldens are the reference's numpy execution,
# which has no such guard (jumpy.py:190); without it (as tests/test_oracle.py
# runs the oracle, and as below) both fixtures agree to 1e-9.


def env_gate_fixtures():
  """(golden name, file) of every fixture test_env_step_vs_golden loads."""
  from tests import test_gpu_parity
  names = sorted(gate_names(test_gpu_parity.test_env_step_vs_golden))
  return [(n, env_golden(n)) for n in names]


def test_model_gaps_are_exactly_the_listed_ones(oracle_lib):
  """The float64 oracle's env step from every recorded state of every fixture
  the env gate loads: next state (per body and field), obs, reward, done and
  metrics equal the recorded arrays to 1e-9 normwise, except for MODEL_GAPS;
  an entry that is no longer needed fails, a new one fails."""
  from tests.helpers import QP_FIELDS, env_coef, normwise, obs_flags, prep_oracle, teleported
  found = {}
  for name, f in env_gate_fixtures():
    _, d, rd, meta = compiled(name)
    bodies = {i: b for b, i in meta['body_index'].items()}
    # the numpy backend's plain norm: the execution the goldens come from
    o = prep_oracle(oracle_lib.Oracle(d, rd, np.float64, safe_guard=False), name)
    T = golden(f)
    O, M = T['obs'].shape[-1], T['metrics'].shape[-1]
    for t in range(T['action'].shape[0]):
      qp, obs, rew, done, met = o.env_step(env_kind(name), T['qp'][t], T['action'][t], O, M,
                                           obs_flags=obs_flags(name),
                                           coef=env_coef(env_kind(name)))
      ref = T['qp'][t + 1]
      for fld, sl in QP_FIELDS.items():
        scale = np.maximum(1.0, np.abs(ref[..., sl]).max((1, 2)))
        err = np.abs(qp[..., sl] - ref[..., sl]).max(-1) / scale[:, None]  # (B, N)
        for e, b in zip(*np.nonzero(err > GAP_TOL)):
          found.setdefault((f, 'qp', fld, bodies[int(b)]), []).append((t, int(e)))
      flat = {'obs': normwise(obs, T['obs'][t + 1]),
              'reward': normwise(rew[:, None], T['reward'][t][:, None]),
              'done': (done != T['done'][t]).astype(float)}
      if M:
        flat['metrics'] = normwise(met, T['metrics'][t])
      for k, v in flat.items():
        for e in np.flatnonzero(v > GAP_TOL):
          found.setdefault((f, k, None, None), []).append((t, int(e)))
  found = sorted((f, (a, fld, b, tuple(sorted(s)))) for (f, a, fld, b), s in found.items())
  assert found == sorted((f, what) for f, what, _ in MODEL_GAPS)
  # the listed cause, checked: the samples are the recorded hits, all of them
  for f, (_, _, body, samples), why in MODEL_GAPS:
    if why is _TELEPORT:
      name = next(n for n, g in env_gate_fixtures() if g == f)
      tbody, thit = teleported(name, golden(f))
      assert compiled(name)[3]['body_index'][body] == tbody
      assert sorted(zip(*map(np.ndarray.tolist, np.nonzero(thit)))) == sorted(samples), f
  # and the other target envs' fixtures record no hit at all
  for name, f in env_gate_fixtures():
    tbody, thit = teleported(name, golden(f))
    if tbody is not None and f not in [g for g, _, _ in MODEL_GAPS]:
      assert not thit.any(), f


@pytest.fixture(scope='module')
def grasp_layers(oracle_lib):
  """mid_grasp under the GPU gates' own rule, the oracle alone: per layer
  ('env': the env step on the recorded arrays; 'sys': System.step on
  `pre_step` of them) and step, the envelope's realisations and the recorded
  reference, the teleported target's pos taken out of both as the gates do."""
  from oracle import mid_states
  from tests.helpers import Envelope, env_coef, teleported, without_teleported
  name = 'mid_grasp'
  T = golden(name)
  meta = compiled(name)[3]
  env32 = Envelope(oracle_lib, name, n_perturb=ENVELOPE_N)
  O, M = T['obs'].shape[-1], T['metrics'].shape[-1]
  tbody, thit = teleported(name, T)
  A = int(compiled(name)[1]['action_size'])
  out = {'env': [], 'sys': [], 'T': T, 'hit': thit}
  for t in range(T['action'].shape[0]):
    ref = without_teleported(T['qp'][t + 1], tbody, thit[t])
    eo = env32.env('grasp', T['qp'][t], T['action'][t], O, M, 0, env_coef('grasp'))
    out['env'].append({
        'ref': {'qp': ref, 'obs': T['obs'][t + 1], 'reward': T['reward'][t][:, None],
                'metrics': T['metrics'][t]},
        'runs': [{'qp': without_teleported(x[0], tbody, thit[t]), 'obs': x[1],
                  'reward': x[2][:, None], 'metrics': x[4], 'qp_raw': x[0]} for x in eo]})
    sq, sa = mid_states.pre_step('grasp', meta, T['qp'][t], T['action'][t])
    so = env32.system(sq, sa[:, :A])
    keys = ('contact_pos', 'contact_normal', 'contact_penetration')
    out['sys'].append({
        'ref': dict({'qp': ref, 'contact': T['info_contact'][t]}, **{k: T[k][t] for k in keys}),
        'runs': [dict({'qp': without_teleported(x[0], tbody, thit[t]),
                       'contact': x[1]['contact']}, **{k: x[1][k] for k in keys}) for x in so]})
  return out


def _e32(layer_step):
  """{gated field: E32 per env} of one layer's step, as the gates split it."""
  from tests.helpers import QP_FIELDS, normwise
  ref, runs = layer_step['ref'], layer_step['runs']
  out = {}
  for k, r in ref.items():
    parts = QP_FIELDS.items() if k == 'qp' else [(None, Ellipsis)]
    for fld, sl in parts:
      rr = r[..., sl] if fld else r
      out[k if fld is None else 'qp_' + fld] = np.max(
          [normwise(x[k][..., sl] if fld else x[k], rr) for x in runs], axis=0)
  return out


# mid_grasp's samples whose bound 2 x E32 exceeds WIDE with the teleport out,
# (layer, step, gated field, env): one, and not on the state. On env 11 at step
# 0 the Object rests on the ground (rows 0 and 1 penetrate, no target row
# does), and the fp32 runs fall on two branches: about a quarter of the 66 sum
# 0.195 more or less into the Object's Info.contact (17.8) than the reference,
# 1.09e-2 normwise, the others agree to 2e-4: a contact gate of one substep
# deciding on rounding, which is what `ill-conditioned` is for. The same
# sample's next state stays within 1e-3. The system gate holds that one
# Info.contact entry to the nearest realisation, and `_pattern_gate` leaves
# the sample out (none of its target rows penetrates anyway).
MID_GRASP_ILL = [('sys', 0, 'contact', 11)]


def test_mid_grasp_is_well_conditioned_once_the_teleport_is_out(grasp_layers):
  """With the teleported target's pos out, no sample of mid_grasp is
  ill-conditioned (2 x E32 > WIDE) on any state field, obs, reward or metric
  of either layer at the gates' own envelope size, and over every gated field
  the ill-conditioned samples are exactly MID_GRASP_ILL: the gates'
  nearest-realisation branch, which compares with Brax's fp32 runs rather
  than the reference, cannot absorb a kernel error on this fixture's state
  without this list changing. Every realisation agrees with the reference on
  `hits`, so the env gate may assert that metric exactly. Without the mask
  the recorded hits, and only they, read as ill-conditioned `qp_pos`: the old
  failure."""
  from tests.helpers import QP_FIELDS, WIDE, normwise
  T, thit = grasp_layers['T'], grasp_layers['hit']
  k = [str(x) for x in T['metric_keys']].index('hits')
  worst, ill = {}, []
  for layer in ('env', 'sys'):
    for t, st in enumerate(grasp_layers[layer]):
      for f, e in _e32(st).items():
        ill += [(layer, t, f, int(b)) for b in np.flatnonzero(2.0 * e > WIDE)]
        worst[f] = max(worst.get(f, 0.0), float(e.max()))
      if layer == 'env':
        for x in st['runs']:
          assert np.array_equal(x['metrics'][:, k], T['metrics'][t][:, k]), t
  print('mid_grasp largest E32 per gated field:', {f: f'{v:.2e}' for f, v in worst.items()})
  assert ill == MID_GRASP_ILL
  # unmasked, as the env gate ran before: exactly the hit samples
  sl = QP_FIELDS['pos']
  for t in range(thit.shape[0]):
    raw = [x['qp_raw'][..., sl] for x in grasp_layers['env'][t]['runs']]
    ref = T['qp'][t + 1][..., sl]
    e = np.max([normwise(q, ref) for q in raw], axis=0)
    assert np.array_equal(2.0 * e > WIDE, thit[t]), t
    if thit[t].any():
      # and no rounding: the runs agree with each other, far from the reference
      spread = np.max([normwise(q, raw[0]) for q in raw], axis=0)
      assert spread[thit[t]].max() < 1e-5 and e[thit[t]].min() > 0.1


def test_mid_grasp_pattern_gate_has_work_on_every_target_row(grasp_layers):
  """The system gate's `_pattern_gate` compares a target row on a sample when
  the sample is well-conditioned on every gated field and the row's contact
  test is decided (every realisation agrees with the reference on
  `penetration > 0`): every one of rows 2..6 has such a penetrating entry."""
  from tests.helpers import WIDE
  T = grasp_layers['T']
  rows = T['row_target']
  n = np.zeros(len(rows), int)
  per_step = []
  for t, st in enumerate(grasp_layers['sys']):
    well = 2.0 * np.max(list(_e32(st).values()), axis=0) <= WIDE
    ref_on = st['ref']['contact_penetration'][:, rows] > 0
    dec = np.all([(x['contact_penetration'][:, rows] > 0) == ref_on for x in st['runs']], axis=0)
    on = dec & ref_on & well[:, None]
    n += on.sum(0)
    per_step.append(int(on.sum()))
  print('mid_grasp decided, well-conditioned, penetrating target-row entries per step:',
        per_step, 'per row:', dict(zip(rows.tolist(), n.tolist())))
  assert (n > 0).all(), dict(zip(rows.tolist(), n.tolist()))
