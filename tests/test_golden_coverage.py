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
* joint-limit census: dofs past their limit at each gated sample's input.

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


def fixtures_of(system):
  """The golden files the GPU gates load for `system`."""
  names = [env_golden(system)]
  if system in ROBOTS or system in ENV_TRAJ:
    names.append(sys_golden(system))
  if system + '_xy' in XY_ENVS:
    names.append(env_golden(system + '_xy'))
  if 'mid_' + system in MID + MID_ENV:
    names.append('mid_' + system)
  return sorted(set(names))


def test_env_traj_list_is_the_gates():
  from tests import test_gpu_parity
  assert ENV_TRAJ == test_gpu_parity.ENV_TRAJ


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
