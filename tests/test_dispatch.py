"""Which kernel a SINGLE-mode system gets, pinned on the host (no GPU, no HIP):
tests/dispatch_grid.cpp prints the decisions of brax_amd/csrc/pbd_dispatch.h
over a grid of (lanes, features, gather width, env kind, fold bits), and
tests/golden/dispatch_decisions.txt holds what the five launchers chose when
each spelled the conditions out by hand."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'dispatch_decisions.txt')
VARIANT_LIST = ['-'] * 5  # step, policy, eval_policy, eval_open, population


@pytest.fixture(scope='module')
def grid(tmp_path_factory):
  cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  exe = str(tmp_path_factory.mktemp('dispatch') / 'dispatch_grid')
  subprocess.run([cxx, '-std=c++17', '-O0', '-o', exe, os.path.join(ROOT, 'tests', 'dispatch_grid.cpp')],
                 check=True)
  out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
  return [l.split() for l in out.splitlines()]


@pytest.fixture(scope='module')
def recorded():
  with open(FIXTURE) as f:
    return [l.split() for l in f if l.strip() and not l.startswith('#')]


def test_the_grid_is_the_one_asked_for(grid):
  kind = [r for r in grid if r[0] == 'kind']
  assert {r[1] for r in kind} == {'16', '32', '64'}
  assert {r[3] for r in kind} == {'4', '8'}
  assert {r[4] for r in kind} == {'ant', 'humanoid', 'humanoidstandup', 'halfcheetah', 'pusher', 'hopper'}
  assert {r[5] for r in kind} == {'0', '1', '3', '5', '7'}
  # the 18 feature sets of BX_SINGLE16_VARIANTS and the five env-kind masks
  # with and without F_G1 (32): Ant 160, Humanoid 33, HalfCheetah 1420, Pusher
  # 1932, HumanoidStandup 289
  feats = {int(r[2]) for r in kind}
  assert len(feats) >= 18
  for m in (160, 33, 1420, 1932, 289):
    assert {m | 32, m & ~32} <= feats
  assert len(kind) == 3 * len(feats) * 2 * 6 * 5


def test_kind_kernels_are_the_recorded_ones(grid, recorded):
  """Every grid point where some family took an env kind's own kernel takes
  the same (F, M, EK) in the same families; every other point takes the
  variant list in all five."""
  want = [r for r in recorded if r[0] == 'kind']
  assert len(want) > 0
  got = [r for r in grid if r[0] == 'kind' and r[6:] != VARIANT_LIST]
  assert got == want
  rest = [r for r in grid if r[0] == 'kind' and r[:6] not in [w[:6] for w in want]]
  assert len(rest) + len(want) == len([r for r in grid if r[0] == 'kind'])
  assert all(r[6:] == VARIANT_LIST for r in rest)


def test_humanoid_kernels_only_in_the_step_and_open_loop_families(grid, recorded):
  for rows in (grid, recorded):
    hum = [r for r in rows if r[0] == 'kind' and any(c.endswith('/2') for c in r[6:])]
    assert hum
    for r in hum:
      step, policy, eval_policy, eval_open, population = r[6:]
      assert step == eval_open and step.endswith('/2')
      assert [policy, eval_policy, population] == ['-'] * 3


def test_ant_wide_rule(grid, recorded):
  want = [r for r in recorded if r[0] == 'wide']
  assert [r for r in grid if r[0] == 'wide'] == want
  # below, at and above 4 workgroups per compute unit, for 32 and 64 threads
  assert {(r[2], r[3]) for r in want} >= {('32', '256'), ('64', '256')}
  for r in want:
    assert int(r[4]) == (int(r[1]) > 4 * int(r[3]))


def test_step_family_kernel_names(grid, recorded):
  want = [r for r in recorded if r[0] == 'step_kernel']
  assert len(want) == 7 * 3 * 2
  assert [r for r in grid if r[0] == 'step_kernel'] == want


def test_every_decision_is_instantiated(grid):
  """dispatch_grid.cpp prints `bad` for a kind_variant() result outside
  BX_KIND_VARIANTS (or outside its family), a single_variant() result outside
  BX_SINGLE_VARIANTS, and a fold_bits() value off the launchers' bits."""
  assert [r for r in grid if 'bad' in r] == []
  assert {r[0] for r in grid} == {'kind', 'wide', 'step_kernel'}
