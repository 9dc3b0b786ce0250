"""Which systems the Ant env kernels may resolve contacts for on the body
lanes (CB, pbd_features.h cb_feat; bx_blob.cpp cb_rows_ok), as build_plan
reports it under BX_PLAN_DEBUG: `contact_on_body=1` needs the body copies (JB)
and one collider group of one-way capsule-plane rows against bodies on no
joint side, at most one row per body. Every other system keeps the row-lane
passes: an Ant-kind system among them takes the all-kinds kernel.

bx_system_plan runs in child processes (the flag is printed to stderr by the
library, and BX_NO_JB is read from the environment)."""
import functools
import os
import re
import subprocess
import sys

import pytest

from brax_amd.envs import configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Ant with a second capsule on one foot: "$ Body 4" gets the mirror end of its
# own capsule, so that body is the a body of two ground rows
_FOOT = ('bodies { name: "$ Body 4" colliders { rotation { x: 90 y: -45 } '
         'capsule { radius: 0.08 length: 0.7256854 end: -1 } }')
_FOOT2 = _FOOT + (' colliders { rotation { x: 90 y: -45 } '
                  'capsule { radius: 0.08 length: 0.7256854 end: 1 } }')


def two_row_ant_config():
  assert configs.ANT_CONFIG.count(_FOOT) == 1
  return configs.ANT_CONFIG.replace(_FOOT, _FOOT2)


_CHILD = r"""
import sys
from brax_amd import config as cfgmod
from brax_amd.system import System
from tests.helpers import config_for
from tests.test_plan_contact_body import two_row_ant_config
for name in sys.argv[1:]:
  cfg = cfgmod.parse(two_row_ant_config()) if name == 'ant_two_rows' else config_for(name)
  sys.stderr.write(f'plan of {name}\n')
  sys.stderr.flush()
  System.plan(cfg)
"""


@functools.lru_cache(maxsize=None)
def _flags(names, no_jb):
  env = dict(os.environ, BX_PLAN_DEBUG='1', PYTHONPATH=ROOT)
  env.pop('BX_NO_JB', None)
  if no_jb:
    env['BX_NO_JB'] = '1'
  r = subprocess.run([sys.executable, '-c', _CHILD, *names], env=env, cwd=ROOT, text=True,
                     capture_output=True, timeout=120)
  assert r.returncode == 0, r.stderr[-2000:]
  out = {}
  for part in r.stderr.split('plan of ')[1:]:
    name = part.split('\n', 1)[0]
    m = re.findall(r'contact_on_body=(\d)', part)
    assert len(m) == 1, (name, part)
    out[name] = int(m[0])
  return out


NAMES = ('ant', 'ant_two_rows', 'halfcheetah', 'humanoid')


@pytest.mark.parametrize('name,want', [('ant', 1), ('ant_two_rows', 0), ('halfcheetah', 0),
                                       ('humanoid', 0)])
def test_contact_on_body_flag(name, want):
  assert _flags(NAMES, False)[name] == want


def test_no_body_copies_no_contact_on_body():
  """BX_NO_JB=1: without the body copies there is nothing to resolve the row
  from."""
  assert _flags(('ant',), True)['ant'] == 0


def test_two_row_ant_has_two_rows_on_one_body():
  """The variant's own precondition: six rows, two of them on the foot."""
  from brax_amd import compiler
  from brax_amd import config as cfgmod
  _, d, meta = compiler.compile_system(cfgmod.parse(two_row_ant_config()))
  a = list(d['row_body_a'])
  foot = meta['body_index']['$ Body 4']
  assert len(a) == 6 and a.count(foot) == 2, a
  _, d0, _ = compiler.compile_system(cfgmod.parse(configs.ANT_CONFIG))
  assert len(d0['row_body_a']) == 5 and len(set(d0['row_body_a'])) == 5
