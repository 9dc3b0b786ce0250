"""The host blob of every system the tests know, bit for bit: n_words, the
eight plan integers, the sha256 of the words and one per blob section
(tests/golden/blob_fingerprints.json, written by
tools/record_blob_fingerprints.py from the builder before it was split into
stages; a change to the builder that moves a word fails here, on the CPU,
and names the section)."""
import json

import pytest

from tests import blob_cases as bc

FIX = json.load(open(bc.FIXTURE))
_seen = {}  # case id -> (fingerprint, header)


def _run(case, monkeypatch):
  if case[0] not in _seen:
    for k in bc.KNOBS:
      monkeypatch.delenv(k, raising=False)
    for k, v in case[3].items():
      monkeypatch.setenv(k, v)
    words, plan = bc.case_blob(case)
    _seen[case[0]] = (bc.fingerprint(words, plan), bc.header(words))
  return _seen[case[0]]


def test_fixture_holds_exactly_the_cases():
  assert sorted(FIX) == sorted(bc.CASE_IDS)


@pytest.mark.parametrize('case', bc.CASES, ids=bc.CASE_IDS)
def test_blob_matches_its_fingerprint(case, monkeypatch):
  got, _ = _run(case, monkeypatch)
  want = FIX[case[0]]
  moved = [s for s in sorted(set(got['sections']) | set(want['sections']))
           if got['sections'].get(s) != want['sections'].get(s)]
  assert not moved, f'sections that moved: {moved}'
  assert got == want


def test_capacity_too_small_is_an_error():
  import ctypes as C
  from brax_amd import _native, abi
  from tests.helpers import compiled
  _, desc, _, _ = compiled('ant')
  cd, keep = abi.make_desc(desc)
  n, plan, buf = C.c_int64(), (C.c_int32 * 8)(), (C.c_uint32 * 4)()
  lib = _native.lib()
  assert lib.bx_system_blob(C.byref(cd), None, buf, 4, C.byref(n), plan) != 0
  assert b'capacity' in lib.bx_last_error() and n.value > 4
  assert lib.bx_system_blob(None, None, None, 0, C.byref(n), plan) != 0
  assert b'null' in lib.bx_last_error()
  del keep


def test_cases_reach_every_plan_branch(monkeypatch):
  """From the plan integers and header fields of the cases themselves."""
  F = bc.features()
  runs = [_run(c, monkeypatch) for c in bc.CASES]
  plans = [dict(zip(('mode', 'lanes', 'lds_bytes', 'feat', 'gw', 'fold', 'jb', 'cb'), fp['plan']))
           for fp, _ in runs]
  hdrs = [h for _, h in runs]
  secs = [fp['sections'] for fp, _ in runs]
  empty = bc._sha([])
  for f in ('F_JH', 'F_R2', 'F_R2G', 'F_C16', 'F_SPH', 'F_FORCE', 'F_X'):
    assert any(p['feat'] & F[f] for p in plans), f
  assert any(p['feat'] & F['F_R2'] and not p['feat'] & F['F_R2G'] for p in plans)
  assert any(p['jb'] == 1 and p['cb'] == 1 for p in plans)
  assert any(p['jb'] == 1 and p['cb'] == 0 for p in plans)
  assert any(p['jb'] == 0 and p['feat'] & F['F_JH'] for p in plans)
  assert any(p['fold'] == 0 for p in plans) and any(p['fold'] == 1 for p in plans)
  assert {p['mode'] for p in plans} == {0, 1, 3}
  assert {p['gw'] for p in plans} == {4, 8}
  assert {16, 32, 64, 128, 256} <= {p['lanes'] for p in plans}
  assert {128, 256} <= {h['multi_L'] for p, h in zip(plans, hdrs) if p['mode'] == 3}
  assert any(h['o_mjh'] != 0 for h in hdrs)
  assert any(h['multi'] and h['o_mjh'] == 0 for h in hdrs)
  assert any(h['multi'] == 0 and h['L'] > 64 for h in hdrs)  # a large scene on the item loops
  assert any(h['n_nn'] > 0 for h in hdrs)
  assert any(h['spring'] == 1 for h in hdrs)
  assert any(h['l_jlim'] != 0 for h in hdrs) and any(h['single'] and h['l_jlim'] == 0 for h in hdrs)
  assert any(h['o_base'] == 0 for h in hdrs)  # reset = NULL
  for s in ('o_hull', 'o_hm', 'o_force', 'o_bimg', 'o_cen', 'o_lane', 'o_zpt'):
    assert any(x.get(s, empty) != empty for x in secs), s
