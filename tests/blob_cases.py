"""The systems whose host blobs tests/golden/blob_fingerprints.json pins, and
a blob's fingerprint; shared by tests/test_blob_fingerprint.py and
tools/record_blob_fingerprints.py.

A case is (id, system name, variant words, env knobs). Variants: '' (the
system's own descriptor and reset descriptor), 'noreset' (reset = NULL),
'materials' (every contact row its own friction: past the MULTI kernel's 255
materials, tests/test_plan.py), 'forces' (one thruster on body 0),
'sparse' (Ant Mountain with only the bodies' ground pairs and the first Ant's
pairs with the second; nine Ants' 72 joints as joint halves are past 128 lanes,
so the MULTI kernel runs at 256 threads per env; past 49 bodies the reset
kernel's LDS is full, so without reset tables)."""
import hashlib
import os
import re

import numpy as np

from brax_amd import compiler
from brax_amd import config as cfgmod
from brax_amd.envs import configs
from brax_amd.system import desc_blob
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'blob_fingerprints.json')
# build_plan's A/B knobs, read at call time
KNOBS = ('BX_NO_JOINT_HALVES', 'BX_NO_R2', 'BX_NO_MULTI_JH', 'BX_NO_JB', 'BX_PLAN_DEBUG')

NAMES = (list(helpers.ENV_CONFIG) + helpers.SPRING_ENVS + helpers.XY_ENVS + helpers.ROBOTS +
         helpers.SPRING_ROBOTS + helpers.CAPSULES + helpers.XCOL + helpers.POINTS +
         helpers.SHORT_SCENES + helpers.NN_MASKED +
         ['mountain1', 'mountain2', 'mountain4', 'mountain1nn', 'mountain2nn', 'mountain4nn'])
CASES = ([(n, n, '', {}) for n in NAMES] +
         [('mountain4_materials', 'mountain4', 'materials', {}),
          ('mountain9_sparse', 'mountain9', 'sparse noreset', {}),
          ('ant_noreset', 'ant', 'noreset', {}),
          ('ant_forces', 'ant', 'forces', {}),
          ('ant_no_jb', 'ant', '', {'BX_NO_JB': '1'}),
          ('halfcheetah_no_jb', 'halfcheetah', '', {'BX_NO_JB': '1'}),
          ('halfcheetah_no_r2', 'halfcheetah', '', {'BX_NO_R2': '1'}),
          ('humanoidstandup_no_r2', 'humanoidstandup', '', {'BX_NO_R2': '1'}),
          ('ant_no_joint_halves', 'ant', '', {'BX_NO_JOINT_HALVES': '1'}),
          ('mountain4_no_multi_jh', 'mountain4', '', {'BX_NO_MULTI_JH': '1'})])
CASE_IDS = [c[0] for c in CASES]


def header_fields():
  """BlobHdr's field names in order (pbd_layout.h; every field is one word)."""
  src = open(os.path.join(ROOT, 'brax_amd', 'csrc', 'pbd_layout.h')).read()
  body = re.search(r'struct BlobHdr \{(.*?)\n\};', src, re.S).group(1)
  body = re.sub(r'//[^\n]*', '', body)
  names = []
  for typ, decl in re.findall(r'\b(int32_t|float)\s+([^;]+);', body):
    names += [n.strip() for n in decl.split(',')]
  return names


def features():
  """The F_* masks of pbd_features.h by name."""
  src = open(os.path.join(ROOT, 'brax_amd', 'csrc', 'pbd_features.h')).read()
  return {k: int(v) for k, v in re.findall(r'\b(F_\w+) = (\d+)', src)}


def header(words):
  """The blob's BlobHdr as a dict of its words (floats as their bits)."""
  names = header_fields()
  return dict(zip(names, (int(w) for w in words[:len(names)].view(np.int32))))


def sections(words):
  """The blob cut at the header's o_* offsets: [(name, words)], the header
  itself first. A section runs to the next larger offset (so it carries the
  16-byte alignment pad after it); offsets that are 0 mark absent sections."""
  names = header_fields()
  H = header(words)
  offs = sorted({H[n] for n in names if n.startswith('o_') and H[n] > 0} | {len(words)})
  out = [('hdr', words[:len(names)])]
  for n in names:
    if n.startswith('o_') and H[n] > 0:
      out.append((n, words[H[n]:offs[offs.index(H[n]) + 1]] if H[n] < len(words) else words[:0]))
  return out


def _sha(a):
  return hashlib.sha256(np.ascontiguousarray(a, np.uint32).tobytes()).hexdigest()


def case_blob(case):
  """(words, plan) of a case; the caller has set the case's env knobs."""
  _, name, variant, _ = case
  cfg = helpers.config_for(name)
  if 'sparse' in variant:
    ant = [b.name for b in cfgmod.parse(configs.ANT_CONFIG).bodies if b.name != 'Ground']
    for b in cfg.bodies:
      if b.name != 'Ground':
        cfg.collide_include.add(first=b.name, second='Ground')
    for a in ant:
      for b in ant:
        cfg.collide_include.add(first=a, second=b + '_0')
  vc, desc, meta = compiler.compile_system(cfg)
  rdesc = compiler.compile_reset(vc, meta['body_index'])
  if 'materials' in variant:
    desc['row_friction'] = np.linspace(0.5, 1.5, len(desc['row_friction']))
  if 'forces' in variant:
    desc.update(force_type=[0], force_body=[0], force_index=[[0, 1, 2]], force_strength=[1.0])
  return desc_blob(desc, None if 'noreset' in variant else rdesc, meta['num_joint_dof'])


def fingerprint(words, plan):
  return {'n_words': int(len(words)),
          'plan': [int(plan[k]) for k in ('mode', 'lanes', 'lds_bytes', 'feat', 'gw', 'fold',
                                          'jb', 'cb')],
          'sha256': _sha(words),
          'sections': {n: _sha(w) for n, w in sections(words)}}
