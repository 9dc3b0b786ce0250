"""The C-ABI library builds, loads without a GPU and exports every symbol
declared in include/brax_amd.h, and the Python mirror (`brax_amd.abi`) is the
header's, declaration by declaration: every function's parameter names, order
and types, every struct's fields and layout, every mirrored constant (no
compute calls here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from brax_amd import _native
from brax_amd import abi
from tests.helpers import HEADER_PATH, Header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = Header()
MIRRORS = {n.lower(): c for n, c in vars(abi).items()
           if isinstance(c, type) and issubclass(c, C.Structure)}
SCALARS = {'int64_t': C.c_int64, 'int32_t': C.c_int32, 'uint64_t': C.c_uint64, 'int': C.c_int,
           'float': C.c_float, 'double': C.c_double}
# what a pointer may point at besides the scalars above and the structs
POINTEES = dict(SCALARS, uint32_t=C.c_uint32, uint8_t=C.c_uint8, void=None,
                **{'unsigned long long': C.c_ulonglong})


def mirror(struct):
  """The ctypes mirror of `bx_<struct>`: abi.Bx<Struct>, whatever its capitals."""
  return MIRRORS.get(struct.replace('_', ''))


def _kind(t):
  """(float or integer, bytes, signed) of a ctypes scalar."""
  return t._type_ in 'fd', C.sizeof(t), t._type_.islower()


def accepts(ctype, dim, t):
  """The type rule: whether the ctypes type `t` may stand for a parameter
  declared `ctype name` (`ctype name[dim]` with a `dim`)."""
  base = ctype.replace('const ', '').rstrip('*')
  stars = len(ctype) - len(ctype.rstrip('*')) + (dim is not None)
  if stars == 0:
    return t is SCALARS[base]  # the exact ctypes scalar
  if base == 'bx_system':
    return t is (C.c_void_p if stars == 1 else C.POINTER(C.c_void_p))
  assert stars == 1, ctype
  if base.startswith('bx_'):
    return t is C.POINTER(mirror(base))  # and nothing else
  if t is C.c_void_p:
    return True
  scalar = POINTEES[base]
  return (scalar is not None and isinstance(t, type) and issubclass(t, C._Pointer)
          and issubclass(t._type_, C._SimpleCData) and _kind(t._type_) == _kind(scalar))


def test_header_declares_the_boundary():
  for n in ('bx_system_create', 'bx_system_step', 'bx_env_step', 'bx_system_default_qp',
            'bx_system_info', 'bx_last_error'):
    assert n in HEADER.functions


def test_the_parser_sees_every_declaration():
  """51 functions and 17 structs, counted twice: by the parser and by a plain
  search of the header; the parametrised tests below run over the parser's."""
  assert len(HEADER.functions) == len(re.findall(r'\bbx_\w+\s*\(', HEADER.text)) == 51
  assert len(HEADER.structs) == len(re.findall(r'typedef\s+struct\s+bx_\w+\s*\{', HEADER.text)) == 17
  assert list(abi.ARGS) == list(HEADER.functions)  # all 51, in the header's order
  assert sorted(s.replace('_', '') for s in HEADER.structs) == sorted(MIRRORS)
  assert sum(len(f) for f in HEADER.structs.values()) == 180
  # the parser's own cases: comments, `T name[N]`, several declarators
  assert HEADER.functions['bx_system_blob'][1][-1] == ('int32_t', 'plan', '8')
  assert HEADER.functions['bx_abi_version'] == ('int', [])
  assert HEADER.functions['bx_last_error'][0] == 'const char*'
  assert HEADER.structs['bx_qp'] == [('bx_field', n, None) for n in ('pos', 'rot', 'vel', 'ang')]
  assert HEADER.structs['bx_mlp'][-1] == ('const float*', 'b', 'BX_MLP_MAX_LAYERS')
  assert 'contact_cell' in [f for _, f, _ in HEADER.structs['bx_info']]


def test_library_exports_every_declared_symbol():
  if not os.path.exists(_native.LIB_PATH):
    _native.build()
  lib = C.CDLL(_native.LIB_PATH)
  for n in HEADER.functions:
    assert hasattr(lib, n), n
  assert set(_native.EXPORTS) == set(HEADER.functions)


@pytest.mark.parametrize('name', list(HEADER.functions))
def test_signature_is_the_headers(name):
  res, params = HEADER.functions[name]
  table = abi.ARGS[name]
  assert [n for n, _ in table] == [n for _, n, _ in params]
  for (ctype, arg, dim), (_, t) in zip(params, table):
    assert accepts(ctype, dim, t), (arg, ctype, t)
  restype = {'int': C.c_int, 'const char*': C.c_char_p}[res]
  assert abi.SIGNATURES[name] == ([t for _, t in table], restype)
  assert _native._SIGS[name] == abi.SIGNATURES[name]  # pylint: disable=protected-access
  fn = getattr(_native.lib(), name)
  assert list(fn.argtypes) == [t for _, t in table] and fn.restype is restype


def test_the_type_rule_refuses_what_it_should():
  """`accepts` on types that would corrupt a call."""
  assert not accepts('int64_t', None, C.c_int32) and not accepts('uint64_t', None, C.c_int64)
  assert not accepts('float', None, C.c_double)
  assert not accepts('const bx_desc*', None, C.c_void_p)
  assert not accepts('const bx_qp*', None, C.POINTER(abi.BxInfo))
  assert not accepts('bx_system*', None, C.POINTER(C.c_void_p))
  assert not accepts('bx_system**', None, C.c_void_p)
  assert not accepts('int32_t*', None, C.POINTER(C.c_int64))
  assert not accepts('const uint32_t*', None, C.POINTER(C.c_int32))
  assert not accepts('int32_t', '8', C.c_int32) and not accepts('void*', None, C.POINTER(C.c_int))
  assert accepts('int32_t', '8', C.POINTER(C.c_int32)) and accepts('int64_t*', None, C.c_void_p)


@pytest.mark.parametrize('struct', list(HEADER.structs))
def test_struct_fields_are_the_headers(struct):
  cls = mirror(struct)
  assert cls is not None, struct
  assert [f for f, _ in cls._fields_] == [f for _, f, _ in HEADER.structs[struct]]


# abi's constants and the macro or enumerator each mirrors
CONSTANTS = {
    'BX_ABI_VERSION': abi.ABI_VERSION, 'BX_OBS_XY': abi.OBS_XY, 'BX_DYN_PBD': abi.DYN_PBD,
    'BX_DYN_LEGACY_SPRING': abi.DYN_LEGACY_SPRING, 'BX_POLICY_MAX_LAYERS': abi.POLICY_MAX_LAYERS,
    'BX_POLICY_MAX_WIDTH': abi.POLICY_MAX_WIDTH, 'BX_POLICY_MAX_OBS': abi.POLICY_MAX_OBS,
    'BX_POP_NO_STAGE': abi.POP_NO_STAGE, 'BX_POPULATION_DELTA_CHUNK': abi.POPULATION_DELTA_CHUNK,
    'BX_FIELDS_MAX': abi.FIELDS_MAX, 'BX_MLP_MAX_LAYERS': abi.MLP_MAX_LAYERS,
    'BX_MLP_MAX_WIDTH': abi.MLP_MAX_WIDTH, 'BX_MLP_MAX_IN': abi.MLP_MAX_IN,
    'BX_SAC_MAX_CRITICS': abi.SAC_MAX_CRITICS, 'BX_SAC_MAX_JOBS': abi.SAC_MAX_JOBS,
    'BX_OPT_MAX_TENSORS': abi.OPT_MAX_TENSORS,
    **{'BX_POLICY_' + k.upper(): v for k, v in abi.POLICY_ACTIVATIONS.items()},
    **{'BX_HEAD_' + k.upper(): v for k, v in abi.HEADS.items()},
}


def test_layout_and_constants_as_the_compiler_has_them(tmp_path):
  """One generated program, built with the host compiler of the library's own
  host unit (the Makefile's HOSTCXX), prints sizeof of every struct, offsetof
  and size of every field and every mirrored constant; ctypes must agree."""
  assert set(CONSTANTS) <= set(HEADER.constants)
  # every integer constant of abi with a BX_ namesake in the header is listed
  assert {'BX_' + n for n, v in vars(abi).items() if n.isupper() and isinstance(v, int)
          and 'BX_' + n in HEADER.constants} <= set(CONSTANTS)
  lines, want = [], []
  for struct, fields in HEADER.structs.items():
    cls = mirror(struct)
    lines.append(f'std::printf("{struct} %zu\\n", sizeof({struct}));')
    want.append(f'{struct} {C.sizeof(cls)}')
    for _, f, _ in fields:
      lines.append(f'std::printf("{struct}.{f} %zu %zu\\n", offsetof({struct}, {f}), '
                   f'sizeof((({struct}*)0)->{f}));')
      want.append(f'{struct}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}')
  for name, value in CONSTANTS.items():
    lines.append(f'std::printf("{name} %lld\\n", (long long)({name}));')
    want.append(f'{name} {value}')
  src = tmp_path / 'layout.cpp'
  src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() {\n  %s\n}\n'
                 % (HEADER_PATH, '\n  '.join(lines)))
  exe = tmp_path / 'layout'
  subprocess.run([os.environ.get('HOSTCXX', 'c++'), '-std=c++17', str(src), '-o', str(exe)],
                 check=True, timeout=120)
  got = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
  assert got.splitlines() == want
  assert len(want) == 17 + 180 + len(CONSTANTS)


def test_abi_version_and_error_path():
  lib = _native.lib()
  assert lib.bx_abi_version() == abi.ABI_VERSION
  # a null descriptor fails at create with a message, no GPU touched
  h = C.c_void_p()
  rc = lib.bx_system_create(None, None, 0, C.byref(h))
  assert rc != 0 and b'null' in lib.bx_last_error()


def test_missing_library_fails_loudly(tmp_path):
  """No CPU fallback: with the HIP library absent, the product path raises
  NativeError at its first native call instead of computing anything."""
  import sys
  code = ('import brax_amd, sys\n'
          'from brax_amd._native import NativeError\n'
          'from brax_amd.system import System\n'
          'from tests.helpers import config_for\n'
          'try:\n'
          '  System.plan(config_for("ant"))\n'
          'except NativeError as e:\n'
          '  print("raised", e)\n'
          '  sys.exit(0)\n'
          'sys.exit(3)\n')
  env = dict(os.environ, BRAX_AMD_LIB=str(tmp_path / 'absent' / 'libbrax_amd.so'))
  r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True,
                     text=True, timeout=120)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'raised' in r.stdout
