"""Loader of the in-tree HIP library `brax_amd/_lib/libbrax_amd.so`.

There is no CPU fallback: if the library or a GPU is missing, every device
entry point raises. Build with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C brax_amd/csrc`.
"""
import ctypes as C
import os
import subprocess

from brax_amd import abi, abi_mlp_group

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BRAX_AMD_LIB') or os.path.join(HERE, '_lib', 'libbrax_amd.so')
CSRC = os.path.join(HERE, 'csrc')


class NativeError(RuntimeError):
  pass


def build(arch='gfx950', jobs=4):
  subprocess.run(['make', '-s', f'-j{jobs}', '-C', CSRC, f'ARCH={arch}'], check=True)


_lib = None

_SIGS = abi.SIGNATURES  # name -> (argtypes, restype), from the one table abi.ARGS
EXPORTS = tuple(_SIGS)
# the headers on top of it (include/brax_amd_mlp_group.h), each with its own table
_MORE_SIGS = abi_mlp_group.SIGNATURES
# what an argument nobody names is: a null pointer, a zero scalar
_UNNAMED = {name: tuple(0 if issubclass(t, C._SimpleCData) and t is not C.c_void_p else None
                        for _, t in sig) for name, sig in abi.ARGS.items()}


def args(entry, **named):
  """The positional arguments of the entry point `entry`, in the header's
  order, from the ones given by name; the others are NULL or 0 (what its
  zero-step probes and optional outputs mean). A name the entry point does not
  have is a TypeError, as a repeated one is for any call."""
  sig = abi.ARGS[entry]
  unknown = named.keys() - {n for n, _ in sig}
  if unknown:
    raise TypeError(f'{entry} has no argument {sorted(unknown)}')
  return tuple(named.get(n, d) for (n, _), d in zip(sig, _UNNAMED[entry]))


def lib():
  """Returns the loaded library; raises NativeError if it is not built."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise NativeError(
          f'{LIB_PATH} is missing: the MI355X kernels are not built '
          '(run __graft_entry__.build() or make -C brax_amd/csrc). '
          'brax_amd has no CPU fallback.')
    l = C.CDLL(LIB_PATH)
    for name, (args, res) in {**_SIGS, **_MORE_SIGS}.items():
      f = getattr(l, name)
      f.argtypes = args
      f.restype = res
    if l.bx_abi_version() != abi.ABI_VERSION:
      raise NativeError('libbrax_amd ABI version mismatch')
    _lib = l
  return _lib


def check(rc):
  if rc != 0:
    raise NativeError(lib().bx_last_error().decode())
