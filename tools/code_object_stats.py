"""Register, spill and scratch figures of a library's kernels, from the code
objects' metadata notes (no GPU needed).

  python tools/code_object_stats.py <libbrax_amd.so> [<name substring> ...]

Cuts every gfx950 code object out of the library's offload bundles, reads its
AMDGPU metadata with llvm-readelf and prints, per kernel whose demangled-ish
name contains every given substring: VGPRs, AGPRs, SGPRs, VGPR / SGPR spill
counts, scratch bytes (private_segment_fixed_size) and LDS bytes.
"""
import os
import re
import subprocess
import sys
import tempfile

READELF = os.environ.get('LLVM_READELF', '/opt/rocm/llvm/bin/llvm-readelf')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count',
        '.private_segment_fixed_size', '.group_segment_fixed_size')


def code_objects(path):
  data = open(path, 'rb').read()
  at = data.find(MAGIC)
  while at >= 0:
    n = int.from_bytes(data[at + 24:at + 32], 'little')
    p = at + 32
    for _ in range(n):
      off, size, tl = (int.from_bytes(data[p + 8 * k:p + 8 * k + 8], 'little') for k in range(3))
      triple = data[p + 24:p + 24 + tl].decode()
      p += 24 + tl
      if 'gfx' in triple and size:
        yield triple, data[at + off:at + off + size]
    at = data.find(MAGIC, at + 1)


def kernels(blob):
  with tempfile.NamedTemporaryFile(suffix='.co') as f:
    f.write(blob)
    f.flush()
    notes = subprocess.run([READELF, '--notes', f.name], capture_output=True, text=True,
                           check=True).stdout
  for part in notes.split('- .agpr_count:')[1:]:
    part = '.agpr_count:' + part
    name = re.search(r'\.name:\s+(\S+)', part)
    vals = {k: int(m.group(1)) for k in KEYS if (m := re.search(re.escape(k) + r':\s+(\d+)', part))}
    if name:
      yield name.group(1), vals


def main():
  lib, subs = sys.argv[1], sys.argv[2:]
  for triple, blob in code_objects(lib):
    for name, v in kernels(blob):
      if all(s in name for s in subs):
        print(name)
        print('   ' + '  '.join(f'{k.lstrip(".")} {v.get(k)}' for k in KEYS))


if __name__ == '__main__':
  main()
