"""Writes tests/golden/blob_fingerprints.json: the fingerprint of the host blob
(bx_system_blob) of every case of tests/blob_cases.py, from the library as
built. The fixture pins the blob builder, so record it only from a tree
whose builder is trusted (a kernel change that moves a blob word on purpose),
never to make tests/test_blob_fingerprint.py pass after a refactor.

  python tools/record_blob_fingerprints.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import blob_cases as bc  # noqa: E402


def main():
  out = {}
  for case in bc.CASES:
    for k in bc.KNOBS:
      os.environ.pop(k, None)
    os.environ.update(case[3])
    out[case[0]] = bc.fingerprint(*bc.case_blob(case))
    print(case[0], out[case[0]]['n_words'], out[case[0]]['plan'])
  with open(bc.FIXTURE, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
