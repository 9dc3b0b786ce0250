"""Host time of naming a K-step launch's arguments, on the CPU (no device):
`_native.args` on the 20 arguments of bx_env_eval_population, and the whole of
`packed.launch` around a library call that returns at once, beside the same
tuple written out positionally. One JSON line; medians of `--runs` regions of
`--calls` calls.

  python tools/native_args_cost.py
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brax_amd import _native, abi  # noqa: E402
from brax_amd.envs import packed  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=9)
  ap.add_argument('--calls', type=int, default=20000)
  a = ap.parse_args()
  B, K, A = 4096, 5, 8
  f = lambda *s: torch.zeros(s, dtype=torch.float32)  # noqa: E731
  p, desc, pop = abi.BxEnvParams(), abi.BxPolicy(), abi.BxPopulation()
  inputs = (p, f(B), f(B), None)
  qbuf, obs, ev, out = f(B, 9, 16), f(B, 87), f(13, B), f(16)
  stream, h = C.c_void_p(0), C.c_void_p(1)

  class Env:
    class sys:  # pylint: disable=invalid-name
      _h, device = h, torch.device('cpu')

  class Lib:
    bx_env_eval_population = staticmethod(lambda *args: 0)

  _native.lib = Lib
  packed._stream = lambda index: stream  # pylint: disable=protected-access
  named = dict(sys=h, env=C.byref(p), n_envs=B, n_steps=K, qp_in=1, obs_in=2, done_in=3, steps_in=4,
               policy=C.byref(desc), seed=1, offset=2, step_stride=3, eval_in=5, out=6, eval_out=5,
               pop=C.byref(pop), stream=stream)

  def positional():
    done, steps = inputs[1], inputs[2]
    return Lib.bx_env_eval_population(
        h, C.byref(p), B, K, qbuf.data_ptr(), obs.data_ptr(), done.data_ptr(), steps.data_ptr(),
        None, C.byref(desc), 1, 2, 3, ev.data_ptr(), out.data_ptr(), ev.data_ptr(), None,
        C.byref(pop), stream)

  def launch():
    return packed.launch(Env, 'bx_env_eval_population', inputs, qbuf, K, out, False, obs_in=obs,
                         policy=C.byref(desc), seed=1, offset=2, step_stride=3, eval_in=ev,
                         eval_out=ev, pop=C.byref(pop))

  def us(fn):
    regions = []
    for _ in range(a.runs):
      t = time.perf_counter()
      for _ in range(a.calls):
        fn()
      regions.append((time.perf_counter() - t) / a.calls * 1e6)
    return {'median': round(statistics.median(regions), 3), 'min': round(min(regions), 3),
            'max': round(max(regions), 3)}

  print(json.dumps({
      'measure': 'host time of one bx_env_eval_population call site, no device', 'unit': 'us',
      'arguments': len(abi.ARGS['bx_env_eval_population']), 'runs': a.runs,
      'calls_per_region': a.calls, 'native_args_alone': us(lambda: _native.args(
          'bx_env_eval_population', **named)),
      'packed_launch': us(launch), 'positional_call_site': us(positional)}))


if __name__ == '__main__':
  main()
