"""`tools/measure.py`, what the `*_bench.py` tools share, on a fake clock and a
fake device: the order of the timed regions, the rounding, the owner tables,
and each tool's frame (`--help`, the GPU refusal) in one child process."""
import glob
import itertools
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')
BENCHES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, '*_bench.py')))


@pytest.fixture(scope='module')
def tool_modules():
  """The tools import `measure` and each other as siblings."""
  sys.path.insert(0, TOOLS)
  try:
    import measure, optim_bench, ppo_head_bench, sac_head_bench  # pylint: disable=import-outside-toplevel,multiple-imports
    yield types.SimpleNamespace(measure=measure, optim_bench=optim_bench,
                                ppo_head_bench=ppo_head_bench, sac_head_bench=sac_head_bench)
  finally:
    sys.path.remove(TOOLS)


@pytest.fixture
def measure(tool_modules):
  return tool_modules.measure


@pytest.fixture
def log(measure, monkeypatch):
  """Every synchronise and every reading of the clock, in order; the clock
  advances one second per reading."""
  out = []
  ticks = itertools.count()

  def clock():
    out.append('clock')
    return float(next(ticks))
  monkeypatch.setattr(measure.torch.cuda, 'synchronize', lambda dev=None: out.append(('sync', dev)))
  monkeypatch.setattr(measure, 'time', types.SimpleNamespace(perf_counter=clock))
  return out


def test_region_synchronises_around_the_clock_and_divides_by_calls(measure, log):
  t = measure.region(lambda: log.append('call'), 4, 'dev')
  assert log == [('sync', 'dev'), 'clock', 'call', 'call', 'call', 'call', ('sync', 'dev'), 'clock']
  assert t == 1.0 / 4


def test_timed_returns_seconds_and_result(measure, log):
  assert measure.timed(lambda: log.append('call') or 'r', 'dev') == (1.0, 'r')
  assert log == [('sync', 'dev'), 'clock', 'call', ('sync', 'dev'), 'clock']


@pytest.mark.parametrize('warmup_calls, warm', [(None, 6), (1, 1), (2, 2)])
def test_alternate_warms_each_form_once_then_interleaves(measure, log, warmup_calls, warm):
  runs, calls = 3, 6
  forms = {'b': lambda: log.append('b'), 'a': lambda: log.append('a')}
  times = measure.alternate(forms, runs, calls, 'dev', warmup_calls=warmup_calls)
  # the regions, as (form, calls): the maximal runs of one form's calls between two clock readings
  seen = [(k, len(list(g))) for k, g in itertools.groupby(x for x in log if x in ('a', 'b', 'clock'))]
  seen = [r for r in seen if r[0] != 'clock']
  assert seen == [('b', warm), ('a', warm)] + [('b', calls), ('a', calls)] * runs
  assert list(times) == ['b', 'a']
  assert times == {'b': [1.0 / calls] * runs, 'a': [1.0 / calls] * runs}
  # one clock pair and one pair of synchronises per region, warm-ups included
  assert log.count('clock') == log.count(('sync', 'dev')) == 2 * (2 + 2 * runs)


def test_regions_warm_up_untimed_then_time_each_region(measure, log):
  times = measure.regions(lambda: log.append('call'), 2, 3, 'dev', warmup=2)
  assert log[:3] == ['call', 'call', ('sync', 'dev')]
  assert 'clock' not in log[:3] and log.count('clock') == 4
  assert times == [1.0 / 3] * 2


def test_spread_rounds_after_scaling(measure):
  assert measure.spread([3e-6, 1.234567e-6, 2e-6], 1e6) == {'median': 2.0, 'min': 1.23, 'max': 3.0}
  assert measure.spread([1.23456, 2.0], 1e3, 3) == {'median': 1617.28, 'min': 1234.56, 'max': 2000.0}
  assert measure.spread([0.12345], digits=3) == {'median': 0.123, 'min': 0.123, 'max': 0.123}
  assert measure.spread([7, 9, 8], 1, 0) == {'median': 8, 'min': 7, 'max': 9}


def _events(*pairs):
  return [types.SimpleNamespace(name=name, device_time=us) for name, us in pairs]


EVENTS = _events(('bx_mlp_forward_k', 10.0), ('bx_mlp_backward_k', 30.0), ('bx_PPO_head_fwd', 4.0),
                 ('bx_sac_head_losses', 6.0), ('bx_compute_gae_k', 2.0),
                 ('multi_tensor_apply_kernel<Adam>', 8.0), ('bx_fused_adam_k', 5.0),
                 # matches 'ppo_head' and 'mlp_': the first entry of each table takes it
                 ('ppo_head_mlp_tail', 1.0), ('elementwise_kernel', 3.0), ('reduce_kernel', 7.0))


def test_split_by_owner_optim_bench(tool_modules):
  m = tool_modules.measure
  assert m.split_by_owner(EVENTS, 2, tool_modules.optim_bench.OWNERS) == {
      'head kernels': [1.0, 2.5], 'network kernels': [1.0, 20.0], 'optimiser': [1.0, 6.5],
      'other torch': [2.0, 9.0]}
  assert m.all_kernels(EVENTS, 2) == [5.0, 38.0]


def test_split_by_owner_sac_head_bench(tool_modules):
  m = tool_modules.measure
  assert m.split_by_owner(EVENTS, 4, tool_modules.sac_head_bench.OWNERS) == {
      'head kernels': [0.2, 1.5], 'network kernels': [0.8, 10.2], 'optimiser': [0.5, 3.2],
      'other torch': [1.0, 4.0]}


def test_split_by_owner_ppo_head_bench_keeps_its_names(tool_modules):
  m = tool_modules.measure
  assert m.split_by_owner(EVENTS, 1, tool_modules.ppo_head_bench.OWNERS) == {
      'head kernels': [2.0, 5.0], 'network kernels': [2.0, 40.0], 'gae kernel': [1.0, 2.0],
      'adam': [2.0, 13.0], 'other torch': [3.0, 16.0]}


def test_owner_of_takes_the_first_match(tool_modules):
  m = tool_modules.measure
  assert m.owner_of('PPO_HEAD_mlp_tail', tool_modules.ppo_head_bench.OWNERS) == 'head kernels'
  assert m.owner_of('ppo_head_mlp_tail', tool_modules.sac_head_bench.OWNERS) == 'network kernels'
  assert m.owner_of('Optimizer.step#Adam.step', tool_modules.ppo_head_bench.OWNERS) == 'adam'


def test_emit_is_one_json_line(measure, capsys):
  measure.emit({'measure': 'x', 'v': [1, 2.5]})
  assert capsys.readouterr().out == '{"measure": "x", "v": [1, 2.5]}\n'


def test_use_tree_puts_the_root_ahead_of_the_tools_tree(measure, monkeypatch, tmp_path):
  monkeypatch.setattr(sys, 'path', [ROOT, TOOLS] + sys.path)
  monkeypatch.delitem(sys.modules, 'brax_amd', raising=False)
  measure.use_tree(str(tmp_path))
  assert sys.path[0] == str(tmp_path)
  assert sys.path.index(str(tmp_path)) < sys.path.index(measure.TOOLS_TREE) and measure.TOOLS_TREE == ROOT


def test_use_tree_refuses_once_the_package_is_imported(measure, monkeypatch):
  monkeypatch.setitem(sys.modules, 'brax_amd', types.ModuleType('brax_amd'))
  with pytest.raises(RuntimeError, match='already chosen'):
    measure.use_tree(ROOT)


def test_tool_args_gives_each_tool_its_own_defaults(measure):
  a = measure.tool_args('doc', runs=7, calls=50, steps=5, parts='head,sac').parse_args(['--parent'])
  assert (a.runs, a.calls, a.steps, a.parts, a.parent, a.root) == (7, 50, 5, 'head,sac', True, ROOT)
  assert measure.parts_of(a, in_parent=('sac',)) == ['sac']
  a = measure.tool_args('doc', runs=5).parse_args(['--root', '/elsewhere'])
  assert vars(a) == {'runs': 5, 'root': '/elsewhere'}


# One child for all the tools: each is run as `python tools/X.py ARGS` would run it (its directory
# first on the path, `__main__` as its name), and the child cannot see a GPU. Importing torch ten
# or twenty times over would cost this suite more than everything above together.
_CHILD = r'''
import json, os, runpy, sys
import torch
torch.cuda.is_available = lambda: False
tools, names = sys.argv[1], sys.argv[2:]
sys.path.insert(0, tools)
out = {}
for name in names:
  for args in (['--help'], []):
    sys.argv = [os.path.join(tools, name + '.py')] + args
    try:
      runpy.run_path(sys.argv[0], run_name='__main__')
      code = 'returned'
    except SystemExit as e:
      code = e.code
    out[name + ' ' + ' '.join(args)] = [code, 'brax_amd' in sys.modules]
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def frames():
  env = {**os.environ, 'HIP_VISIBLE_DEVICES': '', 'CUDA_VISIBLE_DEVICES': ''}
  r = subprocess.run([sys.executable, '-c', _CHILD, TOOLS] + BENCHES, env=env, cwd=ROOT,
                     capture_output=True, text=True, timeout=120, check=True)
  return json.loads(r.stdout.rsplit('RESULT ', 1)[1]), r.stdout


def test_there_are_ten_tools():
  assert len(BENCHES) == 10


@pytest.mark.parametrize('tool', BENCHES)
def test_help_needs_neither_the_package_nor_a_gpu(frames, tool):
  results, stdout = frames
  assert results[tool + ' --help'] == [0, False]
  assert f'usage: {tool}.py' in stdout and '--root ROOT' in stdout


@pytest.mark.parametrize('tool', BENCHES)
def test_without_a_gpu_the_tool_refuses(frames, tool):
  results, _ = frames
  assert results[tool + ' '] == [f'{tool} needs a GPU: a CPU run gives no time', False]
