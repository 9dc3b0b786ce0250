"""The MULTI kernel past its first contact chunk, with finite contacts.

`pbd_step_multi` lists each collision pass's penetrating rows: the first
MCBUF = 128 contacts in LDS, the rest in the env's slice of the System's
global overflow buffer, and computes their impulses MCAP = 128 rows at a
time, the task sums carrying a partial from one chunk to the next
(pbd_layout.h). The spiral-drop Mountain(4) of the other parity and scale
tests lists about 43 rows per pass, so these run everything past the first
chunk: the overflow records (row index kept as float bits, `dlambda` written
back for the velocity pass), the carried partials, the chunk's slot mapping,
the index clean-up between passes and the growth of the overflow buffer.

The scene is `tests.helpers.piled_mountain4`: the four ants translated onto
one spot. With `substeps = 2` the step's only collision pass is its last, so
its Info shows the listed rows: 184-186 penetrating rows per env with all
pairs, 165-167 at NearNeighbors cutoff 300 (the float64 oracle, 64 envs,
step 0), two chunks each; step 1 of the same rollout has 122-154, on both
sides of the boundary. At the workload's `substeps = 10` the first pass
overflows and the later ones do not (57-79 rows on the last). At
`substeps = 4` both passes reach the boundary (184, then 113-134), and in
some envs a row listed past MCBUF in the first pass is gone from a second
pass that still has a second chunk: the one place where the index clean-up
of the overflow rows shows (a build that skipped it passed everything else
here).

Every state gate is tests/test_gpu_parity.py's `_gate`: env i's normwise error
against the float64 oracle <= max(1e-5, 2 x E32_i) over 66 fp32 realisations
of the reference algorithm, the ill-conditioned envs on their nearest
realisation.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import QP_FIELDS, normwise, piled_actions, piled_mountain4, set_variant

MCBUF = 128  # pbd_layout.h: the listed contacts kept in LDS (MCAP, the rows per chunk, is 128 too)
B = 64
CUTOFFS = [0, 300]
VARIANTS = ['multi', 'multi256']
SAMPLE = np.sort(np.random.default_rng(11).choice(B, 8, replace=False))

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  return torch.device('cuda', 0)


class _Scene:
  """The piled scene at one (cutoff, substeps): config, descriptors, the 64
  envs' start state and actions, the float64 oracle and the fp32 envelope."""

  def __init__(self, oracle_lib, cutoff, substeps, dt_scale=1.0):
    from brax_amd import compiler
    from tests.test_gpu_parity import Envelope
    self.cfg, q0 = piled_mountain4(cutoff, substeps)
    self.cfg.dt *= dt_scale
    vc, d, meta = compiler.compile_system(self.cfg)
    rd = compiler.compile_reset(vc, meta['body_index'])
    self.culled = cutoff > 0
    self.o64 = oracle_lib.Oracle(d, rd, np.float64, safe_guard=True)
    self.env32 = Envelope(oracle_lib, None, desc=(d, rd))
    self.qp0 = np.repeat(q0[None], B, axis=0)  # (B, N, 13) fp32
    self.act = piled_actions(B, 2)

  @functools.cached_property
  def ref0(self):
    """Step 0 of all 64 envs on the float64 oracle: (qp, info). Read-only."""
    return self.o64.system_step(self.qp0, self.act[0])

  @functools.cached_property
  def outs0(self):
    """Step 0's 66 fp32 realisations of the sampled envs. Read-only."""
    return self.env32.system(self.qp0[SAMPLE], self.act[0][SAMPLE])


@functools.lru_cache(maxsize=None)
def _scene_cached(oracle_lib, cutoff, substeps, dt_scale=1.0):
  return _Scene(oracle_lib, cutoff, substeps, dt_scale)


@pytest.fixture
def scene(oracle_lib):
  return lambda cutoff, substeps: _scene_cached(oracle_lib, cutoff, substeps)


def _system(sc, dev, variant):
  import brax_amd
  from brax_amd import _native
  sys_ = brax_amd.System(sc.cfg, device=dev)
  _native.check(set_variant(sys_, variant))
  return sys_


def _to_qp(a, dev):
  from brax_amd.base import qp_from_numpy
  return qp_from_numpy(a, dev)


def _act(a, dev):
  return torch.as_tensor(a, dtype=torch.float32, device=dev)


def _penetrating(pen):
  return (np.asarray(pen) > 0).sum(axis=-1)


def _paired_counts(hip, ref, culled):
  """One env's penetrating Info rows on both sides, over the rows where
  neither side's |penetration| <= 1e-5 (a sign rounding may flip). All pairs:
  Info row x is contact row x on both sides. Culled: the Info rows follow the
  selected cells, so the rows are paired by rank of penetration instead."""
  h, r = np.asarray(hip, np.float64), np.asarray(ref, np.float64)
  if culled:
    h, r = np.sort(h), np.sort(r)
  keep = (np.abs(h) > 1e-5) & (np.abs(r) > 1e-5)
  return int((h[keep] > 0).sum()), int((r[keep] > 0).sum())


def _gate_state(got, ref, outs):
  from tests.test_gpu_parity import _env_err, _gate
  for f, sl in QP_FIELDS.items():
    _gate(got[..., sl], ref[..., sl], _env_err([o[0][..., sl] for o in outs], ref[..., sl]), f)


def _gate_info(info, rinfo, outs, culled, idx):
  """Info.contact per body and contact_penetration per row (sorted, clamped
  at zero where NearNeighbors orders the rows), as test_system_step_vs_golden."""
  from tests.test_gpu_parity import _env_err, _gate
  ic = torch.cat([info.contact.vel, info.contact.ang], -1).cpu().numpy()[idx]
  _gate(ic, rinfo['contact'], _env_err([o[1]['contact'] for o in outs], rinfo['contact']),
        'info_contact')
  pen = info.contact_penetration.cpu().numpy()[idx]
  ref_pen = rinfo['contact_penetration']
  o_pen = [o[1]['contact_penetration'] for o in outs]
  if culled:
    srt = lambda a: np.sort(np.maximum(a, 0), -1)  # noqa: E731
    pen, ref_pen, o_pen = srt(pen), srt(ref_pen), [srt(x) for x in o_pen]
  _gate(pen, ref_pen, _env_err(o_pen, ref_pen), 'pen')


@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_piled_scene_overflows_on_the_oracle(scene, cutoff):
  """The scene's own precondition, on the CPU: step 0 at `substeps = 2` lists
  more than MCBUF + 32 penetrating rows in every env on the float64 oracle
  (measured 184-186 with all pairs, 165-167 at cutoff 300) and at most 4 rows
  per env within 1e-5 of the sign change (measured 0). If the scene's
  constants ever change, they change in `piled_mountain4` and are re-measured
  here."""
  sc = scene(cutoff, 2)
  pen = sc.ref0[1]['contact_penetration']
  assert np.isfinite(sc.ref0[0]).all() and np.isfinite(pen).all()
  n = _penetrating(pen)
  amb = (np.abs(pen) <= 1e-5).sum(axis=-1)
  print(f'cutoff {cutoff}: penetrating rows {n.min()}-{n.max()}, ambiguous {amb.max()}')
  assert n.min() > MCBUF + 32, n
  assert amb.max() <= 4, amb


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_overflow_reached_on_the_device(dev, scene, cutoff, variant):
  """The `substeps = 2` step's Info on the device: every env lists more
  penetrating rows than MCBUF, and each sampled env's count is the float64
  oracle's (rows within 1e-5 of zero on either side left out)."""
  sc = scene(cutoff, 2)
  sys_ = _system(sc, dev, variant)
  _, info = sys_.step(_to_qp(sc.qp0, dev), _act(sc.act[0], dev))
  pen = info.contact_penetration.cpu().numpy()
  ref_pen = sc.ref0[1]['contact_penetration']
  assert pen.shape == ref_pen.shape
  n = _penetrating(pen)
  print(f'cutoff {cutoff} {variant}: device penetrating rows {n.min()}-{n.max()}')
  assert n.min() > MCBUF, n
  for e in SAMPLE:
    h, r = _paired_counts(pen[e], ref_pen[e], sc.culled)
    assert h == r, (e, h, r)
    assert h > MCBUF, (e, h)


@gpu
@pytest.mark.parametrize('info', [True, False], ids=['info', 'noinfo'])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_parity_past_the_first_chunk(dev, scene, cutoff, variant, info):
  """Steps 0 and 1 of the `substeps = 2` scene chained on the device, each
  against the float64 oracle stepped from the same input: state, Info.contact
  and contact_penetration of 8 sampled envs. With Info the pass runs every
  row (no broad phase on a step's last pass); without, the broad phase's near
  list feeds the listing: two routes into the overflow records."""
  sc = scene(cutoff, 2)
  sys_ = _system(sc, dev, variant)
  qp_in = sc.qp0
  for t in range(2):
    out, hinfo = sys_.step(_to_qp(qp_in, dev), _act(sc.act[t], dev), info=info)
    got = out.numpy()
    assert np.isfinite(got).all()
    if t == 0:
      ref, rinfo = sc.ref0[0][SAMPLE], {k: v[SAMPLE] for k, v in sc.ref0[1].items()}
      outs = sc.outs0
    else:
      ref, rinfo = sc.o64.system_step(qp_in[SAMPLE], sc.act[t][SAMPLE])
      outs = sc.env32.system(qp_in[SAMPLE], sc.act[t][SAMPLE])
    _gate_state(got[SAMPLE], ref, outs)
    if info:
      _gate_info(hinfo, rinfo, outs, sc.culled, SAMPLE)
    qp_in = got  # chained on the device's own fp32 state


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_parity_at_the_workloads_substeps(dev, scene, cutoff, variant):
  """The same piled state at `substeps = 10`, one step: the first collision
  pass overflows, the later ones list fewer rows than a chunk (two chunks
  shrinking to one; the listed rows leave the index between passes). Envs
  ill-conditioned on the last passes take `_gate`'s nearest-realisation
  bound."""
  sc = scene(cutoff, 10)
  sys_ = _system(sc, dev, variant)
  out, hinfo = sys_.step(_to_qp(sc.qp0, dev), _act(sc.act[0], dev))
  got = out.numpy()
  assert np.isfinite(got).all()
  _gate_state(got[SAMPLE], sc.ref0[0][SAMPLE], sc.outs0)
  _gate_info(hinfo, {k: v[SAMPLE] for k, v in sc.ref0[1].items()}, sc.outs0, sc.culled, SAMPLE)


@functools.lru_cache(maxsize=None)
def _two_pass(oracle_lib, cutoff):
  """The piled state at `substeps = 4` (two collision passes) and the envs
  where the index clean-up of a row listed past MCBUF shows: a row whose
  compact index in pass 1 was y >= MCBUF, which pass 2 does not list, while
  pass 2 still lists more than y rows, so a stale index would read another
  row's slot in pass 2's second chunk. Both passes' rows are the float64
  oracle's Info rows (pass 1: the one pass of `substeps = 2` at half the dt,
  the same h); the kernel lists the rows in Info order (ascending work row).
  Returns (scene, up to 8 such envs, how many of the 64 there are)."""
  sc = _scene_cached(oracle_lib, cutoff, 4)
  first = _scene_cached(oracle_lib, cutoff, 2, 0.5)
  p1 = first.ref0[1]['contact_penetration'] > 0
  p2 = sc.ref0[1]['contact_penetration'] > 0
  y1 = np.cumsum(p1, axis=-1) - 1
  stale = p1 & ~p2 & (y1 >= MCBUF) & (y1 < p2.sum(axis=-1, keepdims=True))
  envs = np.flatnonzero(stale.any(axis=-1))
  return sc, envs[:8], len(envs)


@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_two_pass_scene_has_rows_leaving_the_overflow_on_the_oracle(oracle_lib, cutoff):
  """CPU precondition of the two-pass test below: on the float64 oracle some
  envs drop a row listed past MCBUF in pass 1 from a pass 2 that still has a
  second chunk (measured: 15 of 64 envs with all pairs)."""
  sc, envs, n = _two_pass(oracle_lib, cutoff)
  n2 = _penetrating(sc.ref0[1]['contact_penetration'])
  print(f'cutoff {cutoff}: pass 2 rows {n2.min()}-{n2.max()}, envs with such a row {n}')
  assert len(envs) >= 1


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_parity_over_two_overflowing_passes(dev, oracle_lib, cutoff, variant):
  """`substeps = 4`, one step: pass 1 lists ~184 rows, pass 2 113-134, on both
  sides of the chunk boundary. Gated on the envs (up to 8) where a row leaves
  the overflow part of the list between the passes (`_two_pass`): the
  clean-up of `sidx` through the overflow records' row indices."""
  sc, envs, _ = _two_pass(oracle_lib, cutoff)
  sys_ = _system(sc, dev, variant)
  out, hinfo = sys_.step(_to_qp(sc.qp0, dev), _act(sc.act[0], dev))
  got = out.numpy()
  assert np.isfinite(got).all()
  outs = sc.env32.system(sc.qp0[envs], sc.act[0][envs])
  _gate_state(got[envs], sc.ref0[0][envs], outs)
  _gate_info(hinfo, {k: v[envs] for k, v in sc.ref0[1].items()}, outs, sc.culled, envs)


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_multi_vs_item_loops_past_the_first_chunk(dev, scene, cutoff, variant):
  """Step 0 of the `substeps = 2` scene on all 64 envs: each env's normwise
  distance between the MULTI kernel and the item loops, against the sum of
  the two kernels' parity bounds on the sampled envs (2 x max(1e-5, 2 x
  E32_i), as test_mountain4_multi_vs_item_loops), finite on every env;
  recorded as `multi_overflow_vs_items:<field>`."""
  from tests.margins import record_margin
  from tests.test_gpu_parity import _env_err
  sc = scene(cutoff, 2)
  sys_ = _system(sc, dev, variant)
  out = {}
  for v in (variant, 'items'):
    from brax_amd import _native
    _native.check(set_variant(sys_, v))
    out[v] = sys_.step(_to_qp(sc.qp0, dev), _act(sc.act[0], dev), info=False)[0].numpy()
  ref = sc.ref0[0][SAMPLE]
  for f, sl in QP_FIELDS.items():
    dist = normwise(out[variant][..., sl], out['items'][..., sl])
    e32 = np.asarray(_env_err([o[0][..., sl] for o in sc.outs0], ref[..., sl]))
    bound = 2 * np.maximum(1e-5, 2 * e32)
    ds = dist[SAMPLE]
    k = int(np.argmax(ds / bound))
    record_margin(f'multi_overflow_vs_items:{f}', float(ds[k]), float(bound[k]), n=len(SAMPLE),
                  pair_ratios=(ds / bound).tolist(), role='record',
                  full_batch_max=float(dist.max()), full_batch_p50=float(np.median(dist)))
    assert (ds <= bound).all(), (f, ds, bound)
    assert np.isfinite(dist).all()


def _bits(qp, info):
  """A step's outputs as numpy arrays: state, then every Info field."""
  a = [qp.numpy(), info.contact.vel, info.contact.ang, info.actuator.vel, info.actuator.ang,
       info.contact_pos, info.contact_normal, info.contact_penetration]
  if info.contact_cell is not None:
    a.append(info.contact_cell)
  return [x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in a]


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cutoff', CUTOFFS)
def test_overflow_buffer_slices_and_growth(dev, scene, cutoff, variant):
  """A fresh System steps envs [:3] (the overflow buffer sized for 3), then
  all 64 (the buffer grows: a new allocation, the old one kept until destroy),
  then [:3] again (three slices of the larger buffer): both 3-env results are
  the first three rows of the 64-env result bit for bit, state and Info;
  the 64 stepped twice give identical bits; every env lists more than MCBUF
  rows, rotations are unit and everything is finite."""
  sc = scene(cutoff, 2)
  sys_ = _system(sc, dev, variant)
  act = _act(sc.act[0], dev)

  def step(n):
    qp, info = sys_.step(_to_qp(sc.qp0[:n], dev), act[:n].contiguous())
    torch.cuda.synchronize()
    return _bits(qp, info)

  small, full, again, small2 = step(3), step(B), step(B), step(3)
  for k, (s, f, a, s2) in enumerate(zip(small, full, again, small2)):
    assert np.array_equal(f, a), k
    assert np.array_equal(s, f[:3]), k
    assert np.array_equal(s2, f[:3]), k
    assert np.isfinite(f).all(), k
  n = _penetrating(full[7])
  print(f'cutoff {cutoff} {variant}: device penetrating rows {n.min()}-{n.max()}')
  assert n.min() > MCBUF, n
  rot = full[0][..., QP_FIELDS['rot']]
  assert np.abs(np.linalg.norm(rot, axis=-1) - 1).max() <= 1e-5
