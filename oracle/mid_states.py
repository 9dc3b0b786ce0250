"""Mid-episode goldens (`mid_<system>`): their start states and their census.

TEST INFRASTRUCTURE ONLY. The trajectory goldens start at `reset`, 3-8 steps
from it, where most contact rows never penetrate. The `mid_*` fixtures start
from states further into an episode. A start state is an INPUT: the C
restatement (oracle/pbd_oracle.c, float64; tests/test_oracle.py pins it to
the reference) picks it, by seeded burn-in from the golden reset state
(Pusher, Grasp: a seeded search over placements of the object at the arm /
hand), and the
reference records what follows (oracle/gen_golden.py, `--only mid_<system>`).

A candidate is scored with the parity gate's own envelope
(tests/helpers.py `Envelope`: both float32 oracle builds, the exact
input and N_PERTURB fp32-ulp perturbed copies): a sample (one env at one
step) is WELL-CONDITIONED when 2 x E32 <= WIDE for every gated field, and a
row's contact test is DECIDED on a sample when every float32 realisation
agrees with the float64 oracle on `penetration > 0`. Nothing here runs a
kernel. Every function takes the oracle front-end module (`oracle/oracle.py`)
as `lib`, as the tests' `oracle_lib` fixture hands it out.
"""
import numpy as np

B, T = 8, 2
# Grasp's palm row resolves within one step (the object is pushed off), so no
# env has it on both samples: 16 envs give both of its capsule groups 8 samples
ENVS = {'grasp': 16}
ACT_SEED = 70_000  # recorded actions: default_rng(ACT_SEED + t).uniform(-1, 1, (B, A))
N_PERTURB = 32     # envelope copies per oracle build, as the GPU gates' default

# the contact rows each fixture exists for: the rows of the system that no
# other committed fixture ever sees penetrate
TARGET = {
    'pusher': list(range(16, 23)),  # arm capsule - object capsule, two-way (group 1)
    'halfcheetah': [16],            # bfoot - ffoot capsule-capsule (group 1)
    'hopper': [6, 7],               # foot - floor
    'walker2d': [7, 13],            # foot / foot_left - floor
    'humanoidstandup': [0, 1, 5, 6, 7, 10, 11, 12, 13, 15, 16, 17, 19, 20, 21],
    'grasp': [2, 3, 4, 5, 6],       # Object - palm (group 1), Object - fingertips (group 2)
}
# the systems whose object is placed: (body, half-range of the placement per
# axis: absolute, or None for half the sum of the row's two radii)
PLACED = {'pusher': ('object', 0.08), 'grasp': ('Object', None)}
# a dof counts as past its limit when it is outside by more than this (rad):
# limits at 0 are straddled by reset noise alone, which shows nothing
LIMIT_MARGIN = 1e-2
# burn-in steps searched per candidate run, candidate runs per env slot
BURN = {'halfcheetah': (40, 24), 'hopper': (12, 24), 'walker2d': (80, 24),
        'humanoidstandup': (48, 24), 'pusher': (24, 128), 'grasp': (8, 64)}
MIN_GROUP = 8    # active samples per collider group the census asserts
SHORTLIST = 160  # candidates per env slot that get the envelope


def actions(A, nb=B):
  return np.stack([np.random.default_rng(ACT_SEED + t).uniform(-1, 1, (nb, A)) for t in range(T)])


def _rotate(v, q):
  """v rotated by the unit quaternion q (w, x, y, z)."""
  u, w = q[1:4], q[0]
  return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def _oracles(lib, name, n_perturb=N_PERTURB):
  from tests.helpers import Envelope, compiled, env_coef, prep_oracle
  lib.build()
  _, d, rd, meta = compiled(name)
  o64 = prep_oracle(lib.Oracle(d, rd, np.float64, safe_guard=True), name)
  return o64, Envelope(lib, name, n_perturb=n_perturb), d, meta, env_coef(name)


def past_limit(o64, qp, margin=0.0):
  """(B, J, 3) bool: the joint dofs whose angle is outside its limit in `qp`
  by more than `margin`."""
  d = o64.desc
  ang = o64.joint_angles(qp)
  lim = np.asarray(d['joint_limit'], np.float64).reshape(-1, 3, 2)
  # a joint's limited angles: 1 (revolute), 2 (universal), 3 (spherical)
  dof = np.asarray(d['joint_type'])[:, None] > np.arange(3)[None]
  return dof[None] & ((ang < lim[None, ..., 0] - margin) | (ang > lim[None, ..., 1] + margin))


def pre_step(name, meta, qp, act):
  """What the env does before System.step: (qp, act) as System.step gets
  them. Grasp maps the action into the actuators' ranges and moves the palm
  towards its last three components (grasp.py:73-87); the others pass both on."""
  if name != 'grasp':
    return qp, act
  from brax_amd.envs import tasks
  from tests.helpers import config_for
  m = np.asarray(tasks.grasp_act_map(config_for(name)), np.float64)
  a = m[0] + m[1] * ((np.asarray(act, np.float64) + 1) / 2.0)
  palm = meta['body_index']['HandPalm']
  delta = a[:, -3:] - qp[:, palm, 0:3]
  norm = np.linalg.norm(delta, axis=-1, keepdims=True)
  scale = np.where(norm > 2.0, 2.0 / np.maximum(norm, 1e-30), 1.0)
  qp = np.array(qp, np.float64, copy=True)
  qp[:, palm, 0:3] += scale * delta * 0.15
  return qp, a


def conditioning(o64, env32, name, meta, qp, act, O, M, coef):
  """One env step from `qp` (B, N, 13) under `act`: (e32 (B,), decided (B, R),
  pen (B, R)). e32: the largest normwise error, against the float64 oracle,
  of the envelope's float32 realisations over every field the system and env
  gates compare. decided: every realisation agrees with the float64 oracle's
  `penetration > 0` on that row. pen: the float64 oracle's penetrations."""
  from tests.helpers import QP_FIELDS, normwise
  sq, sa = pre_step(name, meta, qp, act)
  ref_q, ref_i = o64.system_step(sq, sa)
  outs = env32.system(sq, sa)
  pairs = [(ref_q[..., sl], [o[0][..., sl] for o in outs]) for sl in QP_FIELDS.values()]
  keys = ['contact'] + (['contact_pos', 'contact_normal', 'contact_penetration']
                        if ref_i['contact_penetration'].size else [])
  pairs += [(ref_i[k], [o[1][k] for o in outs]) for k in keys]
  r = o64.env_step(name, qp, act, O, M, coef=coef)
  eo = env32.env(name, qp, act, O, M, 0, coef)
  pairs += [(r[1], [x[1] for x in eo]), (r[2][:, None], [x[2][:, None] for x in eo])]
  if M:
    pairs.append((r[4], [x[4] for x in eo]))
  e32 = np.zeros(qp.shape[0])
  for ref, vals in pairs:
    for v in vals:
      e32 = np.maximum(e32, normwise(v, ref))
  pen = ref_i['contact_penetration']
  decided = np.all([(o[1]['contact_penetration'] > 0) == (pen > 0) for o in outs], axis=0)
  return e32, decided, pen


def _burn_candidates(name, o64, G, A, nb):
  """Seeded burn-in from the golden reset states: per env slot b, BURN runs of
  float64 oracle steps, odd runs under one held action, even runs under a
  fresh action per step. Returns per slot the candidate states (C, N, 13)."""
  steps, runs = BURN[name]
  base = G['qp'][0]
  q = np.stack([base[b % base.shape[0]] for b in range(nb) for _ in range(runs)])
  rngs = [np.random.default_rng(80_000 + 1000 * b + s) for b in range(nb) for s in range(runs)]
  held = np.stack([r.uniform(-1, 1, A) for r in rngs])
  snaps = []
  for _ in range(steps):
    a = np.stack([held[i] if i % runs % 2 else r.uniform(-1, 1, A) for i, r in enumerate(rngs)])
    q, _ = o64.system_step(q, a)
    snaps.append(q)
  snaps = np.stack(snaps).reshape(steps, nb, runs, *q.shape[1:])
  return [snaps[:, b].reshape(-1, *q.shape[1:]) for b in range(nb)]


def _placed_candidates(name, o64, d, meta, G, A, nb):
  """Seeded search over placements of the object: the arm / hand moves under
  one held action for 0..BURN steps from the golden reset state, then the
  object is put so that its capsule's centre lies within the PLACED half-range
  per axis of the centre of the other capsule of one target row, and 0..2
  more steps follow."""
  steps, runs = BURN[name]
  base = G['qp'][0]
  obj, half = meta['body_index'][PLACED[name][0]], PLACED[name][1]
  pos = {0: np.asarray(d['row_a_pos'], np.float64), 1: np.asarray(d['row_b_pos'], np.float64)}
  body = {0: np.asarray(d['row_body_a']), 1: np.asarray(d['row_body_b'])}
  rad = np.asarray(d['row_a_radius'], np.float64) + np.asarray(d['row_b_radius'], np.float64)
  out = []
  for b in range(nb):
    cands = []
    for s in range(runs):
      rng = np.random.default_rng(81_000 + 1000 * b + s)
      held = rng.uniform(-1, 1, (1, A))
      q = base[b % base.shape[0]][None].copy()
      for _ in range(int(rng.integers(0, steps + 1))):
        q, _ = o64.system_step(q, held)
      row = int(rng.choice(TARGET[name]))
      h = half if half is not None else 0.5 * rad[row]
      off = rng.uniform(-h, h, 3)
      mine = 0 if body[0][row] == obj else 1  # the object's side of the row
      other = body[1 - mine][row]
      centre = q[0, other, 0:3] + _rotate(pos[1 - mine][row], q[0, other, 3:7])
      q[0, obj, 0:3] = centre + off - _rotate(pos[mine][row], q[0, obj, 3:7])
      cands.append(q[0])
      for _ in range(2):
        q, _ = o64.system_step(q, held)
        cands.append(q[0])
    out.append(np.stack(cands))
  return out


def select(lib, name, verbose=True):
  """The start states of `mid_<name>` (B or ENVS[name], N, 13) and a comment line."""
  from tests.conftest import golden
  from tests.helpers import WIDE, env_golden
  o64, env32, d, meta, coef = _oracles(lib, name)
  G = golden(env_golden(name))
  O, M = G['obs'].shape[-1], G['metrics'].shape[-1]
  nb = ENVS.get(name, B)
  acts = actions(G['action'].shape[-1], nb)  # the env's action width (Grasp: 3 past the system's)
  target = np.asarray(TARGET[name])
  cands = (_placed_candidates(name, o64, d, meta, G, o64.A, nb) if name in PLACED
           else _burn_candidates(name, o64, G, o64.A, nb))
  covered, jl_done, picks, notes = set(), False, [], []
  # the census wants MIN_GROUP active samples per collider group: the target
  # rows' groups are filled up to it
  tgroup = np.asarray(d['row_group'])[target]
  count = {int(g): 0 for g in np.unique(tgroup)}
  for b in range(nb):
    c = cands[b]
    # the two recorded steps of every candidate, in float64
    q0 = c
    a0, a1 = (np.repeat(acts[t, b][None], len(c), 0) for t in range(T))
    q1, i0 = o64.system_step(*pre_step(name, meta, q0, a0))
    q2, i1 = o64.system_step(*pre_step(name, meta, q1, a1))
    ok = np.isfinite(q2).all((1, 2)) & (np.abs(q2[..., 0:3]).max((1, 2)) < 50)
    hit = np.stack([i['contact_penetration'][:, target] > 0 for i in (i0, i1)])  # (T, C, rows)
    n_hit = hit.any(-1).sum(0) + 0.1 * hit.any(0).sum(-1)
    jl = (past_limit(o64, q0, LIMIT_MARGIN).any((1, 2))
          | past_limit(o64, q1, LIMIT_MARGIN).any((1, 2)))
    order = np.argsort(-(n_hit + 0.5 * jl) * ok, kind='stable')[:SHORTLIST]
    order = np.asarray([k for k in order if ok[k] and n_hit[k] > 0], int)
    assert order.size, f'{name}: env slot {b} has no candidate with a target row active'
    wc, dec = [], []
    for q, a in ((q0[order], a0[order]), (q1[order], a1[order])):
      e32, de, _ = conditioning(o64, env32, name, meta, q, a, O, M, coef)
      wc.append(2.0 * e32 <= WIDE)
      dec.append(de[:, target])
    wc, dec = np.stack(wc), np.stack(dec)  # (T, K), (T, K, rows)
    best, best_gain = None, -np.inf
    for k, ci in enumerate(order):
      act_rows = hit[:, ci] & dec[:, k]                       # decided active target rows
      good = wc[:, k] & act_rows.any(-1)                      # well-conditioned active samples
      bad = ~wc[:, k] & hit[:, ci].any(-1)                    # ill-conditioned active samples
      rows = set(target[(act_rows & wc[:, k][:, None]).any(0)].tolist())
      gain = (10 * len(rows - covered) + 3 * int(good.sum()) - 3 * int(bad.sum())
              + 4 * int(bool(jl[ci]) and not jl_done))
      per_group = {g: int(hit[:, ci][:, tgroup == g].any(-1).sum()) for g in count}
      gain += sum(8 * min(n, max(0, MIN_GROUP - count[g])) for g, n in per_group.items())
      if gain > best_gain:
        best, best_gain, best_rows, best_groups = ci, gain, rows, per_group
    covered |= best_rows
    for g, n in best_groups.items():
      count[g] += n
    jl_done |= bool(jl[best])
    picks.append(c[best])
    notes.append(f'env {b}: candidate {int(best)} of {len(c)}, rows {sorted(best_rows)}, '
                 f'past-limit {bool(jl[best])}')
    if verbose:
      print('  ' + notes[-1], flush=True)
  missing = sorted(set(target.tolist()) - covered)
  comment = (f'mid_{name}: start states picked by the float64 C oracle; target rows '
             f'{target.tolist()}; rows active, decided and well-conditioned: {sorted(covered)}; '
             f'not reached by the search: {missing}')
  return np.stack(picks), comment


def census(lib, name, T_, n_perturb=N_PERTURB):
  """Per sample of one fixture (golden arrays `T_`, system `name`): `pen > 0`
  of the recorded reference (T, B, R), well-conditioned (T, B), decided
  (T, B, R) and dofs past their limit by more than LIMIT_MARGIN at the
  sample's input (T, B)."""
  from tests.helpers import WIDE
  o64, env32, _, meta, coef = _oracles(lib, name, n_perturb)
  O, M = T_['obs'].shape[-1], T_['metrics'].shape[-1]
  well, dec, lim = [], [], []
  for t in range(T_['action'].shape[0]):
    e32, de, _ = conditioning(o64, env32, name, meta, T_['qp'][t], T_['action'][t], O, M, coef)
    well.append(2.0 * e32 <= WIDE)
    dec.append(de)
    lim.append(past_limit(o64, T_['qp'][t], LIMIT_MARGIN).sum((1, 2)))
  return T_['contact_penetration'] > 0, np.stack(well), np.stack(dec), np.stack(lim)
