"""Golden-vector generator — TEST INFRASTRUCTURE ONLY, never shipped.

Drives the reference's own numpy backend (`/root/reference/brax/jumpy.py:16-48`
dispatches every op to numpy when no jax array is present) through the test-only
stubs in `oracle/refstub/` and writes small `.npz` fixtures to `tests/golden/`:

  desc_<env>.npz   the reference System's compiled constant arrays
                   (`bodies.py:38-44`, `joints.py:418-474`, `actuators.py:115-164`,
                   `colliders.py:891-1023`, `integrators.py:32-48`), in the
                   descriptor layout of `brax_amd/system.py`.
  traj_<env>.npz   seeded reset states + random-action rollouts of the unwrapped
                   env (`Ant.step` `ant.py:222-255`, `Humanoid.step`
                   `humanoid.py:246-280`) or of `System.step` (`system.py:244-325`).
  wrap_ant.npz     an Episode+AutoReset wrapped rollout (`wrappers.py:83-148`).
  kat.npz          known answers from the reference's own tests/functions.

The reference computes in float64 here. The JAX PRNG is not
available, so reset noise is numpy `default_rng` (`jumpy.py:408-460`) and is
recorded explicitly: parity is defined on explicit states, never on seeds.

Refuses to run when /root/reference is absent, so nothing reference-derived can
run on the GPU box.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden')


def _setup():
  if not os.path.isdir(os.path.join(REF, 'brax')):
    raise SystemExit('gen_golden: /root/reference is absent; refusing to run')
  sys.path[:0] = [os.path.join(HERE, 'refstub'), REF]
  import warnings
  warnings.simplefilter('ignore')


# ---------------------------------------------------------------------------
# descriptor dump (reference objects -> flat arrays)
# ---------------------------------------------------------------------------

def dump_desc(sys_):
  """Flattens a reference brax.System into the brax_amd descriptor layout."""
  from brax.physics import joints as rj
  from brax.physics import actuators as ra
  from brax.physics import colliders as rc
  from brax.physics import geometry as rg
  d = {}
  body = sys_.body
  integ = sys_.integrator
  cfg = sys_.config
  d['n_bodies'] = np.int32(sys_.num_bodies)
  d['body_mass'] = np.asarray(body.mass, np.float64)
  d['body_inv_inertia'] = np.asarray(body.inertia, np.float64)
  d['pos_mask'] = np.asarray(integ.pos_mask, np.float64)
  d['rot_mask'] = np.asarray(integ.rot_mask, np.float64)
  d['quat_mask'] = np.asarray(integ.quat_mask, np.float64)
  d['h'] = np.float64(integ.dt)
  d['dt'] = np.float64(cfg.dt)
  d['substeps'] = np.int32(cfg.substeps)
  d['gravity'] = np.asarray(integ.gravity, np.float64)
  d['velocity_damping'] = np.float64(integ.velocity_damping)
  d['angular_damping'] = np.float64(integ.angular_damping)

  from brax.physics import spring_joints as sj
  jt, jd, jfree, jbp, jbc, joffp, joffc, jaxp, jaxc, jlim, jdamp = ([] for _ in range(11))
  jsp, jsa, jgrp = [], [], []
  jstiff, jsdamp, jlstr = [], [], []
  joint_base = []
  kinds = {rj.Revolute: 1, rj.Spherical: 3, sj.Revolute: 1, sj.Universal: 2, sj.Spherical: 3}
  spring = cfg.dynamics_mode == 'legacy_spring'
  d['dynamics_mode'] = np.int32(1 if spring else 0)
  for g, j in enumerate(sys_.joints):
    if type(j) not in kinds:
      raise RuntimeError('unsupported joint type %r' % type(j))
    n = len(j.body_p.idx)
    joint_base.append(len(jt))
    for k in range(n):
      jt.append(kinds[type(j)])
      if spring:
        jstiff.append(j.stiffness[k])
        jsdamp.append(j.spring_damping[k])
        jlstr.append(j.limit_strength[k])
      else:
        jstiff.append(0.)
        jsdamp.append(0.)
        jlstr.append(0.)
      jd.append(j.dof)
      jfree.append(j.free_dofs[k] if j.free_dofs is not None else -1)
      jbp.append(j.body_p.idx[k])
      jbc.append(j.body_c.idx[k])
      joffp.append(j.off_p[k])
      joffc.append(j.off_c[k])
      jaxp.append(j.axis_p[k])
      jaxc.append(j.axis_c[k])
      lim = np.zeros((3, 2))
      lim[:j.dof] = j.limit[k]
      jlim.append(lim)
      jdamp.append(j.angular_damping[k])
      jsp.append(j.scale_pos[k] if not spring else 0.)
      jsa.append(j.scale_ang[k] if not spring else 0.)
      jgrp.append(g)
  d['joint_type'] = np.asarray(jt, np.int32)
  d['joint_dof'] = np.asarray(jd, np.int32)
  d['joint_free_dofs'] = np.asarray(jfree, np.int32)
  d['joint_body_p'] = np.asarray(jbp, np.int32)
  d['joint_body_c'] = np.asarray(jbc, np.int32)
  d['joint_off_p'] = np.asarray(joffp, np.float64).reshape(-1, 3)
  d['joint_off_c'] = np.asarray(joffc, np.float64).reshape(-1, 3)
  d['joint_axis_p'] = np.asarray(jaxp, np.float64).reshape(-1, 3, 3)
  d['joint_axis_c'] = np.asarray(jaxc, np.float64).reshape(-1, 3, 3)
  d['joint_limit'] = np.asarray(jlim, np.float64).reshape(-1, 3, 2)
  d['joint_damping'] = np.asarray(jdamp, np.float64)
  d['joint_scale_pos'] = np.asarray(jsp, np.float64)
  d['joint_scale_ang'] = np.asarray(jsa, np.float64)
  d['joint_group'] = np.asarray(jgrp, np.int32)
  d['joint_stiffness'] = np.asarray(jstiff, np.float64)
  d['joint_spring_damping'] = np.asarray(jsdamp, np.float64)
  d['joint_limit_strength'] = np.asarray(jlstr, np.float64)

  at, aj, astr, aidx, agrp = [], [], [], [], []
  for g, a in enumerate(sys_.actuators):
    # locate the joint group this actuator's joints came from
    for k in range(len(a.strength)):
      at.append(0 if isinstance(a, ra.Torque) else 1)
      # global joint index: match by (parent, child) body indices
      bp, bc = a.joint.body_p.idx[k], a.joint.body_c.idx[k]
      cand = [i for i in range(len(jt)) if jbp[i] == bp and jbc[i] == bc]
      aj.append(cand[0])
      astr.append(a.strength[k])
      idx = -np.ones(3, np.int64)
      idx[:a.act_index.shape[1]] = a.act_index[k]
      aidx.append(idx)
      agrp.append(g)
  d['act_type'] = np.asarray(at, np.int32)
  d['act_joint'] = np.asarray(aj, np.int32)
  d['act_strength'] = np.asarray(astr, np.float64)
  d['act_index'] = np.asarray(aidx, np.int32).reshape(-1, 3)
  d['act_group'] = np.asarray(agrp, np.int32)

  # forces (forces.py:27-138), application order
  from brax.physics import forces as rf
  ft, fb, fs, fi = [], [], [], []
  for f in sys_.forces:
    for k in range(len(f.strength)):
      ft.append(0 if isinstance(f, rf.Thruster) else 1)
      fb.append(int(f.body.idx[k]))
      fs.append(float(f.strength[k]))
      fi.append(np.asarray(f.act_index[k]))
  d['force_type'] = np.asarray(ft, np.int32)
  d['force_body'] = np.asarray(fb, np.int32)
  d['force_strength'] = np.asarray(fs, np.float64)
  d['force_index'] = np.asarray(fi, np.int32).reshape(-1, 3)
  d['action_size'] = np.int32(sys_.num_joint_dof + sys_.num_forces_dof)
  d['num_joint_dof'] = np.int32(sys_.num_joint_dof)

  goneway, gfn, gscale, gthr, gerp = [], [], [], [], []
  rows = {k: [] for k in ('group', 'body_a', 'body_b', 'a_pos', 'a_end', 'a_radius',
                          'b_pos', 'b_end', 'b_radius', 'friction', 'elasticity', 'flat',
                          'nn_masked', 'ext', 'hm')}
  hm_data = []
  hull_ix, hull_v, hull_f, hull_n = {}, [], [], []
  gcut = []
  for g, c in enumerate(sys_.colliders):
    if isinstance(c.cull, rc.NearNeighbors):
      # the reference's own NN object: its allowed cells are the finite
      # entries of dist_off (colliders.py:63-66), in flat order
      cand_a, cand_b = c.cull.candidate_a, c.cull.candidate_b
      off = np.asarray(c.cull.dist_off)
      U = off.shape[1]
      cells = np.flatnonzero(np.isfinite(off.ravel()))
      # more cutoff than allowed cells: top_k's tail is the masked (-inf)
      # cells of lowest flat index (jax.lax.top_k's order for equal values)
      extra = np.flatnonzero(~np.isfinite(off.ravel()))[:max(int(c.cull.cutoff) - len(cells), 0)]
      cells = np.sort(np.concatenate([cells, extra]))
      nn_masked = list((~np.isfinite(off.ravel()[cells])).astype(int))
      ia, ib = cells // U, cells % U
      from brax import jumpy as jp
      ca, cb = jp.take(cand_a, ia), jp.take(cand_b, ib)
      flats = list(cells)
      gcut.append(int(c.cull.cutoff))
    else:
      ca, cb = c.cull.get()
      flats = None
      nn_masked = None
      gcut.append(0)
    goneway.append(1 if isinstance(c, rc.OneWayCollider) else 0)
    fn = c.contact_fn.__name__
    gfn.append({'capsule_plane': 0, 'capsule_capsule': 1, 'box_plane': 0,
                'mesh_plane': 0, 'box_heightmap': 2, 'capsule_clippedplane': 3,
                'capsule_mesh': 4, 'hull_hull': 5}[fn])
    gscale.append(c.collide_scale)
    gthr.append(c.velocity_threshold)
    gerp.append(c.baumgarte_erp)
    P = len(ca.body.idx)
    for p in range(P):
      ext = None
      hm = (-1, 0)
      if fn in ('box_plane', 'box_heightmap'):
        ends = list(ca.corner[p])  # corner rows, zero radius
        if fn == 'box_heightmap':
          hm = (len(hm_data), int(cb.height[p].shape[0]))
          hm_data.extend(np.asarray(cb.height[p], np.float64).reshape(-1).tolist())
          ext = [np.r_[cb.cell_size[p], np.zeros(15)]] * len(ends)
      elif fn == 'mesh_plane':
        ends = list(ca.vertices[p])
      elif fn == 'capsule_mesh':
        F = cb.faces[p].shape[0]
        ends = [ca.end[p]] * F
        ext = [np.r_[np.asarray(cb.faces[p][f]).reshape(-1), cb.face_normals[p][f], np.zeros(4)]
               for f in range(F)]
      elif fn == 'hull_hull':
        ends = [np.zeros(3)] * 4
        hx = []
        for col, p_ in ((ca, p), (cb, p)):
          key = (int(col.body.idx[p_]), tuple(np.round(np.asarray(col.vertices[p_]).ravel(), 12)))
          if key not in hull_ix:
            hull_ix[key] = len(hull_v)
            hull_v.append(np.asarray(col.vertices[p_]))
            hull_f.append(np.asarray(col.faces[p_]))
            hull_n.append(np.asarray(col.face_normals[p_]))
          hx.append(hull_ix[key])
        ext = [np.r_[hx[0], hx[1], e, np.zeros(13)] for e in range(4)]
      elif fn == 'capsule_clippedplane':
        ends = list(ca.end[p])
        ext = [np.r_[cb.normal[p], cb.x[p], cb.y[p], cb.pos[p], cb.halfsize_x[p],
                     cb.halfsize_y[p], np.zeros(2)]] * len(ends)
      else:
        ends = [ca.end[p]] if fn == 'capsule_capsule' else list(ca.end[p])
      if ext is None:
        ext = [np.zeros(16)] * len(ends)
      for ei, e in enumerate(ends):
        rows['ext'].append(ext[ei])
        rows['hm'].append(hm)
        rows['flat'].append(-1 if flats is None else int(flats[p]))
        rows['nn_masked'].append(0 if nn_masked is None else int(nn_masked[p]))
        rows['group'].append(g)
        rows['body_a'].append(ca.body.idx[p])
        rows['body_b'].append(cb.body.idx[p])
        rows['a_pos'].append(ca.pos[p])
        rows['a_end'].append(e)
        rows['a_radius'].append(ca.radius[p] if fn not in ('box_plane', 'mesh_plane',
                                                           'box_heightmap', 'hull_hull') else 0.)
        rows['b_pos'].append(cb.pos[p])
        rows['b_end'].append(cb.end[p] if fn == 'capsule_capsule' else np.zeros(3))
        rows['b_radius'].append(cb.radius[p] if fn == 'capsule_capsule' else 0.)
        rows['friction'].append(ca.friction[p] * cb.friction[p])
        rows['elasticity'].append(ca.elasticity[p] * cb.elasticity[p])
  d['col_oneway'] = np.asarray(goneway, np.int32)
  d['col_cutoff'] = np.asarray(gcut, np.int32)
  d['col_fn'] = np.asarray(gfn, np.int32)
  d['col_scale'] = np.asarray(gscale, np.float64)
  d['col_velocity_threshold'] = np.asarray(gthr, np.float64)
  d['col_baumgarte_erp'] = np.asarray(gerp, np.float64)
  d['row_ext'] = np.asarray(rows.pop('ext'), np.float64).reshape(-1, 16)
  d['row_hm'] = np.asarray(rows.pop('hm'), np.int32).reshape(-1, 2)
  d['hm_data'] = np.asarray(hm_data, np.float64)
  d['hull_vert'] = np.asarray(hull_v, np.float64).reshape(-1, 8, 3)
  d['hull_face'] = np.asarray(hull_f, np.float64).reshape(-1, 6, 4, 3)
  d['hull_norm'] = np.asarray(hull_n, np.float64).reshape(-1, 6, 3)
  ints = ('group', 'body_a', 'body_b', 'flat', 'nn_masked')
  if not any(rows['nn_masked']):
    rows.pop('nn_masked')  # the key exists only where a masked cell is a row
  for k, v in rows.items():
    if k in ints:
      d['row_' + k] = np.asarray(v, np.int32)
    else:
      arr = np.asarray(v, np.float64)
      d['row_' + k] = arr.reshape(-1, 3) if k.endswith(('pos', 'end')) else arr
  return d


def qp_pack(qp):
  """QP -> (..., N, 13) float64: pos, rot(wxyz), vel, ang."""
  return np.concatenate([np.asarray(qp.pos), np.asarray(qp.rot),
                         np.asarray(qp.vel), np.asarray(qp.ang)], axis=-1)


def qp_unpack(a):
  from brax.physics.base import QP
  a = np.asarray(a, np.float64)
  return QP(pos=a[..., 0:3].copy(), rot=a[..., 3:7].copy(), vel=a[..., 7:10].copy(),
            ang=a[..., 10:13].copy())


# ---------------------------------------------------------------------------
# trajectories
# ---------------------------------------------------------------------------

def env_traj(env, name, n_envs, n_steps, act_seed_base=10_000, qp0=None):
  """Unwrapped env: reset from seeds 0..B-1, then T random-action steps.
  `qp0`: a list of per-env start states (n_envs of (N, 13) arrays); each
  env's State is its reset State with `qp` replaced, so `qp[0]` is the start
  state while `obs[0]`, `reset_obs`, `reset_qpos` and `reset_qvel` stay the
  reset's."""
  A = env.action_size
  label, name = name, name[len('mid_'):] if name.startswith('mid_') else name
  out = {k: [] for k in ('qp', 'obs', 'reward', 'done', 'metrics', 'info_contact',
                         'info_actuator', 'contact_pos', 'contact_normal',
                         'contact_penetration')}
  qpos_l, qvel_l = [], []
  states = []
  from brax import jumpy as jp
  for s in range(n_envs):
    rng = np.array([s, 0], np.uint32)
    if hasattr(env, '_noise'):
      # re-derive the reset noise exactly as Env.reset does (`ant.py:198-203`)
      _, r1, r2 = jp.random_split(rng, 3)
      qpos_l.append(env.sys.default_angle() + env._noise(r1))
      qvel_l.append(env._noise(r2))
    elif name in ('reacher', 'reacherangle'):
      # reacher.py:172-176 / reacherangle.py:60-64 draw their noise inline
      _, r1, r2 = jp.random_split(rng, 3)
      D = env.sys.num_joint_dof
      qpos_l.append(env.sys.default_angle() + jp.random_uniform(r1, (D,), -.1, .1))
      qvel_l.append(jp.random_uniform(r2, (D,), -.005, .005))
    elif name == 'pusher':
      # pusher.py:178-195: default angles, velocity noise on all but 4 dofs
      _, _, r2 = jp.random_split(rng, 3)
      D = env.sys.num_joint_dof
      qpos_l.append(env.sys.default_angle())
      qvel_l.append(np.concatenate([jp.random_uniform(r2, (D - 4,), -0.005, 0.005), np.zeros(4)]))
    elif name in ('ur5e', 'fetch', 'grasp'):
      # ur5e.py:59, fetch.py:43, grasp.py:43: the default pose, at rest
      qpos_l.append(env.sys.default_angle())
      qvel_l.append(np.zeros(env.sys.num_joint_dof))
    elif name == 'acrobot':
      # acrobot.py:56-61 draws the same U[-.01, .01) noise inline
      _, r1, r2 = jp.random_split(rng, 3)
      D = env.sys.num_joint_dof
      qpos_l.append(env.sys.default_angle() + jp.random_uniform(r1, (D,), -.01, .01))
      qvel_l.append(jp.random_uniform(r2, (D,), -.01, .01))
    states.append(env.reset(rng))
  if qp0 is not None:
    assert len(qp0) == n_envs
    states = [s.replace(qp=qp_unpack(q)) for s, q in zip(states, qp0)]
  acts = np.stack([np.random.default_rng(act_seed_base + t).uniform(-1, 1, (n_envs, A))
                   for t in range(n_steps)])
  metric_keys = sorted(states[0].metrics.keys())

  def rec(sts, sys_infos):
    out['qp'].append(np.stack([qp_pack(s.qp) for s in sts]))
    out['obs'].append(np.stack([np.asarray(s.obs) for s in sts]))

  rec(states, None)
  reset_obs = out['obs'][0]
  t0 = time.time()
  for t in range(n_steps):
    new = []
    infos = []
    for b, s in enumerate(states):
      # capture the Info of the System.step that Env.step makes
      captured = []
      orig = env.sys.step
      def spy(qp, act, _orig=orig):
        r = _orig(qp, act)
        captured.append(r[1])
        return r
      env.sys.step = spy
      try:
        new.append(env.step(s, acts[t, b]))
      finally:
        del env.sys.step
      infos.append(captured[0])
    states = new
    rec(states, infos)
    out['reward'].append(np.array([float(s.reward) for s in states]))
    out['done'].append(np.array([float(s.done) for s in states]))
    out['metrics'].append(np.array([[float(s.metrics[k]) for k in metric_keys]
                                    for s in states]))
    out['info_contact'].append(np.stack([np.concatenate(
        [i.contact.vel, i.contact.ang], -1) for i in infos]))
    out['info_actuator'].append(np.stack([np.concatenate(
        [i.actuator.vel, i.actuator.ang], -1) for i in infos]))
    out['contact_pos'].append(np.stack([i.contact_pos for i in infos]))
    out['contact_normal'].append(np.stack([i.contact_normal for i in infos]))
    out['contact_penetration'].append(np.stack([i.contact_penetration for i in infos]))
    print(f'  {label}: step {t + 1}/{n_steps}  ({time.time() - t0:.1f}s)', flush=True)
  res = {k: np.stack(v) for k, v in out.items() if v}
  res['action'] = acts
  if qpos_l:
    res['reset_qpos'] = np.stack(qpos_l)
    res['reset_qvel'] = np.stack(qvel_l)
  res['reset_obs'] = reset_obs
  res['metric_keys'] = np.array(metric_keys)
  return res


class record_top_k:
  """Records every NearNeighbors selection `NearNeighbors.update` makes
  (colliders.py:71-85): each `jumpy.top_k` call's operand (sim = -(dist +
  dist_off), all candidate cells, flat) and the indices it returns (the
  selected cells, nearest first), in call (= collider) order. Wraps
  whichever top_k is installed (numpy's, or stable_top_k's)."""

  def __enter__(self):
    from brax import jumpy
    self.jp, self.orig = jumpy, jumpy.top_k
    self.calls = []

    def top_k(operand, k):
      val, idx = self.orig(operand, k)
      self.calls.append((np.asarray(operand, np.float64).copy(), np.asarray(idx).copy()))
      return val, idx
    jumpy.top_k = top_k
    return self

  def take(self):
    c, self.calls = self.calls, []
    return c

  def __exit__(self, *exc):
    self.jp.top_k = self.orig


def sys_traj(sys_, name, qp0, n_envs, n_steps, act_scale, A, seed_base=20_000):
  """Physics-only System.step rollout from a fixed state. For systems with
  NearNeighbors culling, also the reference's own selection per step and
  env: `nn_cell` (T, B, sum of cutoffs) the top_k indices (flat cells i * U +
  j, nearest first, culled groups in collider order) and `nn_sim` (T, B,
  sum of U * U) the similarities top_k ranked."""
  from brax.physics import colliders as rc
  out = {k: [] for k in ('qp', 'info_contact', 'info_actuator', 'contact_penetration')}
  acts = np.stack([np.random.default_rng(seed_base + t).uniform(-1, 1, (n_envs, A))
                   * act_scale for t in range(n_steps)])
  # one start state for every env, or a list of per-env start states
  qps = list(qp0) if isinstance(qp0, list) else [qp0 for _ in range(n_envs)]
  out['qp'].append(np.stack([qp_pack(q) for q in qps]))
  t0 = time.time()
  culled = any(isinstance(c.cull, rc.NearNeighbors) for c in sys_.colliders)
  cells, sims = [], []
  for t in range(n_steps):
    if culled:
      res, cs, ss = [], [], []
      with record_top_k() as rec:
        for b, q in enumerate(qps):
          res.append(sys_.step(q, acts[t, b]))
          calls = rec.take()
          cs.append(np.concatenate([i for _, i in calls]).astype(np.int32))
          ss.append(np.concatenate([o for o, _ in calls]))
      cells.append(np.stack(cs))
      sims.append(np.stack(ss))
    else:
      res = [sys_.step(q, acts[t, b]) for b, q in enumerate(qps)]
    qps = [r[0] for r in res]
    out['qp'].append(np.stack([qp_pack(q) for q in qps]))
    out['info_contact'].append(np.stack([np.concatenate(
        [r[1].contact.vel, r[1].contact.ang], -1) for r in res]))
    out['info_actuator'].append(np.stack([np.concatenate(
        [r[1].actuator.vel, r[1].actuator.ang], -1) for r in res]))
    out['contact_penetration'].append(np.stack([r[1].contact_penetration for r in res]))
    print(f'  {name}: step {t + 1}/{n_steps}  ({time.time() - t0:.1f}s)', flush=True)
  r = {k: np.stack(v) for k, v in out.items()}
  r['action'] = acts
  if culled:
    r['nn_cell'] = np.stack(cells)
    r['nn_sim'] = np.stack(sims)
  return r


def ant_mountain_sys(count, cutoff=0):
  """Ant Mountain scene, as built in `notebooks/multiagent.ipynb` cell 3."""
  from brax import envs
  import brax
  config = envs.create('ant').sys.config
  repeat = count - 1
  for lst in (config.bodies, config.joints, config.actuators):
    for obj in list(lst):
      if obj.name == 'Ground':
        continue
      for i in range(repeat):
        new_obj = lst.add()
        new_obj.CopyFrom(obj)
        for attr in ('name', 'joint', 'parent', 'child'):
          if hasattr(new_obj, attr):
            setattr(new_obj, attr, f'{getattr(new_obj, attr)}_{i}')
  default = config.defaults.add()
  for i in range(repeat):
    qp = default.qps.add(name=f'$ Torso_{i}')
    qp.pos.x = np.sin(i * np.pi / 2)
    qp.pos.y = np.cos(i * np.pi / 2)
    qp.pos.z = (i + 1) * 2
  del config.collide_include[:]
  config.collider_cutoff = cutoff
  return brax.System(config)


# the CapsuleTest scene (`physics_test.py:292-328`), as test input data
CAPSULE_TEST_CONFIG = """
dt: 20.0 substeps: 10000 friction: 0.6 gravity { z: -9.8 }
bodies { name: "Capsule1" mass: 1 colliders { capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule2" mass: 1 colliders { rotation { y: 90 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule3" mass: 1 colliders { rotation { y: 45 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Capsule4" mass: 1 colliders { rotation { x: 45 } capsule { radius: 0.25 length: 1.0 } } inertia { x: 1 y: 1 z: 1 } }
bodies { name: "Ground" frozen { all: true } colliders { plane {} } }
defaults { qps { name: "Capsule1" pos { z: 1 } } qps { name: "Capsule2" pos { x: 1 z: 1 } } qps { name: "Capsule3" pos { x: 3 z: 1 } } qps { name: "Capsule4" pos { x: 5 z: 1 } } }
defaults { qps { name: "Capsule1" pos { z: 1 } } qps { name: "Capsule2" pos { z: 2 } } qps { name: "Capsule3" pos { x: 3 z: 1 } } qps { name: "Capsule4" pos { x: 5 z: 1 } } }
"""


def capsule_sys(kind):
  """`physics_test.py:290-361` CapsuleTest scenes (numpy backend, not jit):
  'ground' (default 0, dt 20, 10000 substeps), 'capsule' (default 1, dt 2,
  400 substeps) and 'cull' (as 'capsule' with collider_cutoff = 1)."""
  import brax
  from google.protobuf import text_format
  config = text_format.Parse(CAPSULE_TEST_CONFIG, brax.Config())
  if kind != 'ground':
    config.dt = 2.0
    config.substeps = 400
  if kind == 'cull':
    config.collider_cutoff = 1
  return brax.System(config), (0 if kind == 'ground' else 1)


class stable_top_k:
  """jumpy.top_k's numpy path with jax.lax.top_k's order for equal values
  (lower index first); the numpy path (argpartition + argsort) picks among
  ties arbitrarily, which decides WHICH masked NearNeighbors cells a cutoff
  past the allowed cells returns. Used for twin_cull only."""

  def __enter__(self):
    from brax import jumpy
    self.jp, self.orig = jumpy, jumpy.top_k

    def top_k(operand, k):
      if jumpy._which_np(operand) is not np:  # pylint: disable=protected-access
        return self.orig(operand, k)
      idx = np.argsort(-np.asarray(operand), kind='stable')[:k]
      return operand[idx], idx
    jumpy.top_k = top_k
    return self

  def __exit__(self, *exc):
    self.jp.top_k = self.orig


class jit_index_update:
  """jumpy.index_update (`jumpy.py:161-167`) with jit's scatter semantics:
  under jit `x.at[idx].set(y)` drops the index tuples that fall outside x
  (XLA scatter), where the numpy path raises IndexError. NearNeighbors sets its
  allowed cells with BODY indices into the (U, U) candidate matrix
  (`colliders.py:63-67`); in Ant Mountain(2+) the last ants' bodies index past
  U, so only the jit semantics construct the scene. Used for mountain4nn."""

  def __enter__(self):
    from brax import jumpy
    self.jp, self.orig = jumpy, jumpy.index_update

    def index_update(x, idx, y):
      if jumpy._which_np(x, idx, y) is not np or not isinstance(idx, tuple):  # pylint: disable=protected-access
        return self.orig(x, idx, y)
      shape = np.shape(x)
      ii = [np.asarray(i) for i in idx]
      keep = np.ones(np.broadcast(*ii).shape, bool)
      for i, n in zip(ii, shape):
        keep &= (i >= -n) & (i < n)
      x = np.copy(x)
      x[tuple(np.broadcast_to(i, keep.shape)[keep] for i in ii)] = y
      return x
    jumpy.index_update = index_update
    return self

  def __exit__(self, *exc):
    self.jp.index_update = self.orig


def wrapped_ant(n_envs=8, n_steps=6, episode_length=3, action_repeat=1):
  """Episode + AutoReset wrapped Ant (`envs/__init__.py:74-92`); with
  action_repeat > 1 the EpisodeWrapper scans that many env steps per step
  and sums their rewards (`wrappers.py:105-120`)."""
  from brax import envs
  env = envs.create('ant', episode_length=episode_length, action_repeat=action_repeat,
                    auto_reset=True, batch_size=n_envs)
  st = env.reset(np.array([7, 0], np.uint32))
  out = {k: [] for k in ('qp', 'obs', 'reward', 'done', 'steps', 'truncation')}
  out['first_qp'] = qp_pack(st.info['first_qp'])
  out['first_obs'] = np.asarray(st.info['first_obs'])
  def rec(s):
    out['qp'].append(qp_pack(s.qp))
    out['obs'].append(np.asarray(s.obs))
    out['reward'].append(np.asarray(s.reward, np.float64))
    out['done'].append(np.asarray(s.done, np.float64))
    out['steps'].append(np.asarray(s.info['steps'], np.float64))
    out['truncation'].append(np.asarray(s.info['truncation'], np.float64))
  rec(st)
  acts = np.stack([np.random.default_rng(30_000 + t).uniform(-1, 1, (n_envs, 8))
                   for t in range(n_steps)])
  # force an unhealthy env to exercise done-driven auto-reset: lift env 0's ant
  for t in range(n_steps):
    st = env.step(st, acts[t])
    rec(st)
  r = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
  r['action'] = acts
  r['episode_length'] = np.int32(episode_length)
  r['action_repeat'] = np.int32(action_repeat)
  return r


def gym_ant(n_envs=8, n_steps=6, episode_length=3):
  """The reference's gym path: `envs.create_gym_env('ant', batch_size=B,
  episode_length=L)` (`envs/__init__.py:118-130`) -> VectorGymWrapper, whose
  jitted step returns (obs, reward, done, info = {**state.metrics,
  **state.info}) (`wrappers.py:311-314`); JaxToTorchWrapper (`to_torch.py:
  28-64`) only converts those leaves. Records every leaf of every step's
  return and the wrapped state the steps start from (`_state` after reset:
  the reset key is parity-unpinned, so the build starts from these arrays).
  jax.jit and jax.random.PRNGKey are absent offline: during this call jit is
  the identity (the numpy backend runs the same function eagerly) and
  PRNGKey(seed) is the (2,) uint32 key layout [0, seed]."""
  import types
  import jax
  from brax import envs
  saved = {k: getattr(jax, k, None) for k in ('jit', 'random')}
  jax.jit = lambda fun, **_: fun
  jax.random = types.SimpleNamespace(PRNGKey=lambda seed: np.array([0, seed], np.uint32))
  try:
    g = envs.create_gym_env('ant', batch_size=n_envs, seed=5, episode_length=episode_length)
    g.reset()
    st = g._state  # pylint: disable=protected-access
    out = {'qp0': qp_pack(st.qp), 'obs0': np.asarray(st.obs),
           'reward0': np.asarray(st.reward, np.float64), 'done0': np.asarray(st.done, np.float64),
           'first_qp': qp_pack(st.info['first_qp']), 'first_obs': np.asarray(st.info['first_obs']),
           'steps0': np.asarray(st.info['steps'], np.float64),
           'truncation0': np.asarray(st.info['truncation'], np.float64)}
    acts = np.stack([np.random.default_rng(40_000 + t).uniform(-1, 1, (n_envs, 8))
                     for t in range(n_steps)])
    rec = {}
    keys = None
    for t in range(n_steps):
      obs, reward, done, info = g.step(acts[t])
      if keys is None:
        keys = sorted(info)
      assert sorted(info) == keys
      rec.setdefault('obs', []).append(np.asarray(obs))
      rec.setdefault('reward', []).append(np.asarray(reward, np.float64))
      rec.setdefault('done', []).append(np.asarray(done, np.float64))
      rec.setdefault('qp', []).append(qp_pack(g._state.qp))  # pylint: disable=protected-access
      for k in keys:
        v = info[k]
        v = qp_pack(v) if k == 'first_qp' else np.asarray(v, np.float64)
        rec.setdefault('info_' + k, []).append(v)
  finally:
    for k, v in saved.items():
      if v is None:
        delattr(jax, k)
      else:
        setattr(jax, k, v)
  out.update({k: np.stack(v) for k, v in rec.items()})
  out['action'] = acts
  out['info_keys'] = np.array(keys)
  out['episode_length'] = np.int32(episode_length)
  return out


# NaN / Inf poisoning (`step` never raises, NaN/Inf propagate):
# (env, what, where, value). 'qp' entries poison the state the rollout starts
# from (field slice start, body, component); 'act' entries poison one action
# element at one step (step, index). The other envs stay clean, so a test can
# also hold them to the bits of an unpoisoned run (batch isolation).
NAN_PLAN = {
    'ant': [(1, 'qp', (7, 0, 0), np.nan),      # torso vel x
            (2, 'act', (1, 3), np.nan),        # one action element at step 1
            (4, 'act', (0, 0), np.inf),        # +Inf action at step 0
            (6, 'qp', (0, 3, 2), -np.inf)],    # a leg's pos z = -Inf
    'humanoid': [(1, 'qp', (7, 0, 0), np.nan),
                 (2, 'act', (1, 5), np.nan),
                 (4, 'act', (0, 0), np.inf),
                 (6, 'qp', (0, 0, 2), np.inf)],  # torso pos z = +Inf
}


def _poison_qp(a, plan):
  a = np.array(a, np.float64, copy=True)
  for b, what, loc, v in plan:
    if what == 'qp':
      f, body, k = loc
      a[b, body, f + k] = v
  return a


def _poison_act(acts, plan):
  acts = np.array(acts, np.float64, copy=True)
  for b, what, loc, v in plan:
    if what == 'act':
      t, i = loc
      acts[t, b, i] = v
  return acts


def nan_env(kind, n_envs=8, n_steps=6, episode_length=4):
  """The reference's Episode+AutoReset wrapped `kind` (`envs/__init__.py:74-92`)
  stepped from its reset with NaN / Inf put into some envs' state or actions
  (NAN_PLAN). Records the poisoned start state, the actions and every step's
  qp / obs / reward / done / steps / truncation / metrics. The episode ends
  inside the run, so a poisoned env that the reference keeps (done = 0:
  `jp.where(z < min_z, 0, 1)` is 1 for NaN, `ant.py:229-231`) is reset at the
  truncation step (`wrappers.py:138-148`)."""
  from brax import envs
  from brax.physics.base import QP
  plan = NAN_PLAN[kind]
  from brax.envs import wrappers
  # the registry's 'humanoid' is the fork's humanoid_new; the kernel's Humanoid
  # kind is `brax/envs/humanoid.py` (as traj_humanoid): the create() chain
  # (`envs/__init__.py:74-92`) built around that class
  base = (importlib.import_module('brax.envs.humanoid').Humanoid() if kind == 'humanoid'
          else envs.get_environment(kind))
  env = wrappers.AutoResetWrapper(wrappers.VectorWrapper(
      wrappers.EpisodeWrapper(base, episode_length, 1), n_envs))
  st = env.reset(np.array([11, 0], np.uint32))
  qp0 = _poison_qp(qp_pack(st.qp), plan)
  st = st.replace(qp=qp_unpack(qp0))
  out = {k: [] for k in ('qp', 'obs', 'reward', 'done', 'steps', 'truncation', 'metrics')}
  out['first_qp'] = qp_pack(st.info['first_qp'])
  out['first_obs'] = np.asarray(st.info['first_obs'])
  keys = sorted(st.metrics)
  def rec(s):
    out['qp'].append(qp_pack(s.qp))
    out['obs'].append(np.asarray(s.obs))
    out['reward'].append(np.asarray(s.reward, np.float64))
    out['done'].append(np.asarray(s.done, np.float64))
    out['steps'].append(np.asarray(s.info['steps'], np.float64))
    out['truncation'].append(np.asarray(s.info['truncation'], np.float64))
    out['metrics'].append(np.stack([np.asarray(s.metrics[k], np.float64) for k in keys], -1))
  rec(st)
  A = env.action_size
  acts = _poison_act(np.stack([np.random.default_rng(50_000 + t).uniform(-1, 1, (n_envs, A))
                               for t in range(n_steps)]), plan)
  with np.errstate(all='ignore'):
    for t in range(n_steps):
      st = env.step(st, acts[t])
      rec(st)
      print(f'  nan_{kind}: step {t + 1}/{n_steps}', flush=True)
  r = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
  r['action'] = acts
  r['metric_keys'] = np.array(keys)
  r['episode_length'] = np.int32(episode_length)
  r['poisoned'] = np.array(sorted({p[0] for p in plan}), np.int32)
  return r


def nan_mountain(n_steps=2):
  """Ant Mountain(4), all pairs (the MULTI kernel's scene): `System.step`
  from default_qp with env 1's first ant's torso velocity NaN and env 2's
  last ant's torso pos z +Inf; env 0 clean. The reference's capsule-capsule
  rows multiply their impulses by masks (`p = dlambda * n * coll_mask`,
  colliders.py:332-333), so a NaN pair's impulse is NaN even where the mask
  is 0 and reaches the other body of the pair."""
  s = ant_mountain_sys(4)
  q0 = qp_pack(s.default_qp())
  qs = np.stack([q0, q0, q0])
  qs[1, 0, 7] = np.nan
  qs[2, s.body.index['$ Torso_2'], 2] = np.inf  # the last ant's torso
  with np.errstate(all='ignore'):
    r = sys_traj(s, 'nan_mountain4', [qp_unpack(q) for q in qs], 3, n_steps, 1.0, 32)
  return r


def eval_ant(n_envs=8, n_steps=7, episode_length=3):
  """The reference's `envs.create('ant', ..., eval_metrics=True)` chain
  (`envs/__init__.py:74-92`: Episode, Vector, AutoReset, then EvalWrapper,
  `wrappers.py:168-202`) stepped from its reset: every step's state and
  `eval_metrics` (episode_metrics per key, active_episodes, episode_steps).
  The episode ends inside the run, so the metrics stop accumulating for every
  env at the truncation step and active_episodes drops to 0 there; env 3's
  torso is lifted above the healthy range at the start, so it terminates
  (done from `is_healthy`, `ant.py:229-241`) on the first step."""
  from brax import envs
  env = envs.create('ant', episode_length=episode_length, batch_size=n_envs, eval_metrics=True)
  st = env.reset(np.array([9, 0], np.uint32))
  q = qp_pack(st.qp)
  q[3, :, 2] += 2.0  # env 3 above max_z = 1.0: unhealthy after one step
  st = st.replace(qp=qp_unpack(q))
  em = st.info['eval_metrics']
  keys = sorted(em.episode_metrics)
  out = {'qp0': qp_pack(st.qp), 'obs0': np.asarray(st.obs),
         'first_qp': qp_pack(st.info['first_qp']), 'first_obs': np.asarray(st.info['first_obs']),
         'reset_metrics': np.stack([np.asarray(st.metrics[k], np.float64) for k in keys], -1)}
  acts = np.stack([np.random.default_rng(60_000 + t).uniform(-1, 1, (n_envs, 8))
                   for t in range(n_steps)])
  rec = {}
  for t in range(n_steps):
    st = env.step(st, acts[t])
    em = st.info['eval_metrics']
    for k, v in (('qp', qp_pack(st.qp)), ('obs', np.asarray(st.obs)),
                 ('reward', np.asarray(st.reward, np.float64)),
                 ('done', np.asarray(st.done, np.float64)),
                 ('steps', np.asarray(st.info['steps'], np.float64)),
                 ('episode_metrics', np.stack([np.asarray(em.episode_metrics[k], np.float64)
                                               for k in keys], -1)),
                 ('active_episodes', np.asarray(em.active_episodes, np.float64)),
                 ('episode_steps', np.asarray(em.episode_steps, np.float64))):
      rec.setdefault(k, []).append(v)
  out.update({k: np.stack(v) for k, v in rec.items()})
  out['action'] = acts
  out['metric_keys'] = np.array(keys)
  out['episode_length'] = np.int32(episode_length)
  return out


def kats():
  """Known answers: the reference's own geometry/math functions."""
  from brax import math as bm
  from brax.physics import geometry as g
  k = {}
  rng = np.random.default_rng(123)
  segs = rng.normal(size=(64, 4, 3))
  # the reference's own test inputs (`geometry_test.py:217-272`)
  segs[0] = [[0., 0., -1.], [0., 0., 1.], [1., 2., -1.], [-1., -2., 1.]]
  a_best, b_best = [], []
  for s in segs:
    a, b = g.closest_segment_to_segment_points(*s)
    a_best.append(a)
    b_best.append(b)
  k['seg_in'] = segs
  k['seg_a'] = np.array(a_best)
  k['seg_b'] = np.array(b_best)
  v = rng.normal(size=(32, 3))
  q = rng.normal(size=(32, 4))
  q /= np.linalg.norm(q, axis=-1, keepdims=True)
  k['rot_v'], k['rot_q'] = v, q
  k['rot_out'] = np.array([bm.rotate(a, b) for a, b in zip(v, q)])
  e = rng.uniform(-180, 180, size=(32, 3))
  k['euler_in'] = e
  k['euler_quat'] = np.array([bm.euler_to_quat(x) for x in e])
  return k


# registered envs whose pbd systems get physics goldens: (envs, steps, action
# width; 0 = num_joint_dof + num_forces_dof). inverted_pendulum uses width 1 as
# its Env does (action_size = 1, inverted_pendulum.py:151-153): the thruster's
# indices 1, 2 clip to 0 (jp.take mode='clip').
ROBOTS = {
    'inverted_pendulum': (8, 6, 1),
    'inverted_double_pendulum': (8, 6, 1),
    'swimmer': (8, 6, 0),
    'hopper': (8, 6, 0),
    'walker2d': (8, 6, 0),
    'reacher': (8, 6, 0),
    'reacherangle': (8, 6, 0),
    'acrobot': (8, 6, 0),
    'ur5e': (4, 4, 0),
    'pusher': (8, 4, 0),
    'grasp': (4, 3, 0),
    'fetch': (4, 4, 0),
}


# legacy_spring variants (`_SYSTEM_CONFIG_SPRING`, system.py:342-390): physics
# rollouts of the registered envs' spring systems, from default_qp
SPRING_ROBOTS = {
    'inverted_pendulum': (8, 4, 1),
    'inverted_double_pendulum': (8, 4, 1),
    'swimmer': (8, 4, 0),
    'hopper': (8, 4, 0),
    'walker2d': (8, 4, 0),
    'reacher': (8, 4, 0),
    'reacherangle': (8, 4, 0),
    'acrobot': (8, 4, 0),
    'ur5e': (4, 3, 0),
    'grasp': (4, 3, 0),
    'fetch': (4, 3, 0),
}


def _short_scenes():
  import scenes
  picks = [0, 1, 7, 17, 19, 21, 23]
  return {'capsule_ground_s': (CAPSULE_TEST_CONFIG, 0, 5, None),
          'capsule_capsule_s': (CAPSULE_TEST_CONFIG, 1, 17, picks),
          'capsule_cull_s': (CAPSULE_TEST_CONFIG, 1, 17, picks),
          'box_ground_s': (scenes.BOX_TEST_CONFIG, 0, 5, None),
          'box_slide_s': (scenes.BOX_TEST_CONFIG, 1, 10, None)}


# mid-episode fixtures (oracle/mid_states.py): 8 envs, 2 steps, recorded by
# the reference from start states the float64 C oracle picked
MID = ['pusher', 'halfcheetah', 'hopper', 'walker2d', 'humanoidstandup', 'grasp']


def mid_traj(name):
  """`mid_<name>`: the env-layer rollout (the keys of traj_* / envtraj_*)
  from the picked start states, plus `row_target` (the contact rows the
  fixture exists for) and `comment`."""
  from brax import envs
  # this directory is on the path (`oracle` is oracle/oracle.py here); the
  # repository root after it, for `tests.helpers` and `brax_amd`
  if os.path.dirname(HERE) not in sys.path:
    sys.path.append(os.path.dirname(HERE))
  import mid_states
  import oracle as oracle_lib
  t0 = time.time()
  starts, comment = mid_states.select(oracle_lib, name)
  t1 = time.time()
  env = envs.get_environment(name)
  r = env_traj(env, 'mid_' + name, len(starts), mid_states.T,
               act_seed_base=mid_states.ACT_SEED, qp0=list(starts))
  assert np.array_equal(r['action'], mid_states.actions(env.action_size, len(starts)))
  r['row_target'] = np.asarray(mid_states.TARGET[name], np.int32)
  r['comment'] = np.array(comment)
  print(f'  mid_{name}: start states {t1 - t0:.1f}s, reference rollout {time.time() - t1:.1f}s',
        flush=True)
  return r


TORCH_ENVS = ['hopper', 'walker2d', 'inverted_pendulum', 'inverted_double_pendulum',
              'swimmer', 'reacher', 'reacherangle', 'acrobot', 'pusher', 'ur5e', 'grasp', 'fetch']


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--only', default='')
  ap.add_argument('--desc-only', action='store_true',
                  help='write only the desc_*.npz descriptor dumps (no rollouts)')
  args = ap.parse_args()
  _setup()
  if args.desc_only:
    global env_traj, sys_traj, wrapped_ant, kats, gym_ant  # pylint: disable=global-statement
    env_traj = sys_traj = wrapped_ant = kats = gym_ant = lambda *a, **k: None  # noqa: E731
  os.makedirs(OUT, exist_ok=True)
  from brax import envs
  from brax.envs import ant as ant_mod
  only = set(args.only.split(',')) if args.only else None

  def want(n):
    return only is None or n in only

  def save(name, d):
    if d is None:
      return
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)

  if want('kat'):
    save('kat', kats())
  if want('ant'):
    env = ant_mod.Ant(use_contact_forces=True)
    save('desc_ant', dump_desc(env.sys))
    save('traj_ant', env_traj(env, 'ant', 64, 8))
  if want('humanoid'):
    env = importlib.import_module('brax.envs.humanoid').Humanoid()
    save('desc_humanoid', dump_desc(env.sys))
    save('traj_humanoid', env_traj(env, 'humanoid', 16, 4))
  if want('humanoidstandup'):
    env = envs.get_environment('humanoidstandup')
    save('desc_humanoidstandup', dump_desc(env.sys))
    save('traj_humanoidstandup', env_traj(env, 'humanoidstandup', 16, 4))
  # legacy_spring envs with the kernel env layer (Env(legacy_spring=True))
  if want('ant_spring'):
    env = ant_mod.Ant(use_contact_forces=True, legacy_spring=True)
    save('desc_ant_spring', dump_desc(env.sys))
    save('traj_ant_spring', env_traj(env, 'ant_spring', 16, 4))
  if want('humanoid_spring'):
    env = importlib.import_module('brax.envs.humanoid').Humanoid(legacy_spring=True)
    save('desc_humanoid_spring', dump_desc(env.sys))
    save('traj_humanoid_spring', env_traj(env, 'humanoid_spring', 8, 3))
  if want('halfcheetah_spring'):
    env = envs.get_environment('halfcheetah', legacy_spring=True)
    save('desc_halfcheetah_spring', dump_desc(env.sys))
    save('traj_halfcheetah_spring', env_traj(env, 'halfcheetah_spring', 8, 3))
  if want('humanoidstandup_spring'):
    env = envs.get_environment('humanoidstandup', legacy_spring=True)
    save('desc_humanoidstandup_spring', dump_desc(env.sys))
    save('traj_humanoidstandup_spring', env_traj(env, 'humanoidstandup_spring', 8, 3))
  for mod, (B, T, aw) in SPRING_ROBOTS.items():
    if want(mod + '_spring'):
      m = importlib.import_module('brax.envs.' + mod)
      from google.protobuf import text_format
      import brax
      s = brax.System(text_format.Parse(m._SYSTEM_CONFIG_SPRING, brax.Config()))  # pylint: disable=protected-access
      save(f'desc_{mod}_spring', dump_desc(s))
      A = aw or (s.num_joint_dof + s.num_forces_dof)
      save(f'traj_{mod}_spring', sys_traj(s, mod + '_spring', s.default_qp(), B, T, 1.0, A))
  # exclude_current_positions_from_observation=False (ant.py:262-265,
  # humanoid.py:289-292, half_cheetah.py:206-209)
  if want('ant_xy'):
    env = ant_mod.Ant(use_contact_forces=True, exclude_current_positions_from_observation=False)
    save('traj_ant_xy', env_traj(env, 'ant_xy', 4, 2))
  if want('humanoid_xy'):
    env = importlib.import_module('brax.envs.humanoid').Humanoid(
        exclude_current_positions_from_observation=False)
    save('traj_humanoid_xy', env_traj(env, 'humanoid_xy', 4, 2))
  if want('halfcheetah_xy'):
    env = envs.get_environment('halfcheetah', exclude_current_positions_from_observation=False)
    save('traj_halfcheetah_xy', env_traj(env, 'halfcheetah_xy', 4, 2))
  if want('halfcheetah'):
    env = envs.get_environment('halfcheetah')
    save('desc_halfcheetah', dump_desc(env.sys))
    save('traj_halfcheetah', env_traj(env, 'halfcheetah', 16, 4))
  # torch env layer over the other registered envs' systems
  for name in TORCH_ENVS:
    if want('env_' + name):
      env = envs.get_environment(name)
      save(f'envtraj_{name}', env_traj(env, name, 8, 4))
  for name in MID:
    if want('mid_' + name) and not args.desc_only:
      save('mid_' + name, mid_traj(name))
  if want('wrap'):
    save('wrap_ant', wrapped_ant())
  if want('wrap_ar2'):
    save('wrap_ant_ar2', wrapped_ant(n_steps=6, episode_length=5, action_repeat=2))
  if want('gym_ant'):
    save('gym_ant', gym_ant())
  if want('eval_ant'):
    save('eval_ant', eval_ant())
  for kind in NAN_PLAN:
    if want('nan_' + kind):
      save('nan_' + kind, nan_env(kind))
  if want('nan_mountain4'):
    save('nan_mountain4', nan_mountain())
  # physics-only rollouts of the other registered envs' systems (their pbd
  # configs): Thruster/Twister forces, frozen bodies, systems without contacts
  for mod, (B, T, aw) in ROBOTS.items():
    if want(mod):
      m = importlib.import_module('brax.envs.' + mod)
      from google.protobuf import text_format
      import brax
      s = brax.System(text_format.Parse(m._SYSTEM_CONFIG, brax.Config()))  # pylint: disable=protected-access
      save(f'desc_{mod}', dump_desc(s))
      A = aw or (s.num_joint_dof + s.num_forces_dof)
      qp0 = s.default_qp()
      save(f'traj_{mod}', sys_traj(s, mod, qp0, B, T, 1.0, A))
  if want('mountain1nn'):
    s = ant_mountain_sys(1, cutoff=9)
    save('desc_mountain1nn', dump_desc(s))
    save('traj_mountain1nn', sys_traj(s, 'mountain1nn', s.default_qp(), 4, 4, 1.0, 8))
  # BASELINE configs[4]'s culled leg: Ant Mountain(4), cutoff 36 (9 per ant,
  # `notebooks/multiagent.ipynb:87-115`), the scene the MULTI kernel runs;
  # jit's scatter for the out-of-range allowed cells, jax.lax.top_k's tie order
  if want('mountain4nn'):
    with jit_index_update():
      s = ant_mountain_sys(4, cutoff=36)
    save('desc_mountain4nn', dump_desc(s))
    with stable_top_k():
      save('traj_mountain4nn', sys_traj(s, 'mountain4nn', s.default_qp(), 4, 3, 1.0, 32))
  # short-horizon twins of the reference's long physics-test scenes: the same
  # bodies at the Ant's dt 0.05 / 10 substeps, from `burn` zero-action steps
  # past default_qp (falling into contact), 8 steps recorded, so the fp32
  # envelope stays small enough for the state gate to mean something (the
  # long scenes integrate 400-10,000 substeps per step; they stay KATs)
  sys.path.insert(0, HERE)
  for name, (txt, di, burn, picks) in _short_scenes().items():
    if want(name):
      from google.protobuf import text_format
      import brax
      cfg = text_format.Parse(txt, brax.Config())
      cfg.dt, cfg.substeps = 0.05, 10
      if name.startswith('capsule_cull'):
        cfg.collider_cutoff = 1
      s = brax.System(cfg)
      qp = s.default_qp(di)
      for _ in range(burn):
        qp, _ = s.step(qp, np.zeros(0))
      save(f'desc_{name}', dump_desc(s))
      if picks is None:
        save(f'traj_{name}', sys_traj(s, name, qp, 1, 8, 1.0, 0))
        continue
      # resting contacts chatter at their gates (penetration > 0, the sinking
      # test) every other step, where even float64 loses digits: one step
      # each from the states `picks` steps past the burn-in whose capsule-
      # capsule contact is active and well conditioned, as a batch of envs
      states = [qp]
      for _ in range(max(picks)):
        states.append(s.step(states[-1], np.zeros(0))[0])
      save(f'traj_{name}', sys_traj(s, name, [states[k] for k in picks], len(picks), 1, 1.0, 0))
  for kind in ('ground', 'capsule', 'cull'):
    if want('capsule_' + kind):
      s, di = capsule_sys(kind)
      save(f'desc_capsule_{kind}', dump_desc(s))
      save(f'traj_capsule_{kind}', sys_traj(s, 'capsule_' + kind, s.default_qp(di), 1, 1, 1.0, 0))
  # point-plane scenes (box corners, mesh vertices): oracle/scenes.py
  import scenes
  from google.protobuf import text_format
  import brax
  point_scenes = {
      'box_ground': (scenes.BOX_TEST_CONFIG, 0, 1),
      'box_slide': (scenes.BOX_TEST_CONFIG, 1, 1),
      'mesh_ground': (scenes.mesh_test_config(), 0, 30),
      'mesh_tilt': (scenes.mesh_test_config(), 1, 12),
      # extended contact functions (colliders.py:699-739, 762-802, 822-848)
      'heightmap': (scenes.heightmap_config(0.05, 10), 1, 8),
      'clipped': (scenes.clipped_plane_config(0.05, 10), 1, 8),
      'box_capsule': (scenes.BOX_CAPSULE_NO_HULL_CONFIG, 1, 4),
      'mesh_capsule': (scenes.mesh_capsule_config(), 0, 8),
      # hull-hull SAT (colliders.py:851-888): edge and face manifolds
      'box_box': (scenes.box_box_config(0.05, 20), 0, 10),
      'box_capsule_hull': (scenes.BOX_CAPSULE_TEST_CONFIG, 1, 3),
  }
  # NearNeighbors with more cutoff than allowed cells (colliders.py:78-85):
  # run under jax.lax.top_k's tie order
  if want('twin_cull'):
    s = brax.System(text_format.Parse(scenes.TWIN_CULL_CONFIG, brax.Config()))
    save('desc_twin_cull', dump_desc(s))
    with stable_top_k():
      save('traj_twin_cull', sys_traj(s, 'twin_cull', s.default_qp(), 1, 8, 1.0, 0))
  for name, (txt, di, T) in point_scenes.items():
    if want(name):
      s = brax.System(text_format.Parse(txt, brax.Config()))
      save(f'desc_{name}', dump_desc(s))
      save(f'traj_{name}', sys_traj(s, name, s.default_qp(di), 1, T, 1.0, 0))
  for n in (1, 2, 4):
    if want(f'mountain{n}'):
      s = ant_mountain_sys(n)
      save(f'desc_mountain{n}', dump_desc(s))
      B, T = {1: (4, 4), 2: (2, 3), 4: (1, 2)}[n]
      save(f'traj_mountain{n}', sys_traj(s, f'mountain{n}', s.default_qp(), B, T,
                                         1.0, 8 * n))


if __name__ == '__main__':
  main()
