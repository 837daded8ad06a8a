"""Reference of the rotating colliders (gsmpm_mpm_add_rotating_collider; the
specification is DESIGN.md "Rotating colliders" / include/gsmpm.h), numpy
only, for operator lists that may hold rotating records, in collider_ref's and
moving_ref's two forms:

* node_update_ref: float64.  What the specification stores in f32 is taken in
  f32 and then as float64: the pose {R, c, o} of the record at the substep's
  time (pose32, or the pose the caller hands over -- the GPU's own, read back
  with Simulator.poses), the node position, the geometry, w32, om32 and the
  moving flag.  Every operation on them is float64: the node goes to the body
  frame (d = R^T (p - c)), the relative velocity too (u = R^T (v - wc), wc =
  w + om x (p - o) inside the window), collider_ref's record acts on u at the
  offset d (_inside_and_normals, _response64), and a node it hit is rotated
  back (v = R u + wc).  The ambiguity mask is collider_ref's 1e-6 rule on d.
* node_update_f32: the f32 transcription in the stated order.
* node_update_world: the same physics in the world frame, float64 -- normals
  and box axes rotated by R, the response on v - wc -- written without the
  body-frame helpers, as an independent check of the formulation.  The two
  forms are equal for an orthogonal R.  The stored R, nine f32 roundings, is
  orthogonal to 6e-8 only, and with it they differ by 3e-7 of v; so the check
  feeds both the unrounded pose (pose16: float64 poses are taken as given).

pose64(op, t) is the pose before its rounding: R, c and o in float64 from the
f32 stored values, for the pose table's test.

Operators: moving_ref's, plus rot(ext_op, omega, pivot, velocity, t_start,
t_end).  A list without a rotating record gives moving_ref's results exactly
(asserted in test_rotating_ref.py).  Also the constants shared by the tests.
"""
from __future__ import annotations

import numpy as np

import collider_ref as CR
import grid_ref as G
import moving_ref as M

F32 = np.float32

OMEGA = (7.0, -4.0, 11.0)  # |omega| = 13.64: 31.7 degrees after T[2] - WINDOW[0]
PIVOT = (0.95, 1.05, 1.0)
PLANE = G.OP_LISTS["b"][0][0]  # the oblique legacy plane of list b
# times per shape: moving_ref.T, except the plane's second (at 0.0123 one massive node of scene S lies within
# 1e-6 of the turned plane)
T = {"plane": (0.0, 0.0124, 0.0507, 0.1), "ball": M.T, "box": M.T, "walls": M.T}
T_IN = M.T[2]
# massive nodes of scene S whose relative velocity points into the collider turning with OMEGA about PIVOT and
# translating with moving_ref.W, at the times of T (none of them ambiguous; test_rotating_ref.py recomputes both)
ACTING = {"plane": (1346, 2439, 3409, 2228), "ball": (572, 596, 589, 553), "box": (774, 752, 811, 771),
          "walls": (1349, 1497, 2275, 1854)}


def geo(name):
    """The shared geometry: collider_ref.GEOMETRY, and the oblique plane of list b."""
    return dict(point=PLANE[1], normal=PLANE[2]) if name == "plane" else CR.GEOMETRY[name]


def rot(op, omega=OMEGA, pivot=PIVOT, velocity=M.W, t_start=M.WINDOW[0], t_end=M.WINDOW[1]):
    """("rot", ext op, w, t0, t1, omega, pivot): the record `op` (collider_ref.ext) turning and translating."""
    assert op[0] == "ext"
    return ("rot", op, tuple(float(a) for a in velocity), float(t_start), float(t_end),
            tuple(float(a) for a in omega), tuple(float(a) for a in pivot))


def _clock32(op, t):
    """(tau f32, moving flag) as the moving record's."""
    t, t0, t1 = F32(t), F32(op[3]), F32(op[4])
    tc = np.minimum(np.maximum(t, t0), t1)
    return F32(tc - t0), bool(t >= t0) and bool(t < t1)


def rotation64(op, tau):
    """R = I + sin(theta) K + (1 - cos(theta)) K K in float64, theta = |omega| * tau, k = omega / |omega| (f64)."""
    om = np.asarray(op[5], np.float64)
    wm = np.sqrt((om * om).sum())
    k = om / wm
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    theta = wm * float(tau)
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def pose64(op, t):
    """The pose before its rounding: dict(R [3, 3], c [3], o [3]) in float64 from the stored f32 values."""
    tau, _ = _clock32(op, t)
    w, piv, a = G.f32(op[2]), G.f32(op[6]), G.f32(op[1][3])
    R = rotation64(op, tau)
    o = piv + w * float(tau)
    return dict(R=R, c=o + R @ (a - piv), o=o)


def pose32(op, t):
    """The pose as the specification stores it, 16 f32: R rounded once, o and c in f32, unfused, left to right."""
    tau, _ = _clock32(op, t)
    w, piv, a = np.asarray(op[2], F32), np.asarray(op[6], F32), np.asarray(op[1][3], F32)
    R = rotation64(op, tau).astype(F32)
    e = (a - piv).astype(F32)
    o = (piv + (w * tau).astype(F32)).astype(F32)
    c = np.array([o[i] + F32(F32(R[i, 0] * e[0] + R[i, 1] * e[1]) + R[i, 2] * e[2]) for i in range(3)], F32)
    return np.concatenate([R.reshape(9), c, o, np.zeros(1, F32)]).astype(F32)


def pose16(op, t):
    """pose64 laid out as a pose, kept in float64 (R orthogonal to rounding in f64, which the f32 R is not)."""
    P = pose64(op, t)
    return np.concatenate([P["R"].reshape(9), P["c"], P["o"], np.zeros(1)])


def _split(pose):
    pose = np.asarray(pose)
    pose = (pose if pose.dtype == np.float64 else pose.astype(F32)).reshape(16)
    return pose[:9].reshape(3, 3), pose[9:12], pose[12:15]


def _body_op(e):
    """The ext op with its point / centre at the origin: collider_ref's helpers then take d for p - a."""
    return e[:3] + ((0.0, 0.0, 0.0),) + e[4:]


def wc64(op, t, x, o):
    """The collider's velocity at the points x [k, 3] (float64), o the travelling pivot: w32 + om32 x (x - o)
    inside the motion window, 0 outside."""
    if not _clock32(op, t)[1]:
        return np.zeros_like(x)
    return G.f32(op[2])[None, :] + np.cross(G.f32(op[5])[None, :], x - np.asarray(o, np.float64)[None, :])


# ------------------------------------------------------------- float64 --
def _apply_rot64(v, p, live, op, t, pose):
    """One rotating record on v (in place), body frame; returns (ambiguous, hit)."""
    R, c, o = (a.astype(np.float64) for a in _split(pose))
    d = (p - c[None, :]) @ R  # R^T q, row by row
    wc = wc64(op, t, p, o)
    u = (v - wc) @ R
    amb, hit = M._apply_ext64(u, d, live, _body_op(op[1]), None)
    v[hit] = u[hit] @ R.T + wc[hit]
    return amb, hit


def _free64(mv, m, n_grid, dx32, dt_g32):
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, np.float64).reshape(nn, 3)
    m = np.asarray(m, np.float64).reshape(nn)
    p = CR.node_positions32(n_grid, dx32)
    live = m > float(F32(1e-15))
    v = np.zeros((nn, 3))
    v[live] = mv[live] / m[live, None] + G.f32(dt_g32)[None, :]
    return v, p, live


def node_update_ref(mv, m, n_grid, dx32, dt_g32, ops, active, t=0.0, poses=None):
    """moving_ref.node_update_ref for lists that may hold rot(...) records, at
    caller time t.  poses: {index in ops: 16 f32} to use instead of pose32.
    Returns (v_out [ng^3, 3] float64, ambiguous [ng^3])."""
    v, p, live = _free64(mv, m, n_grid, dx32, dt_g32)
    ambiguous = np.zeros(len(v), bool)
    for i, (op, act) in enumerate(zip(ops, active)):
        if op[0] == "cube":
            d = np.abs(p - G.f32(op[1])[None, :]) - G.f32(op[2])[None, :]
            ambiguous |= (np.abs(d) < G.AMBIG).any(1)
            if act:
                v[(d < 0).all(1) & live] = 0.0
            continue
        if op[0] == "rot":
            pose = pose32(op, t) if poses is None or i not in poses else poses[i]
            if act:
                ambiguous |= _apply_rot64(v, p, live, op, t, pose)[0]
            else:
                R, c, _ = (a.astype(np.float64) for a in _split(pose))
                ambiguous |= CR._inside_and_normals((p - c[None, :]) @ R, _body_op(op[1]))[1]
            continue
        wc = None
        if op[0] == "collider":  # the legacy plane: separate, 0.99f, always on
            op, act = CR.ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        elif op[0] == "mov":
            wc = M.placement32(op, t)[1].astype(np.float64)
            op = M.static_at(op, t)
        if not act:
            ambiguous |= CR._inside_and_normals(p, op)[1]
            continue
        ambiguous |= M._apply_ext64(v, p, live, op, wc)[0]
    return v, ambiguous


def node_update_world(mv, m, n_grid, dx32, dt_g32, ops, active, t=0.0, poses=None):
    """The rotating records of `ops` (only such records, all active) in the world frame, float64."""
    v, p, live = _free64(mv, m, n_grid, dx32, dt_g32)
    for i, (op, act) in enumerate(zip(ops, active)):
        assert op[0] == "rot" and act
        _, shape, surface, _, b, fr, damp = op[1]
        R, c, o = (a.astype(np.float64) for a in _split(pose32(op, t) if poses is None else poses[i]))
        b, mu, damp = G.f32(b), float(F32(fr)), float(F32(damp))
        wc = wc64(op, t, p, o)
        s = v - wc
        q = p - c[None, :]
        axes = [R[:, i] for i in range(3)]  # the body's axes in the world
        done = np.zeros(len(v), bool)
        if shape == "plane":
            n = R @ b
            todo = [((q @ n < 0) & live, np.broadcast_to(n, q.shape))]
        elif shape == "ball":
            L = np.sqrt((q * q).sum(1))
            with np.errstate(invalid="ignore", divide="ignore"):
                todo = [((L < b[0]) & live, q / L[:, None])]
        elif shape == "box":
            depth = np.stack([b[i] - np.abs(q @ axes[i]) for i in range(3)], 1)
            ax = np.argmin(depth, 1)
            sign = np.stack([np.where(q @ axes[i] < 0, -1.0, 1.0) for i in range(3)], 1)
            n = np.stack(axes, 0)[ax] * sign[np.arange(len(q)), ax][:, None]
            todo = [((depth > 0).all(1) & live, n)]
        else:
            todo = [((np.abs(q @ axes[i]) > b[i]) & live,
                     np.where(q @ axes[i] < 0, 1.0, -1.0)[:, None] * axes[i][None, :]) for i in range(3)]
        for hit, n in todo:
            if surface == "sticky":
                s[hit] = 0.0
            else:
                s[hit] = CR._response64(s[hit], n[hit], surface, mu)
            done |= hit
        if surface != "sticky":
            s[done] = s[done] * damp
        v[done] = s[done] + wc[done]
    return v


def _body(mv, m, n_grid, dx32, dt_g32, op, t):
    v, p, live = _free64(mv, m, n_grid, dx32, dt_g32)
    R, c, o = (a.astype(np.float64) for a in _split(pose32(op, t)))
    d = (p - c[None, :]) @ R
    u = (v - wc64(op, t, p, o)) @ R
    return d, u, live


def acting_nodes(mv, m, n_grid, dx32, dt_g32, op, t):
    """(massive nodes in the rotating collider at time t, those whose relative
    velocity points into it for a normal it applies, massive nodes the 1e-6 rule marks ambiguous)."""
    d, u, live = _body(mv, m, n_grid, dx32, dt_g32, op, t)
    hits, amb = CR._inside_and_normals(d, _body_op(op[1]))
    inside, acting = np.zeros(len(d), bool), np.zeros(len(d), bool)
    for hit, n in hits:
        hit = hit & live
        inside |= hit
        with np.errstate(invalid="ignore"):
            acting |= hit & (((u * n).sum(1) if n.ndim == 2 else u @ n) < 0)
    return int(inside.sum()), int(acting.sum()), int((amb & live).sum())


def hit_nodes(n_grid, dx32, op, t, pose=None):
    """Nodes inside the record at time t (geometry only, f32 positions and pose)."""
    if op[0] != "rot":
        return M.hit_nodes(n_grid, dx32, op, t)
    p = CR.node_positions32(n_grid, dx32)
    R, c, _ = (a.astype(np.float64) for a in _split(pose32(op, t) if pose is None else pose))
    hit = np.zeros(len(p), bool)
    for h, _ in CR._inside_and_normals((p - c[None, :]) @ R, _body_op(op[1]))[0]:
        hit |= h
    return hit


# ------------------------------------------------------ f32 transcription --
def _hit32(d, live, e):
    """The inside test of moving_ref._apply_ext32, expression for expression."""
    _, shape, _, _, b, _, _ = e
    b = np.asarray(b, F32)
    if shape == "walls":
        return live & ((np.abs(d[0]) > b[0]) | (np.abs(d[1]) > b[1]) | (np.abs(d[2]) > b[2]))
    if shape == "plane":
        return live & (d[0] * b[0] + d[1] * b[1] + d[2] * b[2] < F32(0))
    if shape == "ball":
        return live & (np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < b[0])
    return live & (np.abs(d[0]) < b[0]) & (np.abs(d[1]) < b[1]) & (np.abs(d[2]) < b[2])


def _apply_rot32(v, p, live, op, t, pose):
    """One rotating record; v, p: lists of three f32 arrays.  Unfused, left to right, sums in index order."""
    R, c, o = _split(pose)
    w, om = np.asarray(op[2], F32), np.asarray(op[5], F32)
    moving = _clock32(op, t)[1]
    q = [p[e] - c[e] for e in range(3)]
    r = [p[e] - o[e] for e in range(3)]
    x = [om[1] * r[2] - om[2] * r[1], om[2] * r[0] - om[0] * r[2], om[0] * r[1] - om[1] * r[0]]
    wc = [(w[e] + x[e]).astype(F32) if moving else np.zeros_like(p[e]) for e in range(3)]
    s = [(v[e] - wc[e]).astype(F32) for e in range(3)]
    d = [(R[0, e] * q[0] + R[1, e] * q[1] + R[2, e] * q[2]).astype(F32) for e in range(3)]
    u = [(R[0, e] * s[0] + R[1, e] * s[1] + R[2, e] * s[2]).astype(F32) for e in range(3)]
    e0 = _body_op(op[1])
    hit = _hit32(d, live, e0)
    u = M._apply_ext32(u, d, live, e0, None)
    back = [((R[e, 0] * u[0] + R[e, 1] * u[1] + R[e, 2] * u[2]) + wc[e]).astype(F32) for e in range(3)]
    return [np.where(hit, back[e], v[e]).astype(F32) for e in range(3)]


def node_update_f32(mv, m, n_grid, dx32, dt_g32, ops, active, t=0.0, poses=None):
    """The same update with every operation in f32, unfused, left to right."""
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, F32).reshape(nn, 3)
    m = np.asarray(m, F32).reshape(nn)
    idx = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = [(idx[:, d].astype(F32) * F32(dx32)).astype(F32) for d in range(3)]
    live = m > F32(1e-15)
    g = np.asarray(dt_g32, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = [np.where(live, mv[:, d] / m + g[d], F32(0)).astype(F32) for d in range(3)]
    for i, (op, act) in enumerate(zip(ops, active)):
        if op[0] == "cube":
            c, s = np.asarray(op[1], F32), np.asarray(op[2], F32)
            if act:
                hit = live & (np.abs(p[0] - c[0]) < s[0]) & (np.abs(p[1] - c[1]) < s[1]) & (np.abs(p[2] - c[2]) < s[2])
                v = [np.where(hit, F32(0), v[d]).astype(F32) for d in range(3)]
            continue
        if op[0] == "rot":
            if act:
                v = _apply_rot32(v, p, live, op, t, pose32(op, t) if poses is None or i not in poses else poses[i])
            continue
        wc = None
        if op[0] == "collider":
            op, act = CR.ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        elif op[0] == "mov":
            wc = M.placement32(op, t)[1]
            op = M.static_at(op, t)
        if act:
            v = M._apply_ext32(v, p, live, op, wc)
    return np.stack(v, 1)
