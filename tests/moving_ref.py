"""Reference of the moving colliders (gsmpm_mpm_add_moving_collider; the
specification is DESIGN.md "Moving colliders" / include/gsmpm.h), numpy only,
for operator lists that may hold moving records, in collider_ref's two forms:

* node_update_ref: float64.  What the specification fixes in f32 is taken in
  f32 and then as float64, the convention collider_ref follows for the
  geometry: the placement c = a + w * tau, tau and the collider's velocity wc
  are formed in f32 exactly as stated (placement32), every other operation
  is float64.  Inside test, normals and response are collider_ref's
  (_inside_and_normals, _response64) at the placement c, on the relative
  velocity u = v - wc; only the nodes the record hits are rewritten.
* node_update_f32: the f32 transcription in the stated order (_response32).

Operators: collider_ref's, plus mov(ext_op, velocity, t_start, t_end).  A
list without a moving record gives collider_ref's results exactly (asserted
in test_moving_ref.py).  Also the constants shared by the tests: velocity W,
the motion window, the times T and the acting counts on scene S.
"""
from __future__ import annotations

import numpy as np

import collider_ref as CR
import grid_ref as G

F32 = np.float32

W = (3.1, -2.3, 1.7)
WINDOW = (0.0101, 0.0803)
T = (0.0, 0.0123, 0.0507, 0.1)
# massive nodes of scene S whose relative velocity points into the collider moving with W, at the times of T
ACTING = {"ball": (572, 589, 587, 548), "box": (774, 751, 687, 704), "walls": (1349, 1538, 2622, 1987)}


def mov(op, velocity=W, t_start=WINDOW[0], t_end=WINDOW[1]):
    """("mov", ext op, w, t0, t1): the record `op` (collider_ref.ext) moving."""
    assert op[0] == "ext"
    return ("mov", op, tuple(float(a) for a in velocity), float(t_start), float(t_end))


def placement32(op, t):
    """(c [3], wc [3], tau) in f32, unfused, left to right, as the kernels form them."""
    _, e, w, t0, t1 = op
    t, t0, t1 = F32(t), F32(t0), F32(t1)
    w, a = np.asarray(w, F32), np.asarray(e[3], F32)
    tc = np.minimum(np.maximum(t, t0), t1)
    tau = F32(tc - t0)
    c = (a + (w * tau).astype(F32)).astype(F32)
    moving = bool(t >= t0) and bool(t < t1)
    wc = w if moving else np.zeros(3, F32)
    return c, wc, tau


def static_at(op, t):
    """The static ext op standing where the moving one is at time t (its f32 placement)."""
    e = op[1]
    c = placement32(op, t)[0]
    return e[:3] + (tuple(float(a) for a in c),) + e[4:]


# ------------------------------------------------------------- float64 --
def _apply_ext64(v, p, live, e, wc):
    """collider_ref.node_update_ref's extended record, on u = v - wc where wc is given."""
    _, shape, surface, _, _, fr, damp = e
    hits, amb = CR._inside_and_normals(p, e)
    mu, damp = float(F32(fr)), float(F32(damp))
    u = v if wc is None else v - wc[None, :]
    any_hit = np.zeros(len(v), bool)
    for hit, n in hits:
        hit = hit & live
        any_hit |= hit
        nh = n if n.ndim == 1 else n[hit]
        if shape == "ball":  # no normal at the centre: sticky
            ub = u[hit]
            centre = ~np.isfinite(nh).all(1) | (np.sqrt(((p[hit] - G.f32(e[3])) ** 2).sum(1)) <= 1e-20)
            out = np.zeros_like(ub)
            out[~centre] = CR._response64(ub[~centre], nh[~centre], surface, mu)
            u[hit] = out
        else:
            u[hit] = CR._response64(u[hit], nh, surface, mu)
    if surface != "sticky":
        u[any_hit] = u[any_hit] * damp
    if wc is not None:
        v[any_hit] = u[any_hit] + wc[None, :]
    return amb, any_hit


def node_update_ref(mv, m, n_grid, dx32, dt_g32, ops, active, t=0.0):
    """collider_ref.node_update_ref for lists that may hold mov(...) records,
    at caller time t.  Returns (v_out [ng^3, 3] float64, ambiguous [ng^3])."""
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, np.float64).reshape(nn, 3)
    m = np.asarray(m, np.float64).reshape(nn)
    p = CR.node_positions32(n_grid, dx32)
    live = m > float(F32(1e-15))
    v = np.zeros((nn, 3))
    v[live] = mv[live] / m[live, None] + G.f32(dt_g32)[None, :]
    ambiguous = np.zeros(nn, bool)
    for op, act in zip(ops, active):
        if op[0] == "cube":
            d = np.abs(p - G.f32(op[1])[None, :]) - G.f32(op[2])[None, :]
            ambiguous |= (np.abs(d) < G.AMBIG).any(1)
            if act:
                v[(d < 0).all(1) & live] = 0.0
            continue
        wc = None
        if op[0] == "collider":  # the legacy plane: separate, 0.99f, always on
            op, act = CR.ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        elif op[0] == "mov":
            wc = placement32(op, t)[1].astype(np.float64)
            op = static_at(op, t)
        if not act:
            ambiguous |= CR._inside_and_normals(p, op)[1]
            continue
        ambiguous |= _apply_ext64(v, p, live, op, wc)[0]
    return v, ambiguous


def acting_nodes(mv, m, n_grid, dx32, dt_g32, op, t):
    """(massive nodes in the moving collider at time t, those whose relative
    velocity v - wc points into it for a normal it applies), v = mv / m + dt g."""
    nn = int(n_grid) ** 3
    v, _ = CR.node_update_ref(mv, m, n_grid, dx32, dt_g32, [], [])
    live = np.asarray(m, np.float64).reshape(nn) > float(F32(1e-15))
    u = v - placement32(op, t)[1].astype(np.float64)[None, :]
    hits, _ = CR._inside_and_normals(CR.node_positions32(n_grid, dx32), static_at(op, t))
    inside, acting = np.zeros(nn, bool), np.zeros(nn, bool)
    for hit, n in hits:
        hit = hit & live
        inside |= hit
        with np.errstate(invalid="ignore"):
            acting |= hit & (((u * n).sum(1) if n.ndim == 2 else u @ n) < 0)
    return int(inside.sum()), int(acting.sum())


def hit_nodes(n_grid, dx32, op, t):
    """Nodes inside the record at time t (geometry only, f32 positions)."""
    p = CR.node_positions32(n_grid, dx32)
    hit = np.zeros(len(p), bool)
    for h, _ in CR._inside_and_normals(p, static_at(op, t) if op[0] == "mov" else op)[0]:
        hit |= h
    return hit


# ------------------------------------------------------ f32 transcription --
def _apply_ext32(v, p, live, e, wc):
    """collider_ref.node_update_f32's extended record on u = v - wc; v, p: lists of three f32 arrays."""
    nn = len(v[0])
    _, shape, surface, a, b, fr, damp = e
    a, b, mu, damp = np.asarray(a, F32), np.asarray(b, F32), F32(fr), F32(damp)
    u = v if wc is None else [(v[t] - wc[t]).astype(F32) for t in range(3)]

    def put(old, hit, new):
        return [np.where(hit, new[t], old[t]).astype(F32) for t in range(3)]

    d = [p[t] - a[t] for t in range(3)]
    any_hit = np.zeros(nn, bool)
    if shape == "walls":
        for axis in range(3):
            hit = live & (np.abs(d[axis]) > b[axis])
            n = [np.zeros(nn, F32)] * 3
            n[axis] = np.where(d[axis] < F32(0), F32(1), F32(-1)).astype(F32)
            u = put(u, hit, CR._response32(u, n, surface, mu))
            any_hit |= hit
    else:
        if shape == "plane":
            hit = d[0] * b[0] + d[1] * b[1] + d[2] * b[2] < F32(0)
            u_new = CR._response32(u, [np.full(nn, b[t], F32) for t in range(3)], surface, mu)
        elif shape == "ball":
            L = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            hit = L < b[0]
            with np.errstate(invalid="ignore", divide="ignore"):
                n = [(d[t] / L).astype(F32) for t in range(3)]
                u_new = CR._response32(u, n, surface, mu)
            u_new = [np.where(L <= F32(1e-20), F32(0), u_new[t]).astype(F32) for t in range(3)]
        else:
            q = [b[t] - np.abs(d[t]) for t in range(3)]
            hit = (np.abs(d[0]) < b[0]) & (np.abs(d[1]) < b[1]) & (np.abs(d[2]) < b[2])
            ax = np.where((q[0] <= q[1]) & (q[0] <= q[2]), 0, np.where(q[1] <= q[2], 1, 2))
            n = [np.where(ax == t, np.where(d[t] < F32(0), F32(-1), F32(1)), F32(0)).astype(F32) for t in range(3)]
            u_new = CR._response32(u, n, surface, mu)
        any_hit = live & hit
        u = put(u, any_hit, u_new)
    if surface != "sticky":
        u = put(u, any_hit, [(u[t] * damp).astype(F32) for t in range(3)])
    if wc is None:
        return u
    return put(v, any_hit, [(u[t] + wc[t]).astype(F32) for t in range(3)])


def node_update_f32(mv, m, n_grid, dx32, dt_g32, ops, active, t=0.0):
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
    for op, act in zip(ops, active):
        if op[0] == "cube":
            c, s = np.asarray(op[1], F32), np.asarray(op[2], F32)
            if act:
                hit = live & (np.abs(p[0] - c[0]) < s[0]) & (np.abs(p[1] - c[1]) < s[1]) & (np.abs(p[2] - c[2]) < s[2])
                v = [np.where(hit, F32(0), v[d]).astype(F32) for d in range(3)]
            continue
        wc = None
        if op[0] == "collider":
            op, act = CR.ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        elif op[0] == "mov":
            wc = placement32(op, t)[1]
            op = static_at(op, t)
        if act:
            v = _apply_ext32(v, p, live, op, wc)
    return np.stack(v, 1)
