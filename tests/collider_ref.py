"""Reference of the extended colliders (gsmpm_mpm_add_collider; the
specification is DESIGN.md "Extended colliders" / include/gsmpm.h), numpy
only, in two forms over the same operator lists:

* node_update_ref: float64, extending grid_ref.node_update_ref's conventions
  -- what the library stores in f32 is taken in f32 (the geometry, friction,
  damping, dt*g, and here the node position p = f32(i) * dx32 rounded to f32,
  which the specification fixes: a ball's normal is (p - c) / |p - c|, so the
  1e-7 between the rounded and the exact product would show as ~1e-6 of v),
  every other operation float64; plus the ambiguity mask (geometry only): a
  node within 1e-6 of a surface, a face, or a tie between two penetration
  depths of a box may be decided either way in f32.
* node_update_f32: the f32 transcription in the stated operation order
  (unfused, left to right), whose error against the float64 form is the
  yardstick the GPU's error is held to.

Operators: grid_ref's ("cube", c, s) and ("collider", point, normal, mu) --
the legacy plane, always active -- and ext(...) below, which honours its
activity flag.  Also the three geometry lists of scene S and their counts.
"""
from __future__ import annotations

import numpy as np

import grid_ref as G

F32 = np.float32
SHAPES = ("plane", "ball", "box", "walls")
SURFACES = ("sticky", "slip", "separate")

# geometry off the lattice of scene S (grid_ref.scene): name -> geometry keywords
CENTRE = (1.013, 0.987, 0.913)
GEOMETRY = {
    "ball": dict(center=CENTRE, radius=0.407),
    "box": dict(center=CENTRE, half=(0.41, 0.37, 0.33)),
    "walls": dict(center=(1.013, 0.987, 1.013), half=(0.51, 0.47, 0.43)),
}
# massive nodes of scene S in the collider, and those of them with v . n < 0
# for some normal the collider applies (v = mv / m + dt g, float64 P2G sums)
COUNTS = {"ball": (1162, 572), "box": (1560, 774), "walls": (2523, 1349)}
WALLS_MULTI = 354  # massive nodes beyond two or more walls
MIN_ACTING = 500


def ext(shape, surface="separate", friction=0.0, damping=1.0, **geo):
    """("ext", shape, surface, a, b, friction, damping): a = point / centre,
    b = normal (normalised in f64) / (radius, 0, 0) / half extents."""
    assert shape in SHAPES and surface in SURFACES
    if shape == "plane":
        n = np.asarray(geo["normal"], np.float64)
        a, b = geo["point"], n / np.sqrt((n * n).sum())
    elif shape == "ball":
        a, b = geo["center"], (geo["radius"], 0.0, 0.0)
    else:
        a, b = geo["center"], geo["half"]
    return ("ext", shape, surface, tuple(float(t) for t in a), tuple(float(t) for t in b), float(friction),
            float(damping))


def geometry_kw(op):
    """The keywords Simulator.add_collider takes for an ext op."""
    _, shape, surface, a, b, fr, damp = op
    geo = {"plane": dict(point=a, normal=b), "ball": dict(center=a, radius=b[0])}.get(shape, dict(center=a, half=b))
    return dict(shape=shape, surface=surface, friction=fr, damping=damp, **geo)


def node_positions32(n_grid, dx32):
    """p = (float) i * dx in f32, as float64."""
    idx = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (idx.astype(F32) * F32(dx32)).astype(F32).astype(np.float64)


# ------------------------------------------------------------- float64 --
def _response64(v, n, surface, mu):
    """R(v, n) without the damping; v [k, 3], n [3] or [k, 3].  The separate
    case is grid_ref.node_update_ref's collider, expression for expression."""
    if surface == "sticky":
        return np.zeros_like(v)
    nc = v @ n if n.ndim == 1 else (v * n).sum(1)
    mn = np.minimum(nc, 0.0) if surface == "separate" else nc
    v = v - mn[:, None] * (n[None, :] if n.ndim == 1 else n)
    ln = np.sqrt((v * v).sum(1))
    fric = (nc < 0) & (ln > 1e-20)
    sc = np.maximum(0.0, ln[fric] + nc[fric] * mu)
    v[fric] = sc[:, None] * (v[fric] / ln[fric, None])
    return v


def _inside_and_normals(p, op):
    """Per node: list of (hit mask, normals [nn, 3] or [3]) the collider
    applies in order, and the geometric ambiguity mask."""
    _, shape, _, a, b, _, _ = op
    a, b = G.f32(a), G.f32(b)
    d = p - a[None, :]
    if shape == "plane":
        dot = d @ b
        return [(dot < 0, b)], np.abs(dot) < G.AMBIG
    if shape == "ball":
        L = np.sqrt((d * d).sum(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            n = d / L[:, None]
        return [(L < b[0], n)], np.abs(L - b[0]) < G.AMBIG
    q = b[None, :] - np.abs(d)  # penetration depth per axis (box), minus the overshoot (walls)
    face = (np.abs(q) < G.AMBIG).any(1)
    if shape == "box":
        inside = (q > 0).all(1)
        ax = np.argmin(q, 1)  # the first axis that attains the minimum
        qs = np.sort(q, 1)
        rows = np.arange(len(p))
        tie = inside & ((qs[:, 1] - qs[:, 0] < G.AMBIG) | (np.abs(d[rows, ax]) < G.AMBIG))
        n = np.zeros_like(d)
        n[rows, ax] = np.where(d[rows, ax] < 0, -1.0, 1.0)
        return [(inside, n)], face | tie
    out = []
    for axis in range(3):
        n = np.zeros_like(d)
        n[:, axis] = np.where(d[:, axis] < 0, 1.0, -1.0)
        out.append((q[:, axis] < 0, n))
    return out, face


def node_update_ref(mv, m, n_grid, dx32, dt_g32, ops, active):
    """v = mv / m + dt g where m > 1e-15 (else 0), then `ops` in order; an
    inactive cube or ext op is skipped, a legacy collider never.  Returns
    (v_out [ng^3, 3] float64, ambiguous [ng^3] bool)."""
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, np.float64).reshape(nn, 3)
    m = np.asarray(m, np.float64).reshape(nn)
    p = node_positions32(n_grid, dx32)
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
        if op[0] == "collider":  # the legacy plane: separate, 0.99f, always on
            op, act = ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        _, shape, surface, _, _, fr, damp = op
        hits, amb = _inside_and_normals(p, op)
        ambiguous |= amb
        if not act:
            continue
        mu, damp = float(F32(fr)), float(F32(damp))
        any_hit = np.zeros(nn, bool)
        for hit, n in hits:
            hit = hit & live
            any_hit |= hit
            nh = n if n.ndim == 1 else n[hit]
            if shape == "ball":  # no normal at the centre: sticky
                vb = v[hit]
                centre = ~np.isfinite(nh).all(1) | (np.sqrt(((p[hit] - G.f32(op[3])) ** 2).sum(1)) <= 1e-20)
                out = np.zeros_like(vb)
                out[~centre] = _response64(vb[~centre], nh[~centre], surface, mu)
                v[hit] = out
            else:
                v[hit] = _response64(v[hit], nh, surface, mu)
        if surface != "sticky":
            v[any_hit] = v[any_hit] * damp
    return v, ambiguous


def acting_nodes(mv, m, n_grid, dx32, dt_g32, op):
    """(massive nodes in the collider, those with v . n < 0 for a normal it
    applies, massive nodes hit on >= 2 normals), v = mv / m + dt g."""
    nn = int(n_grid) ** 3
    v, _ = node_update_ref(mv, m, n_grid, dx32, dt_g32, [], [])
    live = np.asarray(m, np.float64).reshape(nn) > float(F32(1e-15))
    hits, _ = _inside_and_normals(node_positions32(n_grid, dx32), op)
    inside, acting, count = np.zeros(nn, bool), np.zeros(nn, bool), np.zeros(nn, int)
    for hit, n in hits:
        hit = hit & live
        inside |= hit
        count += hit
        with np.errstate(invalid="ignore"):
            acting |= hit & (((v * n).sum(1) if n.ndim == 2 else v @ n) < 0)
    return int(inside.sum()), int(acting.sum()), int((count >= 2).sum())


# ------------------------------------------------------ f32 transcription --
def _response32(v, n, surface, mu):
    """v, n: lists of three f32 arrays; every operation rounded to f32, in order."""
    if surface == "sticky":
        return [np.zeros_like(c) for c in v]
    nc = v[0] * n[0] + v[1] * n[1] + v[2] * n[2]
    mn = np.minimum(nc, F32(0)) if surface == "separate" else nc
    v = [v[d] - mn * n[d] for d in range(3)]
    ln = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    fric = (nc < F32(0)) & (ln > F32(1e-20))
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.maximum(F32(0), ln + nc * mu)
        return [np.where(fric, sc * (v[d] / ln), v[d]).astype(F32) for d in range(3)]


def node_update_f32(mv, m, n_grid, dx32, dt_g32, ops, active):
    """The same update with every operation in f32, unfused, left to right
    (what the kernels' source says).  Returns v_out [ng^3, 3] f32."""
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, F32).reshape(nn, 3)
    m = np.asarray(m, F32).reshape(nn)
    idx = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = [(idx[:, d].astype(F32) * F32(dx32)).astype(F32) for d in range(3)]
    live = m > F32(1e-15)
    g = np.asarray(dt_g32, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = [np.where(live, mv[:, d] / m + g[d], F32(0)).astype(F32) for d in range(3)]

    def put(hit, new):
        return [np.where(hit, new[d], v[d]).astype(F32) for d in range(3)]

    for op, act in zip(ops, active):
        if op[0] == "cube":
            c, s = np.asarray(op[1], F32), np.asarray(op[2], F32)
            if act:
                hit = live & (np.abs(p[0] - c[0]) < s[0]) & (np.abs(p[1] - c[1]) < s[1]) & (np.abs(p[2] - c[2]) < s[2])
                v = put(hit, [np.zeros(nn, F32)] * 3)
            continue
        if op[0] == "collider":
            op, act = ext("plane", "separate", op[3], float(F32(0.99)), point=op[1], normal=op[2]), True
        if not act:
            continue
        _, shape, surface, a, b, fr, damp = op
        a, b, mu, damp = np.asarray(a, F32), np.asarray(b, F32), F32(fr), F32(damp)
        d = [p[t] - a[t] for t in range(3)]
        any_hit = np.zeros(nn, bool)
        if shape == "walls":
            for axis in range(3):
                hit = live & (np.abs(d[axis]) > b[axis])
                n = [np.zeros(nn, F32)] * 3
                n[axis] = np.where(d[axis] < F32(0), F32(1), F32(-1)).astype(F32)
                v = put(hit, _response32(v, n, surface, mu))
                any_hit |= hit
        else:
            if shape == "plane":
                hit = d[0] * b[0] + d[1] * b[1] + d[2] * b[2] < F32(0)
                v_new = _response32(v, [np.full(nn, b[t], F32) for t in range(3)], surface, mu)
            elif shape == "ball":
                L = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                hit = L < b[0]
                with np.errstate(invalid="ignore", divide="ignore"):
                    n = [(d[t] / L).astype(F32) for t in range(3)]
                    v_new = _response32(v, n, surface, mu)
                v_new = [np.where(L <= F32(1e-20), F32(0), v_new[t]).astype(F32) for t in range(3)]
            else:
                q = [b[t] - np.abs(d[t]) for t in range(3)]
                hit = (np.abs(d[0]) < b[0]) & (np.abs(d[1]) < b[1]) & (np.abs(d[2]) < b[2])
                ax = np.where((q[0] <= q[1]) & (q[0] <= q[2]), 0, np.where(q[1] <= q[2], 1, 2))
                n = [np.where(ax == t, np.where(d[t] < F32(0), F32(-1), F32(1)), F32(0)).astype(F32) for t in range(3)]
                v_new = _response32(v, n, surface, mu)
            any_hit = live & hit
            v = put(any_hit, v_new)
        if surface != "sticky":
            v = put(any_hit, [(v[t] * damp).astype(F32) for t in range(3)])
    return np.stack(v, 1)
