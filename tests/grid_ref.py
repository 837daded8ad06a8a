"""Plain float64 numpy reference of the stress-free P2G sums and of the grid
update (normalisation + gravity, fixed cubes, plane colliders), written from
the formulas (utils.py:89-134 with zero stress, utils.py:177-183,
boundary_conditions.py:23-27, collider.py:13-44), plus the operator lists and
scene S shared by test_grid_ref_oracle.py and test_gpu_grid_ops.py.

numpy only: no device code, nothing from the oracle.  What is taken in f32 is
what the library stores in f32 (dx, inv_dx, dt*g, the operator constants, the
collider's 0.99) and the one discrete decision the particles make (the base
cell); every sum, product, division and square root is float64.
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -23          # f32 unit roundoff x2 (one ulp at 1.0): the unit of every bound below
AMBIG = 1e-6              # a node this close to a plane or a cube face may be decided either way in f32
F32 = np.float32


def f32(a):
    """The f32 value(s) of `a`, as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ P2G --
def p2g_ref(x, v, C, mass, n_grid, dx32, inv_dx32, kick=None):
    """m_i = sum_p w m_p, (mv)_i = sum_p w m_p (v_p + C_p dpos), and per node
    sum_p |w m_p (v_p + C_p dpos)| (the scale a summation error is relative
    to).  `kick`: [n, 3] float64 added to v first (impulses).  Base cell from
    the f32 decision int(f32(x * inv_dx) - 0.5f); the rest float64.
    Returns (m [ng^3], mv [ng^3, 3], abs_terms [ng^3, 3])."""
    ng = int(n_grid)
    x32 = np.ascontiguousarray(x, F32).reshape(-1, 3)
    n = x32.shape[0]
    gp32 = (x32 * F32(inv_dx32)).astype(F32)
    base = (gp32 - F32(0.5)).astype(F32).astype(np.int64)  # truncation toward zero
    dx, inv_dx = float(F32(dx32)), float(F32(inv_dx32))
    x64 = x32.astype(np.float64)
    v64 = np.asarray(v, np.float64).reshape(n, 3).copy()
    if kick is not None:
        v64 += np.asarray(kick, np.float64).reshape(n, 3)
    C64 = np.asarray(C, np.float64).reshape(n, 3, 3)
    m64 = np.asarray(mass, np.float64).reshape(n)
    fx = x64 * inv_dx - base
    w = np.stack([0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1.0) ** 2, 0.5 * (fx - 0.5) ** 2], 0)  # [3, n, 3(axis)]
    m = np.zeros(ng ** 3)
    mv = np.zeros((ng ** 3, 3))
    ab = np.zeros((ng ** 3, 3))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                o = np.array([i, j, k], np.float64)
                dpos = (o - fx) * dx
                wm = w[i, :, 0] * w[j, :, 1] * w[k, :, 2] * m64
                term = wm[:, None] * (v64 + np.einsum("nrc,nc->nr", C64, dpos))
                node = base + np.array([i, j, k])
                ok = np.all((node >= 0) & (node < ng), axis=1)
                g = (node[ok, 0] * ng + node[ok, 1]) * ng + node[ok, 2]
                np.add.at(m, g, wm[ok])
                np.add.at(mv, g, term[ok])
                np.add.at(ab, g, np.abs(term[ok]))
    return m, mv, ab


# ----------------------------------------------------------- grid update --
def collider(point, normal, friction=0.0):
    return ("collider", tuple(point), tuple(normal), float(friction))


def cube(center, half):
    return ("cube", tuple(center), tuple(half))


def unit_normal32(normal):
    """Normalised in float64, then stored as f32 (gsmpm_mpm_add_plane_collider)."""
    n = np.asarray(normal, np.float64)
    return f32(n / np.sqrt((n * n).sum()))


def node_positions(n_grid, dx32):
    idx = np.stack(np.meshgrid(*[np.arange(n_grid)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return idx.astype(np.float64) * float(F32(dx32))


def node_update_ref(mv, m, n_grid, dx32, dt_g32, ops, active):
    """v = mv / m + dt g where m > 1e-15 (else 0), then `ops` in order: a
    fixed cube (strict |p - c| < s on all axes, skipped when its `active`
    entry is false) zeroes v; a collider (always active) is collider.py's
    collide.  Returns (v_out [ng^3, 3], ambiguous [ng^3] bool): ambiguous
    marks a node within 1e-6 of a collider plane or of a cube face plane --
    geometry only."""
    nn = int(n_grid) ** 3
    mv = np.asarray(mv, np.float64).reshape(nn, 3)
    m = np.asarray(m, np.float64).reshape(nn)
    p = node_positions(n_grid, dx32)
    live = m > float(F32(1e-15))
    v = np.zeros((nn, 3))
    v[live] = mv[live] / m[live, None] + f32(dt_g32)[None, :]
    ambiguous = np.zeros(nn, bool)
    damp = float(F32(0.99))
    for op, act in zip(ops, active):
        if op[0] == "cube":
            d = np.abs(p - f32(op[1])[None, :]) - f32(op[2])[None, :]
            ambiguous |= (np.abs(d) < AMBIG).any(1)
            if act:
                v[(d < 0).all(1) & live] = 0.0
        else:
            n = unit_normal32(op[2])
            fr = float(F32(op[3]))
            dot = (p - f32(op[1])[None, :]) @ n
            ambiguous |= np.abs(dot) < AMBIG
            below = (dot < 0) & live
            vb = v[below]
            nc = vb @ n
            vb = vb - np.minimum(nc, 0.0)[:, None] * n[None, :]
            ln = np.sqrt((vb * vb).sum(1))
            fric = (nc < 0) & (ln > 1e-20)
            sc = np.maximum(0.0, ln[fric] + nc[fric] * fr)
            vb[fric] = sc[:, None] * (vb[fric] / ln[fric, None])
            v[below] = vb * damp
    return v, ambiguous


def acting_nodes(mv, m, n_grid, dx32, dt_g32, ops):
    """How many massive nodes lie below a collider plane of `ops` with inward
    velocity (v . n < 0, v = mv / m + dt g before any operator): the nodes on
    which a collider does more than the 0.99 damping."""
    nn = int(n_grid) ** 3
    v, _ = node_update_ref(mv, m, n_grid, dx32, dt_g32, [], [])
    live = np.asarray(m, np.float64).reshape(nn) > float(F32(1e-15))
    p = node_positions(n_grid, dx32)
    hit = np.zeros(nn, bool)
    for op in ops:
        if op[0] == "collider":
            n = unit_normal32(op[2])
            hit |= ((p - f32(op[1])[None, :]) @ n < 0) & (v @ n < 0)
    return int((hit & live).sum())


# ------------------------------------------------------- operator lists --
def _col1(fr):
    return collider((1.013, 0.987, 0.913), (0.3, -0.5, 0.81), fr)


COL2 = collider((0.95, 1.02, 1.1), (-0.6, 0.2, 0.77), 0.25)
CUBE = cube((1.013, 1.207, 0.513), (0.41, 0.83, 0.29))
LEGO_CUBE = cube((1.0, 1.2, 0.5), (1.0, 0.8, 0.3))

# name -> (ops in order, active flag per op)
OP_LISTS = {
    "a": ([_col1(0.0)], [1]),
    "b": ([_col1(0.5)], [1]),
    "c": ([_col1(3.0)], [1]),          # friction 3: the tangential speed clamps to 0
    "d": ([_col1(0.5), COL2], [1, 1]),
    "e": ([_col1(0.5), CUBE], [1, 1]),
    "f": ([CUBE, _col1(0.5)], [1, 1]),
    "g": ([CUBE, _col1(0.5)], [0, 1]),  # as f, the cube inactive
    "h": ([collider((0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 0.5), LEGO_CUBE], [1, 1]),  # on the lattice at n_grid 50
}


def add_ops_oracle(ref, ops):
    """The list on an OracleMPM; returns nothing (op index = list index)."""
    for op in ops:
        if op[0] == "cube":
            ref.add_fixed_box(list(op[1]), list(op[2]))
        else:
            ref.add_collider(list(op[1]), list(op[2]), op[3])


def add_ops_sim(sim, ops, active):
    """The list on a gsmpm Simulator; returns the activity mask of `active`."""
    mask = 0
    for op, act in zip(ops, active):
        if op[0] == "cube":
            b = sim.add_fixed_cube(list(op[1]), list(op[2]))
        else:
            b = sim.add_plane_collider(list(op[1]), list(op[2]), op[3])
        if act:
            mask |= 1 << b
    return mask


# --------------------------------------------------------------- scene S --
def scene(n=4000, n_grid=32, c_scale=20.0):
    """Scene S: lego_problem(n, n_grid), v = 2 N(0,1) from default_rng(11),
    random C of scale `c_scale`, jelly as written (stress-free), the config's
    gravity, dt 1e-4."""
    from scenarios import lego_problem
    prob = lego_problem(n, n_grid)
    cfg = prob["cfg"]
    rng = np.random.default_rng(11)
    x = np.ascontiguousarray(prob["x"], F32)
    v = (2.0 * rng.standard_normal(x.shape)).astype(F32)
    C = (c_scale * rng.standard_normal((len(x), 9))).astype(F32)
    kw = dict(n_grid=n_grid, grid_extent=cfg["grid_extent"], material="jelly", E=cfg["E"], nu=cfg["nu"],
              density=cfg["density"], gravity=tuple(cfg["gravity"]))
    dt = 1e-4
    dx32 = F32(cfg["grid_extent"] / n_grid)
    inv_dx32 = F32(n_grid / cfg["grid_extent"])
    dt_g32 = np.array([F32(dt) * F32(g) for g in cfg["gravity"]], F32)
    mass = (F32(cfg["density"]) * prob["vol"].astype(F32)).astype(F32)
    return dict(x=x, v=v, C=C, cov=prob["cov"], vol=prob["vol"], mass=mass, kw=kw, dt=dt, dx32=dx32,
                inv_dx32=inv_dx32, dt_g32=dt_g32, n_grid=n_grid)
