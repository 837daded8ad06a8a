"""The CPU oracle's grid operators and P2G sums against the float64 reference
of tests/grid_ref.py, so that the GPU tests (test_gpu_grid_ops.py) have two
independent witnesses: the f32 oracle (which decides the lattice-aligned
predicates as the kernels must) and float64 numpy written from the formulas.

Operators (om_grid_ops on random gv_out, as test_oracle_kat.py drives it):
grids 16, 24, 50; velocity scales 1e-3, 1, 50 with a random per-node factor
of 1 or 1e-4; lists a-h of grid_ref.OP_LISTS.  Metric: per node
max|got - ref| / ||v_before|| over the nodes grid_ref does not mark ambiguous
(within 1e-6 of a plane or cube face).  Lists a-g are off the lattice: they
have no ambiguous node at any of the three grids (asserted; smallest plane
distance 7.0e-5).  Bound 8 * 2^-23: the operator chain is about 25 roundings
and the oracle measures at most 2.1 * 2^-23 on a-g (1.92 when the issue
was written, with other random draws), so the bound is about 4x the measured
value.  List h sits on the lattice at n_grid 50 (dx = 0.04f is
inexact): there the test shows that the ambiguous set holds nodes that the
oracle's f32 predicates and a float64 reading of the same geometry decide
differently -- the case the GPU test pins the kernels' predicates with.

P2G (OracleMPM.substep_begin on scene S: lego 4000 at 32^3, v = 2 N(0,1), C of
scale 20, stress-free jelly): errors are scaled by the global maxima max m
and max sum|terms| (a node that only sees near-zero spline weights inherits
the f32 error of fx, so a per-node scale would measure that instead).
Measured at this shape: mass 1.55 * 2^-23, momentum 1.42 * 2^-23 (the serial
f32 sum of up to ~100 terms a node); asserted at 4x those.  Total mass and
total momentum are within 1e-7 relative of the particle sums (measured:
the reference 1e-15, the oracle 1e-9 mass and 4e-8 momentum)."""
import ctypes

import numpy as np
import pytest

import grid_ref as G
import oracle as O

OPS_BOUND = 8 * G.EPS
P2G_MEASURED = {"m": 1.55, "mv": 1.42}  # in units of 2^-23, at scene S's shape


def _oracle(n_grid):
    x = np.full((1, 3), 1.0, np.float32)
    cov = np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32), (1, 1))
    return O.OracleMPM(x, cov, np.full(1, 1e-4, np.float32), n_grid=n_grid, grid_extent=2.0, material="jelly",
                       E=2e5, nu=0.3, density=200.0, gravity=(0.0, 0.0, 0.0))


def _apply(s, active):
    n = len(s.ops)
    ops = (O._GridOp * n)()
    for i, (k, a, b, fr) in enumerate(s.ops):
        ops[i].kind, ops[i].friction = k, fr
        ops[i].a[:] = list(a)
        ops[i].b[:] = list(b)
    O.lib().om_grid_ops(ctypes.byref(s._st), n, ops, (ctypes.c_int32 * n)(*[int(a) for a in active]))


def _random_velocities(n_grid, scale, seed):
    rng = np.random.default_rng(seed)
    nn = n_grid ** 3
    v = rng.standard_normal((nn, 3)) * scale * rng.choice([1.0, 1e-4], size=(nn, 1))
    return v.astype(np.float32)


def _run_ops(name, n_grid, scale):
    ops, active = G.OP_LISTS[name]
    s = _oracle(n_grid)
    G.add_ops_oracle(s, ops)
    before = _random_velocities(n_grid, scale, seed=n_grid + ord(name))
    s.gv_out[:] = before
    _apply(s, active)
    ref, amb = G.node_update_ref(before, np.ones(n_grid ** 3), n_grid, s._st.dx, np.zeros(3), ops, active)
    norm = np.sqrt((before.astype(np.float64) ** 2).sum(1))
    assert norm.min() > 0
    err = np.abs(s.gv_out.astype(np.float64) - ref).max(1) / norm
    return before, s.gv_out.copy(), ref, amb, err


@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0])
@pytest.mark.parametrize("n_grid", [16, 24, 50])
@pytest.mark.parametrize("name", list("abcdefg"))
def test_oracle_grid_ops_match_float64(name, n_grid, scale):
    before, got, ref, amb, err = _run_ops(name, n_grid, scale)
    assert not amb.any(), f"list {name} at {n_grid}^3: {int(amb.sum())} ambiguous nodes"
    changed = int((np.abs(ref - before).max(1) > 0).sum())
    print(f"list {name} n_grid {n_grid} scale {scale:g}: max err {err.max() / G.EPS:.2f} * 2^-23, "
          f"{changed} nodes changed, 0 excluded")
    assert changed > n_grid ** 3 // 20  # the operators act on a good share of the grid
    assert err.max() <= OPS_BOUND, err.max() / G.EPS


@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0])
def test_oracle_lattice_list_f32_decisions(scale):
    """List h at n_grid 50: off the ambiguous set the oracle meets the same
    bound; inside it there are nodes where the float64 reading of the
    geometry and the oracle's f32 predicates differ (25 * 0.04f rounds to
    exactly 1.0 in f32: not below the plane z = 1; unrounded it is 2.2e-8
    below)."""
    before, got, ref, amb, err = _run_ops("h", 50, scale)
    assert err[~amb].max() <= OPS_BOUND, err[~amb].max() / G.EPS
    differ = amb & (err > 1e-3)  # a different decision changes v by 1 % (the 0.99) at the least
    print(f"list h scale {scale:g}: {int(amb.sum())} ambiguous nodes, {int(differ.sum())} decided differently, "
          f"max err elsewhere {err[~amb].max() / G.EPS:.2f} * 2^-23")
    assert differ.sum() >= 1000, int(differ.sum())
    assert not (~amb & (err > 1e-3)).any()
    # the layer k = 25 is the bulk of them: the oracle leaves it alone where the cube does not reach
    layer = np.zeros((50, 50, 50), bool)
    layer[:, :, 25] = True
    assert (differ & layer.reshape(-1)).sum() >= 1000


def _p2g_errors(got_m, got_mv, m, mv, ab):
    em = np.abs(got_m.astype(np.float64) - m).max() / m.max()
    emv = np.abs(got_mv.astype(np.float64) - mv).max() / ab.max()
    return em, emv


def test_oracle_p2g_matches_float64():
    S = G.scene()
    ref = O.OracleMPM(S["x"], S["cov"], S["vol"], v=S["v"], **S["kw"])
    ref.C[:] = S["C"]
    assert np.array_equal(ref.mass, S["mass"])
    ref.substep_begin(S["dt"])
    assert np.abs(ref.stress).max() == 0.0  # jelly as written: stress-free
    m, mv, ab = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    em, emv = _p2g_errors(ref.gm, ref.gv_in, m, mv, ab)
    m64 = S["mass"].astype(np.float64)
    mom = (m64[:, None] * S["v"].astype(np.float64)).sum(0)
    cons_m = abs(m.sum() - m64.sum()) / m64.sum()
    cons_p = np.abs(mv.sum(0) - mom).max() / np.abs(mom).max()
    om = abs(ref.gm.astype(np.float64).sum() - m64.sum()) / m64.sum()
    op = np.abs(ref.gv_in.astype(np.float64).sum(0) - mom).max() / np.abs(mom).max()
    print(f"P2G oracle vs float64: mass {em / G.EPS:.2f} * 2^-23, momentum {emv / G.EPS:.2f} * 2^-23; "
          f"totals: reference {cons_m:.1e} / {cons_p:.1e}, oracle {om:.1e} / {op:.1e}")
    assert em <= 4 * P2G_MEASURED["m"] * G.EPS, em / G.EPS
    assert emv <= 4 * P2G_MEASURED["mv"] * G.EPS, emv / G.EPS
    assert cons_m < 1e-7 and cons_p < 1e-7, (cons_m, cons_p)
    assert om < 1e-7 and op < 1e-7, (om, op)


def test_scene_collider_acts():
    """Scene S with the oblique plane: thousands of nodes carry mass, and on
    at least 500 of them the collider acts (below the plane, moving inward)."""
    S = G.scene()
    m, mv, _ = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    n = G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], G.OP_LISTS["b"][0])
    print(f"scene S: {int((m > 1e-15).sum())} massive nodes, collider acting on {n}")
    assert n >= 500
