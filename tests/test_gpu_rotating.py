"""Rotating colliders (gsmpm_mpm_add_rotating_collider, gsmpm_mpm_get_poses;
k_set_poses and the ROT instantiations of k_grid and k_grid_f) on the GPU: the
pose table against the float64 pose, the grid update against the float64
reference of tests/rotating_ref.py, mixed tables, a translating record in a
rotating table against the MOV kernels bit for bit, the two pipelines against
each other, exact particle-level bounds for particles a sticky box carries,
the cached graphs, the drop-in; plus what is refused.

Scene S (grid_ref.scene): 4,000 particles at 32^3, stress-free, dt 1e-4.
Velocity W, the motion window and the times are moving_ref's (the plane's
second time is 0.0124, rotating_ref.T), omega = (7, -4, 11) about the pivot
(0.95, 1.05, 1.0); geometry is collider_ref.GEOMETRY and the oblique plane of
list b.  At every shape x time pair no massive node is ambiguous and >= 500
nodes have their relative velocity pointing into the collider; every
grid-level case asserts both from the reference side.

Bounds:
* pose table, against rotating_ref.pose64 (float64 from the stored f32 values,
  the f32 tau included): R one ulp32 of 1 = 2^-23 per entry (one rounding of an
  f64 value whose own error is far below it); o = piv + w tau is two roundings,
  EPS |o|inf; c = o + R (a - piv) adds the final rounding, EPS / 2 |c|inf, and
  2.5 EPS |a - piv|_1 for a row of R (a - piv): EPS / 2 |a - piv|_1 each for
  the rounding of a - piv, of R's entries (|R_ij| <= 1), of the three products
  and of each of the two sums.  With |a - piv|_1 < 0.4 |c|inf that is below
  3 EPS |c|inf, which the test asserts of its own bound.
* v_out against the float64 reference fed the GPU's own mass, v_in and pose,
  per node in units of ||v_in / m|| + ||dt g||, on the nodes the reference
  does not mark ambiguous: max(4 e32, 8 EPS), test_gpu_colliders.py's own, e32
  the f32 transcription's error on the same inputs and the same pose, computed
  in the test.  Massless nodes exactly 0; nodes outside every operator
  bit-equal to the update without operators.
* a translating record in a rotating table: bit for bit the MOV kernels'
  v_out on the nodes where the two handles read bit-equal mass and v_in
  (test_gpu_moving.py's _same_inputs rule).
* fused against per-phase after 40 substeps: 1e-4 of each field's maximum.
* carried particles, K = 40 substeps inside a sticky box turning with omega and
  moving with W, against the float64 recurrence x <- x + dt wc(x, t_s) started
  from the GPU's x_0; V = |W|inf + 2 |omega|inf rmax bounds the node velocities
  of the stencils (rmax: the farthest selected particle from the pivot, plus
  two cells).  Node values: four roundings of wc and the f32 o and p - o,
  (4 V + 8 |omega|inf) EPS.  G2P: a 27-term weighted sum, 32 EPS V as in
  test_gpu_moving.py.  So bv = (36 V + 8 |omega|inf) EPS, plus 2 |omega|inf
  times the position error so far; a substep adds EPS / 2 ulp32(1.5) (one
  rounding of x), dt (bv + EPS V) and grows what was there by 1 + 2 dt
  |omega|inf: bx is that recurrence.  C = sum 4 inv_dx^2 w_i v_i (p_i - x_p)^T
  weighs the same errors with at most 6 inv_dx: bC = 6 inv_dx bv.
* graphs: as many after six timed calls at advancing times as after the first.
* drop-in against direct calls: 1e-6 of the field's maximum on x and v, as the
  moving drop-in test.

Measured on an MI355X, in EPS = 2^-23.  Pose table, 300 substeps x 2 records:
worst error over its bound R 0.25, c 0.46, o 0.51, and bit-equal to pose32 on
all 600 poses.  v_out against float64 at t = 0.0507: sticky 8.7 (ball), 18.7
(box), 31.5 (plane), 38.3 (walls); slip 21.2 (box), 33.5 (ball), 44.2
(plane), 58.5 (walls); separate 15.1 (box), 24.4 (ball), 45.1 (plane), 62.5
(walls); 21.4 and 25.5 on the mixed table in its two orders; at the second
time 24.0 .. 32.1, outside the window 0.94 .. 1.54 (bound 8).  The response
runs on u = R^T (v - wc) with |wc| up to 14, so the figure is large in units
of a small node velocity, and the transcription's own error e32 is the same
figure, the GPU being bit-equal to the transcription in every case (bound
4 e32 = 35 .. 250).  A translating box in a rotating table: array_equal to the
MOV kernels on 2,465 .. 2,886 of the 5,883 massive nodes, 267 .. 303 of them
inside the box.  Fused against per-phase: x 7.8e-8, v 5.3e-7, C 5.9e-7,
F_trial 2.9e-7.  Carried: 924 particles, V 14.42; |v - wc(x)| 2.31e-5 (bound
1.32e-4), |x_K - recurrence| 2.04e-6 (bound 2.80e-6), |C - [omega]x| 2.19e-5
(bound 1.27e-2: the 6 inv_dx weighting assumes no cancellation, which a
linear field has plenty of).  Graphs: 1 after each of six calls.  Drop-in:
x 7.9e-8, v 4.4e-7, not bit-equal (two handles), poses bit-equal.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import collider_ref as CR
import grid_ref as G
import moving_ref as M
import rotating_ref as R
from conftest import rel_err
from test_gpu_grid_ops import _grid_sim, _read_grid, _t

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "C", "F_trial")
SURF = {"sticky": 0.0, "slip": 0.5, "separate": 0.5}
SHAPES = ("plane", "ball", "box", "walls")
T_IN = R.T_IN


@functools.lru_cache(maxsize=None)
def _witness():
    """Scene S and its float64 P2G sums (the counts are taken from them)."""
    S = G.scene()
    m, mv, _ = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    return S, m, mv


def _add(sim, ops, active):
    """The list on a Simulator; returns the activity mask."""
    mask = 0
    for op, act in zip(ops, active):
        if op[0] == "rot":
            b = sim.add_collider(**CR.geometry_kw(op[1]), velocity=op[2], move_start=op[3], move_end=op[4],
                                 angular_velocity=op[5], pivot=op[6])
        elif op[0] == "mov":
            b = sim.add_collider(**CR.geometry_kw(op[1]), velocity=op[2], move_start=op[3], move_end=op[4])
        elif op[0] == "ext":
            b = sim.add_collider(**CR.geometry_kw(op))
        elif op[0] == "cube":
            b = sim.add_fixed_cube(list(op[1]), list(op[2]))
        else:
            b = sim.add_plane_collider(list(op[1]), list(op[2]), op[3])
        if act:
            mask |= 1 << b
    return mask


def _poses_of(ops, table):
    """{index in ops: pose} from one substep's row of Simulator.poses (rotating records in table order)."""
    rots = [i for i, op in enumerate(ops) if op[0] == "rot"]
    assert table.shape == (len(rots), 16)
    return {i: table[j] for j, i in enumerate(rots)}


def _hit_any(S, ops, t, poses):
    p = CR.node_positions32(S["n_grid"], S["dx32"])
    hit = np.zeros(len(p), bool)
    for i, op in enumerate(ops):
        if op[0] == "cube":
            hit |= (np.abs(p - G.f32(op[1])) < G.f32(op[2])).all(1)
            continue
        if op[0] == "collider":
            op = CR.ext("plane", point=op[1], normal=op[2])
        hit |= R.hit_nodes(S["n_grid"], S["dx32"], op, t, poses.get(i))
    return hit


def _check(S, grid, ops, active, t, poses, tag):
    """v_out of one substep at time t against the float64 reference and the f32 transcription, both on the
    GPU's own pose."""
    ng = S["n_grid"]
    mass, v_in, v_out = grid["mass"].reshape(-1), grid["v_in"], grid["v_out"]
    args = (v_in, mass, ng, S["dx32"], S["dt_g32"])
    ref, amb = R.node_update_ref(*args, ops, active, t, poses)
    t32 = R.node_update_f32(*args, ops, active, t, poses)
    free32 = R.node_update_f32(*args, [], [])
    live = mass > np.float32(1e-15)
    scale = np.zeros(ng ** 3)
    scale[live] = np.sqrt(((v_in[live].astype(np.float64) / mass[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum())
    ok = ~amb
    e32 = (np.abs(t32.astype(np.float64) - ref).max(1) / scale)[ok].max()
    e = (np.abs(v_out.astype(np.float64) - ref).max(1) / scale)[ok].max()
    bound = max(4 * e32, 8 * G.EPS)
    outside = ~_hit_any(S, ops, t, poses) & ok
    changed = int((np.abs(ref - free32.astype(np.float64)).max(1) > 1e-3 * scale)[live].sum())
    print(f"ROTATING {tag} t={t}: massive {int(live.sum())} ambiguous {int((amb & live).sum())} changed {changed} | "
          f"v_out vs f64 {e / G.EPS:.2f} EPS (transcription {e32 / G.EPS:.2f}, bound {bound / G.EPS:.2f}); "
          f"bit-equal to the transcription: {bool(np.array_equal(v_out, t32))}")
    assert not (amb & live).any()
    assert np.all(v_out[~live] == 0)
    assert (outside & live).sum() >= 500 and np.array_equal(v_out[outside], free32[outside])
    assert changed >= CR.MIN_ACTING
    assert e <= bound, (e / G.EPS, bound / G.EPS)
    return e, e32


def _assert_acting(name, t):
    S, m, mv = _witness()
    op = R.rot(CR.ext(name, "slip", 0.5, **R.geo(name)))
    _, acting, amb = R.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], op, t)
    assert acting >= CR.MIN_ACTING and amb == 0
    assert acting == R.ACTING[name][R.T[name].index(t)]


def _same_inputs(S, a, b, ops, t, tag):
    """test_gpu_moving.py's rule: the nodes on which two handles' grid updates read the same bits, at least 100
    of them massive and inside the operators, at least 1,000 massive in all."""
    same = (a["mass"].reshape(-1) == b["mass"].reshape(-1)) & (a["v_in"] == b["v_in"]).all(1)
    live = a["mass"].reshape(-1) > np.float32(1e-15)
    inside = _hit_any(S, ops, t, {}) & live
    print(f"ROTATING {tag}: inputs bit-equal on {int((same & live).sum())} of {int(live.sum())} massive nodes, "
          f"{int((same & inside).sum())} of the {int(inside.sum())} inside")
    assert (same & inside).sum() >= 100 and (same & live).sum() >= 1000
    return same


def _one_substep(dev, S, ops, active, t):
    """A fresh per-phase keep-grid handle, the list, one timed substep; (grid, {op index: the GPU's pose})."""
    sim = _grid_sim(dev, S)
    assert sim.pipeline == "phased"
    mask = _add(sim, ops, active)
    sim.step(S["dt"], [mask], [t])
    grid = _read_grid(sim)
    poses = _poses_of(ops, sim.poses(1)[0]) if any(op[0] == "rot" for op in ops) else {}
    return grid, poses


# ------------------------------------------------------ 1. the pose table --
def _pose_bounds(op, t):
    P = R.pose64(op, t)
    e1 = np.abs(G.f32(op[1][3]) - G.f32(op[6])).sum()
    bo = G.EPS * np.abs(P["o"]).max()
    bc = bo + 0.5 * G.EPS * np.abs(P["c"]).max() + 2.5 * G.EPS * e1
    assert bc <= 3 * G.EPS * np.abs(P["c"]).max()
    return P, 2.0 ** -23, bc, bo


def test_pose_table(dev):
    """One call of 300 substeps (two k_set_times batches) with two rotating records whose window edges fall
    inside the call, in a table that also holds a cube and a translating record: the whole table against pose64."""
    from gsmpm.bc import substep_times
    from gsmpm.sim import Simulator
    S = _witness()[0]
    n, t_start = 300, 0.005
    a = R.rot(CR.ext("box", "slip", 0.5, 0.9, **CR.GEOMETRY["box"]))  # its window opens inside the call
    b = R.rot(CR.ext("plane", "separate", 0.5, 0.9, **R.geo("plane")), omega=(-3.0, 9.0, 5.0), pivot=(1.1, 0.9, 1.05),
              velocity=(0.0, 0.0, 0.0), t_start=0.001, t_end=0.0203)  # its window closes inside the call
    ops = [G.CUBE, a, M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])), b]
    sim = Simulator(len(S["x"]), **S["kw"])
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    mask = _add(sim, ops, [1, 1, 1, 1])
    first = sim.poses(1)  # the add filled substep 0 at t = 0: both stand in the pose of t0
    for j, op in enumerate((a, b)):
        assert np.array_equal(first[0, j, :9].reshape(3, 3), np.eye(3, dtype=np.float32))
        assert np.array_equal(first[0, j], R.pose32(op, 0.0))
    times, t_end = substep_times(t_start, S["dt"], n)
    assert times[0] < M.WINDOW[0] < times[-1] < M.WINDOW[1] and times[0] > 0.001 and 0.0203 < times[-1]
    sim.step(S["dt"], [mask] * n, times)
    table = sim.poses(n)
    assert table.shape == (n, 2, 16) and np.all(table[:, :, 15] == 0)
    worst = {"R": 0.0, "c": 0.0, "o": 0.0}
    equal = 0
    for s, t in enumerate(times):
        for j, op in enumerate((a, b)):
            P, bR, bc, bo = _pose_bounds(op, t)
            got = table[s, j].astype(np.float64)
            eR = np.abs(got[:9].reshape(3, 3) - P["R"]).max()
            ec, eo = np.abs(got[9:12] - P["c"]).max(), np.abs(got[12:15] - P["o"]).max()
            worst = {"R": max(worst["R"], eR / bR), "c": max(worst["c"], ec / bc), "o": max(worst["o"], eo / bo)}
            assert eR <= bR and ec <= bc and eo <= bo, (s, j, eR, ec, eo)
            equal += bool(np.array_equal(table[s, j], R.pose32(op, t)))
    print(f"ROTATING pose table, 300 substeps x 2 records: worst error over its bound R {worst['R']:.3f} "
          f"(bound 2^-23), c {worst['c']:.3f}, o {worst['o']:.3f}; bit-equal to pose32 on {equal} of {2 * n}")
    # the edges: a stands until its window opens, b stands from its end on
    k = sum(t < M.WINDOW[0] for t in times)
    assert 0 < k < n and all(np.array_equal(table[s, 0], table[0, 0]) for s in range(k))
    assert not np.array_equal(table[k + 1, 0], table[0, 0])
    k = sum(t < 0.0203 for t in times)
    assert 0 < k < n - 1 and all(np.array_equal(table[s, 1], table[n - 1, 1]) for s in range(k + 1, n))
    assert not np.array_equal(table[k - 2, 1], table[n - 1, 1])
    # past the first batch of 256 the poses still advance with the times
    assert not np.array_equal(table[255, 0], table[256, 0]) and not np.array_equal(table[256, 0], table[299, 0])
    assert np.isfinite(sim.get("v").cpu().numpy()).all()
    with pytest.raises(RuntimeError, match="more substeps"):
        sim.poses(n + 1)


# ------------------------------------------------------ 2. grid level --
@pytest.mark.parametrize("surface", list(SURF))
@pytest.mark.parametrize("name", SHAPES)
def test_grid_level_shapes(dev, name, surface):
    """Each shape with each surface inside the window, damping 0.9 (ignored by sticky)."""
    S = _witness()[0]
    _assert_acting(name, T_IN)
    ops, active = [R.rot(CR.ext(name, surface, SURF[surface], 0.9, **R.geo(name)))], [1]
    grid, poses = _one_substep(dev, S, ops, active, T_IN)
    _check(S, grid, ops, active, T_IN, poses, f"{name} {surface}")


@pytest.mark.parametrize("name", SHAPES)
def test_three_phases_of_the_window(dev, name):
    """Before the window (the pose of t0: R = I, and no velocity), inside it, and from its end on (the pose of
    t1, and no velocity)."""
    S = _witness()[0]
    op = R.rot(CR.ext(name, "slip", 0.5, 0.9, **R.geo(name)))
    for t in R.T[name]:
        _assert_acting(name, t)
        grid, poses = _one_substep(dev, S, [op], [1], t)
        if t < M.WINDOW[0]:
            assert np.array_equal(poses[0][:9].reshape(3, 3), np.eye(3, dtype=np.float32))
        if t >= M.WINDOW[1]:  # the pose of t1
            assert np.abs(poses[0][:9].reshape(3, 3) - R.pose64(op, M.WINDOW[1])["R"]).max() <= 2.0 ** -23
        _check(S, grid, [op], [1], t, poses, f"phases {name}")


# -------------------------------------------------------- 3. mixed tables --
def _mixed(order):
    ops = [G.CUBE, R.rot(CR.ext("box", "separate", 0.5, 0.9, **CR.GEOMETRY["box"])),
           CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]),
           M.mov(CR.ext("plane", "separate", 0.5, 0.9, **R.geo("plane"))),
           R.rot(CR.ext("walls", "slip", 0.5, 0.9, **CR.GEOMETRY["walls"]), omega=(-3.0, 9.0, 5.0),
                 pivot=(1.1, 0.9, 1.05))]
    return ops[::-1] if order == "reversed" else ops


@pytest.mark.parametrize("order", ["cube_box_ball_plane_walls", "reversed"])
def test_grid_level_mixed_tables(dev, order):
    """A fixed cube, a rotating box, a static ball, a translating plane and rotating walls in one table, in two
    orders: the rotating index differs from the op index, and every substep has two poses."""
    S = _witness()[0]
    ops, active = _mixed(order), [1] * 5
    grid, poses = _one_substep(dev, S, ops, active, T_IN)
    assert sorted(poses) == ([1, 4] if order != "reversed" else [0, 3])
    assert not np.array_equal(poses[sorted(poses)[0]], poses[sorted(poses)[1]])
    _check(S, grid, ops, active, T_IN, poses, f"mixed {order}")


# --------------------- 4. a translating record in a rotating table is MOV's --
@pytest.mark.parametrize("surface", list(SURF))
def test_translating_record_in_a_rotating_table_equals_the_mov_kernels(dev, surface):
    """k_grid<EXT, ROT> on a translating box (the table's rotating ball switched off) == k_grid<EXT, MOV>."""
    S = _witness()[0]
    box = M.mov(CR.ext("box", surface, SURF[surface], 0.9, **CR.GEOMETRY["box"]))
    ball = R.rot(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]))
    got, _ = _one_substep(dev, S, [ball, box], [0, 1], T_IN)
    want, _ = _one_substep(dev, S, [box], [1], T_IN)
    same = _same_inputs(S, got, want, [box], T_IN, f"translating box {surface} in a rotating table")
    assert np.array_equal(got["v_out"][same], want["v_out"][same])
    free32 = M.node_update_f32(want["v_in"], want["mass"], S["n_grid"], S["dx32"], S["dt_g32"], [], [])
    assert (np.abs(want["v_out"] - free32).max(1) > 1e-3).sum() >= CR.MIN_ACTING  # the box acted


# ------------------------------------------------- 5. fused vs per-phase --
NSUB = 40
T_START = 0.02  # inside the motion window for all of the 40 substeps


def _run(dev, S, ops, active, phased, calls=(NSUB,), t_start=T_START):
    import torch
    from gsmpm.bc import substep_times
    from gsmpm.sim import Simulator
    sim = Simulator(len(S["x"]), phased=phased, **S["kw"])
    assert sim.pipeline == ("phased" if phased else "fused") and not sim.folded
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    if not phased:
        sim.set_rebin_interval(NSUB // 2)  # one re-binning inside a call of 40
    mask = _add(sim, ops, active)
    t = t_start
    for n in calls:
        times, t = substep_times(t, S["dt"], n)
        sim.step(S["dt"], [mask] * n, times)
    torch.cuda.synchronize()
    return {k: sim.get(k).cpu().numpy() for k in FIELDS}, sim


def test_fused_matches_per_phase(dev):
    """A rotating slip box, 40 substeps with one re-binning inside: k_grid_f's ROT form against k_grid's."""
    S = _witness()[0]
    ops, active = [R.rot(CR.ext("box", "slip", 0.5, 0.9, **CR.GEOMETRY["box"]))], [1]
    fused, sf = _run(dev, S, ops, active, phased=False)
    phased, sp = _run(dev, S, ops, active, phased=True)
    assert sf.pipeline == "fused" and sp.pipeline == "phased"
    errs = {k: rel_err(fused[k], phased[k]) for k in FIELDS}
    print("ROTATING fused vs per-phase, box slip: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(np.isfinite(fused[k]).all() for k in FIELDS)
    for k, e in errs.items():
        assert e < 1e-4, (k, e, errs)
    # the spin mattered: the same box only translating ends elsewhere
    plain, _ = _run(dev, S, [M.mov(ops[0][1])], active, phased=False)
    assert rel_err(plain["v"], fused["v"]) > 1e-2


# ------------------------------------------------- 6. carried particles --
def _carried_reference(S, op, K, t_start):
    """The float64 recurrence x <- x + dt wc(x, t_s) from x_0 for every particle, and which particles keep
    their whole 27-node stencil inside the box on every substep (0.01 cell inside, against rounding)."""
    from gsmpm.bc import substep_times
    dt32, dx, inv_dx = float(np.float32(S["dt"])), float(S["dx32"]), float(S["inv_dx32"])
    half = G.f32(op[1][4])
    x = S["x"].astype(np.float64).copy()
    keep = np.ones(len(x), bool)
    offs = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    times, _ = substep_times(t_start, S["dt"], K)
    xs = []
    for t in times:
        P = R.pose64(op, t)
        base = np.floor(x * inv_dx - 0.5)
        nodes = (base[:, None, :] + offs[None, :, :]) * dx
        d = (nodes - P["c"]) @ P["R"]
        keep &= (np.abs(d) < half - 0.01 * dx).all((1, 2))
        xs.append(x.copy())
        x = x + dt32 * R.wc64(op, t, x, P["o"])
    return x, xs[-1], keep, times


def test_sticky_box_carries_the_particles_inside(dev):
    """Particles whose stencils stay inside a sticky box that turns and translates move rigidly with it: v_p is
    the box's velocity at x_p, C is [omega]x (quadratic B-splines reproduce a linear field), x follows the
    recurrence; through the graph."""
    S = _witness()[0]
    K, dt32 = NSUB, float(np.float32(S["dt"]))
    op = R.rot(CR.ext("box", "sticky", **CR.GEOMETRY["box"]), t_start=T_START, t_end=float("inf"))
    xK, xlast, sel, times = _carried_reference(S, op, K, T_START)
    assert sel.sum() >= 100
    om, w = G.f32(R.OMEGA), G.f32(M.W)
    omax = np.abs(om).max()
    P = R.pose64(op, times[-1])
    rmax = np.abs(xlast[sel] - P["o"]).max() + 2 * float(S["dx32"])
    V = np.abs(w).max() + 2 * omax * rmax
    bv0 = (36 * V + 8 * omax) * G.EPS
    bx = 0.0
    for s in range(K):
        if s == K - 1:
            bx_last = bx  # the position error the last velocity sees
        bx = bx * (1 + 2 * dt32 * omax) + 2.0 ** -24 + dt32 * (bv0 + G.EPS * V)
    bv = bv0 + 2 * omax * bx_last
    bC = 6 * float(S["inv_dx32"]) * bv
    got, sim = _run(dev, S, [op], [1], phased=False)
    assert sim.graph_count() == 1  # it went through a graph
    v = got["v"].reshape(-1, 3).astype(np.float64)
    x = got["x"].reshape(-1, 3).astype(np.float64)
    C = got["C"].reshape(-1, 3, 3).astype(np.float64)
    want_v = R.wc64(op, times[-1], xlast, P["o"])
    Kx = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    ev = np.abs(v[sel] - want_v[sel]).max()
    ex = np.abs(x[sel] - xK[sel]).max()
    eC = np.abs(C[sel] - Kx[None]).max()
    print(f"ROTATING carried: {int(sel.sum())} particles, V {V:.2f}; |v - wc(x)| {ev:.2e} (bound {bv:.2e}), "
          f"|x_K - recurrence| {ex:.2e} (bound {bx:.2e}), |C - [omega]x| {eC:.2e} (bound {bC:.2e})")
    assert x[sel].max() < 1.5
    assert ev <= bv and ex <= bx and eC <= bC
    assert np.abs(v[~sel] - want_v[~sel]).max() > 1e-2  # and not everybody is carried
    moved = np.abs(xK[sel] - S["x"][sel] - K * dt32 * w).max()
    assert moved > 100 * bx  # the turning shows in the positions, far above the bound


# ---------------------------------------- 7. graphs do not depend on time --
def test_graph_count_does_not_depend_on_time(dev):
    """Six timed calls of 20 substeps at advancing times: the graphs of the first call serve them all."""
    from gsmpm.bc import substep_times
    from gsmpm.sim import Simulator
    S = _witness()[0]
    op = R.rot(CR.ext("box", "slip", 0.5, 0.9, **CR.GEOMETRY["box"]))
    sim = Simulator(len(S["x"]), **S["kw"])
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    mask = _add(sim, [op], [1])
    assert sim.graph_count() == 0
    t, counts, last = 0.0, [], []
    for _ in range(6):
        times, t = substep_times(t, S["dt"], 20)
        sim.step(S["dt"], [mask] * 20, times)
        counts.append(sim.graph_count())
        last.append(sim.poses(20)[19, 0])
    print(f"ROTATING graphs after each of six calls: {counts}")
    assert counts[0] >= 1 and all(c == counts[0] for c in counts)
    assert t > M.WINDOW[0] and not np.array_equal(last[0], last[-1])  # the calls crossed into the window
    assert np.isfinite(sim.get("v").cpu().numpy()).all()


# ------------------------------------------------------------ 8. drop-in --
def test_dropin_config_record_equals_direct_steps(dev):
    """MPM_Simulator with a rotating config record, 30 p2g2p calls, against Simulator.step given substep_masks
    and substep_times directly."""
    import torch
    from gpu_helpers import sim_args_from_cfg
    from gsmpm.bc import substep_masks, substep_times, windowed_collider
    from gsmpm.sim import Simulator
    from mpm_solver.solver import MPM_Simulator
    from scenarios import lego_problem
    S = _witness()[0]
    dt = S["dt"]
    cfg = dict(lego_problem(4000, 32)["cfg"])
    rec = dict(type="collider", id=7, shape="box", surface="slip", friction=0.5, damping=0.9,
               start_time=3.5 * dt, end_time=999.0, velocity=list(M.W), angular_velocity=list(R.OMEGA),
               pivot=list(R.PIVOT), move_start=10.5 * dt, move_end=25.5 * dt, **CR.GEOMETRY["box"])
    cfg["boundary_conditions"] = [rec]
    args = sim_args_from_cfg(cfg, 32)
    sim = MPM_Simulator(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), args, init_v=_t(dev, S["v"]))
    sim.set_boundary_conditions(args.boundary_conditions, args)
    bc = sim.grid_postprocess[0]
    assert bc.bit == 0 and bc.motion == dict(velocity=[float(a) for a in M.W], move_start=10.5 * dt,
                                             move_end=25.5 * dt, angular_velocity=[float(a) for a in R.OMEGA],
                                             pivot=[float(a) for a in R.PIVOT])
    for _ in range(30):
        sim.p2g2p(dt)
    masks, _ = substep_masks([windowed_collider(0, 3.5 * dt, 999.0)], 0.0, dt, 30)
    times, t_end = substep_times(0.0, dt, 30)
    assert sim._queue == masks and sim._queue_t == times and sim.time == t_end and masks.count(1) == 26
    sim.flush()
    op = R.rot(CR.ext("box", "slip", 0.5, 0.9, **CR.GEOMETRY["box"]), t_start=10.5 * dt, t_end=25.5 * dt)
    raw = Simulator(len(S["x"]), **S["kw"])
    raw.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    assert _add(raw, [op], [1]) == 1
    raw.step(dt, masks, times)
    plain = Simulator(len(S["x"]), **S["kw"])
    plain.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    _add(plain, [M.mov(op[1], M.W, 10.5 * dt, 25.5 * dt)], [1])
    plain.step(dt, masks, times)
    torch.cuda.synchronize()
    a = {k: sim._sim.get(k).cpu().numpy() for k in ("x", "v")}
    b = {k: raw.get(k).cpu().numpy() for k in ("x", "v")}
    errs = {k: rel_err(a[k], b[k]) for k in ("x", "v")}
    print("ROTATING drop-in against direct steps, 30 substeps: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items())
          + f"; bit-equal: {all(np.array_equal(a[k], b[k]) for k in ('x', 'v'))}")
    for k, e in errs.items():
        assert e < 1e-6, (k, e)
    assert np.array_equal(sim._sim.poses(30), raw.poses(30))
    assert sim._sim.graph_count() == raw.graph_count() == 1
    assert rel_err(plain.get("v").cpu().numpy(), b["v"]) > 1e-3  # the spin mattered
    # add_collider takes the same keys; the window defaults to the activity window, the pivot to the centre
    d = sim.add_collider("box", "sticky", start_time=0.25, end_time=0.5, angular_velocity=(0.0, 0.0, 2.0),
                         **CR.GEOMETRY["box"])
    assert d.bit == 1 and d.motion == dict(angular_velocity=[0.0, 0.0, 2.0], move_start=0.25, move_end=0.5)
    P = sim._sim.poses(1)
    assert P.shape == (1, 2, 16)
    assert np.array_equal(P[0, 1, 9:12], np.asarray(CR.GEOMETRY["box"]["center"], np.float32))
    assert np.array_equal(P[0, 1, 12:15], P[0, 1, 9:12])  # it spins in place


# ------------------------------------------------ 9. refusals and errors --
def _raw_add(sim, omega=(0.0, 0.0, 1.0), pivot=(1.0, 1.0, 1.0), velocity=(0.0, 0.0, 0.0), t_start=0.0, t_end=1.0,
             **kw):
    from gsmpm import _lib
    c = _lib.Collider()
    c.shape, c.surface = kw.get("shape", 1), kw.get("surface", 2)
    c.a[:] = kw.get("a", (1.0, 1.0, 1.0))
    c.b[:] = kw.get("b", (0.3, 0.3, 0.3))
    c.friction, c.damping = kw.get("friction", 0.0), kw.get("damping", 1.0)
    s = _lib.ColliderSpin()
    s.velocity[:] = velocity
    s.omega[:] = omega
    s.pivot[:] = pivot
    s.t_start, s.t_end = t_start, t_end
    rc = _lib.LIB.gsmpm_mpm_add_rotating_collider(sim._h, ctypes.byref(c), ctypes.byref(s))
    return rc, _lib.last_error()


def _bare(**kw):
    from gsmpm.sim import Simulator
    return Simulator(100, n_grid=32, **kw)


def test_invalid_arguments_are_refused(dev):
    from gsmpm import _lib
    sim = _bare()
    inf, nan = float("inf"), float("nan")
    bad = [
        (dict(omega=(0.0, 0.0, 0.0)), "gsmpm_mpm_add_moving_collider"),  # zero omega: the message says what to use
        (dict(omega=(nan, 0.0, 1.0)), "non-finite omega"), (dict(omega=(0.0, inf, 0.0)), "non-finite omega"),
        (dict(pivot=(nan, 1.0, 1.0)), "non-finite pivot"), (dict(pivot=(1.0, 1.0, -inf)), "non-finite pivot"),
        # everything the moving record refuses
        (dict(velocity=(nan, 0.0, 0.0)), "non-finite velocity"), (dict(velocity=(0.0, inf, 0.0)), "non-finite velocity"),
        (dict(t_start=nan), "t_start"), (dict(t_start=inf, t_end=inf), "t_start"), (dict(t_start=-inf), "t_start"),
        (dict(t_end=nan), "t_end is NaN"), (dict(t_start=0.5, t_end=0.25), "t_end < t_start"),
        (dict(t_end=-inf), "t_end < t_start"),
        (dict(shape=4), "unknown shape"), (dict(surface=0, friction=0.5), "sticky"),  # and the static record's
        (dict(shape=1, b=(0.0, 0.0, 0.0)), "radius"),
    ]
    for kw, word in bad:
        rc, msg = _raw_add(sim, **kw)
        assert rc == _lib.GSMPM_EINVAL and word in msg, (kw, rc, msg)
    with pytest.raises(RuntimeError, match="no rotating collider"):
        sim.poses(1)
    assert sim.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0  # no id was taken
    assert _raw_add(sim, t_start=0.5, t_end=0.5)[0] == 1  # legal: an empty window
    assert _raw_add(sim, t_end=inf)[0] == 2
    # Python: a pivot needs an angular velocity; None or zeros route to the other entries
    with pytest.raises(TypeError, match="pivot"):
        sim.add_collider("ball", center=(1, 1, 1), radius=0.1, pivot=(1, 1, 1))
    assert sim.add_collider("ball", center=(1, 1, 1), radius=0.1, angular_velocity=(0, 0, 0)) == 3
    assert sim.add_collider("ball", center=(1, 1, 1), radius=0.1, angular_velocity=(0, 0, 0),
                            velocity=(1, 0, 0)) == 4
    assert sim.add_collider("ball", center=(1, 1, 1), radius=0.1, angular_velocity=(0, 0, 1)) == 5


def test_untimed_step_is_refused_and_the_timing_tools_run_at_zero(dev):
    from gsmpm import _lib
    from gsmpm.sim import Simulator
    S = _witness()[0]
    sim = Simulator(len(S["x"]), **S["kw"])
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    bit = sim.add_collider("box", "slip", 0.5, angular_velocity=R.OMEGA, pivot=R.PIVOT, **CR.GEOMETRY["box"])
    before = sim.get("x").cpu().numpy()
    masks = (ctypes.c_uint32 * 2)(1 << bit, 1 << bit)
    rc = _lib.LIB.gsmpm_mpm_step(sim._h, ctypes.c_float(S["dt"]), 2, masks, None)
    assert rc == _lib.GSMPM_ESTATE and "gsmpm_mpm_step_timed" in _lib.last_error()
    with pytest.raises(RuntimeError, match="moving colliders"):
        sim.step(S["dt"], [1 << bit] * 2)
    assert np.array_equal(sim.get("x").cpu().numpy(), before) and sim.graph_count() == 0  # nothing was launched
    sim.step(S["dt"], [1 << bit] * 2, [0.03, 0.03 + S["dt"]])
    assert sim.graph_count() == 1 and np.isfinite(sim.get("v").cpu().numpy()).all()
    assert not np.array_equal(sim.poses(2)[1, 0, :9].reshape(3, 3), np.eye(3, dtype=np.float32))
    # the timing tools run such a handle at t = 0 and leave the state alone
    x1 = sim.get("x").cpu().numpy()
    assert all(np.isfinite(ms) and ms >= 0 for ms in sim.time_kernels(S["dt"], 1 << bit, reps=2))
    assert np.array_equal(sim.get("x").cpu().numpy(), x1)
    assert np.array_equal(sim.poses(1)[0, 0, :9].reshape(3, 3), np.eye(3, dtype=np.float32))  # t = 0: R = I


def test_slab_and_fold_handles_refuse(dev):
    from gsmpm import _lib
    from gsmpm.sim import Simulator
    S = _witness()[0]
    slab = _bare()
    slab.slab_init(0, 1, 0, 32)
    rc, msg = _raw_add(slab)
    assert rc == _lib.GSMPM_ESTATE and "slab" in msg
    assert slab.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0  # no id was taken
    # the other order: slab_init on a handle that holds one; it stays an ordinary handle that steps
    sim = Simulator(len(S["x"]), **S["kw"])
    bit = sim.add_collider("box", "slip", 0.5, angular_velocity=R.OMEGA, **CR.GEOMETRY["box"])
    rc = _lib.LIB.gsmpm_mpm_slab_init(sim._h, 0, 1, 0, 32, 2, 10)
    assert rc == _lib.GSMPM_ESTATE and "extended colliders" in _lib.last_error()
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    sim.step(S["dt"], [1 << bit] * 2, [0.0, S["dt"]])
    assert sim.pipeline == "fused" and np.isfinite(sim.get("v").cpu().numpy()).all()
    # a handle created with GSMPM_FOLD=1
    old = os.environ.get("GSMPM_FOLD")
    os.environ["GSMPM_FOLD"] = "1"
    try:
        fold = _bare()
    finally:
        if old is None:
            os.environ.pop("GSMPM_FOLD")
        else:
            os.environ["GSMPM_FOLD"] = old
    assert fold.folded
    rc, msg = _raw_add(fold)
    assert rc == _lib.GSMPM_ESTATE and "GSMPM_FOLD" in msg
    assert fold.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0 and fold.folded


def test_fitting_refuses_rotating_records(dev):
    from gpu_helpers import dropin_sim
    from scenarios import lego_problem
    prob = lego_problem(500, 32)
    prob["cfg"] = dict(prob["cfg"], boundary_conditions=[])
    sim, args = dropin_sim(prob, dev, with_collider=False, fitting=True)
    rec = dict(type="collider", shape="box", angular_velocity=list(R.OMEGA), pivot=list(R.PIVOT),
               **CR.GEOMETRY["box"])
    with pytest.raises(TypeError, match="fitting"):
        sim.set_boundary_conditions([rec], args)
    with pytest.raises(TypeError, match="fitting"):
        sim.add_collider("box", angular_velocity=R.OMEGA, **CR.GEOMETRY["box"])
    assert sim.grid_postprocess == []
