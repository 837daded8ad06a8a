"""Moving colliders (gsmpm_mpm_add_moving_collider, gsmpm_mpm_step_timed; the
MOV instantiations of k_grid and k_grid_f) on the GPU: held to the float64
reference of tests/moving_ref.py at grid level, to static twins bit for bit
outside the motion window, to each other across the two pipelines, to exact
particle-level bounds for particles a sticky box carries, through the cached
graphs; plus what is refused.

Scene S (grid_ref.scene): 4,000 particles at 32^3, stress-free, dt 1e-4.
Velocity W, the motion window and the times T are moving_ref's; geometry is
collider_ref.GEOMETRY and, for the plane, the oblique plane of list b.  At
every shape x time pair no massive node is ambiguous and >= 500 nodes have
their relative velocity pointing into the collider; every grid-level case
asserts both from the reference side.

Bounds:
* v_out against the float64 reference fed the GPU's own mass and v_in, per
  node in units of ||v_in / m|| + ||dt g||, on the nodes the reference does
  not mark ambiguous: max(4 e32, 8 EPS), test_gpu_colliders.py's own, e32
  the f32 transcription's error on the same inputs, computed in the test.
  Massless nodes exactly 0; nodes outside every operator bit-equal to the
  update without operators.
* before the window and from its end on: bit for bit the v_out of a handle
  holding the static record at the initial / the f32 end centre, on the
  nodes where the two handles read bit-equal mass and v_in (_same_inputs
  says why not on all, and what keeps the comparison from being vacuous).
* fused against per-phase after 40 substeps: 1e-4 of each field's maximum.
* carried particles, K = 40 substeps inside a sticky box moving with W:
  |v - W| <= 32 EPS ||W||inf (a 27-term weighted sum of equal values) and
  |x_K - x_0 - K dt W| <= K (ulp32(1.5) / 2 + dt 32 EPS ||W||inf) (one
  rounding of x per substep plus the velocity error).
* two handles at particle level (step_timed against step on static records,
  the drop-in against direct calls): 1e-6 of the field's maximum on x and v
  (_two_handles says why not array_equal: two handles on the plain
  gsmpm_mpm_step are not bit-equal on scene S either).

Measured on an MI355X, in EPS = 2^-23: v_out against float64 at t = 0.0507
0.80 .. 0.83 (sticky), 7.48 .. 20.02 (slip: box, walls 7.75, ball 16.12,
plane), 7.86 .. 19.75 (separate: box, ball 8.18, walls 13.98, plane), 12.65
.. 16.31 on the mixed list in its two orders; at t = 0.0123 6.52 .. 23.51; the response runs on
u = v - wc with ||W|| = 4.2, so the figure is large in units of a small node
velocity, and the transcription's own error e32 is the same figure, the GPU
being bit-equal to the transcription in every case (bound 4 e32 = 26 .. 94).
Outside the window 0.89 .. 1.62 (bound 8), array_equal to the static twin on
2,259 .. 2,759 of the 5,883 massive nodes, 285 .. 1,550 of them inside the
collider.  Fused against per-phase: x 7.9e-8, v 5.2e-7, C 1.1e-6, F_trial
2.1e-7.  Carried: 365 particles, |v - W| 4.77e-7 (bound 1.18e-5), |x_K - x_0
- K dt W| 2.23e-6 (bound 2.43e-6) in both runs, which differ by x 7.9e-8,
v 7.7e-7, C 1.6e-6, F_trial 2.1e-7 and are not bit-equal.  Graphs: 1 and 1
after each of six calls.  step_timed against step: x 7.9e-8, v 3.1e-7 (two
handles on the plain call: 4.0e-8, 3.1e-7); drop-in: x 7.9e-8, v 4.5e-7;
neither bit-equal.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import collider_ref as CR
import grid_ref as G
import moving_ref as M
from conftest import rel_err
from test_gpu_grid_ops import _grid_sim, _read_grid, _t

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "C", "F_trial")
SURF = {"sticky": 0.0, "slip": 0.5, "separate": 0.5}
PLANE = G.OP_LISTS["b"][0][0]  # the oblique legacy plane, friction 0.5
SHAPES = ("plane", "ball", "box", "walls")
T_IN = M.T[2]


def _geo(name):
    return dict(point=PLANE[1], normal=PLANE[2]) if name == "plane" else CR.GEOMETRY[name]


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
        if op[0] == "mov":
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


def _hit_any(S, ops, t):
    """Nodes inside some operator of the list at time t (geometry, f32 positions)."""
    p = CR.node_positions32(S["n_grid"], S["dx32"])
    hit = np.zeros(len(p), bool)
    for op in ops:
        if op[0] == "cube":
            hit |= (np.abs(p - G.f32(op[1])) < G.f32(op[2])).all(1)
            continue
        if op[0] == "collider":
            op = CR.ext("plane", point=op[1], normal=op[2])
        hit |= M.hit_nodes(S["n_grid"], S["dx32"], op, t)
    return hit


def _check(S, grid, ops, active, t, tag):
    """v_out of one substep at time t against the float64 reference and the f32 transcription."""
    ng = S["n_grid"]
    mass, v_in, v_out = grid["mass"].reshape(-1), grid["v_in"], grid["v_out"]
    args = (v_in, mass, ng, S["dx32"], S["dt_g32"])
    ref, amb = M.node_update_ref(*args, ops, active, t)
    t32 = M.node_update_f32(*args, ops, active, t)
    free32 = M.node_update_f32(*args, [], [])
    live = mass > np.float32(1e-15)
    scale = np.zeros(ng ** 3)
    scale[live] = np.sqrt(((v_in[live].astype(np.float64) / mass[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum())
    ok = ~amb
    e32 = (np.abs(t32.astype(np.float64) - ref).max(1) / scale)[ok].max()
    e = (np.abs(v_out.astype(np.float64) - ref).max(1) / scale)[ok].max()
    bound = max(4 * e32, 8 * G.EPS)
    outside = ~_hit_any(S, ops, t) & ok
    changed = int((np.abs(ref - free32.astype(np.float64)).max(1) > 1e-3 * scale)[live].sum())
    print(f"MOVING {tag} t={t}: massive {int(live.sum())} ambiguous {int((amb & live).sum())} changed {changed} | "
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
    op = M.mov(CR.ext(name, "slip", **_geo(name)))
    _, acting = M.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], op, t)
    _, amb = M.node_update_ref(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], [op], [1], t)
    assert acting >= CR.MIN_ACTING and not (amb & (m > 1e-15)).any()
    if name != "plane":
        assert acting == M.ACTING[name][M.T.index(t)]


def _same_inputs(S, a, b, ops, t, tag):
    """The nodes on which two handles' grid updates read the same bits.  Two
    handles' P2G sums may differ in the last bit on some nodes (which chunk of
    a multi-chunk tile a particle lands in follows the binning's atomics,
    DESIGN.md "Summation order": scene S holds up to 511 particles a tile, two
    chunks); node_update is pointwise, so v_out is compared bit for bit on
    the nodes whose mass and v_in are bit-equal.  Against a vacuous pass those
    must include 100 massive nodes inside the operators (a misplaced centre
    turns every normal of a ball and moves whole layers of nodes in or out of
    a box, so a handful would show it; 100 is over 5 % of any shape's nodes)
    and 1,000 massive nodes in all.  Every node of both handles is also held
    to the float64 reference by _check."""
    same = (a["mass"].reshape(-1) == b["mass"].reshape(-1)) & (a["v_in"] == b["v_in"]).all(1)
    live = a["mass"].reshape(-1) > np.float32(1e-15)
    inside = _hit_any(S, ops, t) & live
    print(f"MOVING {tag}: inputs bit-equal on {int((same & live).sum())} of {int(live.sum())} massive nodes, "
          f"{int((same & inside).sum())} of the {int(inside.sum())} inside")
    assert (same & inside).sum() >= 100 and (same & live).sum() >= 1000
    return same


def _one_substep(dev, S, ops, active, t=None):
    """A fresh per-phase keep-grid handle, the list, one substep (timed when t is given)."""
    sim = _grid_sim(dev, S)
    assert sim.pipeline == "phased"
    mask = _add(sim, ops, active)
    sim.step(S["dt"], [mask], None if t is None else [t])
    return _read_grid(sim)


# ------------------------------------------------------ 1. grid level --
@pytest.mark.parametrize("surface", list(SURF))
@pytest.mark.parametrize("name", SHAPES)
def test_grid_level_shapes(dev, name, surface):
    """Each shape with each surface inside the window, damping 0.9 (ignored by sticky)."""
    S = _witness()[0]
    _assert_acting(name, T_IN)
    ops, active = [M.mov(CR.ext(name, surface, SURF[surface], 0.9, **_geo(name)))], [1]
    _check(S, _one_substep(dev, S, ops, active, T_IN), ops, active, T_IN, f"{name} {surface}")


# ------------------------------------------- 2. the window's three phases --
@pytest.mark.parametrize("name", SHAPES)
def test_three_phases_of_the_window(dev, name):
    """Before the window: the static record at the initial centre, bit for
    bit; from its end on: the static record at the f32 end centre, bit for
    bit; inside: the reference, within the bound."""
    S = _witness()[0]
    e = CR.ext(name, "slip", 0.5, 0.9, **_geo(name))
    op = M.mov(e)
    for t in M.T:
        _assert_acting(name, t)
        grid = _one_substep(dev, S, [op], [1], t)
        if M.WINDOW[0] <= t < M.WINDOW[1]:
            _check(S, grid, [op], [1], t, f"phases {name}")
            continue
        static = M.static_at(op, t)
        if t < M.WINDOW[0]:
            assert static[3] == tuple(float(a) for a in np.asarray(e[3], np.float32))
        else:
            assert static[3] != tuple(float(a) for a in np.asarray(e[3], np.float32))
        twin = _one_substep(dev, S, [static], [1])
        same = _same_inputs(S, grid, twin, [op], t, f"phases {name} t={t}")
        eq = bool(np.array_equal(grid["v_out"][same], twin["v_out"][same]))
        print(f"MOVING phases {name} t={t}: array_equal to the static twin: {eq}")
        assert eq
        _check(S, twin, [static], [1], t, f"phases {name}, static twin")
        _check(S, grid, [op], [1], t, f"phases {name}")


# -------------------------------------------------------- 3. mixed lists --
@pytest.mark.parametrize("order", ["cube_plane_ball_box", "box_ball_plane_cube"])
def test_grid_level_mixed_lists(dev, order):
    """A fixed cube, the legacy plane, a moving ball and a static extended box in one table, in two orders."""
    S, m, mv = _witness()
    _assert_acting("ball", T_IN)
    assert G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], [PLANE]) >= CR.MIN_ACTING
    ops = [G.CUBE, PLANE, M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])),
           CR.ext("box", "separate", 0.5, 0.9, **CR.GEOMETRY["box"])]
    if order == "box_ball_plane_cube":
        ops = ops[::-1]
    active = [1, 1, 1, 1]
    _check(S, _one_substep(dev, S, ops, active, T_IN), ops, active, T_IN, f"mixed {order}")


@pytest.mark.parametrize("surface", list(SURF))
def test_static_record_in_a_moving_table_equals_the_ext_kernels(dev, surface):
    """k_grid<EXT, MOV> on a static box (the table's moving ball switched off) == k_grid<EXT> on the same box."""
    S = _witness()[0]
    box = CR.ext("box", surface, SURF[surface], 0.9, **CR.GEOMETRY["box"])
    ball = M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]))
    got = _one_substep(dev, S, [ball, box], [0, 1], T_IN)
    want = _one_substep(dev, S, [box], [1])
    same = _same_inputs(S, got, want, [box], T_IN, f"static box {surface} in a moving table")
    assert np.array_equal(got["v_out"][same], want["v_out"][same])
    free32 = M.node_update_f32(want["v_in"], want["mass"], S["n_grid"], S["dx32"], S["dt_g32"], [], [])
    assert (np.abs(want["v_out"] - free32).max(1) > 1e-3).sum() >= CR.MIN_ACTING  # the box acted


# ------------------------------------------------- 4. fused vs per-phase --
NSUB = 40
T_START = 0.02  # inside the motion window for all of the 40 substeps


def _run(dev, S, ops, active, phased, calls=(NSUB,), t_start=T_START, timed=True, sync=False):
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
        sim.step(S["dt"], [mask] * n, times if timed else None)
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return {k: sim.get(k).cpu().numpy() for k in FIELDS}, sim


def test_fused_matches_per_phase(dev):
    """A moving slip ball, 40 substeps with one re-binning inside: k_grid_f's MOV form against k_grid's."""
    S = _witness()[0]
    ops, active = [M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]))], [1]
    fused, sf = _run(dev, S, ops, active, phased=False)
    phased, sp = _run(dev, S, ops, active, phased=True)
    assert sf.pipeline == "fused" and sp.pipeline == "phased"
    errs = {k: rel_err(fused[k], phased[k]) for k in FIELDS}
    print("MOVING fused vs per-phase, ball slip: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(np.isfinite(fused[k]).all() for k in FIELDS)
    for k, e in errs.items():
        assert e < 1e-4, (k, e, errs)
    # the motion mattered: the same ball at rest where it started ends elsewhere
    rest, _ = _run(dev, S, [ops[0][1]], active, phased=False, timed=False)
    assert rel_err(rest["v"], fused["v"]) > 1e-2


# ------------------------------------------------- 5. carried particles --
def test_sticky_box_carries_the_particles_inside(dev):
    """Particles whose stencils stay inside a sticky box moving with W move with W, through the graph,
    in one call of 40 and in calls of 7 + 13 + 20 queued without a sync."""
    S = _witness()[0]
    K, dt32 = NSUB, float(np.float32(S["dt"]))
    geo = CR.GEOMETRY["box"]
    c, half = np.asarray(geo["center"], np.float64), np.asarray(geo["half"], np.float64)
    dx = float(S["dx32"])
    sel = (np.abs(S["x"].astype(np.float64) - c) < half - 2.5 * dx).all(1)
    assert sel.sum() >= 300
    w = G.f32(M.W)
    wmax = np.abs(w).max()
    assert K * dt32 * wmax < 0.25 * dx  # the box travels a fifth of a cell: the stencils stay inside it
    ops, active = [M.mov(CR.ext("box", "sticky", **geo), M.W, T_START, float("inf"))], [1]
    bv = 32 * G.EPS * wmax
    bx = K * (2.0 ** -23 / 2 + dt32 * bv)
    runs = {}
    for tag, calls in (("one call of 40", (40,)), ("calls of 7 + 13 + 20", (7, 13, 20))):
        got, sim = _run(dev, S, ops, active, phased=False, calls=calls)
        if len(calls) == 1:
            assert sim.graph_count() == 1  # it went through a graph
        v = got["v"].reshape(-1, 3).astype(np.float64)
        x = got["x"].reshape(-1, 3).astype(np.float64)
        ev = np.abs(v[sel] - w).max()
        ex = np.abs(x[sel] - S["x"][sel].astype(np.float64) - K * dt32 * w).max()
        print(f"MOVING carried, {tag}: {int(sel.sum())} particles; |v - W| {ev:.2e} (bound {bv:.2e}), "
              f"|x_K - x_0 - K dt W| {ex:.2e} (bound {bx:.2e})")
        assert x[sel].max() < 1.5
        assert ev <= bv and ex <= bx
        assert np.abs(v[~sel] - w).max() > 1e-2  # and not everybody is carried
        runs[tag] = got
    a, b = runs.values()
    errs = {k: rel_err(a[k], b[k]) for k in FIELDS}
    print("MOVING carried, one call against three: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items())
          + f"; bit-equal: {all(np.array_equal(a[k], b[k]) for k in FIELDS)}")
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


# ---------------------------------------- 6. graphs do not depend on time --
def test_graph_count_does_not_depend_on_time(dev):
    """Six timed calls of 20 substeps at advancing times: as many cached graphs as the same ball at rest."""
    from gsmpm.bc import substep_times
    from gsmpm.sim import Simulator
    S = _witness()[0]
    e = CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])
    sims = []
    for op in (M.mov(e), e):
        sim = Simulator(len(S["x"]), **S["kw"])
        sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
        sims.append((sim, _add(sim, [op], [1])))
    assert [s.graph_count() for s, _ in sims] == [0, 0]
    t, counts = 0.0, []
    for _ in range(6):
        times, t = substep_times(t, S["dt"], 20)
        for sim, mask in sims:
            sim.step(S["dt"], [mask] * 20, times)
        counts.append([s.graph_count() for s, _ in sims])
        assert counts[-1][0] == counts[-1][1] >= 1, counts
    print(f"MOVING graphs after each of six calls (moving, at rest): {counts}")
    assert t > M.WINDOW[0]  # the calls crossed into the motion window
    va, vb = (s.get("v").cpu().numpy() for s, _ in sims)
    assert rel_err(va, vb) > 1e-3  # and the motion mattered


# Two handles given the same particles are not bit-equal on scene S, whatever
# steps them: which chunk of a multi-chunk tile a particle lands in follows
# the binning's atomics (DESIGN.md "Summation order"; scene S has tiles of
# 511 particles, two chunks).  Measured with gsmpm_mpm_step on both handles:
# v differs by 4.8e-7 after one substep, 7.2e-7 after 30.  So the comparisons
# of two handles below hold x and v to the bound the project already uses for
# exactly that, 1e-6 of the field's maximum (test_gpu_colliders.py's drop-in
# case), print whether they are bit-equal, and print the same figure for two
# handles that both take the plain call.
def _two_handles(tag, a, b, control=None):
    errs = {k: rel_err(a[k], b[k]) for k in ("x", "v")}
    line = f"MOVING {tag}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()) \
        + f"; bit-equal: {all(np.array_equal(a[k], b[k]) for k in ('x', 'v'))}"
    if control:
        ce = {k: rel_err(control[0][k], control[1][k]) for k in ("x", "v")}
        line += "; two handles on the plain call: " + " ".join(f"{k} {e:.1e}" for k, e in ce.items())
    print(line)
    for k, e in errs.items():
        assert e < 1e-6, (k, e)


# ------------------------------- 7. the same path without moving records --
def test_step_timed_without_moving_records_is_step(dev):
    S = _witness()[0]
    ops, active = [G.CUBE, CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])], [1, 1]
    a, sa = _run(dev, S, ops, active, phased=False, calls=(20,), timed=True)
    b, sb = _run(dev, S, ops, active, phased=False, calls=(20,), timed=False)
    c, _ = _run(dev, S, ops, active, phased=False, calls=(20,), timed=False)
    assert sa.graph_count() == sb.graph_count() == 1
    assert sa.rebin_state()["rebins_last_call"] == sb.rebin_state()["rebins_last_call"]
    _two_handles("step_timed against step, 20 substeps", a, b, control=(b, c))


# ------------------------------------------------------------ 8. drop-in --
def test_dropin_config_record_equals_direct_steps(dev):
    """MPM_Simulator with a moving config record, 30 p2g2p calls, against
    Simulator.step given substep_masks and substep_times directly."""
    import torch
    from gpu_helpers import sim_args_from_cfg
    from gsmpm.bc import substep_masks, substep_times, windowed_collider
    from gsmpm.sim import Simulator
    from mpm_solver.solver import MPM_Simulator
    from scenarios import lego_problem
    S = _witness()[0]
    dt = S["dt"]
    cfg = dict(lego_problem(4000, 32)["cfg"])
    rec = dict(type="collider", id=7, shape="ball", surface="slip", friction=0.5, damping=0.9,
               start_time=3.5 * dt, end_time=999.0, velocity=list(M.W), move_start=10.5 * dt, move_end=25.5 * dt,
               **CR.GEOMETRY["ball"])
    cfg["boundary_conditions"] = [rec]
    args = sim_args_from_cfg(cfg, 32)
    sim = MPM_Simulator(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), args, init_v=_t(dev, S["v"]))
    sim.set_boundary_conditions(args.boundary_conditions, args)
    bc = sim.grid_postprocess[0]
    assert bc.bit == 0 and bc.motion == dict(velocity=[float(a) for a in M.W], move_start=10.5 * dt,
                                             move_end=25.5 * dt)
    for _ in range(30):
        sim.p2g2p(dt)
    masks, _ = substep_masks([windowed_collider(0, 3.5 * dt, 999.0)], 0.0, dt, 30)
    times, t_end = substep_times(0.0, dt, 30)
    assert sim._queue == masks and sim._queue_t == times and sim.time == t_end and masks.count(1) == 26
    sim.flush()
    raw = Simulator(len(S["x"]), **S["kw"])
    raw.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    op = M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]), M.W, 10.5 * dt, 25.5 * dt)
    assert _add(raw, [op], [1]) == 1
    raw.step(dt, masks, times)
    rest = Simulator(len(S["x"]), **S["kw"])
    rest.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    _add(rest, [op[1]], [1])
    rest.step(dt, masks)
    torch.cuda.synchronize()
    _two_handles("drop-in against direct steps, 30 substeps",
                 {k: sim._sim.get(k).cpu().numpy() for k in ("x", "v")},
                 {k: raw.get(k).cpu().numpy() for k in ("x", "v")})
    assert sim._sim.graph_count() == raw.graph_count() == 1
    assert rel_err(rest.get("v").cpu().numpy(), raw.get("v").cpu().numpy()) > 1e-3  # the motion mattered
    # add_collider takes the same keys; move_start / move_end default to the activity window
    d = sim.add_collider("box", "sticky", start_time=0.25, end_time=0.5, velocity=(0.0, 0.0, -0.4),
                         **CR.GEOMETRY["box"])
    assert d.bit == 1 and d.motion == dict(velocity=[0.0, 0.0, -0.4], move_start=0.25, move_end=0.5)


# ------------------------------------------------ 9. refusals and errors --
def _raw_add(sim, velocity=(1.0, 0.0, 0.0), t_start=0.0, t_end=1.0, **kw):
    from gsmpm import _lib
    c = _lib.Collider()
    c.shape, c.surface = kw.get("shape", 1), kw.get("surface", 2)
    c.a[:] = kw.get("a", (1.0, 1.0, 1.0))
    c.b[:] = kw.get("b", (0.3, 0.3, 0.3))
    c.friction, c.damping = kw.get("friction", 0.0), kw.get("damping", 1.0)
    m = _lib.ColliderMotion()
    m.velocity[:] = velocity
    m.t_start, m.t_end = t_start, t_end
    rc = _lib.LIB.gsmpm_mpm_add_moving_collider(sim._h, ctypes.byref(c), ctypes.byref(m))
    return rc, _lib.last_error()


def _bare(**kw):
    from gsmpm.sim import Simulator
    return Simulator(100, n_grid=32, **kw)


def test_invalid_arguments_are_refused(dev):
    from gsmpm import _lib
    sim = _bare()
    inf, nan = float("inf"), float("nan")
    bad = [
        (dict(velocity=(nan, 0.0, 0.0)), "non-finite velocity"), (dict(velocity=(0.0, inf, 0.0)), "non-finite velocity"),
        (dict(velocity=(0.0, 0.0, -inf)), "non-finite velocity"),
        (dict(t_start=nan), "t_start"), (dict(t_start=inf, t_end=inf), "t_start"), (dict(t_start=-inf), "t_start"),
        (dict(t_end=nan), "t_end is NaN"), (dict(t_start=0.5, t_end=0.25), "t_end < t_start"),
        (dict(t_end=-inf), "t_end < t_start"),
        (dict(shape=4), "unknown shape"), (dict(surface=0, friction=0.5), "sticky"),  # and the static record's
        (dict(shape=1, b=(0.0, 0.0, 0.0)), "radius"),
    ]
    for kw, word in bad:
        rc, msg = _raw_add(sim, **kw)
        assert rc == _lib.GSMPM_EINVAL and word in msg, (kw, rc, msg)
    assert sim.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0  # no id was taken
    assert _raw_add(sim, velocity=(0.0, 0.0, 0.0), t_start=0.5, t_end=0.5)[0] == 1  # legal: zero velocity, empty window
    assert _raw_add(sim, t_end=inf)[0] == 2
    with pytest.raises(TypeError):
        sim.add_collider("ball", center=(1, 1, 1), radius=0.1, move_start=0.1)


def test_timed_and_untimed_steps_refuse_what_they_must(dev):
    from gsmpm import _lib
    S = _witness()[0]
    from gsmpm.sim import Simulator
    sim = Simulator(len(S["x"]), **S["kw"])
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    bit = sim.add_collider("ball", "slip", 0.5, velocity=M.W, **CR.GEOMETRY["ball"])
    before = sim.get("x").cpu().numpy()
    masks = (ctypes.c_uint32 * 2)(1 << bit, 1 << bit)
    rc = _lib.LIB.gsmpm_mpm_step(sim._h, ctypes.c_float(S["dt"]), 2, masks, None)
    assert rc == _lib.GSMPM_ESTATE and "gsmpm_mpm_step_timed" in _lib.last_error()
    with pytest.raises(RuntimeError, match="moving colliders"):
        sim.step(S["dt"], [1 << bit] * 2)
    rc = _lib.LIB.gsmpm_mpm_step_timed(sim._h, ctypes.c_float(S["dt"]), 2, masks, None, None)
    assert rc == _lib.GSMPM_EINVAL and "null time" in _lib.last_error()
    for badt in (float("nan"), float("inf")):
        times = (ctypes.c_double * 2)(0.0, badt)
        rc = _lib.LIB.gsmpm_mpm_step_timed(sim._h, ctypes.c_float(S["dt"]), 2, masks, times, None)
        assert rc == _lib.GSMPM_EINVAL and "non-finite time" in _lib.last_error()
    with pytest.raises(ValueError):
        sim.step(S["dt"], [1 << bit] * 2, [0.0])
    assert np.array_equal(sim.get("x").cpu().numpy(), before) and sim.graph_count() == 0  # nothing was launched
    sim.step(S["dt"], [1 << bit] * 2, [0.0, S["dt"]])
    assert sim.graph_count() == 1 and np.isfinite(sim.get("v").cpu().numpy()).all()
    # the timing tools run such a handle (at t = 0) and leave the state alone
    x1 = sim.get("x").cpu().numpy()
    assert all(np.isfinite(ms) and ms >= 0 for ms in sim.time_kernels(S["dt"], 1 << bit, reps=2))
    assert np.array_equal(sim.get("x").cpu().numpy(), x1)


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
    bit = sim.add_collider("ball", "slip", 0.5, velocity=M.W, **CR.GEOMETRY["ball"])
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


def test_fitting_refuses_moving_records(dev):
    from gpu_helpers import dropin_sim
    from scenarios import lego_problem
    prob = lego_problem(500, 32)
    prob["cfg"] = dict(prob["cfg"], boundary_conditions=[])
    sim, args = dropin_sim(prob, dev, with_collider=False, fitting=True)
    rec = dict(type="collider", shape="ball", velocity=list(M.W), **CR.GEOMETRY["ball"])
    with pytest.raises(TypeError, match="fitting"):
        sim.set_boundary_conditions([rec], args)
    with pytest.raises(TypeError, match="fitting"):
        sim.add_collider("ball", velocity=M.W, **CR.GEOMETRY["ball"])
    assert sim.grid_postprocess == []
