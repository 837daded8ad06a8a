"""Extended colliders (gsmpm_mpm_add_collider: ball, box, walls and plane with
sticky / slip / separate surfaces, damping and an activity bit; the EXT
instantiations of k_grid and k_grid_f) on the GPU, held to the float64
reference of tests/collider_ref.py at grid level, to the oracle bit for bit
where the record is the legacy plane, to each other across the two
pipelines, and to exact particle-level invariants; plus what is refused.

Scene S (grid_ref.scene): 4,000 particles at 32^3, stress-free, dt 1e-4.
The geometry lists (collider_ref.GEOMETRY) lie off its lattice: 1,162 /
1,560 / 2,523 massive nodes in the ball / the box / beyond the walls, 572 /
774 / 1,349 of them moving into it, none ambiguous; every grid-level case
asserts both from the reference side.

Bounds:
* v_out against the float64 reference fed the GPU's own mass and v_in, per
  node in units of ||v_in / m|| + ||dt g||, on the nodes the reference does
  not mark ambiguous: max(4 e32, 8 EPS), e32 the f32 transcription's own
  error against float64 on the same inputs, computed in the test (the
  project's rule for the P2G sums; the 4 covers another, equally valid
  rounding of the sqrtf and division chains).  Massless nodes exactly 0;
  nodes outside every operator bit-equal to the update without operators.
* the legacy plane entered as an extended record (separate, damping
  f32(0.99)): equal to the oracle's om_grid_normalize + om_grid_ops bit for
  bit on all nodes, as the legacy path is.
* fused against per-phase after 20 substeps: test_gpu_mpm.py's stress-free
  bound, 1e-4 of each field's maximum.

Measured on an MI355X, in EPS = 2^-23 (two runs; the figures move a little
with the P2G sums' binning order): v_out against float64 0.63 .. 1.48 on the
nine shape x surface lists (sticky 0.63 .. 0.80, slip 0.89 .. 1.48, separate
0.98 .. 1.23) and 1.07 .. 1.63 on the six mixed lists; the f32 transcription's
own error e32 is the same figure on every list, because v_out is bit-equal to
the transcription on all of them, so the bound is its floor, 8 EPS.  The
legacy identity measures 0 on lists a, b, c.  Activity: 0.80 with the bit
clear (bit-equal to the update without operators), 1.24 with it set.  Fused
against per-phase after 20 substeps: x 7.9e-8, v 2.7e-7 .. 4.3e-7, C 4.3e-7 ..
5.5e-7, F_trial 1.1e-7 .. 2.3e-7.  Invariants: 612 particles with the whole
stencil in the ball, 639 / 694 beyond the +z / -z wall.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import collider_ref as CR
import grid_ref as G
from conftest import PKG, rel_err
from test_gpu_grid_ops import _grid_sim, _oracle_grid_update, _read_grid, _t

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "C", "F_trial")
SURF = {"sticky": 0.0, "slip": 0.5, "separate": 0.5}
PLANE = G.OP_LISTS["b"][0][0]  # the oblique legacy plane, friction 0.5


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
        if op[0] == "ext":
            b = sim.add_collider(**CR.geometry_kw(op))
        elif op[0] == "cube":
            b = sim.add_fixed_cube(list(op[1]), list(op[2]))
        else:
            b = sim.add_plane_collider(list(op[1]), list(op[2]), op[3])
        if act:
            mask |= 1 << b
    return mask


def _hit_any(S, ops):
    """Nodes inside some operator of the list (geometry, f32 positions)."""
    p = CR.node_positions32(S["n_grid"], S["dx32"])
    hit = np.zeros(len(p), bool)
    for op in ops:
        if op[0] == "cube":
            hit |= (np.abs(p - G.f32(op[1])) < G.f32(op[2])).all(1)
            continue
        if op[0] == "collider":
            op = CR.ext("plane", point=op[1], normal=op[2])
        for h, _ in CR._inside_and_normals(p, op)[0]:
            hit |= h
    return hit


def _check(S, grid, ops, active, tag):
    """v_out of one substep against the float64 reference and the f32 transcription."""
    ng = S["n_grid"]
    mass, v_in, v_out = grid["mass"].reshape(-1), grid["v_in"], grid["v_out"]
    args = (v_in, mass, ng, S["dx32"], S["dt_g32"])
    ref, amb = CR.node_update_ref(*args, ops, active)
    t32 = CR.node_update_f32(*args, ops, active)
    free32 = CR.node_update_f32(*args, [], [])
    live = mass > np.float32(1e-15)
    scale = np.zeros(ng ** 3)
    scale[live] = np.sqrt(((v_in[live].astype(np.float64) / mass[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum())
    ok = ~amb
    e32 = (np.abs(t32.astype(np.float64) - ref).max(1) / scale)[ok].max()
    e = (np.abs(v_out.astype(np.float64) - ref).max(1) / scale)[ok].max()
    bound = max(4 * e32, 8 * G.EPS)
    outside = ~_hit_any(S, ops) & ok
    changed = int((np.abs(ref - free32.astype(np.float64)).max(1) > 1e-3 * scale)[live].sum())
    print(f"COLLIDER {tag}: massive {int(live.sum())} ambiguous {int((amb & live).sum())} changed {changed} | "
          f"v_out vs f64 {e / G.EPS:.2f} EPS (transcription {e32 / G.EPS:.2f}, bound {bound / G.EPS:.2f}); "
          f"bit-equal to the transcription: {bool(np.array_equal(v_out, t32))}")
    assert not (amb & live).any()
    assert np.all(v_out[~live] == 0)
    assert (outside & live).sum() >= 500 and np.array_equal(v_out[outside], free32[outside])
    assert e <= bound, (e / G.EPS, bound / G.EPS)
    return e, e32


def _assert_acting(name):
    S, m, mv = _witness()
    op = CR.ext(name, "slip", **CR.GEOMETRY[name])
    inside, acting, _ = CR.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], op)
    _, amb = CR.node_update_ref(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], [op], [1])
    assert (inside, acting) == CR.COUNTS[name] and acting >= CR.MIN_ACTING
    assert not (amb & (m > 1e-15)).any()


# ------------------------------------------------------ a. grid level --
@pytest.mark.parametrize("surface", list(SURF))
@pytest.mark.parametrize("name", list(CR.GEOMETRY))
def test_grid_level_shapes(dev, name, surface):
    """Each shape with each surface, damping 0.9 (ignored by sticky), per-phase pipeline."""
    S = _witness()[0]
    _assert_acting(name)
    ops, active = [CR.ext(name, surface, SURF[surface], 0.9, **CR.GEOMETRY[name])], [1]
    sim = _grid_sim(dev, S)
    assert sim.pipeline == "phased"
    mask = _add(sim, ops, active)
    sim.step(S["dt"], [mask])
    _check(S, _read_grid(sim), ops, active, f"{name} {surface}")


@pytest.mark.parametrize("order", ["cube_plane_ball", "ball_plane_cube"])
@pytest.mark.parametrize("surface", list(SURF))
def test_grid_level_mixed_lists(dev, surface, order):
    """A fixed cube, a legacy plane and a ball in one table, in two orders:
    the plain and the extended kinds apply in table order."""
    S, m, mv = _witness()
    _assert_acting("ball")
    assert G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], [PLANE]) >= CR.MIN_ACTING
    ops = [G.CUBE, PLANE, CR.ext("ball", surface, SURF[surface], **CR.GEOMETRY["ball"])]
    if order == "ball_plane_cube":
        ops = ops[::-1]
    active = [1, 1, 1]
    sim = _grid_sim(dev, S)
    mask = _add(sim, ops, active)
    sim.step(S["dt"], [mask])
    grid = _read_grid(sim)
    _check(S, grid, ops, active, f"mixed {order} ball {surface}")
    if surface != "sticky":
        # the order matters, from the reference side: the reversed list is another answer on the nodes
        # in the ball and below the plane that move into both (161 with slip, 89 with separate)
        a = CR.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops, active)[0]
        b = CR.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops[::-1], active)[0]
        assert (np.abs(a - b).max(1) > 1e-3).sum() >= 50


# -------------------------------------------------- b. legacy identity --
@pytest.mark.parametrize("name", list("abc"))
def test_plane_separate_099_is_the_legacy_collider(dev, name):
    """The legacy plane entered through gsmpm_mpm_add_collider runs the same
    operations in the same order: bit-equal to the oracle on all nodes."""
    S, m, mv = _witness()
    ops, active = G.OP_LISTS[name]
    assert G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops) >= CR.MIN_ACTING
    eops = [CR.ext("plane", "separate", o[3], float(np.float32(0.99)), point=o[1], normal=o[2]) for o in ops]
    sim = _grid_sim(dev, S)
    mask = _add(sim, eops, active)
    sim.step(S["dt"], [mask])
    grid = _read_grid(sim)
    orc = _oracle_grid_update(S, grid["mass"], grid["v_in"], ops, active)
    diff = np.abs(grid["v_out"].astype(np.float64) - orc).max()
    print(f"COLLIDER legacy identity list {name}: max |v_out - oracle| {diff:.1e}")
    assert np.array_equal(grid["v_out"], orc)
    # and it is an extended record: it honours its bit, which the legacy plane does not
    sim.step(S["dt"], [0])
    grid = _read_grid(sim)
    free32 = CR.node_update_f32(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], [], [])
    assert np.array_equal(grid["v_out"], free32)


# --------------------------------------------------------- c. activity --
def test_activity_bit_switches_the_record(dev):
    """One handle, one ball: a substep with its bit clear is the update without
    it, the next one, with the bit set, the update with it."""
    S = _witness()[0]
    _assert_acting("ball")
    op = CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])
    sim = _grid_sim(dev, S)
    sim.add_fixed_cube(list(G.CUBE[1]), list(G.CUBE[2]))  # bit 0: the ball's bit is not its table index
    bit = sim.add_collider(**CR.geometry_kw(op))
    assert bit == 1
    ops = [G.CUBE, op]
    sim.step(S["dt"], [0])
    grid = _read_grid(sim)
    free32 = CR.node_update_f32(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], [], [])
    assert np.array_equal(grid["v_out"], free32)
    _check(S, grid, ops, [0, 0], "activity: bit clear")
    sim.step(S["dt"], [1 << bit])
    grid = _read_grid(sim)
    _check(S, grid, ops, [0, 1], "activity: bit set")
    off = CR.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops, [0, 0])[0]
    assert (np.abs(grid["v_out"] - off).max(1) > 1e-3).sum() >= 500  # the record acted


# ---------------------------------------------------- d. both pipelines --
NSUB, CALLS = 10, 2
PARTICLE_CASES = {"ball": ("separate", 0.5, 0.99), "box": ("slip", 0.5, 0.9), "walls": ("slip", 0.5, 1.0)}


def _run(dev, S, ops, active, phased, calls=CALLS, nsub=NSUB):
    import torch
    from gsmpm.sim import Simulator
    sim = Simulator(len(S["x"]), phased=phased, **S["kw"])
    assert sim.pipeline == ("phased" if phased else "fused") and not sim.folded
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    mask = _add(sim, ops, active)
    for _ in range(calls):
        sim.step(S["dt"], [mask] * nsub)
    torch.cuda.synchronize()
    return {k: sim.get(k).cpu().numpy() for k in FIELDS}, sim


@pytest.mark.parametrize("name", list(CR.GEOMETRY))
def test_fused_matches_per_phase(dev, name):
    """20 substeps in two step calls, k_grid_f's EXT instantiation against k_grid's."""
    S = _witness()[0]
    _assert_acting(name)
    surface, mu, damp = PARTICLE_CASES[name]
    ops, active = [G.CUBE, CR.ext(name, surface, mu, damp, **CR.GEOMETRY[name])], [1, 1]
    fused, sf = _run(dev, S, ops, active, phased=False)
    phased, sp = _run(dev, S, ops, active, phased=True)
    assert sf.pipeline == "fused" and sp.pipeline == "phased"
    errs = {k: rel_err(fused[k], phased[k]) for k in FIELDS}
    print(f"COLLIDER fused vs per-phase, {name} {surface}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(np.isfinite(fused[k]).all() for k in FIELDS)
    for k, e in errs.items():
        assert e < 1e-4, (k, e, errs)
    # the collider mattered: the same run without it ends elsewhere
    plain, _ = _run(dev, S, ops[:1], active[:1], phased=False)
    assert rel_err(plain["v"], fused["v"]) > 1e-2


# ------------------------------------------------ e. exact invariants --
def _stencil_positions(S):
    """[n, 27, 3] f32 positions of every particle's stencil nodes (the f32 base cell)."""
    F32 = np.float32
    base = ((S["x"] * F32(S["inv_dx32"])).astype(F32) - F32(0.5)).astype(F32).astype(np.int64)
    offs = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return ((base[:, None, :] + offs[None]).astype(F32) * F32(S["dx32"])).astype(F32)


# the walls of the invariants: the z pair moved in (0.43 -> 0.23) so that whole stencils lie beyond it
WALLS_IN = dict(center=(1.013, 0.987, 1.013), half=(0.51, 0.47, 0.23))


@pytest.mark.parametrize("phased", [False, True], ids=["fused", "phased"])
def test_sticky_ball_stops_the_particles_inside(dev, phased):
    S = _witness()[0]
    geo = CR.GEOMETRY["ball"]
    d = _stencil_positions(S) - np.asarray(geo["center"], np.float32)
    L = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    assert np.abs(L.astype(np.float64) - float(np.float32(geo["radius"]))).min() > G.AMBIG
    inside = (L < np.float32(geo["radius"])).all(1)
    assert inside.sum() >= 20 and (~inside).sum() >= 20
    got, _ = _run(dev, S, [CR.ext("ball", "sticky", **geo)], [1], phased, calls=1, nsub=1)
    v = got["v"].reshape(-1, 3)
    print(f"COLLIDER sticky ball: {int(inside.sum())} particles with the whole stencil inside")
    assert np.all(v[inside] == 0)
    assert (np.abs(v[~inside]).max(1) > 0).sum() >= 20


@pytest.mark.parametrize("phased", [False, True], ids=["fused", "phased"])
def test_slip_walls_leave_no_outward_velocity(dev, phased):
    S = _witness()[0]
    c, h = np.asarray(WALLS_IN["center"], np.float32), np.asarray(WALLS_IN["half"], np.float32)
    d = _stencil_positions(S) - c
    assert np.abs(np.abs(d.astype(np.float64)) - h.astype(np.float64)).min() > G.AMBIG
    above, below = (d[..., 2] > h[2]).all(1), (d[..., 2] < -h[2]).all(1)
    assert above.sum() >= 20 and below.sum() >= 20
    assert (S["v"][above, 2] > 0).sum() >= 10 and (S["v"][below, 2] < 0).sum() >= 10  # some were leaving
    got, _ = _run(dev, S, [CR.ext("walls", "slip", 0.5, 0.9, **WALLS_IN)], [1], phased, calls=1, nsub=1)
    v = got["v"].reshape(-1, 3)
    print(f"COLLIDER slip walls: {int(above.sum())} particles beyond +z, {int(below.sum())} beyond -z")
    assert np.all(v[above, 2] <= 0) and np.all(v[below, 2] >= 0)


# ------------------------------------------------- f. drop-in and main.py --
def test_dropin_window_and_config_records(dev):
    """MPM_Simulator: a collider record of set_boundary_conditions and one of
    add_collider, the second with a window that opens after 4 substeps; the
    queued masks are the float64 clock's, and the run equals the Simulator's
    with those masks."""
    import torch
    from gpu_helpers import sim_args_from_cfg
    from mpm_solver.solver import MPM_Simulator
    from scenarios import lego_problem
    S = _witness()[0]
    cfg = dict(lego_problem(4000, 32)["cfg"])
    box = dict(type="collider", id=7, shape="box", surface="slip", friction=0.5, **CR.GEOMETRY["box"])
    cfg["boundary_conditions"] = [box]
    args = sim_args_from_cfg(cfg, 32)
    sim = MPM_Simulator(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), args, init_v=_t(dev, S["v"]))
    sim.set_boundary_conditions(args.boundary_conditions, args)
    dt = S["dt"]
    ball = sim.add_collider("ball", "separate", 0.5, 0.99, start_time=3.5 * dt, end_time=8.5 * dt,
                            **CR.GEOMETRY["ball"])
    assert [bc.bit for bc in sim.grid_postprocess] == [0, 1] and ball.bit == 1
    for _ in range(10):
        sim.p2g2p(dt)
    t, want = 0.0, []
    for _ in range(10):
        want.append(1 | (2 if 3.5 * dt <= t < 8.5 * dt else 0))
        t += dt
    assert sim._queue == want and want.count(3) == 5
    sim.flush()
    from gsmpm.sim import Simulator
    raw = Simulator(len(S["x"]), **S["kw"])
    raw.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    _add(raw, [CR.ext("box", "slip", 0.5, **CR.GEOMETRY["box"]),
               CR.ext("ball", "separate", 0.5, 0.99, **CR.GEOMETRY["ball"])], [1, 1])
    raw.step(dt, want)
    always = Simulator(len(S["x"]), **S["kw"])
    always.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    _add(always, [CR.ext("box", "slip", 0.5, **CR.GEOMETRY["box"]),
                  CR.ext("ball", "separate", 0.5, 0.99, **CR.GEOMETRY["ball"])], [1, 1])
    always.step(dt, [3] * 10)
    torch.cuda.synchronize()
    for k in ("x", "v"):
        assert rel_err(sim._sim.get(k).cpu().numpy(), raw.get(k).cpu().numpy()) < 1e-6, k
    assert rel_err(always.get("v").cpu().numpy(), raw.get("v").cpu().numpy()) > 1e-3  # the window mattered
    with pytest.raises(KeyError):  # the reference's answer to an unknown type stands
        sim.set_boundary_conditions([dict(type="torus")], args)


def test_lego_ball_config_runs_through_main(dev, tmp_path):
    import main as drv
    from PIL import Image
    out = str(tmp_path / "lego-ball")
    drv.main(["--config_path", os.path.join(PKG, "configs", "lego-ball.json"), "--synthetic", "3000", "--n_grid", "32",
              "--num_frames", "1", "--output_path", out])
    frames = [np.asarray(Image.open(os.path.join(out, "images", f"{f:04d}.png"))) for f in range(2)]
    assert frames[0].shape == frames[1].shape and frames[1].dtype == np.uint8
    assert (frames[0] != frames[1]).any() and frames[1].min() < 255  # it moved, and something is drawn


# ------------------------------------------------ g. refusals and errors --
def _raw_add(sim, **kw):
    from gsmpm import _lib
    c = _lib.Collider()
    c.shape, c.surface = kw.get("shape", 1), kw.get("surface", 2)
    c.a[:] = kw.get("a", (1.0, 1.0, 1.0))
    c.b[:] = kw.get("b", (0.3, 0.3, 0.3))
    c.friction, c.damping = kw.get("friction", 0.0), kw.get("damping", 1.0)
    rc = _lib.LIB.gsmpm_mpm_add_collider(sim._h, ctypes.byref(c))
    return rc, _lib.last_error()


def _bare(**kw):
    from gsmpm.sim import Simulator
    return Simulator(100, n_grid=32, **kw)


def test_invalid_arguments_are_refused(dev):
    from gsmpm import _lib
    sim = _bare()
    bad = [
        (dict(shape=4), "unknown shape"), (dict(shape=-1), "unknown shape"),
        (dict(surface=3), "unknown surface"), (dict(surface=-1), "unknown surface"),
        (dict(shape=1, b=(0.0, 0.0, 0.0)), "radius"), (dict(shape=1, b=(-0.1, 1.0, 1.0)), "radius"),
        (dict(shape=2, b=(0.3, 0.0, 0.3)), "half"), (dict(shape=3, b=(0.3, 0.3, -0.3)), "half"),
        (dict(shape=0, b=(0.0, 0.0, 0.0)), "zero normal"),
        (dict(friction=-0.1), "negative friction"),
        (dict(surface=0, friction=0.5), "sticky"),
    ]
    for kw, word in bad:
        rc, msg = _raw_add(sim, **kw)
        assert rc == _lib.GSMPM_EINVAL and word in msg, (kw, rc, msg)
    assert _raw_add(sim, surface=0, friction=0.0, damping=0.5)[0] == 0  # nothing was added before; sticky ignores damping
    with pytest.raises(ValueError):
        sim.add_collider("torus", center=(1, 1, 1), radius=0.1)
    with pytest.raises(ValueError):
        sim.add_collider("ball", "bouncy", center=(1, 1, 1), radius=0.1)
    with pytest.raises(TypeError):
        sim.add_collider("ball", center=(1, 1, 1), half=(0.1, 0.1, 0.1))
    assert sim.add_collider("ball", center=(1, 1, 1), radius=0.1) == 1


def test_the_33rd_id_is_refused(dev):
    from gsmpm import _lib
    sim = _bare()
    for b in range(32):
        if b % 3 == 0:
            assert sim.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == b
        else:
            assert sim.add_collider("box", "slip", center=(1, 1, 1), half=(0.1, 0.1, 0.1)) == b
    rc, msg = _raw_add(sim)
    assert rc == _lib.GSMPM_EINVAL and "too many boundary conditions (max 32)" in msg


def test_slab_and_fold_handles_refuse(dev):
    from gsmpm import _lib
    S = _witness()[0]
    # a slab handle
    slab = _bare()
    slab.slab_init(0, 1, 0, 32)
    rc, msg = _raw_add(slab)
    assert rc == _lib.GSMPM_ESTATE and "slab" in msg
    assert slab.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0  # no id was taken
    # the other order: slab_init on a handle that holds one; it stays an ordinary handle that steps
    from gsmpm.sim import Simulator
    sim = Simulator(len(S["x"]), **S["kw"])
    bit = sim.add_collider("ball", "slip", 0.5, **CR.GEOMETRY["ball"])
    rc = _lib.LIB.gsmpm_mpm_slab_init(sim._h, 0, 1, 0, 32, 2, 10)
    assert rc == _lib.GSMPM_ESTATE and "extended colliders" in _lib.last_error()
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    sim.step(S["dt"], [1 << bit] * 2)
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


def test_fitting_refuses_collider_records(dev):
    from gpu_helpers import dropin_sim
    from scenarios import lego_problem
    prob = lego_problem(500, 32)
    prob["cfg"] = dict(prob["cfg"], boundary_conditions=[])
    sim, args = dropin_sim(prob, dev, with_collider=False, fitting=True)
    rec = dict(type="collider", shape="ball", **CR.GEOMETRY["ball"])
    with pytest.raises(TypeError, match="fitting"):
        sim.set_boundary_conditions([rec], args)
    with pytest.raises(TypeError, match="fitting"):
        sim.add_collider("ball", **CR.GEOMETRY["ball"])
    assert sim.grid_postprocess == []
