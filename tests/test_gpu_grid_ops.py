"""The grid update (node_update in csrc/mpm.hip: normalisation + gravity,
fixed cubes, plane colliders; shared by k_grid, k_grid_f, the folded path and
the slab path) and the P2G sums, read at grid level and held to the float64
reference of tests/grid_ref.py and to the CPU oracle, with colliders that act:
oblique normals, friction, two colliders, a collider before / after a fixed
cube, an inactive cube, activity bits that differ from the operator's index,
bit 31 of the 32-entry table, and the lattice-aligned list at n_grid 50 whose
predicates depend on unfused f32 rounding (-ffp-contract=off).

Scene S (grid_ref.scene): lego_problem(4000, 32), v = 2 N(0,1) from
default_rng(11), random C of scale 20, stress-free jelly, the config's
gravity, dt 1e-4; list h runs lego_problem(3000, 50).  Every test asserts,
from the reference side, that the colliders act (below the plane, inward
velocity) on at least 500 massive nodes (scene S with the oblique plane:
5,883 massive nodes, 1,346 acting); the 500-particle blobs cannot reach that
(their stencils cover at most 8^3 = 512 nodes, half of them above the plane)
and assert 64.

Bounds, in units of EPS = 2^-23, and where they come from:
* P2G sums (mass, v_in) against float64: 4x the oracle's own error against
  float64 on the same inputs, computed in the test, floor 4 EPS -- errors
  relative to the global maxima max m and max sum|terms|.  The margin is for
  the GPU's other summation order and its fixed-point windows.  Totals of
  mass and momentum: 1e-7 relative of the particle sums.
* v_out against float64 node_update_ref fed the GPU's own mass and v_in (so
  the summation order drops out): 8 EPS of ||v_in / m|| + ||dt g|| per node,
  on the nodes the reference does not mark ambiguous (within 1e-6 of a plane
  or a cube face; none for lists a-g); about 25 roundings in the chain, the
  oracle measures 2.1 EPS.  Massless nodes exactly 0.
* v_out against the oracle's om_grid_normalize + om_grid_ops fed the same
  mass and v_in, on ALL nodes: 16 EPS.  For list h this pins the f32
  predicates on the lattice: one differently decided node is off by >= 1e-2.
* Particle level (20 substeps in two step calls, pipelines fused / phased /
  fold) against OracleMPM: test_gpu_mpm.py's bounds, 1e-4 of the field's max
  on x, v, C, F_trial for a stress-free run; v 2e-3 and C 5e-3 with FCR jelly.

Measured on an MI355X (EPS units; the P2G figures move a little from run to
run with the binning order): P2G mass 0.8-1.3 and momentum 0.8-1.0 at 32^3
against the oracle's 1.55 / 1.42 (50^3: 12.4 / 19.8 against 12.7 / 20.2), totals
mass 4e-11..2.5e-9 and momentum 1.3e-8..4.6e-8; v_out against float64 at most
1.8; against the oracle 0 -- bit for bit on every list, the lattice one
included; particle level x 1e-7, v 7e-7, C 2.4e-6, F_trial 2e-7 (FCR jelly v
2.5e-6, C 6e-6); touched tiles 12 (blob inside a tile column) and 27.

Hand mutation check (scratch builds, none of them failing test_gpu_mpm.py's
collider scenes): dropping `* op.friction` in node_update fails every test
here; swapping the first two operators of the table fails list d at both
levels (only two colliders are order-sensitive: a cube and a collider
commute, since a stopped node stays stopped under the collider); an explicit
fused multiply-subtract in the plane predicate fails list h at both levels.
Building with -ffp-contract=fast alone passes this file: with the present
compiler the node coordinates have several uses and are not fused into the
predicates (foam parity in test_gpu_mpm.py notices that build instead).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import grid_ref as G
from conftest import rel_err

pytestmark = pytest.mark.gpu

FIELDS = ("x", "v", "C", "F_trial")
MIN_ACTING = 500


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """Scene S for a list name (list h: 3000 Gaussians at 50^3)."""
    return G.scene(3000, 50) if name == "h" else G.scene()


def _impulse_kick(S, impulses, active):
    """[n, 3] float64 velocity kick of the active impulses (f32 box test on
    x, constants at their f32 values) and the inside count per impulse."""
    x = S["x"]
    kick = np.zeros(x.shape, np.float64)
    inside = []
    for (c, s, f, sdt), act in zip(impulses, active):
        c32, s32 = np.asarray(c, np.float32), np.asarray(s, np.float32)
        d = np.abs(x - c32) - s32          # f32, as the kernels decide it
        assert np.abs(np.abs(x.astype(np.float64) - G.f32(c)) - G.f32(s)).min() > G.AMBIG  # nobody on a face
        ins = (d < 0).all(1)
        inside.append(int(ins.sum()))
        if act:
            kick[ins] += G.f32(f)[None, :] / S["mass"].astype(np.float64)[ins, None] * float(np.float32(sdt))
    return kick, inside


@functools.lru_cache(maxsize=None)
def _p2g_witnesses(name, imp_key=None):
    """float64 P2G sums of the scene, and the oracle's error against them."""
    import oracle as O
    S = _scene(name)
    impulses, active = imp_key if imp_key else ((), ())
    kick, inside = _impulse_kick(S, impulses, active)
    m, mv, ab = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"], kick=kick)
    ref = O.OracleMPM(S["x"], S["cov"], S["vol"], v=S["v"], **S["kw"])
    ref.C[:] = S["C"]
    for c, s, f, sdt in impulses:
        ref.add_impulse(list(c), list(s), list(f), sdt)
    ref.substep_begin(S["dt"], [int(a) for a in active])
    em = np.abs(ref.gm.astype(np.float64) - m).max() / m.max()
    emv = np.abs(ref.gv_in.astype(np.float64) - mv).max() / ab.max()
    return dict(m=m, mv=mv, ab=ab, em=em, emv=emv, kick=kick, inside=inside)


def _grid_sim(dev, S):
    from gsmpm.sim import Simulator
    sim = Simulator(len(S["x"]), phased=True, keep_grid=True, **S["kw"])
    sim.set_particles(_t(dev, S["x"]), _t(dev, S["cov"]), _t(dev, S["vol"]), _t(dev, S["v"]))
    sim.set("C", _t(dev, S["C"]))
    assert np.array_equal(sim.get("mass").cpu().numpy(), S["mass"])
    return sim


def _read_grid(sim):
    return {k: sim.get_grid(k).cpu().numpy().reshape(sim.n_grid ** 3, -1) for k in ("mass", "v_in", "v_out")}


def _oracle_grid_update(S, mass, v_in, ops, active):
    """om_grid_normalize + om_grid_ops on the given node sums."""
    import oracle as O
    ref = O.OracleMPM(S["x"][:1], S["cov"][:1], S["vol"][:1], **S["kw"])
    G.add_ops_oracle(ref, ops)
    ref.gm[:] = mass.reshape(-1)
    ref.gv_in[:] = v_in
    ref.gv_out[:] = 0
    _, _, tab, oa = ref._tables(None, [int(a) for a in active])
    st = ctypes.byref(ref._st)
    ref._L.om_grid_normalize(st, ctypes.c_float(S["dt"]))
    ref._L.om_grid_ops(st, ctypes.c_int(len(ref.ops)), tab, O._p(oa))
    return ref.gv_out.copy()


def _check_grid(S, W, grid, ops, active, tag):
    """(i) P2G sums vs float64, (ii) v_out vs float64, (iii) v_out vs the oracle."""
    ng = S["n_grid"]
    mass, v_in, v_out = grid["mass"].reshape(-1), grid["v_in"], grid["v_out"]
    acting = G.acting_nodes(W["mv"], W["m"], ng, S["dx32"], S["dt_g32"], ops)
    # (i)
    em = np.abs(mass.astype(np.float64) - W["m"]).max() / W["m"].max()
    emv = np.abs(v_in.astype(np.float64) - W["mv"]).max() / W["ab"].max()
    bm, bmv = max(4 * W["em"], 4 * G.EPS), max(4 * W["emv"], 4 * G.EPS)
    m64 = S["mass"].astype(np.float64)
    mom = (m64[:, None] * (S["v"].astype(np.float64) + W["kick"])).sum(0)
    cm = abs(mass.astype(np.float64).sum() - m64.sum()) / m64.sum()
    cp = np.abs(v_in.astype(np.float64).sum(0) - mom).max() / np.abs(mom).max()
    # (ii)
    ref, amb = G.node_update_ref(v_in, mass, ng, S["dx32"], S["dt_g32"], ops, active)
    live = mass > np.float32(1e-15)
    scale = np.zeros(ng ** 3)
    scale[live] = np.sqrt(((v_in[live].astype(np.float64) / mass[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum())
    e2 = np.abs(v_out.astype(np.float64) - ref).max(1) / scale
    # (iii)
    orc = _oracle_grid_update(S, mass, v_in, ops, active)
    e3 = np.abs(v_out.astype(np.float64) - orc).max(1) / scale
    print(f"GRID {tag}: massive {int(live.sum())} acting {acting} ambiguous {int((amb & live).sum())} | "
          f"P2G mass {em / G.EPS:.2f} (oracle {W['em'] / G.EPS:.2f}) mom {emv / G.EPS:.2f} "
          f"(oracle {W['emv'] / G.EPS:.2f}) EPS, totals {cm:.1e} {cp:.1e} | "
          f"v_out vs f64 {e2[~amb].max() / G.EPS:.2f} EPS, vs oracle {e3.max() / G.EPS:.2f} EPS")
    assert acting >= MIN_ACTING, acting
    assert em <= bm and emv <= bmv, (em / G.EPS, emv / G.EPS, bm / G.EPS, bmv / G.EPS)
    assert cm < 1e-7 and cp < 1e-7, (cm, cp)
    assert np.all(v_out[~live] == 0)
    assert e2[~amb].max() <= 8 * G.EPS, e2[~amb].max() / G.EPS
    assert e3.max() <= 16 * G.EPS, e3.max() / G.EPS
    return amb, live


# ------------------------------------------------------ a. grid level --
@pytest.mark.parametrize("name", list("abcdefgh"))
def test_grid_level_lists(dev, name):
    S, W = _scene(name), _p2g_witnesses(name)
    ops, active = G.OP_LISTS[name]
    sim = _grid_sim(dev, S)
    mask = G.add_ops_sim(sim, ops, active)
    sim.step(S["dt"], [mask])
    amb, live = _check_grid(S, W, _read_grid(sim), ops, active, f"list {name}")
    if name == "h":
        assert (amb & live).sum() >= 100  # the lattice case has massive nodes on the plane / the faces
    else:
        assert not amb.any()


# ------------------------------------------- b. impulses at grid level --
IMPULSES = (((1.013, 0.987, 1.113), (0.207, 0.313, 0.153), (-300.0, 200.0, 500.0), 1e-4),
            ((1.087, 1.013, 1.057), (0.153, 0.207, 0.113), (400.0, 400.0, -600.0), 1e-4))


def test_grid_level_impulses(dev):
    """Two overlapping off-lattice impulse boxes, the second inactive: the
    total of v_in is sum m v + (#inside the first) f sdt, in float64 (1e-7
    relative, the bound of the P2G totals), and v_in matches the float64 sums
    of the kicked velocities."""
    S = _scene("b")
    act = (1, 0)
    W = _p2g_witnesses("b", (IMPULSES, act))
    assert min(W["inside"]) >= 100 and W["inside"][0] != W["inside"][1]
    both = _impulse_kick(S, IMPULSES, (1, 1))[0]
    assert (np.abs(both - W["kick"]).max(1) > 0).sum() >= 100  # the inactive box would change the answer
    ops, active = G.OP_LISTS["b"]
    sim = _grid_sim(dev, S)
    bits = [sim.add_impulse(list(c), list(s), list(f), sdt) for c, s, f, sdt in IMPULSES]
    mask = G.add_ops_sim(sim, ops, active) | (1 << bits[0])
    sim.step(S["dt"], [mask])
    grid = _read_grid(sim)
    m64 = S["mass"].astype(np.float64)
    f, sdt = G.f32(IMPULSES[0][2]), float(np.float32(IMPULSES[0][3]))
    want = (m64[:, None] * S["v"].astype(np.float64)).sum(0) + W["inside"][0] * f * sdt
    got = grid["v_in"].astype(np.float64).sum(0)
    e = np.abs(got - want).max() / np.abs(want).max()
    free = (m64[:, None] * S["v"].astype(np.float64)).sum(0)
    print(f"IMPULSE: inside {W['inside']}, total v_in {got}, want {want} (no kick {free}), rel {e:.1e}")
    assert np.abs(want - free).max() > 0.1 * np.abs(want).max()  # the kick is a good share of the total
    assert e < 1e-7, e
    _check_grid(S, W, grid, ops, active, "impulses")


# ------------------------------------------------ c. id bookkeeping --
CUBE2 = G.cube((0.913, 0.887, 1.187), (0.23, 0.31, 0.17))


def test_ids_differ_from_table_index(dev):
    """Collider first (bit 0), a cube (bit 1), an impulse (bit 2), a second
    cube (bit 3, inactive).  In the operator table the second cube has index
    2 and the impulse index 0: a kernel that indexed the mask by table index
    would apply the inactive cube (bit 2 is set) and skip the impulse (bit 0
    is clear)."""
    S = _scene("b")
    imp = (IMPULSES[0],)
    W = _p2g_witnesses("b", (imp, (1,)))
    col = G.OP_LISTS["b"][0][0]
    ops, active = [col, G.CUBE, CUBE2], [1, 1, 0]
    sim = _grid_sim(dev, S)
    assert sim.add_plane_collider(list(col[1]), list(col[2]), col[3]) == 0
    assert sim.add_fixed_cube(list(G.CUBE[1]), list(G.CUBE[2])) == 1
    assert sim.add_impulse(*[list(a) for a in imp[0][:3]], imp[0][3]) == 2
    assert sim.add_fixed_cube(list(CUBE2[1]), list(CUBE2[2])) == 3
    sim.step(S["dt"], [(1 << 1) | (1 << 2)])
    grid = _read_grid(sim)
    # the inactive cube would matter: it holds massive nodes the others leave moving
    on, _ = G.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops, [1, 1, 1])
    off, _ = G.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops, active)
    assert (np.abs(on - off).max(1) > 0).sum() >= 100
    _check_grid(S, W, grid, ops, active, "ids")


def test_table_of_32_and_the_33rd(dev):
    """32 entries, of which only the last cube (bit 31) is active: it acts,
    the 31 before it (cubes that would stop every node, and impulses) do not.
    A 33rd add fails with the library's error and leaves the table as it was."""
    from gsmpm._lib import GsmpmError
    S, W = _scene("b"), _p2g_witnesses("b")
    col = G.OP_LISTS["b"][0][0]
    everything = G.cube((1.0, 1.0, 1.0), (1.5, 1.5, 1.5))
    sim = _grid_sim(dev, S)
    ops, active = [], []
    for b in range(31):
        if b == 7:
            assert sim.add_plane_collider(list(col[1]), list(col[2]), col[3]) == b
            ops.append(col), active.append(1)
        elif b % 5 == 3:
            assert sim.add_impulse([1.0, 1.0, 1.0], [1.5, 1.5, 1.5], [1.0, 1.0, 1.0], 1e-4) == b
        else:
            assert sim.add_fixed_cube(list(everything[1]), list(everything[2])) == b
            ops.append(everything), active.append(0)
    assert sim.add_fixed_cube(list(G.CUBE[1]), list(G.CUBE[2])) == 31
    ops.append(G.CUBE), active.append(1)
    with pytest.raises(GsmpmError, match=r"too many boundary conditions \(max 32\)"):
        sim.add_fixed_cube(list(everything[1]), list(everything[2]))
    with pytest.raises(GsmpmError, match=r"too many boundary conditions \(max 32\)"):
        sim.add_plane_collider([0.0, 0.0, 1.9], [0.0, 0.0, 1.0], 0.0)
    sim.step(S["dt"], [1 << 31])
    grid = _read_grid(sim)
    ref, _ = G.node_update_ref(grid["v_in"], grid["mass"], S["n_grid"], S["dx32"], S["dt_g32"], ops, active)
    live = grid["mass"].reshape(-1) > np.float32(1e-15)
    stopped = live & (np.abs(ref).max(1) == 0)
    assert stopped.sum() >= 100 and (live & ~stopped).sum() >= 1000  # bit 31 acts, and only it
    _check_grid(S, W, grid, ops, active, "32 entries")


# ---------------------------------------------------- d. particle level --
TOL_FREE = {k: 1e-4 for k in FIELDS}                                  # test_gpu_mpm.py TOL: stress-free run
TOL_STRESS = {"x": 1e-4, "F_trial": 1e-4, "v": 2e-3, "C": 5e-3}       # test_gpu_mpm.py TOL_DERIVED
NSUB, CALLS = 10, 2


def _particles(S):
    return S["x"], S["cov"], S["vol"], S["v"]


@functools.lru_cache(maxsize=None)
def _oracle_run(name, quirk=True):
    import oracle as O
    S = _scene(name)
    ops, active = G.OP_LISTS[name]
    x, cov, vol, v = _particles(S)
    ref = O.OracleMPM(x, cov, vol, v=v, jelly_quirk=quirk, **S["kw"])
    G.add_ops_oracle(ref, ops)
    m, mv, _ = G.p2g_ref(x, v, np.zeros((len(x), 9)), S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    acting = G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops)
    for _ in range(NSUB * CALLS):
        ref.substep(S["dt"], [], [int(a) for a in active])
    return {k: getattr(ref, k).copy() for k in FIELDS}, acting


def _sim_run(dev, pipe, S, ops, active, particles, jelly_fcr=False):
    import torch
    from gsmpm.sim import Simulator
    old = os.environ.get("GSMPM_FOLD")
    os.environ["GSMPM_FOLD"] = "1" if pipe == "fold" else "0"
    try:
        sim = Simulator(len(particles[0]), phased=pipe == "phased", jelly_fcr=jelly_fcr, **S["kw"])
    finally:
        if old is None:
            os.environ.pop("GSMPM_FOLD")
        else:
            os.environ["GSMPM_FOLD"] = old
    assert sim.pipeline == ("phased" if pipe == "phased" else "fused") and sim.folded == (pipe == "fold")
    sim.set_particles(*[_t(dev, a) for a in particles])
    mask = G.add_ops_sim(sim, ops, active)
    for _ in range(CALLS):
        sim.step(S["dt"], [mask] * NSUB)
    torch.cuda.synchronize()
    return {k: sim.get(k).cpu().numpy() for k in FIELDS}, sim


def _compare(got, exp, tol, tag):
    errs = {k: rel_err(got[k].reshape(exp[k].shape), exp[k]) for k in FIELDS}
    print(f"PARTICLES {tag}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < tol[k], (k, e, errs)


@pytest.mark.parametrize("name", list("bdfh"))
@pytest.mark.parametrize("pipe", ["fused", "phased", "fold"])
def test_particle_level(dev, pipe, name):
    S = _scene(name)
    ops, active = G.OP_LISTS[name]
    exp, acting = _oracle_run(name)
    assert acting >= MIN_ACTING, acting
    got, _ = _sim_run(dev, pipe, S, ops, active, _particles(S))
    _compare(got, exp, TOL_FREE, f"{pipe} list {name} (acting {acting})")


def test_particle_level_fcr_jelly(dev):
    """FCR jelly: the collider's effect feeds back through the stress."""
    S = _scene("b")
    ops, active = G.OP_LISTS["b"]
    exp, acting = _oracle_run("b", quirk=False)
    assert acting >= MIN_ACTING, acting
    got, _ = _sim_run(dev, "fused", S, ops, active, _particles(S), jelly_fcr=True)
    _compare(got, exp, TOL_STRESS, f"fused FCR jelly list b (acting {acting})")


# centre -> the most tiles the fused pipeline's touched list can hold for it (see the docstring)
BLOBS = {"inside_a_tile": ((1.27, 1.27, 0.95), 16), "on_a_tile_corner": ((1.0, 1.0, 0.95), 27)}


@pytest.mark.parametrize("where", list(BLOBS))
def test_tiny_blob_few_tiles(dev, where):
    """500 particles in a box of side 0.3 at 32^3, moving at 3 m/s (velocity
    spread 0.5) into the oblique plane that cuts through the blob; 20
    substeps on the fused pipeline, 1e-4 on every field.

    The touched list of the grid update holds the occupied tiles (8 x 8 x 7
    base cells) and their upper neighbours, t + {0, 1}^3.  k_grid_f hands
    touched tiles to the XCDs in groups of 16, so with at most 16 of them one
    XCD's workgroups do all the work and 7/8 of the launch idles: the case
    to cover.  A box of side 0.3 (4.8 cells) around (1.0, 1.0, 0.95) -- grid
    coordinate 16 on x and y, a tile boundary -- occupies 2 x 2 x 2 tiles
    and so touches 27, whatever the kernels do; the same box around
    (1.27, 1.27, 0.95) lies inside one tile on x and y and in two on z:
    2 x 2 x 3 = 12 touched tiles, and at most 16 is asserted.  Both run.

    The blob's stencils cover at most 8^3 = 512 nodes (4.8 cells: 6 base
    cells an axis at the most), so the scene-wide 500 acting nodes cannot
    hold here; the plane passes within
    0.04 of the blob's centre (half-size 0.15), so between a third and two
    thirds of the massive nodes are below it, nearly all moving inward: 64
    is asked."""
    import oracle as O
    centre, max_touched = BLOBS[where]
    S = _scene("b")
    ops, active = G.OP_LISTS["b"]
    rng = np.random.default_rng(23)
    n, ng = 500, S["n_grid"]
    x = (np.array(centre) + rng.uniform(-0.15, 0.15, size=(n, 3))).astype(np.float32)
    nrm = G.unit_normal32(ops[0][2])
    v = (-3.0 * nrm[None, :] + 0.5 * rng.standard_normal((n, 3))).astype(np.float32)
    cov = np.tile(np.array([1e-5, 0, 0, 1e-5, 0, 1e-5], np.float32), (n, 1))
    vol = O.particle_volume(x, ng, S["kw"]["grid_extent"])
    mass = (np.float32(S["kw"]["density"]) * vol).astype(np.float32)
    m, mv, _ = G.p2g_ref(x, v, np.zeros((n, 9)), mass, ng, S["dx32"], S["inv_dx32"])
    acting = G.acting_nodes(mv, m, ng, S["dx32"], S["dt_g32"], ops)
    assert (m > 0).sum() <= 512 and acting >= 64, acting
    ref = O.OracleMPM(x, cov, vol, v=v, **S["kw"])
    G.add_ops_oracle(ref, ops)
    for _ in range(NSUB * CALLS):
        ref.substep(S["dt"], [], [int(a) for a in active])
    got, sim = _sim_run(dev, "fused", S, ops, active, (x, cov, vol, v))
    touched = sim.debug_stats()["touched_tiles"]
    print(f"BLOB {where}: touched tiles {touched}, massive nodes {int((m > 0).sum())}, acting {acting}")
    assert 1 <= touched <= max_touched, touched
    _compare(got, {k: getattr(ref, k) for k in FIELDS}, TOL_FREE, f"blob {where} fused list b")
