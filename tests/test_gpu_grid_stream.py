"""k_grid_f's cover gather on multi-chunk tiles (fused.h node_extra: a node's
second and later chunk windows as one ordered stream, in batches of 8),
against the CPU oracle, on scenes small enough to enumerate.

Scene A: n_grid 32, extent 2.0 (4x4x5 fused tiles of 8x8x7 cells), 2,833
particles around the corner shared by the eight tiles (1..2, 1..2, 1..2):

    tile     particles  chunks
    (1,1,1)    1300       6
    (2,1,1)     600       3
    (1,2,1)     300       2
    (2,2,1)     256       1     the 256 / 257 boundary
    (1,1,2)     257       2     the 256 / 257 boundary
    (2,1,2), (1,2,2), (2,2,2)  40 each, 1 chunk, within two cells of the corner

The nodes at the shared corner have 8 live covers and 6+3+2+1+2+1+1+1 = 17
window loads (9 after the first chunks: two batches of the stream, the last
with one entry); face and edge nodes give the 2- and 4-cover cases, interior
nodes of (1,1,1) the 1-cover, 6-chunk case (5 stream entries).  The per-tile
counts and the corner's covers are asserted on the CPU first.

Scene B: a 1,300-particle tile at the grid's low corner (tile (0,0,0): covers
clipped by the grid edge) and, at the high corner, tiles (3,3,4) with 700 and
(3,3,3) with 600 particles.

No gravity, no collider.  Each scene runs at rest
(every sum of momentum is zero: the expected v, C are 0, or with FCR the f32
roundoff of a zero stress, held to the moving case's scales) -- and with
initial velocities 0.5 N(0,1), without which a dropped or doubled chunk window
could not show in x, v, C or F_trial.  In three substeps of 1e-4 a particle
moves < 1e-2 cell and every particle keeps > 0.05 cell from its tile's faces,
so none leaves its tile: no escapes, nothing order-dependent.

Bounds: those of tests/test_gpu_configs.py::test_dense_tiles_multi_chunk
(_check with stress=True and F_trial 1e-4: x, F_trial 1e-4, v 2e-3, C 5e-3 on
_c_err's scale), imported, not restated.  The dense grid is not compared: the
grid getter (Simulator.get_grid, k_grid_get) exists only on keep_grid handles,
which run the per-phase pipeline, not k_grid_f.
"""
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_configs import _c_err, _check

pytestmark = pytest.mark.gpu

NG, EXT, DT = 32, 2.0, 1e-4
T = (8, 8, 7)
FIELDS = ("x", "v", "C", "F_trial")
V_SCALE = 0.5  # sigma of the moving case's initial velocities
SCENE_A = {(1, 1, 1): 1300, (2, 1, 1): 600, (1, 2, 1): 300, (2, 2, 1): 256, (1, 1, 2): 257,
           (2, 1, 2): 40, (1, 2, 2): 40, (2, 2, 2): 40}
SCENE_B = {(0, 0, 0): 1300, (3, 3, 4): 700, (3, 3, 3): 600}


def _cells(tile, corner=None):
    """Base-cell range [lo, hi) per axis of a tile's particles: the whole tile
    (kept two cells inside the grid), or within two cells of `corner`."""
    lo = [max(tile[d] * T[d], 1) for d in range(3)]
    hi = [min((tile[d] + 1) * T[d], NG - 3) for d in range(3)]
    if corner is not None:
        lo = [max(lo[d], corner[d] - 2) for d in range(3)]
        hi = [min(hi[d], corner[d] + 2) for d in range(3)]
    return lo, hi


def _tiles_of(x):
    base = (x * np.float32(NG / EXT) - np.float32(0.5)).astype(np.int64)  # truncation, as base_of()
    return base, base // np.array(T)


@functools.lru_cache(maxsize=None)
def _scene(name):
    import oracle as O
    rng = np.random.default_rng(17)
    counts = SCENE_A if name == "A" else SCENE_B
    corner = (16, 16, 14)
    xs = []
    for tile, n in counts.items():
        lo, hi = _cells(tile, corner if n == 40 else None)
        u = rng.uniform(np.array(lo) + 0.1, np.array(hi) - 0.1, size=(n, 3))  # base-cell coordinates
        xs.append((u + 0.5) * (EXT / NG))
    x = np.concatenate(xs).astype(np.float32)
    x = x[rng.permutation(len(x))]
    n = len(x)
    cov = np.tile(np.array([4e-5, 0, 0, 4e-5, 0, 4e-5], np.float32), (n, 1))
    vol = O.particle_volume(x, NG, EXT)
    v = (V_SCALE * rng.normal(size=(n, 3))).astype(np.float32)
    # the layout, before any GPU work
    base, t3 = _tiles_of(x)
    got = {}
    for t in map(tuple, t3):
        got[t] = got.get(t, 0) + 1
    assert got == counts, got
    u = x * np.float32(NG / EXT) - np.float32(0.5) - t3 * np.array(T)  # offset in the tile, in cells
    assert u.min() > 0.05 and (np.array(T) - u).min() > 0.05
    if name == "A":
        # the corner node (16, 16, 14) lies in the stencil box of all eight tiles: 8 live covers, 17 windows
        loads = 0
        for tile, c in counts.items():
            b = base[(t3 == np.array(tile)).all(1)]
            if c <= 256:
                assert (b.min(0) <= corner).all() and (b.max(0) + 2 >= corner).all(), tile
            loads += (c + 255) // 256
        assert loads == 17
    return dict(x=x, cov=cov, vol=vol, v=v)


def _kw(fcr):
    return dict(n_grid=NG, grid_extent=EXT, material="jelly", E=2e5, nu=0.3, density=200.0, gravity=(0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def _reference(name, fcr, moving):
    """The oracle's state after 1 and after 3 substeps (computed once, shared)."""
    import oracle as O
    S = _scene(name)
    ref = O.OracleMPM(S["x"], S["cov"], S["vol"], jelly_quirk=not fcr, v=S["v"] if moving else None, **_kw(fcr))
    out = {}
    for k in (1, 2, 3):
        ref.substep(DT, [], [])
        if k in (1, 3):
            out[k] = {f: getattr(ref, f).copy() for f in FIELDS}
    return out


def _sim(dev, name, fcr, moving):
    import torch
    from gsmpm.sim import Simulator
    S = _scene(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sim = Simulator(len(S["x"]), jelly_fcr=fcr, **_kw(fcr))
    sim.set_particles(t(S["x"]), t(S["cov"]), t(S["vol"]), t(S["v"]) if moving else None)
    assert sim.pipeline == "fused"
    return sim


def _state(sim):
    return {f: sim.get(f).cpu().numpy() for f in FIELDS}


def _compare(dev, name, fcr, moving, nsub):
    exp = _reference(name, fcr, moving)[nsub]
    sim = _sim(dev, name, fcr, moving)
    sim.step(DT, [0xFFFFFFFF] * nsub)
    stats = sim.debug_stats()
    assert stats["max_per_tile"] > 1024, stats
    got = _state(sim)
    for f in FIELDS:
        assert np.isfinite(got[f]).all(), f
    errs = {f: rel_err(got[f].reshape(exp[f].shape), exp[f]) for f in FIELDS}
    # at rest the expected v and C are zero (FCR: the f32 roundoff of a zero stress) and no scale of their
    # own: they are held to the moving case's scales, V_SCALE and V_SCALE * inv_dx
    v_scale = exp["v"] if moving else np.array([V_SCALE])
    if not moving:
        errs["v"] = float(np.abs(got["v"].astype(np.float64) - exp["v"]).max() / max(np.abs(exp["v"]).max(), V_SCALE))
    errs["C"] = _c_err(got["C"].reshape(exp["C"].shape), exp["C"], v_scale, NG / EXT)
    print(f"scene {name} fcr {fcr} moving {moving} substeps {nsub}:", {k: f"{e:.2e}" for k, e in errs.items()})
    if moving:
        # a real dynamic (the grid averages tens of particles a node: what is left of the draws)
        assert np.abs(exp["v"]).max() > 0.2 * V_SCALE and np.abs(exp["C"]).max() > 1.0
    _check(errs, f"stream scene {name}", {"F_trial": 1e-4}, stress=True)
    if not moving and not fcr:  # zero stress, zero momentum: every sum is exactly 0
        assert not got["v"].any() and not got["C"].any()


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("fcr", [False, True])
def test_corner_of_eight_tiles_against_oracle(dev, fcr, moving, nsub):
    _compare(dev, "A", fcr, moving, nsub)


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("fcr", [False, True])
def test_dense_tiles_at_the_grid_corners_against_oracle(dev, fcr, moving, nsub):
    _compare(dev, "B", fcr, moving, nsub)


def test_two_simulators_agree_bitwise(dev):
    """Scene A at rest, stress-free jelly, 3 substeps, two simulators built
    from the same arrays.  With momentum in the scene (the moving case, or
    FCR's roundoff forces) two runs differ in the last bit of one or two
    coordinates, before this stream as after it (measured on both: 1-2 of
    8,499 x elements, 6e-8): which particles share a chunk of a multi-chunk
    tile follows the binning's slot reservation, so the chunk windows' f32
    sums are not fixed from run to run.  That case is held to the oracle
    above, not to bit equality."""
    runs = []
    for _ in range(2):
        sim = _sim(dev, "A", False, False)
        sim.step(DT, [0xFFFFFFFF] * 3)
        runs.append(_state(sim))
    for f in FIELDS:
        np.testing.assert_array_equal(runs[0][f], runs[1][f], err_msg=f)
