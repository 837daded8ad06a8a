"""Multi-chunk ("dense") tiles of the fused pipeline: every chunk stores the
hull of its last and its new stencil box and ORs its box into the cover
records, and the grid update reads the union.  Two invariants
carry the results: outside the box a chunk last stored its slot holds +0, and
a record's box is a superset of every chunk's box since the re-binning.

The scenes make a dense tile's boxes move, shrink and differ between chunks,
on a 32^3 grid of extent 2.0 (dx = 0.0625, fused tiles of 8 x 8 x 7 cells:
4 x 4 x 5 of them), jelly as written, no gravity, against the CPU oracle at
the bounds of test_gpu_mpm.py.  Each test first asserts, on the oracle's
positions, that its scene has the property it is about.
"""
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_mpm import TOL, TOL_DERIVED

pytestmark = pytest.mark.gpu

NG, EXT, DT = 32, 2.0, 1e-3
TILE = np.array([8, 8, 7])
CHUNK = 256
KW = dict(n_grid=NG, grid_extent=EXT, E=2e4, nu=0.3, density=200.0, gravity=(0.0, 0.0, 0.0))


def _base(x):
    """base cell of a particle's stencil (nodes base .. base + 2 per axis)"""
    return np.floor(np.asarray(x, np.float64) * (NG / EXT) - 0.5).astype(int)


def _tile(x):
    return _base(x) // TILE


def _box(rng, n, lo, hi):
    return np.stack([rng.uniform(lo[d], hi[d], n) for d in range(3)], 1)


def _one_dense_tile(x, chunks=3):
    """all of x binned into one tile, of at least `chunks` chunks"""
    t = _tile(x)
    return bool((t == t[0]).all()) and len(x) > (chunks - 1) * CHUNK


class _Ref:
    """an oracle run: the final state, and x at the substeps in `keep`"""

    def __init__(self, x, v, material, steps, keep=()):
        import oracle as O
        x = x.astype(np.float32)
        self.x0, self.v0 = x, v.astype(np.float32)
        self.cov = np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32), (len(x), 1))
        self.vol = O.particle_volume(x, NG, EXT).astype(np.float32)
        self.material, self.steps = material, steps
        ref = O.OracleMPM(x, self.cov, self.vol, v=self.v0, material=material, **KW)  # jelly as written
        self.at = {}
        for s in range(steps):
            if s in keep:
                self.at[s] = ref.x.copy()
            ref.substep(DT, [], [])
        self.x, self.v, self.C, self.F_trial = ref.x.copy(), ref.v.copy(), ref.C.copy(), ref.F_trial.copy()


def _run(dev, ref, interval):
    import torch
    from gsmpm.sim import Simulator
    sim = Simulator(len(ref.x0), material=ref.material, **KW)
    assert sim.pipeline == "fused"
    sim.set_rebin_interval(interval)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sim.set_particles(t(ref.x0), t(ref.cov), t(ref.vol), t(ref.v0))
    sim.step(DT, [0] * ref.steps)
    return sim


def _compare(sim, ref, probe=None):
    stress = ref.material != "jelly"
    got = {k: sim.get(k).cpu().numpy().reshape(getattr(ref, k).shape) for k in ("x", "v", "C", "F_trial")}
    errs = {k: rel_err(g, getattr(ref, k)) for k, g in got.items()}
    # C = sum_i w_i v_i dpos_i^T 4 / dx^2 over 27 nodes with |dpos| <= 1.5 dx: each term is of size
    # |v| 6 / dx and is rounded to f32 whatever the sum comes to.  Layers in uniform motion sum to C = 0,
    # where the oracle's own C is that rounding alone (3e-5 here), so the rounding of 27 such terms is
    # taken off C's error before it is measured against max |C| like the other fields.
    floor = 27 * np.finfo(np.float32).eps * 6.0 * np.abs(ref.v).max() / (EXT / NG)
    errs["C"] = float(max(np.abs(got["C"] - ref.C).max() - floor, 0.0) / max(np.abs(ref.C).max(), 1e-30))
    print("rel errs", {k: f"{e:.2e}" for k, e in errs.items()})
    if probe is not None:  # a stale slot term would drag the probe: per element, at the scene's scale
        for k in ("x", "v"):
            r = getattr(ref, k)
            d = np.abs(got[k][probe] - r[probe]).max()
            print("probe", k, got[k][probe], r[probe])
            assert d < TOL * np.abs(r).max(), (k, got[k][probe], r[probe])
    for k, e in errs.items():
        bound = TOL_DERIVED.get(k, TOL) if stress else TOL
        assert e < bound, f"{k}: rel err {e:.3e} > {bound} (all: {errs})"


# ---- leaving slab: one tile of 5 chunks, 2 z-cells thick, moving up and away
# from a probe at rest whose stencil shares the slab's lowest node layer
N_SLAB = 1100


@functools.lru_cache(maxsize=None)
def _slab_ref(material):
    rng = np.random.default_rng(11)
    slab = _box(rng, N_SLAB, (0.56, 0.56, 0.50), (0.98, 0.98, 0.56))
    probe = np.array([[0.77, 0.77, 0.44]])
    x = np.concatenate([slab, probe])
    v = np.zeros_like(x)
    v[:N_SLAB, 2] = 2.0
    return _Ref(x, v, material, 60)


def _slab_preconditions(ref):
    b0, b1 = _base(ref.x0), _base(ref.x)
    assert _one_dense_tile(ref.x0[:N_SLAB], 5)
    assert np.ptp(b0[:N_SLAB, 2]) == 1  # 2 z-cells thick
    # the probe's stencil (nodes base .. base + 2) holds the slab's lowest node layer at the start
    assert b0[N_SLAB, 2] + 2 >= b0[:N_SLAB, 2].min() > b0[N_SLAB, 2]
    # ... and the slab clears that stencil: the node layers it leaves are the old-minus-new part of its
    # chunks' boxes.  (The shared nodes drag the probe along at about half the slab's speed -- the
    # reference's physics -- so at the end its own stencil has moved up a cell; it still gathers from a
    # layer the slab has left, where a stale slot term would reach it.)
    left = np.arange(b0[:N_SLAB, 2].min(), b1[:N_SLAB, 2].min())  # node layers no stencil of the slab holds any more
    assert b1[:N_SLAB, 2].min() > b0[N_SLAB, 2] + 2
    assert np.intersect1d(left, b1[N_SLAB, 2] + np.arange(3)).size > 0


@pytest.mark.parametrize("interval", [1, 10, 50])
def test_leaving_slab(dev, interval):
    """Interval 50 stores the old-minus-new region with no refreshing full
    store in between, interval 1 stores the whole window in every launch."""
    ref = _slab_ref("jelly")
    _slab_preconditions(ref)
    _compare(_run(dev, ref, interval), ref, probe=N_SLAB)


def test_leaving_slab_metal(dev):
    """the stress term in the scatter"""
    ref = _slab_ref("metal")
    _slab_preconditions(ref)
    _compare(_run(dev, ref, 50), ref, probe=N_SLAB)


def test_switch_off(dev, monkeypatch):
    """GSMPM_DENSE_BOX=0 at handle creation: whole windows and full masks (the A/B leg)"""
    monkeypatch.setenv("GSMPM_DENSE_BOX", "0")
    ref = _slab_ref("jelly")
    _slab_preconditions(ref)
    _compare(_run(dev, ref, 50), ref, probe=N_SLAB)


# ---- two layers of one tile approaching each other: chunks with different
# masks, a gap in their union
@functools.lru_cache(maxsize=None)
def _layers_ref():
    rng = np.random.default_rng(12)
    lo = _box(rng, 600, (0.56, 0.56, 0.50), (0.98, 0.98, 0.53))
    hi = _box(rng, 600, (0.56, 0.56, 0.86), (0.98, 0.98, 0.89))
    x = np.concatenate([lo, hi])
    v = np.zeros_like(x)
    v[:600, 2], v[600:, 2] = 1.5, -1.5
    return _Ref(x, v, "jelly", 40)


def test_two_layers(dev):
    ref = _layers_ref()
    b0, b1 = _base(ref.x0), _base(ref.x)
    assert _one_dense_tile(ref.x0, 5)
    # no node between the layers' stencils at the start: a gap in the union of the masks
    assert b0[600:, 2].min() - (b0[:600, 2].max() + 2) > 1
    # both layers' boxes move inwards: each leaves a node layer behind
    assert b1[:600, 2].min() > b0[:600, 2].min() and b1[600:, 2].max() < b0[600:, 2].max()
    _compare(_run(dev, ref, 50), ref)


# ---- neighbourhood: a dense tile moving -x towards an empty tile (its
# stencils reach below the tile, which appends a tile that reads the tile
# tables and whole windows), a second dense tile at +y, a sparse one at +x,
# five of whose particles are fast enough to leave their chunk's window
N_FAST = 5


@functools.lru_cache(maxsize=None)
def _neighbourhood_ref():
    rng = np.random.default_rng(13)
    a = _box(rng, N_SLAB, (0.56, 0.56, 0.50), (0.98, 0.98, 0.56))
    b = _box(rng, N_SLAB, (0.56, 1.06, 0.50), (0.98, 1.48, 0.56))
    c = _box(rng, 100, (1.06, 0.56, 0.50), (1.48, 0.98, 0.56))
    x = np.concatenate([a, b, c])
    v = np.zeros_like(x)
    v[:N_SLAB, 0] = -3.0
    # of the sparse tile, at its (-x, +y, +z) corner and heading that way: they leave the tile at once (among
    # a dense tile's particles the grid shares a fast one's momentum out within a substep), pass over the
    # dense tile at +y and stay inside the grid for the 40 substeps
    d = np.array([-1.0, 1.0, 1.0]) / np.sqrt(3.0)
    fast = 2 * N_SLAB + np.argsort(c @ d)[-N_FAST:]
    v[fast] = 60.0 * d
    return _Ref(x, v, "jelly", 40, keep=(10, 15)), fast


def test_neighbourhood(dev):
    ref, fast = _neighbourhood_ref()
    ta = _tile(ref.x0[:N_SLAB])
    assert _one_dense_tile(ref.x0[:N_SLAB], 5) and _one_dense_tile(ref.x0[N_SLAB:2 * N_SLAB], 5)
    assert (_tile(ref.x0[N_SLAB:2 * N_SLAB])[0] == ta[0] + [0, 1, 0]).all()
    tc = _tile(ref.x0[2 * N_SLAB:])
    assert (tc == ta[0] + [1, 0, 0]).all() and len(tc) <= CHUNK
    assert not (_tile(ref.x0) == ta[0] - [1, 0, 0]).all(1).any()  # the tile at -x is empty
    # the blob's stencils reach below its tile (base cell one under the tile's first) between re-binnings
    assert (_base(ref.at[15][:N_SLAB])[:, 0] < ta[0][0] * TILE[0]).any()
    assert np.abs(np.linalg.norm(ref.v0[fast], axis=1) - 60.0).max() < 1e-3
    # the five leave their chunk's window (the tile and one cell around it) well before a re-binning
    # at the longest interval could follow them
    off = _base(ref.at[10][fast]) - tc[0] * TILE
    assert ((off < -1) | (off > TILE)).any(1).all()
    assert (_base(ref.x) >= 0).all() and (_base(ref.x) < NG).all()
    sim = _run(dev, ref, 50)
    assert sim.escapes() > 0
    _compare(sim, ref)
