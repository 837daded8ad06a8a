"""The interior-filling reference (tests/fill_ref.py) pinned on its own fixture,
a hollow sphere of 4,000 Gaussians at 32^3 (radius 10 cells), without a GPU.

The fixture's conditions that tests/test_gpu_fill.py relies on are asserted
here on the reference alone: at FIX["threshold"] the cells within the per-cell
density bound of the threshold are at most 0.5 % of the grid.
"""
from __future__ import annotations

import numpy as np
import pytest

import fill_ref as R

# the shared fixture: threshold 4 sits in the flank of the shell's density (peak ~14.6)
FIX = dict(n=32, extent=2.0, n_points=4000, radius=10.0, support=4, threshold=4.0, seed=0)


def _radius_cells(n):
    g = np.stack(np.meshgrid(*[np.arange(n) + 0.5] * 3, indexing="ij"), -1) - n / 2.0
    return np.linalg.norm(g, axis=-1)


@pytest.fixture(scope="module")
def sphere():
    x, c, o = R.shell(FIX["n_points"], FIX["n"], FIX["extent"], FIX["radius"], seed=FIX["seed"])
    dens, n_c, skipped = R.density(x, c, o, FIX["n"], FIX["extent"], FIX["support"])
    occ = dens > FIX["threshold"]
    return dict(x=x, cov=c, opa=o, dens=dens, n_c=n_c, skipped=skipped, occ=occ, bits=R.direction_bits(occ))


def test_shell_interior_is_the_ball(sphere):
    rr = _radius_cells(FIX["n"])
    inside = R.interior(sphere["occ"], sphere["bits"])
    assert sphere["skipped"] == 0
    assert inside[rr <= FIX["radius"] - 2].all()       # every cell within R - 2 dx
    assert not inside[rr >= FIX["radius"] + 2].any()   # none beyond R + 2 dx
    assert not (inside & sphere["occ"]).any()


def test_fixture_has_few_borderline_cells(sphere):
    """|density - threshold| <= n_c q/2 + rel density on at most 0.5 % of the cells.  rel is
    the bound's f32 term: 4e-6, or twice what the float32 evaluation of the same formula shows
    against float64 on this fixture (measured 3.7e-6 over the cells of at least one quantum,
    1.2e-6 over those above 1e-3), so 7.4e-6 here."""
    d32, n32, _ = R.density(sphere["x"], sphere["cov"], sphere["opa"], FIX["n"], FIX["extent"], FIX["support"],
                            dtype=np.float32)
    assert np.array_equal(n32, sphere["n_c"])
    rel, measured = R.f32_term(sphere["dens"], d32)
    print("largest relative error of the float32 evaluation:", measured)
    assert 1e-7 < measured < 1e-5 and rel <= 2e-5
    bound = R.density_bound(sphere["dens"], sphere["n_c"], rel)
    share = (np.abs(sphere["dens"] - FIX["threshold"]) <= bound).mean()
    assert share <= 0.005, share


def test_hole_needs_min_hits_5():
    n = FIX["n"]
    x, c, o = R.shell(FIX["n_points"], n, FIX["extent"], FIX["radius"], seed=FIX["seed"], hole_deg=25.0)
    dens, _, _ = R.density(x, c, o, n, FIX["extent"], FIX["support"])
    occ = dens > FIX["threshold"]
    bits = R.direction_bits(occ)
    ball = _radius_cells(n) <= FIX["radius"] - 2
    sees_out = ball & (((bits >> 0) & 1) == 0)          # nothing occupied towards +x: the hole
    assert sees_out.sum() > 20
    assert (((bits >> 1) & 0x1F)[sees_out] == 0x1F).all()  # the other five directions are closed
    in6 = R.interior(occ, bits, min_hits=6)
    in5 = R.interior(occ, bits, min_hits=5)
    assert not in6[sees_out].any()
    assert in5[sees_out].all()
    assert in6[ball & ~sees_out].all()


def test_parity_tells_the_cavity_from_the_wall():
    """Two nested shells (radii 12 and 5 cells): a body with a thick wall and an empty core.
    From the wall (between the shells) every axis ray meets one occupied run, or three across
    the core; from the core it meets two.  parity_dir keeps the odd counts, so the core is
    dropped and the wall stays; without it both are filled.  The runs are counted by walking."""
    n = FIX["n"]
    parts = [R.shell(4000, n, FIX["extent"], 12.0, seed=1), R.shell(900, n, FIX["extent"], 5.0, seed=2)]
    x, c, o = (np.concatenate([p[k] for p in parts]) for k in range(3))
    dens, _, _ = R.density(x, c, o, n, FIX["extent"], FIX["support"])
    occ = dens > FIX["threshold"]
    bits = R.direction_bits(occ)
    rr = _radius_cells(n)
    g = np.stack(np.meshgrid(*[np.arange(n) + 0.5] * 3, indexing="ij"), -1) - n / 2.0
    lateral = np.hypot(g[..., 1], g[..., 2])
    band = (rr >= 7.5) & (rr <= 9.5)
    core = rr <= 2.5
    wall_near = band & (g[..., 0] > 0)                       # +x meets the outer shell only
    wall_far = band & (g[..., 0] < 0) & (lateral <= 2.0)     # +x crosses the core first
    assert not occ[core].any() and not occ[band].any()
    plain = R.interior(occ, bits, parity_dir=-1)
    odd = R.interior(occ, bits, parity_dir=0)
    assert plain[core].all() and plain[band].all()
    assert not odd[core].any() and odd[wall_near].all() and odd[wall_far].all()
    for cell in np.argwhere(core):
        assert R.count_runs(occ, cell, 0) == 2
    for cell in np.argwhere(wall_near)[::7]:
        assert R.count_runs(occ, cell, 0) == 1
    for cell in np.argwhere(wall_far):
        assert R.count_runs(occ, cell, 0) == 3
    # every parity and hit bit against the walk, on a sample of cells and all six directions
    rng = np.random.default_rng(0)
    for cell in rng.integers(0, n, size=(200, 3)):
        for d in range(6):
            runs = R.count_runs(occ, cell, d)
            assert (bits[tuple(cell)] >> (8 + d)) & 1 == runs & 1
            assert (bits[tuple(cell)] >> d) & 1 == (runs > 0)


def test_box_limits_the_interior(sphere):
    box = ([0.0, 0.9, 0.0], [2.0, 1.3, 0.97])
    inside = R.interior(sphere["occ"], sphere["bits"], box=box, extent=FIX["extent"])
    full = R.interior(sphere["occ"], sphere["bits"])
    dx = FIX["extent"] / FIX["n"]
    ctr = (np.arange(FIX["n"]) + 0.5) * dx
    ky = (ctr >= np.float32(0.9)) & (ctr <= np.float32(1.3))
    kz = ctr <= np.float32(0.97)
    want = full & ky[None, :, None] & kz[None, None, :]
    assert np.array_equal(inside, want) and 0 < inside.sum() < full.sum()


def _mix_int(v):
    v ^= v >> 16
    v = (v * 0x7feb352d) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 0x846ca68b) & 0xFFFFFFFF
    return v ^ (v >> 16)


def test_hash_matches_plain_integer_arithmetic():
    for seed, cell, k, axis in ((0, 0, 0, 0), (7, 12345, 3, 2), (0xFFFFFFFF, 32 ** 3 - 1, 7, 1)):
        want = _mix_int((_mix_int((_mix_int(seed) + cell) & 0xFFFFFFFF) + 4 * k + axis) & 0xFFFFFFFF)
        assert int(R.fill_hash(seed, cell, k, axis)) == want


def test_emission_counts_order_and_containment(sphere):
    inside = R.interior(sphere["occ"], sphere["bits"])
    n, dx = FIX["n"], np.float32(FIX["extent"] / FIX["n"])
    cells = np.flatnonzero(inside.ravel())
    for per_cell in (1, 4):
        pos, total = R.emit(inside, per_cell, 3, FIX["extent"])
        assert total == per_cell * len(cells) and pos.shape == (total, 3) and pos.dtype == np.float32
        owner = np.repeat(np.stack(np.unravel_index(cells, inside.shape), -1), per_cell, axis=0)
        lo, hi = owner.astype(np.float32) * dx, (owner + 1).astype(np.float32) * dx
        assert ((pos >= lo) & (pos <= hi)).all()          # each particle in its cell, cells in linear order
        assert len(np.unique(pos, axis=0)) == total
    cut, total = R.emit(inside, 4, 3, FIX["extent"], capacity=10)
    assert total == 4 * len(cells) and np.array_equal(cut, pos[:10])
    other, _ = R.emit(inside, 4, 4, FIX["extent"])
    assert not np.array_equal(other, pos)
    none, zero = R.emit(np.zeros_like(inside), 4, 3, FIX["extent"])
    assert zero == 0 and none.shape == (0, 3)


def test_nearest_takes_the_lowest_index_of_a_tie():
    rng = np.random.default_rng(5)
    src = rng.random((50, 3)).astype(np.float32)
    src = np.concatenate([src, src[:10]])       # duplicates of rows 0..9 at 50..59
    idx = R.nearest(src[50:], src)
    assert idx.tolist() == list(range(10))
    q = rng.random((30, 3)).astype(np.float32)
    d2 = ((q[:, None, :].astype(np.float64) - src[None].astype(np.float64)) ** 2).sum(-1)
    got = R.nearest(q, src)
    assert np.allclose(d2[np.arange(30), got], d2.min(1), rtol=1e-5)


def test_malformed_particles_are_skipped_in_the_reference(sphere):
    x, c, o = sphere["x"][:50].copy(), sphere["cov"][:50].copy(), sphere["opa"][:50].copy()
    x[0, 1] = np.nan
    x[1] = [5.0, 1.0, 1.0]     # outside the grid
    c[2] = 0.0                 # zero covariance: harmless, marks its own cell
    o[3] = 0.0                 # opacity 0: harmless, adds nothing
    c[4, 3] = np.inf
    o[5] = np.nan
    dens, n_c, skipped = R.density(x, c, o, FIX["n"], FIX["extent"], FIX["support"])
    assert skipped == 4
    keep = np.ones(50, bool)
    keep[[0, 1, 3, 4, 5]] = False
    want, _, _ = R.density(x[keep], c[keep], o[keep], FIX["n"], FIX["extent"], FIX["support"])
    assert np.array_equal(dens, want)
    cell2 = tuple(np.floor(x[2] * np.float32(FIX["n"] / FIX["extent"])).astype(int))
    alone, _, _ = R.density(x[2:3], c[2:3], o[2:3], FIX["n"], FIX["extent"], FIX["support"])
    assert alone[cell2] > 0 and np.count_nonzero(alone) == 1
