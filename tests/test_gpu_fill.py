"""Interior filling on the GPU (csrc/fill.hip through gsmpm.fill) against the
numpy reference tests/fill_ref.py.

Shapes: fill grids of 8 (a line shorter than a wave), 32, and 96 (not a power
of two, lines longer than one 64-bit word; the 96 shells straddle cell 64),
with 1, 257 and 4,000 Gaussians.  Density is compared with the float64
reference under the per-cell bound n_c q/2 + rel density; everything after
the occupied mask is integer logic and is compared exactly, the reference
being applied to the GPU's own mask.

rel, the f32 term, is 4e-6 where that covers float32: the float32 evaluation
of the same formula on the reference side (fill_ref.density with
dtype=float32) differs from float64 by 9.9e-7 relative on the 8^3 case, but by
3.7e-6 on the 32^3 shell and by 3.8e-5 / 4.1e-5 on the 96^3 shells (257 /
4,000 Gaussians; dx = 1/48 is not a float32 and the stamp's offsets are
differences of numbers near 1.3), so there rel is twice the measured value
(fill_ref.f32_term, computed from the reference alone).
"""
from __future__ import annotations

import ctypes
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import fill_ref as R
from conftest import GOLDEN
from test_fill_ref import FIX

pytestmark = pytest.mark.gpu

EXTENT = 2.0


def _single():
    return (np.array([[1.1, 0.9, 1.3]], np.float32), np.array([[0.05, 0.01, 0.0, 0.04, 0.0, 0.06]], np.float32),
            np.array([0.9], np.float32))


# name -> (n_grid, support, threshold, particles)
CASES = {
    "n8_1": (8, 2, 0.05, _single),
    "n32_4000": (FIX["n"], FIX["support"], FIX["threshold"],
                 lambda: R.shell(FIX["n_points"], FIX["n"], EXTENT, FIX["radius"], seed=FIX["seed"])),
    "n32_hole": (FIX["n"], FIX["support"], FIX["threshold"],
                 lambda: R.shell(FIX["n_points"], FIX["n"], EXTENT, FIX["radius"], seed=FIX["seed"], hole_deg=25.0)),
    "n96_257": (96, 4, 2.0, lambda: R.shell(257, 96, EXTENT, 5.0, centre_cells=(62, 63.5, 65), seed=3)),
    "n96_4000": (96, 4, 2.0, lambda: R.shell(4000, 96, EXTENT, 14.0, centre_cells=(60, 64, 66), seed=4,
                                             hole_deg=20.0)),
}
_cache = {}


def case(name):
    """The particles and the float64 reference density of a case, computed once."""
    if name not in _cache:
        n, support, thr, make = CASES[name]
        x, c, o = make()
        dens, n_c, skipped = R.density(x, c, o, n, EXTENT, support)
        rel, measured = R.f32_term(dens, R.density(x, c, o, n, EXTENT, support, dtype=np.float32)[0])
        _cache[name] = dict(n=n, support=support, thr=thr, x=x, cov=c, opa=o, dens=dens, n_c=n_c, skipped=skipped,
                            rel=rel, rel_measured=measured)
    return _cache[name]


def filler(cs, **kw):
    from gsmpm.fill import Filler
    return Filler(cs["n"], EXTENT, cs["thr"], support=cs["support"], **kw)


def run(cs, dev, order=None, **kw):
    import torch
    f = filler(cs, **kw)
    sel = slice(None) if order is None else order
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    total, skipped = f.interior(t(cs["x"]), t(cs["cov"]), t(cs["opa"]))
    return f, total, skipped


def grid(f, which):
    return f.grid(which).cpu().numpy()


# ------------------------------------------------------------------ density --
@pytest.mark.parametrize("name", list(CASES))
def test_density_within_the_bound_and_occupied_mask(dev, name):
    cs = case(name)
    f, _, skipped = run(cs, dev)
    assert skipped == cs["skipped"] == 0
    fixed = grid(f, "density_fixed")
    assert fixed.min() >= 0
    got = fixed.astype(np.float64) * R.Q
    bound = R.density_bound(cs["dens"], cs["n_c"], cs["rel"])
    err = np.abs(got - cs["dens"])
    print(name, "f32 term:", cs["rel"], "(float32 evaluation of the reference:", cs["rel_measured"], ")")
    print(name, "largest |err| / bound:", (err / np.maximum(bound, 1e-300))[cs["n_c"] > 0].max(),
          "largest |err|:", err.max())
    assert (err <= bound).all()
    assert np.array_equal(grid(f, "density"), fixed.astype(np.float32) * np.float32(R.Q))
    # occupied: the reference's mask outside the cells too close to the threshold to call
    border = np.abs(cs["dens"] - cs["thr"]) <= bound
    assert border.mean() <= 0.005
    occ = grid(f, "occupied").astype(bool)
    assert np.array_equal(occ[~border], (cs["dens"] > cs["thr"])[~border])
    assert np.array_equal(occ, fixed > np.floor(cs["thr"] * 2.0 ** 24))


@pytest.mark.parametrize("name", ["n32_4000", "n96_257"])
def test_density_is_bit_identical_across_orders_and_runs(dev, name):
    cs = case(name)
    a = grid(run(cs, dev)[0], "density_fixed")
    b = grid(run(cs, dev)[0], "density_fixed")
    perm = np.random.default_rng(1).permutation(len(cs["x"]))
    c = grid(run(cs, dev, order=perm)[0], "density_fixed")
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ------------------------------------------------- interior, direction bits --
BOX = {8: ([0.0, 0.3, 0.0], [2.0, 1.6, 1.4]), 32: ([0.0, 0.9, 0.0], [2.0, 1.3, 0.97]),
       96: ([1.0, 1.3, 0.0], [1.5, 1.45, 1.36])}


@pytest.mark.parametrize("name", ["n8_1", "n32_hole", "n96_257", "n96_4000"])
def test_interior_and_direction_bits_are_exact(dev, name):
    cs = case(name)
    ref_bits = None
    sizes = {}
    for min_hits in (6, 5):
        for parity_dir in (-1, 0):
            for box in (None, BOX[cs["n"]]):
                f, total, _ = run(cs, dev, min_hits=min_hits, parity_dir=parity_dir, box=box)
                occ = grid(f, "occupied").astype(bool)
                if ref_bits is None:
                    ref_bits = R.direction_bits(occ)
                assert np.array_equal(grid(f, "bits").view(np.uint16), ref_bits)
                want = R.interior(occ, ref_bits, min_hits, parity_dir, box, EXTENT)
                assert np.array_equal(grid(f, "interior").astype(bool), want)
                assert total == want.sum()
                sizes[(min_hits, parity_dir, box is not None)] = int(want.sum())
    print(name, sizes)
    if name != "n8_1":  # the options bite: the hole needs min_hits 5, the box and the parity cut cells away
        assert sizes[(6, -1, False)] > 0
        assert sizes[(5, -1, False)] >= sizes[(6, -1, False)]
        assert sizes[(6, -1, True)] < sizes[(6, -1, False)]
    if name in ("n32_hole", "n96_4000"):
        assert sizes[(5, -1, False)] > sizes[(6, -1, False)]


# ----------------------------------------------------------------- emission --
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", ["n32_4000", "n96_4000"])
def test_emission_is_bit_exact(dev, name):
    import torch
    cs = case(name)
    n, dx = cs["n"], np.float32(EXTENT / cs["n"])
    for per_cell in (1, 4):
        for seed in (1, 0xDEADBEEF):
            f, total, _ = run(cs, dev, per_cell=per_cell, seed=seed)
            inside = grid(f, "interior").astype(bool)
            want, ref_total = R.emit(inside, per_cell, seed, EXTENT)
            assert total == ref_total > 0
            got = f.emit().cpu().numpy()
            assert _same_bits(got, want)
            owner = np.repeat(np.argwhere(inside), per_cell, axis=0)
            assert ((got >= owner.astype(np.float32) * dx) & (got <= (owner + 1).astype(np.float32) * dx)).all()
    # a capacity below the total: exactly that prefix, the rest of the buffer untouched
    cap = (total // 8) * 4 + 1  # ends inside a cell
    f, total2, _ = run(cs, dev, per_cell=4, seed=0xDEADBEEF, capacity=cap)
    assert total2 == total
    sentinel = np.float32(-777.25)
    out = torch.full((total, 3), float(sentinel), device=dev)
    f.emit(out=out)
    out = out.cpu().numpy()
    assert _same_bits(out[:cap], want[:cap])
    assert (out[cap:] == sentinel).all()


def test_no_interior_cell_emits_nothing(dev):
    import torch
    cs = case("n8_1")
    f, total, _ = run(cs, dev, per_cell=4)
    assert total == 0 and not grid(f, "interior").any()
    out = torch.full((16, 3), -1.0, device=dev)
    f.emit(out=out)
    assert (out.cpu().numpy() == -1.0).all()
    assert f.emit().shape == (0, 3)


# ------------------------------------------------------------------ nearest --
@pytest.mark.parametrize("nq,ns", [(1000, 3000), (1, 1), (300, 257)])
def test_nearest_index_is_exact(dev, nq, ns):
    import torch
    from gsmpm.fill import nearest
    rng = np.random.default_rng(nq + ns)
    src = rng.random((ns, 3)).astype(np.float32)
    if ns >= 200:  # duplicated source points: ties, the lowest index must win
        dup = rng.integers(0, ns // 2, ns // 4)
        src[ns - len(dup):] = src[dup]
    q = rng.random((nq, 3)).astype(np.float32)
    if nq >= 200:
        q[:100] = src[rng.integers(0, ns, 100)]  # queries on top of (duplicated) sources
    want = R.nearest(q, src)
    got = nearest(torch.from_numpy(q).to(dev), torch.from_numpy(src).to(dev)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if ns >= 200:
        assert (want[:100] < ns - ns // 4).all()


# ---------------------------------------------------------------- malformed --
def test_malformed_particles_are_skipped(dev):
    cs = dict(case("n32_4000"))
    x, c, o = cs["x"].copy(), cs["cov"].copy(), cs["opa"].copy()
    x[0, 1] = np.nan
    x[1] = [5.0, 1.0, 1.0]       # outside the grid
    x[6] = [-0.01, 1.0, 1.0]     # just outside
    c[2] = 0.0                   # zero covariance: harmless
    o[3] = 0.0                   # opacity 0: harmless
    c[4, 3] = np.inf
    o[5] = np.nan
    x[7, 2] = np.inf
    bad = [0, 1, 4, 5, 6, 7]
    cs.update(x=x, cov=c, opa=o)
    f, total, skipped = run(cs, dev)
    assert skipped == len(bad)
    keep = np.ones(len(x), bool)
    keep[bad] = False
    g, total_kept, skipped_kept = run(cs, dev, order=keep)
    assert skipped_kept == 0 and total_kept == total
    for which in ("density_fixed", "occupied", "interior", "bits"):
        assert np.array_equal(grid(f, which), grid(g, which)), which
    ref, ref_nc, ref_skipped = R.density(x, c, o, cs["n"], EXTENT, cs["support"])
    assert ref_skipped == len(bad)
    assert (np.abs(grid(f, "density_fixed") * R.Q - ref) <= R.density_bound(ref, ref_nc, cs["rel"])).all()
    # the zero-covariance particle alone marks exactly its own cell
    alone = dict(cs, x=x[2:3], cov=c[2:3], opa=o[2:3])
    d = grid(run(alone, dev)[0], "density_fixed")
    cell = tuple(np.floor(x[2] * np.float32(cs["n"] / EXTENT)).astype(int))
    assert d[cell] > 0 and np.count_nonzero(d) == 1


def bad_argument_cases():
    """(field, value) pairs gsmpm_fill_params must refuse."""
    return [("n_grid", 3), ("n_grid", 0), ("per_cell", 0), ("per_cell", 9), ("min_hits", 0), ("min_hits", 7),
            ("grid_extent", 0.0), ("grid_extent", -2.0), ("density_threshold", 0.0), ("density_threshold", -1.0),
            ("parity_dir", 6), ("support", -1), ("capacity", -1)]


def good_params():
    from gsmpm import _lib
    p = _lib.FillParams()
    p.n_grid, p.grid_extent, p.density_threshold, p.support = 8, EXTENT, 0.05, 2
    p.min_hits, p.parity_dir, p.per_cell, p.seed, p.capacity = 6, -1, 1, 0, 512
    return p


def refused(rc, needle=""):
    from gsmpm import _lib
    return rc == _lib.GSMPM_EINVAL and needle in _lib.last_error() and _lib.last_error() != ""


def test_bad_arguments_are_refused_and_a_valid_call_follows(dev):
    import torch
    from gsmpm import _lib
    L = _lib.LIB
    nb = ctypes.c_uint64(0)
    p = good_params()
    assert L.gsmpm_fill_workspace_size(ctypes.byref(p), ctypes.byref(nb)) == 0 and nb.value > 0
    ws = torch.zeros(nb.value + 256, dtype=torch.uint8, device=dev)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    x, c, o = (torch.from_numpy(a).to(dev) for a in _single())
    tot, skp = ctypes.c_int64(-5), ctypes.c_int64(-5)
    before = ws.clone()

    def interior(pp, xx=x, cc=c, oo=o, n=1, w=wp, t=tot, s=skp):
        return L.gsmpm_fill_interior(ctypes.byref(pp), xx.data_ptr() if xx is not None else None,
                                     cc.data_ptr() if cc is not None else None,
                                     oo.data_ptr() if oo is not None else None, n, w, nb.value,
                                     ctypes.byref(t) if t is not None else None,
                                     ctypes.byref(s) if s is not None else None, None)

    for field, value in bad_argument_cases():
        q = good_params()
        setattr(q, field, value)
        assert refused(L.gsmpm_fill_workspace_size(ctypes.byref(q), ctypes.byref(nb)), field.split("_")[0]), field
        assert refused(interior(q), "gsmpm_fill_interior"), field
        assert refused(L.gsmpm_fill_emit(ctypes.byref(q), wp, nb.value, x.data_ptr(), None)), field
        assert refused(L.gsmpm_fill_get_grid(ctypes.byref(q), wp, nb.value, 0, x.data_ptr(), None)), field
    assert refused(L.gsmpm_fill_workspace_size(None, ctypes.byref(nb)), "null")
    assert refused(L.gsmpm_fill_workspace_size(ctypes.byref(p), None), "null")
    assert refused(interior(p, xx=None), "null")
    assert refused(interior(p, cc=None), "null")
    assert refused(interior(p, oo=None), "null")
    assert refused(interior(p, w=None), "null")
    assert refused(interior(p, t=None), "null")
    assert refused(interior(p, s=None), "null")
    assert refused(interior(p, n=-1), "count")
    assert refused(interior(p, w=wp + 4), "aligned")
    assert refused(L.gsmpm_fill_emit(ctypes.byref(p), wp, nb.value, None, None), "null")
    assert refused(L.gsmpm_fill_get_grid(ctypes.byref(p), wp, nb.value, 9, x.data_ptr(), None), "unknown")
    assert refused(L.gsmpm_fill_nearest(None, 1, x.data_ptr(), 1, x.data_ptr(), None), "null")
    assert refused(L.gsmpm_fill_nearest(x.data_ptr(), -1, x.data_ptr(), 1, x.data_ptr(), None), "count")
    assert refused(L.gsmpm_fill_nearest(x.data_ptr(), 1, x.data_ptr(), 0, x.data_ptr(), None), "count")
    small = L.gsmpm_fill_interior(ctypes.byref(p), x.data_ptr(), c.data_ptr(), o.data_ptr(), 1, wp, 1024,
                                  ctypes.byref(tot), ctypes.byref(skp), None)
    assert small == _lib.GSMPM_ESPACE
    torch.cuda.synchronize()
    assert torch.equal(ws, before) and tot.value == -5  # nothing was launched
    # a valid call still works
    assert interior(p) == 0 and tot.value == 0 and skp.value == 0
    cs = case("n8_1")
    occ = torch.empty(8 ** 3, dtype=torch.uint8, device=dev)
    assert L.gsmpm_fill_get_grid(ctypes.byref(p), wp, nb.value, 1, occ.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert occ.sum().item() == (cs["dens"] > cs["thr"]).sum()


# ------------------------------------------------------------- Python layer --
def test_fill_particles_and_init_filled_particles(dev):
    import torch
    from internel_filling.filling import fill_particles, get_particle_volume, init_filled_particles
    cs = case("n32_4000")
    t = lambda a: torch.from_numpy(a).to(dev)
    pos, cov, opa = t(cs["x"]), t(cs["cov"]), t(cs["opa"]).reshape(-1, 1)
    shs = torch.from_numpy(np.random.default_rng(0).normal(size=(len(cs["x"]), 16, 3)).astype(np.float32)).to(dev)
    args = {"n_grid": cs["n"], "density_threshold": cs["thr"], "support": cs["support"], "per_cell": 2, "seed": 9}
    new = fill_particles(pos, cov, opa, args)
    m = new.shape[0]
    assert m > 0 and m % 2 == 0 and new.shape == (m, 3)
    capped = fill_particles(pos, cov, opa, dict(args, max_particles=101))
    assert torch.equal(capped, new[:101])
    boxed = fill_particles(pos, cov, opa, dict(args, boundary=[0.0, 2.0, 0.9, 1.3, 0.0, 0.97]))
    assert 0 < boxed.shape[0] < m
    assert (boxed[:, 1] >= 0.9 - EXTENT / cs["n"]).all() and (boxed[:, 1] <= 1.3 + EXTENT / cs["n"]).all()
    with pytest.raises(ValueError):
        fill_particles(pos, cov, opa, dict(args, n_gird=3))
    shs2, opa2, cov2 = init_filled_particles(pos, shs, cov, opa, new)
    n = pos.shape[0]
    assert shs2.shape == (n + m, 16, 3) and opa2.shape == (n + m, 1) and cov2.shape == (n + m, 6)
    idx = torch.from_numpy(R.nearest(new.cpu().numpy(), cs["x"]).astype(np.int64)).to(dev)
    assert torch.equal(shs2[:n], shs) and torch.equal(shs2[n:], shs[idx])
    assert torch.equal(opa2[n:], opa[idx]) and torch.equal(cov2[n:], cov[idx])

    class A:
        n_grid, grid_extent = 32, EXTENT
    vol = get_particle_volume(torch.cat([pos, new]), A)
    assert vol.shape == (n + m,) and torch.isfinite(vol).all() and (vol > 0).all()


# --------------------------------------------------------------- end to end --
def _write_scene(tmp_path, with_filling):
    """A hollow sphere of 6,000 isotropic Gaussians (radius 0.5 in world space = 16 cells of the
    64^3 fill grid after world2grid, sigma 0.8 cells) as a trained-model directory, and its config."""
    from gaussian_splatting.scene import GaussianModel
    x, _, _ = R.shell(6000, 64, EXTENT, 16.0, seed=5, anisotropic=False)
    rng = np.random.default_rng(5)
    n = len(x)
    g = GaussianModel(3, device="cpu")
    rot = np.tile(np.array([1.0, 0, 0, 0]), (n, 1))
    g._set(x - 1.0, rng.normal(0.5, 0.5, (n, 1, 3)), rng.normal(0, 0.05, (n, 15, 3)), np.full((n, 1), 2.0),
           np.full((n, 3), np.log(0.8 * EXTENT / 64)), rot)
    model = tmp_path / "model"
    g.save_ply(str(model / "point_cloud" / "iteration_1" / "point_cloud.ply"))
    cfg = {"model": {"model_path": str(model), "loaded_iter": 1},
           "mpm": {"sim_area": [[-1.3, -1.3, -1.3], [1.3, 1.3, 1.3]], "E": 2e5, "nu": 0.2, "material": "jelly",
                   "density": 200.0, "n_grid": 64, "grid_extent": EXTENT, "substep_dt": 1e-4, "frame_dt": 1e-3,
                   "gravity": [0.0, 0.0, -100.0], "boundary_conditions": []},
           "render": {"output_path": str(tmp_path / ("filled" if with_filling else "plain")), "num_frames": 2}}
    if with_filling:
        cfg["particle_filling"] = {"n_grid": 64, "density_threshold": 1.0, "support": 4, "per_cell": 1, "seed": 2}
    path = tmp_path / ("filled.json" if with_filling else "plain.json")
    path.write_text(json.dumps(cfg))
    return str(path), cfg, n


def _run_main(cfg_path, monkeypatch):
    import main as drv
    counts = []
    real = getattr(drv.MPM_Simulator, "real", drv.MPM_Simulator)  # not a spy of an earlier call

    def spy(xyz, *a, **k):
        sim = real(xyz, *a, **k)
        counts.append(sim.n_particles)
        return sim

    spy.real = real
    monkeypatch.setattr(drv, "MPM_Simulator", spy)
    buf = io.StringIO()
    with redirect_stdout(buf):
        drv.main(["--config_path", cfg_path])
    return buf.getvalue(), counts


def test_main_with_and_without_particle_filling(dev, tmp_path, monkeypatch):
    from PIL import Image
    path, cfg, n = _write_scene(tmp_path, True)
    text, counts = _run_main(path, monkeypatch)
    assert f"Number of simulatable Gaussians: {n}" in text
    line = [ln for ln in text.splitlines() if ln.startswith("Number of filled particles: ")]
    assert len(line) == 1
    filled = int(line[0].split(": ")[1])
    assert filled > 5000           # the ball of radius ~14 cells holds > 11,000 cells
    assert counts == [n + filled]
    frames = []
    for f in range(3):
        img = np.asarray(Image.open(os.path.join(cfg["render"]["output_path"], "images", f"{f:04d}.png")))
        assert img.shape == (800, 800, 3) and img.max() > 0
        frames.append(img)
    # without the record: no filling, the solver sees the sources alone, nothing new is printed
    path0, cfg0, _ = _write_scene(tmp_path, False)
    text0, counts0 = _run_main(path0, monkeypatch)
    assert counts0 == [n] and "filled" not in text0
    assert f"Number of simulatable Gaussians: {n}" in text0
    # ... and the frames are those of the commit before the filling existed
    # (tests/golden/fill_plain/: that commit's main.py on this scene), up to one 8-bit level on
    # a handful of pixels, the allowance of test_gpu_main_e2e.py (to8b truncates)
    for f in range(3):
        img = np.asarray(Image.open(os.path.join(cfg0["render"]["output_path"], "images", f"{f:04d}.png")))
        want = np.asarray(Image.open(os.path.join(GOLDEN, "fill_plain", f"{f:04d}.png")))
        d = np.abs(img.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1 and (d > 0).sum() <= 2e-4 * d.size, (f, d.max(), (d > 0).sum())