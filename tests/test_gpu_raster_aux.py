"""The rasterizer's depth and alpha maps (gsmpm_raster_args.aux_depth /
aux_alpha; k_render<true>, k_render4<true>) on the GPU.

Over the contributors i the colour blend takes, D = sum z_i alpha_i T_i (z_i
the f32 view depth, not normalised) and A = 1 - T_final.  The reference is
tests/raster_aux_ref.py: the CPU oracle rendering colours (z_i, 1, 0) over
black, pinned against float64 in test_raster_aux_ref.py (3e-7 from it).

Bounds: |A - A_ref| < 1e-3, the project's pixel bound (A is a colour channel
of value 1), and |D - D_ref| < 1e-3 z_max with z_max the largest view depth
of a visible Gaussian (a blended channel's error is linear in the colours,
and 1e-3 is stated for colours up to about 1).
"""
from __future__ import annotations

import math
import os

import numpy as np
import pytest

import raster_aux_ref as AR

pytestmark = pytest.mark.gpu


def _camera(W, H, fovx, dist=3.0, yaw=0.3):
    """The camera of test_gpu_raster._camera."""
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    c, s = math.cos(yaw), math.sin(yaw)
    w2c = np.eye(4)
    w2c[:3, :3] = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    w2c[:3, 3] = [0.1, -0.05, dist]
    zn, zf = 0.01, 100.0
    tx, ty = math.tan(fovx / 2), math.tan(fovy / 2)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 1 / tx, 1 / ty
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zf / (zf - zn), -(zf * zn) / (zf - zn)
    view = w2c.T.astype(np.float32)
    full = (P @ w2c).T.astype(np.float32)
    campos = np.linalg.inv(w2c)[:3, 3].astype(np.float32)
    return view, full, campos, tx, ty


def _scene(P, seed):
    """The scene generator of test_gpu_raster._scene."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-0.8, 0.8, size=(P, 3)).astype(np.float32)
    A = rng.normal(0, 1, size=(P, 3, 3)) * 0.03
    cov = A @ A.transpose(0, 2, 1) + np.eye(3) * 1e-4
    c6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)
    opa = rng.uniform(0.05, 0.99, size=(P, 1)).astype(np.float32)
    shs = (rng.normal(0, 0.3, size=(P, 16, 3))).astype(np.float32)
    shs[:, 0] += 0.8
    return means, c6.astype(np.float32), opa, shs


def _opaque_scene(P, seed):
    """Dense and opaque: opacity 0.9-0.99, ~3-pixel footprints at 64x48, the
    centres kept ~10 pixels inside the image so that interior pixels stop at
    T < 1e-4 after a few contributors while the pixels at the image border
    never do (their quarter walks its tile's whole list)."""
    rng = np.random.default_rng(seed)
    means = (rng.uniform(-1, 1, size=(P, 3)) * np.array([1.0, 0.65, 0.5])).astype(np.float32)
    A = rng.normal(0, 1, size=(P, 3, 3)) * 0.07
    cov = A @ A.transpose(0, 2, 1) + np.eye(3) * 1e-3
    c6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)
    opa = rng.uniform(0.9, 0.99, size=(P, 1)).astype(np.float32)
    shs = (rng.normal(0, 0.3, size=(P, 16, 3))).astype(np.float32)
    shs[:, 0] += 0.8
    return means, c6.astype(np.float32), opa, shs


class _Case:
    """A scene on the device, its camera and (computed once, shared, never
    modified) the reference maps."""

    def __init__(self, dev, scene, W, H, bg=0.0):
        import torch
        self.dev, self.W, self.H = dev, W, H
        self.means, self.c6, self.opa, self.shs = scene
        self.view, self.full, self.campos, self.tx, self.ty = _camera(W, H, 0.9)
        t = self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.args = [t(self.means), t(self.opa), t(self.view), t(self.full), t(self.campos),
                     t(np.full(3, bg, np.float32)), H, W, self.tx, self.ty]
        self.kw = dict(sh_degree=3, shs=t(self.shs), cov3D_precomp=t(self.c6))
        self._ref = None

    def ref(self):
        if self._ref is None:
            D, A, radii, z = AR.forward(self.means, self.opa, self.view, self.full, self.campos, self.W, self.H,
                                        self.tx, self.ty, cov3D_precomp=self.c6)
            vis = radii > 0
            for a in (D, A, radii):
                a.setflags(write=False)
            self._ref = (D, A, radii, float(z[vis].min()), float(z[vis].max()))
        return self._ref

    def forward(self, **more):
        from gsmpm import raster
        return raster.forward(*self.args, **self.kw, **more)


_CASES = {}


def _case(dev, name):
    if name not in _CASES:
        if name == "small":
            _CASES[name] = _Case(dev, _scene(800, seed=800 + 97), 97, 61)      # ragged tiles and quarters
        elif name == "square":
            _CASES[name] = _Case(dev, _scene(2000, seed=2000 + 200), 200, 200)
        elif name == "opaque":
            _CASES[name] = _Case(dev, _opaque_scene(3000, seed=3000), 64, 48)
    return _CASES[name]


def _check_vs_ref(c, depth, alpha, label):
    D_ref, A_ref, _, zmin, zmax = c.ref()
    D, A = depth.cpu().numpy(), alpha.cpu().numpy()
    eA, eD = np.abs(A - A_ref).max(), np.abs(D - D_ref).max()
    print(f"aux maps vs reference [{label}]: |dA| {eA:.2e}  |dD| {eD:.2e} = {eD / zmax:.2e} z_max (z_max {zmax:.3f})")
    assert eA < 1e-3, (eA, int((np.abs(A - A_ref) >= 1e-3).sum()))
    assert eD < 1e-3 * zmax, (eD, zmax, int((np.abs(D - D_ref) >= 1e-3 * zmax).sum()))
    return D, A


@pytest.mark.parametrize("name", ["small", "square"])
def test_maps_vs_reference(dev, name):
    """(P, W, H) = (800, 97, 61) and (2000, 200, 200), the scenes, camera and
    seeds of test_gpu_raster.test_render_vs_oracle."""
    c = _case(dev, name)
    _, color, radii, depth, alpha = c.forward(depth=True, alpha=True)
    assert depth.shape == (c.H, c.W) and alpha.shape == (c.H, c.W)
    assert np.array_equal(radii.cpu().numpy(), c.ref()[2])
    _check_vs_ref(c, depth, alpha, name)


def test_long_lists_and_early_stop(dev):
    """3,000 opaque Gaussians on 64x48 (4x3 tiles).  Lists: the binned pair
    count exceeds 512 x 10 + 2 P, so even with every Gaussian in both interior
    tiles one of the ten border tiles lists more than 512 entries -- more than
    the two batches in flight at the start, so the ids prefetched inside the
    loop are used -- and every border tile has a pixel with A < 0.99, which
    cannot have stopped (a stop needs T (1 - alpha) < 1e-4 with alpha <= 0.99,
    so T < 1e-2): its quarter walks the whole list.  Stops: more than half the
    pixels end with T < 1e-3 under dozens of further opaque Gaussians, which
    only the T < 1e-4 stop explains."""
    from gsmpm import raster
    c = _case(dev, "opaque")
    P = c.means.shape[0]
    D_ref, A_ref, _, zmin, zmax = c.ref()
    ctx = raster.SharedContext()
    _, color, radii, depth, alpha = c.forward(depth=True, alpha=True, context=ctx)
    binned, rendered = raster.pair_counts(ctx)
    print(f"opaque scene: binned pairs {binned} (3-sigma {rendered}), 12 tiles; "
          f"pixels with T_final < 1e-3: {(A_ref > 0.999).mean():.2f}, with A < 0.99: {(A_ref < 0.99).mean():.2f}")
    assert binned > 512 * 10 + 2 * P
    for ty in range(3):
        for tx in range(4):
            if tx in (0, 3) or ty in (0, 2):
                assert A_ref[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].min() < 0.99, (tx, ty)
    assert (A_ref > 0.999).mean() > 0.5
    D, A = _check_vs_ref(c, depth, alpha, "opaque")
    assert A.min() >= 0.0 and A.max() <= 1.0
    tol = 1e-3 * zmax
    assert (D >= zmin * A - tol).all() and (D <= zmax * A + tol).all()


@pytest.mark.parametrize("name", ["small", "opaque"])
def test_colour_and_backward_untouched(dev, name):
    """color and radii are bit-identical with and without the maps; on a
    backward-capable context every gradient of raster.backward is too (the
    AUX kernel records the same final T and last contributor)."""
    import torch
    from gsmpm import raster
    c = _case(dev, name)
    _, col0, rad0 = c.forward()
    _, col1, rad1, _, _ = c.forward(depth=True, alpha=True)
    assert torch.equal(col0, col1) and torch.equal(rad0, rad1)
    rng = np.random.default_rng(4)
    wgt = c.t(rng.normal(0, 1, (3, c.H, c.W)).astype(np.float32))
    grads = []
    for on in (False, True):
        ctx = raster.RasterContext()
        out = c.forward(depth=on, alpha=on, context=ctx, return_args=True)
        a, keep = out[-2:]
        assert torch.equal(out[1], col0) and torch.equal(out[2], rad0)
        grads.append(raster.backward(ctx, keep, a, out[2], wgt))
    assert set(grads[0]) == set(grads[1])
    n = 0
    for k, g0 in grads[0].items():
        if g0 is not None:
            assert torch.equal(g0, grads[1][k]), k
            assert bool(g0.abs().sum() > 0) or k in ("scales", "rotations"), k
            n += 1
    assert n >= 6


@pytest.mark.parametrize("name", ["small", "opaque"])
def test_paths_agree(dev, monkeypatch, name):
    """The maps are bit-identical between the context, workspace and async
    forwards, between k_render and k_render4 (GSMPM_RASTER_TILE_SHARED=1),
    with GSMPM_RASTER_XCD=0, and a plane requested alone equals the plane
    requested with the other."""
    import torch
    from gsmpm import raster
    c = _case(dev, name)
    _, col, rad, d_ws, a_ws = c.forward(depth=True, alpha=True)  # gsmpm_raster_forward_ws
    assert bool(torch.isfinite(d_ws).all()) and bool((a_ws > 0).any())
    ctx = raster.RasterContext()
    _, _, _, d_cx, a_cx = c.forward(depth=True, alpha=True, context=ctx)  # gsmpm_raster_forward
    assert torch.equal(d_cx, d_ws) and torch.equal(a_cx, a_ws)
    d_as = torch.full((c.H, c.W), float("nan"), device=dev)
    a_as = torch.full((c.H, c.W), float("nan"), device=dev)
    ar = raster.forward_async(*c.args, **c.kw, ws=raster.Workspace(dev), depth=d_as, alpha=a_as)
    assert ar.result()[1] == 0 and ar.depth is d_as and ar.alpha is a_as
    assert torch.equal(ar.color, col) and torch.equal(d_as, d_ws) and torch.equal(a_as, a_ws)
    # one plane alone
    _, _, _, d_only = c.forward(depth=True)
    _, _, _, a_only = c.forward(alpha=True)
    assert torch.equal(d_only, d_ws) and torch.equal(a_only, a_ws)
    # the row-major grid of quarters
    monkeypatch.setenv("GSMPM_RASTER_XCD", "0")
    _, col_x, _, d_x, a_x = c.forward(depth=True, alpha=True)
    assert torch.equal(col_x, col) and torch.equal(d_x, d_ws) and torch.equal(a_x, a_ws)
    monkeypatch.delenv("GSMPM_RASTER_XCD")
    # k_render4, with every combination of planes
    monkeypatch.setenv("GSMPM_RASTER_TILE_SHARED", "1")
    _, col_4, _, d_4, a_4 = c.forward(depth=True, alpha=True)
    assert torch.equal(col_4, col) and torch.equal(d_4, d_ws) and torch.equal(a_4, a_ws)
    assert torch.equal(c.forward(depth=True)[3], d_ws) and torch.equal(c.forward(alpha=True)[3], a_ws)


def test_edges(dev):
    """No Gaussians, and every Gaussian behind the camera: maps all zero, on
    every form; NaN-filled caller tensors come back fully written, partial
    tiles included (97x61)."""
    import torch
    from gsmpm import raster
    c = _case(dev, "small")
    W, H, t = c.W, c.H, c.t
    nan = lambda: torch.full((H, W), float("nan"), device=dev)
    # P = 0: the Python forward, and the library's async form
    empty = [t(np.zeros((0, 3), np.float32)), t(np.zeros((0, 1), np.float32)), *c.args[2:]]
    ekw = dict(sh_degree=3, shs=t(np.zeros((0, 16, 3), np.float32)), cov3D_precomp=t(np.zeros((0, 6), np.float32)))
    _, col, _, d, a = raster.forward(*empty, **ekw, depth=True, alpha=True)
    assert d.shape == (H, W) and not bool(d.any()) and not bool(a.any())
    d, a = nan(), nan()
    ar = raster.forward_async(*empty, **ekw, ws=raster.Workspace(dev), depth=d, alpha=a)
    assert ar.result() == (0, 0) and not bool(d.any()) and not bool(a.any())
    # every Gaussian behind the camera (K = 0), workspace and context forms
    behind = np.tile(np.array([[0.0, 0.0, -10.0]], np.float32), (10, 1))
    bargs = [t(behind), t(np.ones((10, 1), np.float32)), *c.args[2:]]
    bkw = dict(colors_precomp=t(np.ones((10, 3), np.float32)),
               cov3D_precomp=t(np.tile(np.array([[1e-2, 0, 0, 1e-2, 0, 1e-2]], np.float32), (10, 1))))
    for more in (dict(), dict(context=raster.RasterContext())):
        _, col, rad, d, a = raster.forward(*bargs, **bkw, depth=True, alpha=True, **more)
        assert int(rad.abs().sum()) == 0 and not bool(d.any()) and not bool(a.any())
    # a real frame into NaN-filled tensors: every pixel written
    _, _, _, d_ws, a_ws = c.forward(depth=True, alpha=True)
    d, a = nan(), nan()
    assert raster.forward_async(*c.args, **c.kw, ws=raster.Workspace(dev), depth=d, alpha=a).result()[1] == 0
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(a).all())
    assert torch.equal(d, d_ws) and torch.equal(a, a_ws)
    with pytest.raises(ValueError):
        raster.forward_async(*c.args, **c.kw, ws=raster.Workspace(dev), depth=torch.zeros((W, H), device=dev))


def test_drop_in_returns_four(dev):
    import torch
    from diff_gaussian_rasterization import (GaussianRasterizationSettings, GaussianRasterizer,
                                             rasterize_gaussians)
    c = _case(dev, "small")
    t = c.t
    st = GaussianRasterizationSettings(image_height=c.H, image_width=c.W, tanfovx=c.tx, tanfovy=c.ty, bg=c.args[5],
                                       scale_modifier=1.0, viewmatrix=c.args[2], projmatrix=c.args[3], sh_degree=3,
                                       campos=c.args[4], prefiltered=False, debug=False)
    _, _, _, d_ref, a_ref = c.forward(depth=True, alpha=True)
    # off: exactly two outputs; no grad needed: the workspace form
    out = GaussianRasterizer(st)(means3D=c.args[0], means2D=None, opacities=c.args[1], shs=c.kw["shs"],
                                 cov3D_precomp=c.kw["cov3D_precomp"])
    assert len(out) == 2
    out = GaussianRasterizer(st)(means3D=c.args[0], means2D=None, opacities=c.args[1], shs=c.kw["shs"],
                                 cov3D_precomp=c.kw["cov3D_precomp"], return_depth_alpha=True)
    assert len(out) == 4 and torch.equal(out[2], d_ref) and torch.equal(out[3], a_ref)
    # means3D requires grad: a leased context; the maps stay out of the graph, the colour backward runs
    m3 = c.args[0].clone().requires_grad_(True)
    color, radii, depth, alpha = GaussianRasterizer(st)(means3D=m3, means2D=None, opacities=c.args[1],
                                                        shs=c.kw["shs"], cov3D_precomp=c.kw["cov3D_precomp"],
                                                        return_depth_alpha=True)
    assert color.requires_grad and not depth.requires_grad and not alpha.requires_grad and not radii.requires_grad
    assert torch.equal(depth, d_ref) and torch.equal(alpha, a_ref)
    color.sum().backward()
    g1 = m3.grad.clone()
    m3.grad = None
    color2, _ = GaussianRasterizer(st)(means3D=m3, means2D=None, opacities=c.args[1], shs=c.kw["shs"],
                                       cov3D_precomp=c.kw["cov3D_precomp"])
    color2.sum().backward()
    assert torch.equal(color2, color) and torch.equal(m3.grad, g1) and bool(g1.abs().sum() > 0)
    # upstream's positional signature, then the additions by keyword
    e = torch.Tensor([])
    out = rasterize_gaussians(c.args[0], None, c.kw["shs"], e, c.args[1], e, e, c.kw["cov3D_precomp"], st,
                              return_depth_alpha=True)
    assert len(out) == 4 and torch.equal(out[3], a_ref)
    assert len(rasterize_gaussians(c.args[0], None, c.kw["shs"], e, c.args[1], e, e, c.kw["cov3D_precomp"], st)) == 2


@pytest.fixture(scope="module")
def driver_runs(dev, tmp_path_factory):
    """main.py on lego.json (5,000 synthetic Gaussians, 64^3, one frame), once
    without and once with --save_alpha --save_depth: the two output paths."""
    import main as drv
    from scenarios import CONFIGS
    base = ["--config_path", os.path.join(CONFIGS, "lego.json"), "--synthetic", "5000", "--n_grid", "64",
            "--num_frames", "1"]
    root = tmp_path_factory.mktemp("aux_driver")
    plain, matte = str(root / "plain"), str(root / "matte")
    drv.main(base + ["--output_path", plain])
    drv.main(base + ["--output_path", matte, "--save_alpha", "--save_depth"])
    return plain, matte


def _frames(driver_runs):
    from PIL import Image
    plain, matte = driver_runs
    for f in range(2):
        yield (f, np.asarray(Image.open(os.path.join(plain, "images", f"{f:04d}.png"))),
               np.asarray(Image.open(os.path.join(matte, "images", f"{f:04d}.png"))),
               os.path.join(matte, "depth", f"{f:04d}.npy"))


def test_main_py_rgba_frames_and_depth(driver_runs):
    """main.py --save_alpha --save_depth: RGBA PNGs whose RGB planes are the
    PNGs of the same run without the flags, and depth/%04d.npy, f32 [H,W],
    finite, zero exactly where A < 1/255.  The cut is taken on the float alpha
    (exactly so: test_frame_writer_planes); the PNG's A plane is that alpha
    rounded to nearest, so level 0 lies below the cut, levels >= 2 above it and
    level 1 ([0.5/255, 1.5/255)) straddles it."""
    assert not os.path.exists(os.path.join(driver_runs[0], "depth"))
    for f, rgb, rgba, dpath in _frames(driver_runs):
        assert rgb.shape == (800, 800, 3) and rgba.shape == (800, 800, 4) and rgba.dtype == np.uint8
        assert np.array_equal(rgba[..., :3], rgb)
        A8 = rgba[..., 3]
        depth = np.load(dpath)
        assert depth.dtype == np.float32 and depth.shape == (800, 800) and np.isfinite(depth).all()
        assert (depth[A8 == 0] == 0).all() and (depth[A8 >= 2] > 0).all()
        assert (depth >= 0).all() and depth[depth > 0].min() > 0.2  # a view depth in front of the near cut


def test_main_py_alpha_plane_spans_0_to_255(driver_runs):
    """The A plane is non-trivial: both 0 and 255 occur.  A = 1 - T_final never
    exceeds 0.9999 (the blend stops before T falls below 1e-4), so 255 occurs
    only because main.alpha8 rounds to nearest where to8b would truncate
    254.97 to 254."""
    for f, _, rgba, _ in _frames(driver_runs):
        A8 = rgba[..., 3]
        print(f"frame {f}: A plane min {A8.min()} max {A8.max()}, "
              f"pixels at 0: {(A8 == 0).mean():.3f}, at 255: {(A8 == 255).mean():.3f}")
        assert (A8 == 0).any() and (A8 == 255).any()


def test_frame_writer_planes(dev, tmp_path):
    """FrameWriter's extra planes on hand-made tensors: RGB stays to8b's
    truncation, A is rounded to nearest (0.9999, a stopped pixel, is 255), and
    the depth file holds D / A exactly where the float alpha >= 1/255, else 0."""
    import torch
    from PIL import Image

    import main as drv
    from utils.render_utils import to8b
    cut = np.float32(1.0 / 255.0)
    a = np.array([[0.0, 0.4 / 255, 0.6 / 255, np.nextafter(cut, np.float32(0))],
                  [cut, 0.5, 0.9999, 1.0]], np.float32)
    d = (np.float32(3.0) * a + np.float32(0.25)).astype(np.float32)  # nonzero everywhere: only the cut zeroes it
    rng = np.random.default_rng(0)
    img = rng.uniform(-0.1, 1.1, (3, 2, 4)).astype(np.float32)
    img[0, 0, 0] = 0.9999
    t = lambda x: torch.from_numpy(x).to(dev)
    (tmp_path / "depth").mkdir()
    seq = []
    w = drv.FrameWriter(str(tmp_path), seq, workers=1, save_alpha=True, depth_path=str(tmp_path / "depth"))
    w.submit(t(img), 7, t(d), t(a))
    w.close()
    rgba = np.asarray(Image.open(tmp_path / "0007.png"))
    assert rgba.shape == (2, 4, 4) and rgba.dtype == np.uint8
    assert np.array_equal(rgba[..., :3], to8b(img.transpose(1, 2, 0))) and rgba[0, 0, 0] == 254
    assert rgba[..., 3].tolist() == [[0, 0, 1, 1], [1, 128, 255, 255]]
    depth = np.load(tmp_path / "depth" / "0007.npy")
    assert depth.dtype == np.float32 and depth.shape == (2, 4)
    assert np.array_equal(depth[0], np.zeros(4, np.float32))  # every alpha of row 0 is below the cut
    assert np.array_equal(depth[1], d[1] / a[1])
    assert np.array_equal(seq[0], img.transpose(1, 2, 0))
    # without the flags: an RGB file, the same bytes in its planes, no depth
    w = drv.FrameWriter(str(tmp_path), [], workers=1)
    w.submit(t(img), 8)
    w.close()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "0008.png")), rgba[..., :3])
