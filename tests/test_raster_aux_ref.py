"""Pins the reference of the rasterizer's depth and alpha maps (CPU only).

tests/raster_aux_ref.py reads D and A off an oracle render with colours
(z_i, 1, 0).  Here that construction is held against the float64 rasterizer
of tests/raster_torch_ref.py fed the same colours, and against a case with a
known answer.  The measured distance is printed: the GPU bounds of
test_gpu_raster_aux.py (1e-3 on A, 1e-3 z_max on D) rest on the reference
being far inside them.

Bound of the float64 comparison, 1e-5 on A and 1e-5 z_max on D: the oracle
blends in f32 (unit roundoff 6e-8); a pixel here sums at most ~60
contributions whose alpha and T each carry a few roundings of the conic, the
exponential and the running product, so ~60 x 4 x 6e-8 = 1.4e-5 is a ceiling
no pixel approaches (errors do not all align), and the bound is 100 times
tighter than what the GPU tests allow.  A contribution sitting on the 1/255
or T < 1e-4 threshold in one precision and not the other would show as ~4e-3;
the seed below has none.
"""
from __future__ import annotations

import math

import numpy as np

import raster_aux_ref as AR


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


def test_args_struct_carries_the_map_pointers():
    """gsmpm_raster_args ends ..., sh_rotations, aux_depth, aux_alpha (include/gsmpm.h)."""
    import ctypes

    from gsmpm import _lib
    names = [f[0] for f in _lib.RasterArgs._fields_]
    assert names[-3:] == ["sh_rotations", "aux_depth", "aux_alpha"]
    assert _lib.RasterArgs.aux_depth.offset == _lib.RasterArgs.sh_rotations.offset + ctypes.sizeof(ctypes.c_void_p)
    a = _lib.RasterArgs()
    assert a.aux_depth is None and a.aux_alpha is None  # off by default


def test_view_depth_is_the_oracles_depth():
    """z_i formed on the host equals the per-Gaussian depth the oracle's preprocess returns."""
    import oracle as O
    rng = np.random.default_rng(5)
    P, W, H = 60, 24, 20
    means = rng.uniform(-0.8, 0.8, size=(P, 3)).astype(np.float32)
    c6 = np.tile(np.array([4e-3, 0, 0, 4e-3, 0, 4e-3], np.float32), (P, 1))
    opa = rng.uniform(0.1, 0.9, size=(P, 1)).astype(np.float32)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    _, radii, _, depth, _ = O.raster_forward(means, opa, view, full, campos, np.zeros(3, np.float32), W, H, tx, ty,
                                             colors_precomp=np.zeros((P, 3), np.float32), cov3D_precomp=c6)
    z = AR.view_depth(means, view)
    vis = radii > 0
    assert vis.sum() > P // 2
    err = np.abs(z[vis] - depth[vis]).max()
    print(f"host view depth vs oracle depth: max abs {err:.2e} (z up to {z.max():.2f})")
    assert err <= 4 * np.finfo(np.float32).eps * z.max()  # the same three products and sums, in either order


def test_reference_vs_float64():
    import torch

    import raster_torch_ref as TR
    rng = np.random.default_rng(11)
    P, W, H = 60, 24, 20
    means = rng.uniform(-0.8, 0.8, size=(P, 3)).astype(np.float32)
    A = rng.normal(0, 1, size=(P, 3, 3)) * 0.12
    cov = A @ A.transpose(0, 2, 1) + np.eye(3) * 1e-3
    c6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]],
                  1).astype(np.float32)
    opa = rng.uniform(0.05, 0.99, size=(P, 1)).astype(np.float32)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    D, Am, radii, z = AR.forward(means, opa, view, full, campos, W, H, tx, ty, cov3D_precomp=c6)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    inp = dict(means3D=d(means), opacities=d(opa), viewmatrix=d(view), projmatrix=d(full), campos=d(campos),
               bg=d(np.zeros(3)), colors_precomp=d(AR.aux_colors(means, view)), cov3D_precomp=d(c6))
    inp["means3D"].requires_grad_(True)  # the float64 rasterizer keeps ndc's gradient
    img, _, rad64, _ = TR.forward(inp, W, H, tx, ty, D=0)
    img = img.detach().numpy()
    assert np.array_equal(np.asarray(rad64), radii)
    zmax = float(z[radii > 0].max())
    eD, eA = np.abs(D - img[0]).max(), np.abs(Am - img[1]).max()
    print(f"aux reference (oracle, f32) vs f64: |dD| {eD:.2e} (z_max {zmax:.2f}: {eD / zmax:.2e} relative) "
          f"|dA| {eA:.2e}; A in [{Am.min():.3f}, {Am.max():.3f}], covered pixels {(Am > 0).mean():.2f}")
    assert (Am > 0.5).sum() > 50  # a scene that exercises the blend
    assert np.abs(img[2]).max() == 0
    assert eA < 1e-5 and eD < 1e-5 * zmax


def test_known_answer_single_gaussian():
    """One isotropic Gaussian whose centre projects exactly onto a pixel centre:
    there G = 1, so alpha = min(0.99, o), T = 1: A = alpha and D = z alpha."""
    W, H, t, dist = 24, 20, 0.5, 3.0
    ty = t * H / W
    view = np.eye(4, dtype=np.float32)
    view[3, 2] = dist
    proj = np.array([[1 / t, 0, 0, 0], [0, 1 / ty, 0, 0], [0, 0, 100 / 99.99, 1], [0, 0, -1 / 99.99, 0]], np.float32)
    full = view @ proj
    kx, ky = 9, 6  # the pixel
    zw = 0.25      # world z: view depth 3.25
    z = dist + zw
    x = ((2 * kx + 1) / W - 1) * z * t
    y = ((2 * ky + 1) / H - 1) * z * ty
    means = np.array([[x, y, zw]], np.float32)
    c6 = np.array([[2e-3, 0, 0, 2e-3, 0, 2e-3]], np.float32)
    for o in (0.6, 1.0, 0.05):
        D, A, radii, zv = AR.forward(means, np.array([[o]], np.float32), view, full, np.zeros(3, np.float32), W, H,
                                     t, ty, cov3D_precomp=c6)
        assert radii[0] > 0 and abs(zv[0] - z) < 1e-6
        want = min(0.99, o)
        print(f"known answer o={o}: A {A[ky, kx]:.7f} (want {want}), D {D[ky, kx]:.7f} (want {z * want:.7f})")
        assert abs(A[ky, kx] - want) < 1e-6
        assert abs(D[ky, kx] - z * want) < 1e-6 * z
        assert A.argmax() == ky * W + kx  # the peak is that pixel
        assert (A >= 0).all() and A[0, 0] == 0 and D[0, 0] == 0  # a pixel nothing reaches
