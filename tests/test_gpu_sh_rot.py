"""sh_rotations on the GPU: the rasterizer evaluates each Gaussian's SH at
Q d instead of the view direction d (include/gsmpm.h), forward and backward,
in all three forward forms; gsmpm_mpm_sh_rotations hands out the Q that
belongs to the last postprocess; main.py --rotate_sh joins the two.

Reference: tests/sh_rot_ref.py (float64 colours + the oracle rasterizer),
pinned against all-float64 autograd in test_sh_rot_ref.py.
Bounds: 1e-3 absolute on pixels (the project's pixel bound, test_gpu_raster.py);
gradients under test_gpu_raster_bwd._close as it stands.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG, rel_err
from sh_rot_ref import backward_ref, forward_ref, random_rotations
from test_gpu_raster import _camera, _scene
from test_gpu_raster_bwd import _close

pytestmark = pytest.mark.gpu


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rot32(rng, n):
    return random_rotations(rng, n).astype(np.float32)


@pytest.mark.parametrize("P,W,H,D", [(2000, 200, 200, 3), (1500, 160, 112, 1), (300, 48, 32, 2)])
def test_forward_vs_reference(dev, P, W, H, D):
    """Random proper rotations per Gaussian: the image within 1e-3 of the
    reference; radii and num_rendered equal to the run without rotations (and
    to the oracle's), because the geometry is untouched."""
    from gsmpm import raster
    means, c6, opa, shs = _scene(P, seed=P + W)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    bgv = np.full(3, 0.2, np.float32)
    Q = _rot32(np.random.default_rng(P + D), P)
    img, orad, oK = forward_ref(means, opa, view, full, campos, bgv, W, H, tx, ty, shs, D, Q, cov3D_precomp=c6)
    t = _t(dev)
    args = (t(means), t(opa), t(view), t(full), t(campos), t(bgv), H, W, tx, ty)
    kw = dict(sh_degree=D, shs=t(shs), cov3D_precomp=t(c6))
    K0, c0, r0 = raster.forward(*args, **kw)
    K1, c1, r1 = raster.forward(*args, **kw, sh_rotations=t(Q))
    assert K1 == K0 == oK and torch.equal(r1, r0) and np.array_equal(r1.cpu().numpy(), orad)
    err = np.abs(c1.cpu().numpy() - img)
    print(f"sh_rot forward P {P} D {D}: max err {err.max():.2e}; rotated vs unrotated {float((c1 - c0).abs().max()):.2e}")
    assert err.max() < 1e-3, (err.max(), int((err > 1e-3).sum()))
    assert float((c1 - c0).abs().max()) > 1e-2  # the rotations do change the picture
    # [P,9] is the same input
    _, c2, _ = raster.forward(*args, **kw, sh_rotations=t(Q.reshape(P, 9)))
    assert torch.equal(c2, c1)


def test_identity_is_bit_equal_and_degree_zero_ignores_it(dev):
    """Q = I: the multiplications by 1 and 0 are exact, so the image is
    torch.equal to sh_rotations=None (the rotated direction feeds the same
    arithmetic).  With sh_degree 0 any Q is accepted and changes nothing; with
    colors_precomp it is refused."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gsmpm import _lib, raster
    P, W, H = 2000, 200, 200
    means, c6, opa, shs = _scene(P, seed=17)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    t = _t(dev)
    eye = torch.eye(3, device=dev).repeat(P, 1, 1)
    Q = t(_rot32(np.random.default_rng(1), P))
    for D in (3, 0):
        st = GaussianRasterizationSettings(H, W, tx, ty, t(np.zeros(3, np.float32)), 1.0, t(view), t(full), D,
                                           t(campos), False, False)
        inp = dict(means3D=t(means), means2D=None, opacities=t(opa), shs=t(shs), cov3D_precomp=t(c6))
        c0, r0 = GaussianRasterizer(st)(**inp)
        c1, r1 = GaussianRasterizer(st)(**inp, sh_rotations=eye if D else Q)
        assert torch.equal(c1, c0) and torch.equal(r1, r0), D
    with pytest.raises(_lib.GsmpmError, match="sh_rotations needs shs"):
        raster.forward(t(means), t(opa), t(view), t(full), t(campos), t(np.zeros(3, np.float32)), H, W, tx, ty,
                       colors_precomp=t(np.ones((P, 3), np.float32)), cov3D_precomp=t(c6), sh_rotations=eye)


# rigid-motion scene: D = 3 and rest coefficients of order 1, so the unrotated render of the
# turned scene is far from the original; seed and G checked on the CPU with the reference
# (sh_rot_ref.forward_ref: turned + Q = G^T within 5.9e-6 of the original, every radius equal;
# turned without Q off by 2.5 where the image's largest value is 2.7)
def _rigid_scene():
    P, W, H = 1200, 160, 128
    means, c6, opa, shs = _scene(P, seed=4242)
    rng = np.random.default_rng(99)
    shs[:, 1:] = rng.normal(0, 1.0, size=(P, 15, 3)).astype(np.float32)
    G = random_rotations(rng, 1)[0]
    return P, W, H, means, c6, opa, shs, G


def _turned(means, c6, view, full, campos, G):
    """Everything carried through the proper rotation G (float64, then f32)."""
    S = np.zeros((len(c6), 3, 3))
    iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for k, (i, j) in enumerate(iu):
        S[:, i, j] = S[:, j, i] = c6[:, k]
    S2 = G @ S @ G.T
    c6g = np.stack([S2[:, i, j] for i, j in iu], 1).astype(np.float32)
    G4 = np.eye(4)
    G4[:3, :3] = G
    # row-vector matrices: [G m, 1] (G4 V) = [m, 1] V
    return ((means.astype(np.float64) @ G.T).astype(np.float32), c6g, (G4 @ view.astype(np.float64)).astype(np.float32),
            (G4 @ full.astype(np.float64)).astype(np.float32), (G @ campos.astype(np.float64)).astype(np.float32))


def test_rigid_motion_invariance(dev):
    """Turn the whole world (Gaussians, covariances, camera) by a proper G and
    shade with Q = G^T: the picture is the original's within 1e-3.  Without
    sh_rotations the turned scene's colours are taken at the wrong directions
    and the picture is off by more than 1e-2 somewhere."""
    from gsmpm import raster
    P, W, H, means, c6, opa, shs, G = _rigid_scene()
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    mg, cg, vg, fg, pg = _turned(means, c6, view, full, campos, G)
    t = _t(dev)
    bg = t(np.full(3, 0.1, np.float32))
    kw = dict(sh_degree=3, shs=t(shs))
    _, c0, r0 = raster.forward(t(means), t(opa), t(view), t(full), t(campos), bg, H, W, tx, ty, cov3D_precomp=t(c6),
                               **kw)
    turned = (t(mg), t(opa), t(vg), t(fg), t(pg), bg, H, W, tx, ty)
    Q = t(np.tile(G.T.astype(np.float32), (P, 1, 1)))
    _, c1, r1 = raster.forward(*turned, cov3D_precomp=t(cg), **kw, sh_rotations=Q)
    _, c2, _ = raster.forward(*turned, cov3D_precomp=t(cg), **kw)
    same, off = float((c1 - c0).abs().max()), float((c2 - c0).abs().max())
    print(f"rigid motion: with Q = G^T {same:.2e}, without {off:.2e}; radii differing {int((r1 != r0).sum())}")
    assert int((r0 > 0).sum()) > P // 2
    assert same < 1e-3
    assert off > 1e-2


@pytest.mark.parametrize("P,W,H,D,mode", [(2000, 200, 200, 3, "cov"), (1500, 160, 160, 1, "sr")])
def test_backward_vs_reference(dev, P, W, H, D, mode):
    """Gradients of means3D, sh, opacity, cov3D or scales / rotations, means2D
    and sh_rotations against the reference, under test_gpu_raster_bwd._close
    (2e-4 of the max; <= 0.1 % of entries beyond 1e-3, <= 0.01 % beyond 1e-2),
    and exact zeros in dL/dQ for culled Gaussians (seven are put behind the
    camera; the frustum culls more).
    Measured on an MI355X (GSMPM_PRINT_ERRS=1), max error over the output's max:
      (2000, 200 x 200, D 3, cov): means3D 4.4e-7, opacity 4.1e-7, means2D 4.7e-7,
        sh 1.2e-6, sh_rotations 9.3e-7, cov3D 2.7e-5; no entry beyond 1e-3.
      (1500, 160 x 160, D 1, sr): means3D 3.2e-6, opacity 5.2e-6, means2D 1.8e-6,
        sh 1.6e-6, sh_rotations 1.8e-6, scales 4.0e-6, rotations 4.8e-6; 0.02 % of
        the means3D, scales and rotations entries beyond 1e-3, none beyond 1e-2."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    means, c6, opa, shs = _scene(P, seed=P + W + D)
    means[:7, 2] = -10.0  # behind the camera: culled
    rng = np.random.default_rng(P)
    scales = np.exp(rng.normal(-3.2, 0.4, (P, 3))).astype(np.float32)
    rots = rng.normal(0, 1, (P, 4)).astype(np.float32)
    Q = _rot32(rng, P)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    bgv = np.full(3, 0.25, np.float32)
    wgt = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    t = lambda a, g=True: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=t(bgv, False),
                                       scale_modifier=1.0, viewmatrix=t(view, False), projmatrix=t(full, False),
                                       sh_degree=D, campos=t(campos, False), prefiltered=False, debug=False)
    inp = {"means3D": t(means), "means2D": torch.zeros(P, 3, device=dev, requires_grad=True), "opacities": t(opa),
           "shs": t(shs), "sh_rotations": t(Q)}
    if mode == "sr":
        inp["scales"], inp["rotations"] = t(scales), t(rots)
        okw = dict(scales=scales, rotations=rots)
    else:
        inp["cov3D_precomp"] = t(c6)
        okw = dict(cov3D_precomp=c6)
    img, radii = GaussianRasterizer(st)(**inp)
    (img * t(wgt, False)).sum().backward()
    ref = backward_ref(wgt, means, opa, view, full, campos, bgv, W, H, tx, ty, shs, D, Q, **okw)
    pairs = [("means3D", inp["means3D"].grad), ("opacity", inp["opacities"].grad.view(-1)),
             ("means2D", inp["means2D"].grad), ("sh", inp["shs"].grad), ("sh_rotations", inp["sh_rotations"].grad)]
    pairs += [("scales", inp["scales"].grad), ("rotations", inp["rotations"].grad)] if mode == "sr" else \
        [("cov3D", inp["cov3D_precomp"].grad)]
    worst = {}
    for k, g in pairs:
        assert g is not None, k
        worst[k] = rel_err(g.cpu().numpy().reshape(np.shape(ref[k])), ref[k])
    print(f"sh_rot backward P {P} D {D} {mode}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, g in pairs:
        _close(g.cpu().numpy(), ref[k], k)
    culled = (radii == 0).cpu().numpy()
    gq = inp["sh_rotations"].grad.cpu().numpy()
    assert gq.shape == (P, 3, 3)
    assert culled[:7].all() and culled.sum() >= 7
    assert not gq[culled].any() and np.abs(gq[~culled]).max() > 0
    assert np.isfinite(gq).all()


def test_all_three_forward_forms(dev):
    """forward_ws and forward_async with sh_rotations equal the context forward
    bit for bit (they share k_preprocess), and differ from the unrotated one."""
    from gsmpm import raster
    P, W, H = 3000, 256, 192
    means, c6, opa, shs = _scene(P, seed=P + 1)
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    t = _t(dev)
    args = (t(means), t(opa), t(view), t(full), t(campos), t(np.zeros(3, np.float32)), H, W, tx, ty)
    kw = dict(sh_degree=3, shs=t(shs), cov3D_precomp=t(c6), sh_rotations=t(_rot32(np.random.default_rng(2), P)))
    ctx = raster.RasterContext()
    K0, c0, r0 = raster.forward(*args, **kw, context=ctx)
    binned, _ = raster.pair_counts(ctx)
    ws = raster.Workspace(dev)
    K1, c1, r1 = raster.forward(*args, **kw, ws=ws)
    assert K1 == K0 and torch.equal(r1, r0) and torch.equal(c1, c0)
    ar = raster.forward_async(*args, **kw, pairs_cap=binned + binned // 4 + 64, ws=ws)
    nr, flags = ar.result()
    assert flags == 0 and nr == K0
    assert torch.equal(ar.radii, r0) and torch.equal(ar.color, c0)
    plain = dict(kw, sh_rotations=None)
    assert not torch.equal(raster.forward(*args, **plain, ws=ws)[1], c0)


def test_mpm_sh_rotations(dev):
    """gsmpm_mpm_sh_rotations on N = 500, n_grid 32, F_trial = G_p S_p (G_p
    random proper rotations, S_p SPD with eigenvalues in [0.7, 1.4]):
    GSMPM_ESTATE before the first postprocess; A = NULL is bit-equal to
    gsmpm_mpm_get(GSMPM_FIELD_R) and is G_p^T (particle_R = R^T) within 1e-4
    of the max, the particle_R parity bound of test_gpu_mpm.py (TOL) and
    test_gpu_goldens.py; a random proper A gives A R A^T within 5e-6 absolute
    of the float64 product of the readback (two chained 3-term dot products of
    entries <= 1 in f32, under 1e-6 each, with slack)."""
    from gsmpm import _lib
    from gsmpm.sim import Simulator
    n = 500
    rng = np.random.default_rng(12)
    x = rng.uniform(0.6, 1.4, size=(n, 3)).astype(np.float32)
    cov = np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32), (n, 1))
    vol = np.full(n, 1e-5, np.float32)
    sim = Simulator(n, n_grid=32, grid_extent=2.0, material="jelly", E=2e5, nu=0.3, density=200.0, gravity=(0, 0, 0),
                    device=dev)
    t = _t(dev)
    sim.set_particles(t(x), t(cov), t(vol))
    out = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    rc = _lib.LIB.gsmpm_mpm_sh_rotations(sim._h, None, _lib.ptr(out), _lib.stream_of(dev))
    assert rc == _lib.GSMPM_ESTATE and "postprocess" in _lib.last_error()
    G = random_rotations(rng, n)
    U = random_rotations(rng, n)
    lam = rng.uniform(0.7, 1.4, size=(n, 3))
    S = U @ (lam[:, :, None] * U.transpose(0, 2, 1))
    sim.set("F_trial", t((G @ S).astype(np.float32).reshape(n, 9)))
    sim.postprocess()
    R = sim.get("R").reshape(n, 3, 3)
    Q = sim.sh_rotations()
    assert Q.shape == (n, 3, 3) and torch.equal(Q, R)
    e = rel_err(Q.cpu().numpy(), G.transpose(0, 2, 1))
    A = random_rotations(rng, 1)[0].astype(np.float32)
    QA = sim.sh_rotations(A).cpu().numpy()
    A64 = A.astype(np.float64)
    want = A64 @ R.cpu().numpy().astype(np.float64) @ A64.T
    ea = np.abs(QA - want).max()
    print(f"mpm sh_rotations: particle_R vs G^T {e:.2e}; A R A^T abs err {ea:.2e}")
    assert e < 1e-4
    assert ea < 5e-6
    # a new particle set has no particle_R until its own postprocess
    sim.set_particles(t(x), t(cov), t(vol))
    assert _lib.LIB.gsmpm_mpm_sh_rotations(sim._h, None, _lib.ptr(out), _lib.stream_of(dev)) == _lib.GSMPM_ESTATE
    torch.cuda.synchronize()
    # a slab of a multi-GPU domain is refused with a message
    slab = Simulator(n, n_grid=32, grid_extent=2.0, material="jelly", E=2e5, nu=0.3, density=200.0, gravity=(0, 0, 0),
                     device=dev)
    slab.slab_init(0, 1, 0, 32)
    assert _lib.LIB.gsmpm_mpm_sh_rotations(slab._h, None, _lib.ptr(out), _lib.stream_of(dev)) == _lib.GSMPM_ESTATE
    assert "slab" in _lib.last_error()


def test_main_py_rotate_sh(dev, tmp_path, monkeypatch):
    """main.py on a tiny spin scene (lego-spin.json's set-up with a stronger
    impulse, so that three frames already turn the Gaussians by a degree or
    more; 3,000 synthetic Gaussians) with and without --rotate_sh: frame 0 is
    identical (no postprocess yet: None is passed), the last frame's positions
    and covariances are bit-identical (the feature touches colour only), and
    the last images differ by more than 1e-3 somewhere.
    n_grid is 64, as in test_gpu_main_e2e.py, not 32: at 32 these Gaussians
    put ~375 particles into a tile, and a tile of more than one 256-particle
    chunk makes the simulation's float sums depend on the binning atomics'
    order (test_gpu_mpm.py::test_fused_single_chunk_deterministic), so two
    runs of the same command differ in the last bits with or without the
    flag; at 64 every tile is one chunk and a run is reproducible, which is
    what the bit-equality of the positions needs."""
    import main as drv
    with open(os.path.join(PKG, "configs", "lego-spin.json")) as f:
        cfg = json.load(f)
    imp = cfg["mpm"]["boundary_conditions"][0]
    imp["force"], imp["num_dt"] = [-6.0, 0.0, 0.0], 25
    cfg["render"]["rotate_sh"] = False
    path = str(tmp_path / "spin.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    orig = drv.render_frame
    runs = {}
    for flag in ([], ["--rotate_sh"]):
        rec = []

        def spy(*a, **k):
            img = orig(*a, **k)
            rec.append((a[3].clone(), a[4].clone(), img.clone(), k.get("sh_rotations")))
            return img
        monkeypatch.setattr(drv, "render_frame", spy)
        out = str(tmp_path / ("on" if flag else "off"))
        drv.main(["--config_path", path, "--synthetic", "3000", "--n_grid", "64", "--num_frames", "3",
                  "--output_path", out] + flag)
        assert len(rec) == 4 and all(os.path.exists(os.path.join(out, "images", f"{f:04d}.png")) for f in range(4))
        runs[bool(flag)] = rec
    off, on = runs[False], runs[True]
    assert all(r[3] is None for r in off) and on[0][3] is None and all(r[3] is not None for r in on[1:])
    assert torch.equal(on[0][2], off[0][2])
    assert torch.equal(on[-1][0], off[-1][0]) and torch.equal(on[-1][1], off[-1][1])
    eye = torch.eye(3, device=dev)
    turn = float((on[-1][3] - eye).abs().amax(dim=(1, 2)).median())
    diff = float((on[-1][2] - off[-1][2]).abs().max())
    print(f"main.py --rotate_sh: last frame image diff {diff:.2e}; median |particle_R - I| {turn:.2e}")
    assert torch.isfinite(on[-1][0]).all()
    assert diff > 1e-3
