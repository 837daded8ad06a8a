"""sh_rotations without a GPU: the float64 reference (tests/sh_rot_ref.py) is
pinned before the GPU tests lean on it, two closed-form properties of
"evaluate the SH at Q d" are checked, and the C ABI refuses what it must
before touching a device.
"""
from __future__ import annotations

import ctypes
import json
import os
from argparse import ArgumentParser

import numpy as np
import torch

from conftest import PKG, rel_err
from raster_torch_ref import SH_C0, SH_C1, _sh
from sh_rot_ref import backward_ref, random_rotations, rotated_rgb, view_dirs


def test_composed_backward_reference_matches_float64_autograd():
    """The reference backward (oracle backward on the rotated colours + autograd
    of the colour alone) against autograd through the whole float64 forward
    (raster_torch_ref.forward fed the rotated rgb as colors_precomp), P = 40,
    32 x 32, D = 3.  Bound: 2e-3 of each output's max, the bound
    test_oracle_raster_bwd.py holds the f32 oracle's backward to."""
    import oracle as O
    from raster_torch_ref import forward
    from test_oracle_raster_bwd import _camera, _scene
    P, W, H, D = 40, 32, 32, 3
    means, c6, opa, shs, _, _ = _scene(P, seed=7)
    view, full, campos, tx, ty = _camera(W, H, 1.0)
    rng = np.random.default_rng(8)
    Q = random_rotations(rng, P)
    bgv = np.full(3, 0.3, np.float32)
    wgt = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    ref = backward_ref(wgt, means, opa, view, full, campos, bgv, W, H, tx, ty, shs, D, Q, cov3D_precomp=c6)

    d = lambda a, g=True: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    lv = {"means3D": d(means), "opacities": d(opa), "cov3D_precomp": d(c6), "shs": d(shs), "Q": d(Q)}
    cp = d(campos, False)
    rgb = rotated_rgb(D, lv["shs"], lv["means3D"], cp, lv["Q"])
    inp = {"means3D": lv["means3D"], "opacities": lv["opacities"], "cov3D_precomp": lv["cov3D_precomp"],
           "colors_precomp": rgb, "viewmatrix": d(view, False), "projmatrix": d(full, False), "campos": cp,
           "bg": d(bgv, False)}
    img, _, radii, _ = forward(inp, W, H, tx, ty, D=D)
    _, radii32, _, _, _ = O.raster_forward(means, opa, view, full, campos, bgv, W, H, tx, ty,
                                           colors_precomp=rgb.detach().numpy().astype(np.float32), cov3D_precomp=c6)
    assert np.array_equal(radii, radii32), "f64 reference made different culling decisions"
    assert (radii32 > 0).sum() > P // 2
    (img * torch.from_numpy(wgt.astype(np.float64))).sum().backward()
    errs = {k: rel_err(ref[k], g.grad.numpy().reshape(np.shape(ref[k]))) for k, g in
            (("means3D", lv["means3D"]), ("opacity", lv["opacities"]), ("cov3D", lv["cov3D_precomp"]),
             ("sh", lv["shs"]), ("sh_rotations", lv["Q"]))}
    assert np.abs(ref["sh_rotations"]).max() > 0
    assert all(e < 2e-3 for e in errs.values()), errs


def test_degree_one_closed_form():
    """Band 1 is linear in the direction: with b(d) = (-y, z, -x) = B d,
    b(Q d) = (B Q B^T) b(d), so _sh at Q d equals _sh at d with each channel's
    band-1 coefficient triple s replaced by M^T s, where
        M = B Q B^T = [[ Q11, -Q12,  Q10],
                       [-Q21,  Q22, -Q20],
                       [ Q01, -Q02,  Q00]]."""
    rng = np.random.default_rng(3)
    P = 64
    Q = torch.from_numpy(rng.normal(size=(P, 3, 3)))  # any matrix: the caller owns Q
    shs = torch.from_numpy(rng.normal(0, 0.4, size=(P, 4, 3)))
    d = torch.from_numpy(rng.normal(size=(P, 3)))
    d = d / d.norm(dim=1, keepdim=True)
    M = torch.stack([torch.stack([Q[:, 1, 1], -Q[:, 1, 2], Q[:, 1, 0]], 1),
                     torch.stack([-Q[:, 2, 1], Q[:, 2, 2], -Q[:, 2, 0]], 1),
                     torch.stack([Q[:, 0, 1], -Q[:, 0, 2], Q[:, 0, 0]], 1)], 1)
    shs2 = shs.clone()
    shs2[:, 1:4] = M.transpose(1, 2) @ shs[:, 1:4]
    lhs = _sh(1, shs, (Q @ d[:, :, None])[..., 0])
    rhs = _sh(1, shs2, d)
    assert torch.allclose(lhs, rhs, rtol=0, atol=1e-13)
    # and written out: 0.5 + C0 s0 + C1 s_1..3 . b(Q d)
    bq = torch.stack([-(Q @ d[:, :, None])[:, 1, 0], (Q @ d[:, :, None])[:, 2, 0], -(Q @ d[:, :, None])[:, 0, 0]], 1)
    direct = 0.5 + SH_C0 * shs[:, 0] + SH_C1 * (bq[:, :, None] * shs[:, 1:4]).sum(1)
    assert torch.allclose(lhs, direct, rtol=0, atol=1e-13)


def test_rotating_the_view_and_counter_rotating_q_changes_nothing():
    """f(shs, G d, Q = G^T) == f(shs, d, I) for a proper rotation G, every degree."""
    rng = np.random.default_rng(5)
    P = 50
    G = torch.from_numpy(random_rotations(rng, 1)[0])
    assert abs(float(torch.linalg.det(G)) - 1.0) < 1e-12
    means = torch.from_numpy(rng.uniform(-1, 1, size=(P, 3)))
    campos = torch.from_numpy(np.array([0.3, -0.2, 3.0]))
    shs = torch.from_numpy(rng.normal(0, 0.4, size=(P, 16, 3)))
    eye = torch.eye(3, dtype=torch.float64).expand(P, 3, 3)
    assert torch.allclose(view_dirs(means @ G.T, G @ campos), view_dirs(means, campos) @ G.T, atol=1e-14)
    for D in range(4):
        a = rotated_rgb(D, shs, means @ G.T, G @ campos, G.T.expand(P, 3, 3))
        b = rotated_rgb(D, shs, means, campos, eye)
        assert torch.allclose(a, b, rtol=0, atol=1e-13), D
        if D > 0:  # and the rotation matters: the unrotated colours of the turned scene differ
            c = rotated_rgb(D, shs, means @ G.T, G @ campos, eye)
            assert (c - b).abs().max() > 1e-2


def test_sh_rotations_with_colors_precomp_is_refused_before_any_device_call():
    """gsmpm_raster_forward_ws with sh_rotations and colors_precomp both set:
    GSMPM_EINVAL "sh_rotations needs shs", like the other argument checks of
    test_raster_workspace_entry_points_validate_without_a_gpu (fake pointers:
    nothing is dereferenced, no HIP call is made)."""
    from gsmpm import _lib
    a = _lib.RasterArgs()
    a.P, a.W, a.H = 10, 64, 64
    a.colors_precomp = 0x2000
    a.sh_rotations = 0x3000
    need, nr = ctypes.c_int64(0), ctypes.c_int32(0)
    rc = _lib.LIB.gsmpm_raster_forward_ws(ctypes.byref(a), None, None, ctypes.byref(nr), 0x1000, 1 << 20,
                                          ctypes.byref(need), None)
    assert rc == _lib.GSMPM_EINVAL
    assert "sh_rotations needs shs" in _lib.last_error()
    cnt = (ctypes.c_uint32 * 4)()
    rc = _lib.LIB.gsmpm_raster_forward_async(ctypes.byref(a), 0x4000, 0x5000, 0x1000, 1 << 20, 1024, cnt, None)
    assert rc == _lib.GSMPM_EINVAL
    assert "sh_rotations needs shs" in _lib.last_error()


def test_mpm_sh_rotations_null_handle_fails_loudly():
    from gsmpm import _lib
    out = (ctypes.c_float * 9)()
    assert _lib.LIB.gsmpm_mpm_sh_rotations(None, None, out, None) == _lib.GSMPM_EINVAL
    assert "gsmpm_mpm_sh_rotations" in _lib.last_error()


def test_python_surface_takes_sh_rotations():
    """The new argument is last and optional on every layer; upstream's positional order is kept."""
    import inspect

    import diff_gaussian_rasterization as dgr
    from gsmpm import raster, sim
    from mpm_solver.solver import MPM_Simulator
    for fn in (raster.forward, raster.forward_async, raster._args, dgr.rasterize_gaussians,
               dgr.GaussianRasterizer.forward):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "sh_rotations" and p["sh_rotations"].default is None, fn
    assert list(inspect.signature(dgr.rasterize_gaussians).parameters)[:9] == [
        "means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp",
        "raster_settings"]
    assert list(inspect.signature(dgr.GaussianRasterizer.forward).parameters)[1:9] == [
        "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"]
    assert "A" in inspect.signature(sim.Simulator.sh_rotations).parameters
    assert "A" in inspect.signature(MPM_Simulator.sh_rotations).parameters


def test_rotate_sh_flag_and_spin_config():
    """RenderParams.rotate_sh: off by default, --rotate_sh and the JSON key turn
    it on; configs/lego-spin.json sets it, has no gravity and one impulse."""
    from arguments import MPMParams, RenderParams

    def parse(cfg, cli):
        parser = ArgumentParser()
        s, r = MPMParams(parser, cfg.get("mpm", {})), RenderParams(parser, cfg.get("render", {}))
        a = parser.parse_args(cli)
        return s.extract(a), r.extract(a)
    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        lego = json.load(f)
    assert parse(lego, [])[1].rotate_sh is False
    assert parse(lego, ["--rotate_sh"])[1].rotate_sh is True
    with open(os.path.join(PKG, "configs", "lego-spin.json")) as f:
        spin = json.load(f)
    s, r = parse(spin, [])
    assert r.rotate_sh is True and s.gravity == [0.0, 0.0, 0.0]
    assert [b["type"] for b in s.boundary_conditions] == ["impulse"]


def test_render_space_rotation_is_apply_inverse_rotations():
    """main.render_space_rotation composes the A with apply_inverse_rotations(x) = A x;
    None stands for the identity (every shipped config)."""
    import main as drv
    from utils.transform_utils import apply_inverse_rotations, generate_rotation_matrices
    rot0 = generate_rotation_matrices([torch.tensor(0.0)], [torch.tensor(0.0)], device="cpu")
    assert drv.render_space_rotation(rot0) is None
    rots = generate_rotation_matrices([torch.tensor(30.0), torch.tensor(-50.0), torch.tensor(75.0)], [0, 2, 1],
                                      device="cpu")
    A = drv.render_space_rotation(rots)
    x = torch.from_numpy(np.random.default_rng(0).normal(size=(20, 3)).astype(np.float32))
    want = apply_inverse_rotations(x, rots).numpy().astype(np.float64)
    assert np.abs(x.numpy().astype(np.float64) @ A.T - want).max() < 1e-5
    assert abs(np.linalg.det(A) - 1.0) < 1e-6
