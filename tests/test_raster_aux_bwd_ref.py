"""tests/raster_aux_bwd_ref.py (the reference of the depth / alpha map
gradients) against float64 autograd of the forward (tests/raster_torch_ref.py)
rendering colors_precomp = (z_i, 1, 0) over black, z_i a non-leaf of means3D.

Scenes and camera of test_oracle_raster_bwd.py, and its bound: 2e-3 of each
output's max magnitude (f32 oracle vs f64 reference; measured <= 2.1e-6).
These tests need no GPU and pass without the feature: they pin the reference
the GPU tests compare with.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import raster_aux_bwd_ref as ABR
from conftest import rel_err
from test_oracle_raster_bwd import _camera, _scene


def _compare(P, W, H, seed, use_sr):
    from raster_torch_ref import forward
    means, c6, opa, shs, scales, rots = _scene(P, seed)
    view, full, campos, tx, ty = _camera(W, H, 1.0)
    rng = np.random.default_rng(seed + 1)
    gD = rng.normal(0, 1, (H, W)).astype(np.float32)
    gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    cov = dict(scales=scales, rotations=rots) if use_sr else dict(cov3D_precomp=c6)
    # the colour inputs do not enter the map gradients; the helper's colour call gets gC = 0
    kw = dict(colors_precomp=np.zeros((P, 3), np.float32), **cov)
    bgv = np.full(3, 0.3, np.float32)
    got = ABR.backward(None, gD, gA, means, opa, view, full, campos, bgv, W, H, tx, ty, **kw)
    nochain = ABR.backward(None, gD, gA, means, opa, view, full, campos, bgv, W, H, tx, ty, chain=False, **kw)
    d = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    inp = {"means3D": d(means), "opacities": d(opa), "viewmatrix": d(view).detach(), "projmatrix": d(full).detach(),
           "campos": d(campos).detach(), "bg": torch.zeros(3, dtype=torch.float64)}
    if use_sr:
        inp["scales"], inp["rotations"] = d(scales), d(rots)
    else:
        inp["cov3D_precomp"] = d(c6)
    hom = torch.cat([inp["means3D"], torch.ones(P, 1, dtype=torch.float64)], 1)
    z = hom @ inp["viewmatrix"][:, 2]
    inp["colors_precomp"] = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
    img, ndc, radii, stats = forward(inp, W, H, tx, ty)
    (img[0] * torch.from_numpy(gD.astype(np.float64)) + img[1] * torch.from_numpy(gA.astype(np.float64))).sum().backward()
    checks = [("means3D", inp["means3D"].grad, got["means3D"]), ("opacity", inp["opacities"].grad.view(-1), got["opacity"]),
              ("means2D", ndc.grad, got["means2D"][:, :2])]
    if use_sr:
        checks += [("scales", inp["scales"].grad, got["scales"]), ("rotations", inp["rotations"].grad, got["rotations"])]
    else:
        checks.append(("cov3D", inp["cov3D_precomp"].grad, got["cov3D"]))
    errs = {k: rel_err(g, ref.numpy()) for k, ref, g in checks}
    ref_m = inp["means3D"].grad.numpy()
    moved = float(np.abs(nochain["means3D"] - ref_m).max() / np.abs(ref_m).max())
    print("map gradients vs float64 autograd:", {k: f"{e:.1e}" for k, e in errs.items()},
          f"without the z chain term means3D is off by {moved:.3f} of its max")
    assert not np.any(got["colors"]) and np.abs(got["dz"]).max() > 0
    return errs, moved, stats


@pytest.mark.parametrize("P,W,H,seed,use_sr", [(14, 40, 36, 14, False), (12, 36, 36, 5, True)])
def test_map_gradients_vs_float64_autograd(P, W, H, seed, use_sr):
    errs, moved, stats = _compare(P, W, H, seed, use_sr)
    assert stats["pairs"] > 0
    assert all(e < 2e-3 for e in errs.values()), errs
    # the z path is really tested: dropping the chain term is far outside the bound
    assert moved > 1e-2, moved
