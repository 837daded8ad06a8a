"""Reference for the rasterizer backward with the gradients of the depth and
alpha maps (include/gsmpm.h, gsmpm_raster_backward_aux).  Test infrastructure.

No new oracle code, by the trick of raster_aux_ref.py: the maps D and A are
colour channels 0 and 1 of an oracle render with colors_precomp = (z_i, 1, 0)
over black, so the oracle's colour backward called with the weights
(gD, gA, 0), those colours and bg = 0 returns the map part of every geometric
gradient (means2D, opacity, cov3D or scales / rotations, and the part of
means3D that goes through the projection and the covariance), and
g["colors"][:, 0] is dL/dz_i.  The colours (z_i, 1, 0) are inputs to that
call, so the chain through z_i = view[:, 2] . (x, y, z, 1) is added here:

    means3D += dz_i * view[:3, 2]

The gradient is linear in (gC, gD, gA): the full reference is the oracle's
colour backward for gC plus the map part.  Pinned against float64 autograd in
test_raster_aux_bwd_ref.py.
"""
from __future__ import annotations

import numpy as np

import raster_aux_ref as AR

_GEOM = ("means2D", "opacity", "means3D", "cov3D", "scales", "rotations")


def backward(gC, gD, gA, means3D, opacities, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy,
             chain=True, **kw):
    """The dict of oracle.raster_backward (means2D, colors, opacity, means3D,
    cov3D, sh | None, scales | None, rotations | None) for the loss
    sum(gC * color) + sum(gD * D) + sum(gA * A), plus "dz" [P] = dL/dz_i.
    gC [3,H,W], gD / gA [H,W]; any of them may be None (= zero).  kw: the
    colour inputs (shs + sh_degree, or colors_precomp) and the covariance
    inputs (cov3D_precomp, or scales + rotations) of oracle.raster_backward.
    chain=False leaves the z_i chain term out of means3D (for the test that
    shows it matters)."""
    import oracle as O
    zero = np.zeros((H, W), np.float32)
    geo = (means3D, opacities, viewmatrix, projmatrix, campos)
    g = O.raster_backward(np.zeros((3, H, W), np.float32) if gC is None else gC, *geo, bg, W, H, tanfovx, tanfovy,
                          **kw)
    cov = {k: v for k, v in kw.items() if k in ("cov3D_precomp", "scales", "rotations", "scale_modifier")}
    wgt = np.stack([zero if gD is None else np.asarray(gD, np.float32),
                    zero if gA is None else np.asarray(gA, np.float32), zero])
    m = O.raster_backward(wgt, *geo, np.zeros(3, np.float32), W, H, tanfovx, tanfovy,
                          colors_precomp=AR.aux_colors(means3D, viewmatrix), **cov)
    out = dict(g)
    for k in _GEOM:
        if g[k] is not None:
            out[k] = g[k] + m[k]
    dz = m["colors"][:, 0].copy()
    if chain:
        v = np.asarray(viewmatrix, np.float32).reshape(4, 4)
        out["means3D"] = out["means3D"] + dz[:, None] * v[:3, 2][None, :]
    out["dz"] = dz
    return out
