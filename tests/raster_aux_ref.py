"""Reference for the rasterizer's depth and alpha maps (include/gsmpm.h,
gsmpm_raster_args.aux_depth / aux_alpha).  Test infrastructure.

No new oracle code: the CPU oracle's colour blend IS the definition (the maps
take, skip and stop on Gaussians exactly as the colour does), so the maps are
two colour channels of an oracle render with colors_precomp = (z_i, 1, 0) over
a black background:

    channel 0 = sum z_i alpha_i T_i = D
    channel 1 = sum   1 alpha_i T_i = 1 - T_final = A   (the sum telescopes)

oracle.raster_forward copies precomputed colours unclamped, so z_i > 1 is
fine.  z_i is the f32 view-space depth as the preprocess forms it: the view
matrix's third column applied to the mean, left to right, every operation
rounded to f32.
"""
from __future__ import annotations

import numpy as np


def view_depth(means3D, viewmatrix):
    """[P] f32: z_i = m[2] x + m[6] y + m[10] z + m[14] (m = viewmatrix flattened), in f32."""
    p = np.asarray(means3D, np.float32).reshape(-1, 3)
    v = np.asarray(viewmatrix, np.float32).reshape(4, 4)
    z = v[0, 2] * p[:, 0] + v[1, 2] * p[:, 1]
    z = z + v[2, 2] * p[:, 2]
    return (z + v[3, 2]).astype(np.float32)


def aux_colors(means3D, viewmatrix):
    """[P,3] f32 precomputed colours (z_i, 1, 0)."""
    z = view_depth(means3D, viewmatrix)
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)


def forward(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, **cov):
    """(D [H,W], A [H,W], radii [P], z [P]) from the CPU oracle.  cov:
    cov3D_precomp=[P,6], or scales / rotations (/ scale_modifier)."""
    import oracle as O
    col = aux_colors(means3D, viewmatrix)
    img, radii, _, _, _ = O.raster_forward(means3D, opacities, viewmatrix, projmatrix, campos,
                                           np.zeros(3, np.float32), W, H, tanfovx, tanfovy, colors_precomp=col,
                                           **cov)
    return img[0], img[1], radii, col[:, 0]
