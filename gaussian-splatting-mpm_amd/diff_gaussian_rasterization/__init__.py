"""Drop-in for the ``diff_gaussian_rasterization`` package (forward path).

Same Python surface as the graphdeco-inria extension the reference imports at
main.py:16 / extra.py:16 (pre-2024 API: the forward returns ``(color, radii)``,
consumed as ``rendered_image, _ = rasterizer(...)`` at main.py:148), backed by
the HIP kernels in libgsmpm.so.  The backward (upstream's
_RasterizeGaussians.backward, used by extra.py's loss.backward()) returns the
gradients of means3D, means2D (w.r.t. NDC, as upstream), shs / colors_precomp,
opacities, scales / rotations or cov3D_precomp; a forward that needs them runs
on a context of its own (leased from a per-device pool) that keeps its
binning and per-pixel state until the backward.  Three additions, last,
optional and passed by keyword everywhere: ``sh_rotations`` ([P,3,3] or [P,9]) shades each Gaussian
at Q d instead of the view direction d, and gets its gradient too;
``return_depth_alpha=True`` makes the forward return ``(color, radii, depth,
alpha)``, depth [H,W] = sum z_i alpha_i T_i (view-space depth, not normalised)
and alpha [H,W] = 1 - T_final of the colour blend, both non-differentiable
unless ``depth_alpha_grad=True`` is given with it: then the two maps stay in
the autograd graph and their gradients reach means3D, opacities and the
covariance inputs (gsmpm_raster_backward_aux); a normalised depth depth / alpha
is the caller's to form in torch.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from gsmpm import raster as _raster


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_depth_alpha=False, depth_alpha_grad=False, sh_rotations=None):
    """Upstream's positional signature, then the three additions, all passed by
    keyword: return_depth_alpha appends the depth and alpha maps to (color,
    radii); depth_alpha_grad (needs return_depth_alpha) keeps the two maps in
    the autograd graph; sh_rotations ([P,3,3] or [P,9]) evaluates each
    Gaussian's SH at Q d instead of the view direction d."""
    if isinstance(return_depth_alpha, torch.Tensor) or isinstance(depth_alpha_grad, torch.Tensor):
        raise TypeError("rasterize_gaussians: pass sh_rotations by keyword (return_depth_alpha precedes it)")
    if depth_alpha_grad and not return_depth_alpha:
        raise ValueError("rasterize_gaussians: depth_alpha_grad=True needs return_depth_alpha=True")
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, sh_rotations, bool(return_depth_alpha),
                                     bool(depth_alpha_grad))


def _opt(t):
    return None if t is None or t.numel() == 0 else t


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, sh_rotations=None, return_depth_alpha=False, depth_alpha_grad=False):
        s = raster_settings
        if depth_alpha_grad and not return_depth_alpha:
            raise ValueError("_RasterizeGaussians: depth_alpha_grad=True needs return_depth_alpha=True")
        kw = dict(depth=return_depth_alpha, alpha=return_depth_alpha, sh_degree=s.sh_degree, shs=_opt(sh), colors_precomp=_opt(colors_precomp), scales=_opt(scales),
                  rotations=_opt(rotations), cov3D_precomp=_opt(cov3Ds_precomp), scale_modifier=s.scale_modifier,
                  prefiltered=s.prefiltered, sh_rotations=_opt(sh_rotations))
        args = (means3D, opacities.reshape(-1), s.viewmatrix, s.projmatrix, s.campos, s.bg, s.image_height,
                s.image_width, s.tanfovx, s.tanfovy)
        if any(ctx.needs_input_grad[:8]) or ctx.needs_input_grad[9]:
            lease = _raster.ContextLease(means3D.device.index or 0)
            num_rendered, color, radii, *maps, a, keep = _raster.forward(*args, **kw, context=lease.context,
                                                                         return_args=True)
            ctx.state = (lease, a, keep, radii)
            ctx.shapes = [None if t is None else (t.shape, t.dtype) for t in
                          (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                           None, sh_rotations)]
        else:
            num_rendered, color, radii, *maps = _raster.forward(*args, **kw)
        ctx.num_rendered = num_rendered
        ctx.map_grads = bool(depth_alpha_grad)
        if depth_alpha_grad:
            # the maps stay in the graph; an output the loss does not use arrives as None, not as zeros
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(radii)
        else:
            ctx.mark_non_differentiable(radii, *maps)
        return (color, radii, *maps)

    @staticmethod
    def backward(ctx, grad_out_color, *more):
        lease, a, keep, radii = ctx.state
        shp = ctx.shapes
        P = a.P

        def cast(t, i):
            if t is None or shp[i] is None or shp[i][0].numel() == 0 or not ctx.needs_input_grad[i]:
                return None
            return t.reshape(shp[i][0]).to(shp[i][1])
        if P == 0:
            return (None,) * 12
        if ctx.map_grads:
            g_depth, g_alpha = more[1], more[2]
            if grad_out_color is None:
                grad_out_color = torch.zeros((3, a.H, a.W), dtype=torch.float32, device=radii.device)
            g = _raster.backward(lease.context, keep, a, radii, grad_out_color, g_depth, g_alpha)
        else:
            g = _raster.backward(lease.context, keep, a, radii, grad_out_color)
        lease.release()  # back to the pool: the next iteration's forward reuses its buffers
        ctx.state = None
        return (cast(g["means3D"], 0), cast(g["means2D"], 1), cast(g["sh"], 2), cast(g["colors"], 3),
                cast(g["opacity"], 4), cast(g["scales"], 5), cast(g["rotations"], 6), cast(g["cov3D"], 7), None,
                cast(g["sh_rotations"], 9), None, None)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            s = self.raster_settings
            return _raster.mark_visible(positions, s.viewmatrix, s.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, return_depth_alpha=False, depth_alpha_grad=False, sh_rotations=None):
        s = self.raster_settings
        if depth_alpha_grad and not return_depth_alpha:
            raise ValueError("GaussianRasterizer: depth_alpha_grad=True needs return_depth_alpha=True")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.Tensor([])
        return rasterize_gaussians(means3D, means2D, empty if shs is None else shs,
                                   empty if colors_precomp is None else colors_precomp, opacities,
                                   empty if scales is None else scales, empty if rotations is None else rotations,
                                   empty if cov3D_precomp is None else cov3D_precomp, s,
                                   return_depth_alpha=return_depth_alpha, depth_alpha_grad=depth_alpha_grad,
                                   sh_rotations=sh_rotations)
