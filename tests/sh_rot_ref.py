"""Float64 reference for the rasterizer's sh_rotations (include/gsmpm.h,
gsmpm_raster_args.sh_rotations).  Test infrastructure.

The colour of Gaussian p is clamp(_sh(D, shs_p, Q_p d_p), min=0) with d_p the
unit view direction (mean - campos) and _sh the polynomial of
tests/raster_torch_ref.py, in float64 torch.  Everything after the colour is
the oracle rasterizer fed that colour as colors_precomp:

  forward   O.raster_forward(..., colors_precomp=rgb)
  backward  ref = O.raster_backward(..., colors_precomp=rgb); autograd of
            (rgb * ref["colors"]).sum() gives dL/dshs, dL/dQ and the colour
            part of dL/dmeans3D, which is added to ref["means3D"] (the
            geometry part).  test_sh_rot_ref.py pins this composition against
            all-float64 autograd before the GPU is judged against it.
"""
from __future__ import annotations

import numpy as np
import torch

from raster_torch_ref import _sh


def random_rotations(rng, n):
    """n proper rotations (det +1), float64 [n,3,3], from QR of Gaussian matrices."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return q


def view_dirs(means, campos):
    d = means - campos
    return d / d.norm(dim=1, keepdim=True)


def rotated_rgb(D, shs, means, campos, Q):
    """clamp(_sh(D, shs, Q d), 0) in the dtype of its (torch) inputs; shs [P,M,3], Q [P,3,3]."""
    d = view_dirs(means, campos)
    dq = (Q.reshape(-1, 3, 3) @ d[:, :, None])[..., 0]
    return torch.clamp(_sh(D, shs, dq), min=0.0)


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def forward_ref(means, opa, view, full, campos, bg, W, H, tx, ty, shs, D, Q, **cov_kw):
    """(image (3,H,W), radii, num_rendered) of the oracle with the rotated colours."""
    import oracle as O
    rgb = rotated_rgb(D, _t64(shs), _t64(means), _t64(campos), _t64(Q)).numpy().astype(np.float32)
    img, radii, K, _, _ = O.raster_forward(means, opa, view, full, campos, bg, W, H, tx, ty, colors_precomp=rgb,
                                           **cov_kw)
    return img, radii, K


def backward_ref(wgt, means, opa, view, full, campos, bg, W, H, tx, ty, shs, D, Q, **cov_kw):
    """The oracle's backward dict with "sh" [P,M,3], "sh_rotations" [P,3,3] added and the
    colour part of dL/dmeans3D folded into "means3D" (float64 numpy for those three)."""
    import oracle as O
    s, q, m = _t64(shs, True), _t64(np.asarray(Q).reshape(-1, 3, 3), True), _t64(means, True)
    rgb = rotated_rgb(D, s, m, _t64(campos), q)
    ref = O.raster_backward(wgt, means, opa, view, full, campos, bg, W, H, tx, ty,
                            colors_precomp=rgb.detach().numpy().astype(np.float32), **cov_kw)
    (rgb * _t64(ref["colors"])).sum().backward()
    out = dict(ref)
    out["sh"] = s.grad.numpy()
    out["sh_rotations"] = q.grad.numpy()
    out["means3D"] = ref["means3D"].astype(np.float64) + m.grad.numpy()
    return out
