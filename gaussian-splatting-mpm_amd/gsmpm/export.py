"""Deformed Gaussians as a standard 3DGS model (csrc/export.hip) -- thin wrappers
over gsmpm_cov_to_scale_rot / gsmpm_sh_rotate, and the model assembly on top.

    log_scale, quat = cov_to_scale_rot(cov6)          # [P,6] -> [P,3], [P,4] (w, x, y, z)
    shs2 = rotate_sh(shs, Q, degree)                  # sh(shs2, d) = sh(shs, Q d)
    g2 = deformed_model(gaussians, mask, means, cov6, sh_rotations=Q)
    g2.save_ply(path)                                 # any 3DGS viewer shows the deformed state

Tensors in, tensors out, on the tensors' device and current stream.  The file
format stores a Gaussian as log-scales, a quaternion and SH coefficients; the
simulator's frame is a full covariance and a view-direction rotation
(Simulator.world_outputs / sh_rotations).  DESIGN.md 3.12 has the method.
"""
from __future__ import annotations

import torch

from ._lib import LIB, check, ptr, stream_of


def cov_to_scale_rot(cov6, return_bad=False):
    """cov6 [P,6] (xx, xy, xz, yy, yz, zz) -> (log_scale [P,3] descending, quat [P,4] unit, w >= 0) with
    R(quat) diag(exp(2 log_scale)) R(quat)^T = cov6.  return_bad: also the number of rows with a
    NaN / Inf entry (they get the identity quaternion and the floor scale); reading it synchronises."""
    cov6 = cov6.detach().to(torch.float32).contiguous()
    n = cov6.shape[0]
    if cov6.shape != (n, 6):
        raise ValueError("expected cov6 [P,6]")
    log_scale = torch.empty((n, 3), dtype=torch.float32, device=cov6.device)
    quat = torch.empty((n, 4), dtype=torch.float32, device=cov6.device)
    bad = torch.zeros(1, dtype=torch.int64, device=cov6.device) if return_bad else None
    with torch.cuda.device(cov6.device):
        check(LIB.gsmpm_cov_to_scale_rot(ptr(cov6), n, ptr(log_scale), ptr(quat), ptr(bad), stream_of(cov6.device)),
              "gsmpm_cov_to_scale_rot")
    return (log_scale, quat, int(bad.item())) if return_bad else (log_scale, quat)


def rotate_sh(shs, Q, degree):
    """shs [P,M,3], Q [P,3,3] (or [P,9]) -> shs' with sh(degree, shs'_p, d) = sh(degree, shs_p, Q_p d):
    plain SH evaluation of shs' gives what the rasterizer's sh_rotations=Q gives with shs.
    Band 0 and the coefficients past (degree+1)^2 are copied."""
    shs = shs.detach().to(torch.float32).contiguous()
    Q = Q.detach().to(torch.float32).contiguous()
    n = shs.shape[0]
    if shs.dim() != 3 or shs.shape[2] != 3 or Q.numel() != 9 * n or Q.shape[0] != n:
        raise ValueError("expected shs [P,M,3] and Q [P,3,3]")
    out = torch.empty_like(shs)
    with torch.cuda.device(shs.device):
        check(LIB.gsmpm_sh_rotate(ptr(shs), ptr(Q), n, int(degree), shs.shape[1], ptr(out), stream_of(shs.device)),
              "gsmpm_sh_rotate")
    return out


# activated opacities are stored as logits; this keeps the logit finite (|logit| <= 16.1) and
# sigmoid(logit) within 1e-7 of the opacity
_OPACITY_EPS = 1e-7


def _logit(opacity):
    o = opacity.detach().to(torch.float64).reshape(-1, 1).clamp(_OPACITY_EPS, 1.0 - _OPACITY_EPS)
    return torch.log(o / (1.0 - o)).to(torch.float32)


def deformed_model(gaussians, mask, means, cov6, sh_rotations=None, filled=None):
    """A copy of `gaussians` (a GaussianModel) in its deformed state, ready for save_ply.

    The rows under `mask` get `means` [K,3], and _scaling / _rotation from `cov6` [K,6]
    (cov_to_scale_rot); with `sh_rotations` [K,3,3] (the Q for these means, e.g.
    MPM_Simulator.sh_rotations(None) for world-space means) also _features_dc / _features_rest
    rotated by it (rotate_sh).  Rows outside the mask are copied.  `filled` = (shs [F,M,3],
    activated opacity [F] or [F,1], means [F,3], cov6 [F,6][, sh_rotations [F,3,3]]) of
    particles that are not in `gaussians` (interior filling): they are appended as rows of
    their own, their opacity stored as the (finite) logit."""
    from gaussian_splatting.scene import GaussianModel
    dev = gaussians._xyz.device
    g = GaussianModel(gaussians.max_sh_degree, device=dev)
    g.active_sh_degree = gaussians.active_sh_degree
    fields = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    for f in fields:
        setattr(g, f, getattr(gaussians, f).detach().clone())
    k = int(mask.sum())
    if means.shape != (k, 3) or cov6.shape != (k, 6):
        raise ValueError(f"expected means [{k},3] and cov6 [{k},6] for the {k} rows under the mask")
    degree = gaussians.active_sh_degree

    def parts(means, cov6, shs, Q):
        log_scale, quat = cov_to_scale_rot(cov6)
        if Q is not None:
            shs = rotate_sh(shs, Q, degree)
        return means.detach().to(torch.float32), log_scale, quat, shs

    xyz, scl, rot, shs = parts(means, cov6, gaussians.get_features[mask].detach() if sh_rotations is not None else None,
                               sh_rotations)
    g._xyz[mask], g._scaling[mask], g._rotation[mask] = xyz, scl, rot
    if sh_rotations is not None:
        g._features_dc[mask], g._features_rest[mask] = shs[:, :1], shs[:, 1:]
    if filled is not None:
        f_shs, f_opa, f_means, f_cov = filled[:4]
        f_Q = filled[4] if len(filled) > 4 else None
        xyz, scl, rot, shs = parts(f_means, f_cov, f_shs.detach().to(torch.float32), f_Q)
        new = (xyz, shs[:, :1], shs[:, 1:], _logit(f_opa), scl, rot)
        for f, t in zip(fields, new):
            setattr(g, f, torch.cat([getattr(g, f), t.to(dev)], dim=0))
    return g
