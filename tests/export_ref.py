"""Float64 reference for the 3DGS export pass (csrc/export.hip): covariance ->
log-scales + quaternion, and the rotation of SH bands 1..3 by a per-Gaussian
Q.  Test infrastructure; numpy only.

  cov_to_scale_rot   np.linalg.eigh -> descending order -> det fix (negate the
                     last eigenvector) -> largest-component quaternion, w >= 0.
                     The floors are the documented ones of the kernel
                     (DESIGN.md 3.12): lambda >= max(1e-14 lambda_max, 1e-36).
  rotate_sh          per band l the (2l+1)x(2l+1) map X with Y_l(Q d) = Y_l(d) X
                     from a least-squares fit over 256 fixed random unit
                     directions (not the kernel's 2l+1 sample directions), then
                     out_l = X c_l.

The input sets of tests/test_export_ref.py (which measures this reference's
own error after rounding its outputs to f32) and tests/test_gpu_export.py
(which holds the kernels to 4x that) are built here, so both see the same rows.
"""
from __future__ import annotations

import numpy as np

from sh_rot_ref import random_rotations

N_MAX = 1000  # the size the reference's own errors are measured at; smaller input sets are prefixes
REL_FLOOR = 1e-14
ABS_FLOOR = 1e-36
FLOOR_LOG_SCALE = 0.5 * np.log(ABS_FLOOR)

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]


# ------------------------------------------------------------ covariance --
def sym3(cov6):
    c = np.asarray(cov6, np.float64)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def cov6_of(S):
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def quat_to_rot(q):
    """(w, x, y, z) -> R, the formula of GaussianModel._build_rotation (q is normalised first)."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def rot_to_quat(R):
    """Largest-component (Shepperd) selection, unit length, w >= 0."""
    R = np.asarray(R, np.float64)
    out = np.empty((R.shape[0], 4))
    for i, r in enumerate(R):
        tr = r[0, 0] + r[1, 1] + r[2, 2]
        k = int(np.argmax([tr, r[0, 0], r[1, 1], r[2, 2]]))
        if k == 0:
            s = 2.0 * np.sqrt(max(1.0 + tr, 0.0))
            q = [0.25 * s, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s]
        elif k == 1:
            s = 2.0 * np.sqrt(max(1.0 + r[0, 0] - r[1, 1] - r[2, 2], 0.0))
            q = [(r[2, 1] - r[1, 2]) / s, 0.25 * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s]
        elif k == 2:
            s = 2.0 * np.sqrt(max(1.0 + r[1, 1] - r[0, 0] - r[2, 2], 0.0))
            q = [(r[0, 2] - r[2, 0]) / s, (r[0, 1] + r[1, 0]) / s, 0.25 * s, (r[1, 2] + r[2, 1]) / s]
        else:
            s = 2.0 * np.sqrt(max(1.0 + r[2, 2] - r[0, 0] - r[1, 1], 0.0))
            q = [(r[1, 0] - r[0, 1]) / s, (r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, 0.25 * s]
        q = np.asarray(q)
        q = q / np.linalg.norm(q)
        out[i] = -q if q[0] < 0 else q
    out[:, 0] += 0.0
    return out


def finite_rows(cov6):
    return np.isfinite(np.asarray(cov6, np.float64)).all(axis=1)


def eigenvalues(cov6):
    """eigh's eigenvalues in descending order, float64 [P,3]; non-finite rows are treated as zero."""
    c = np.where(finite_rows(cov6)[:, None], np.asarray(cov6, np.float64), 0.0)
    return np.linalg.eigvalsh(sym3(c))[:, ::-1]


def floor_of(lam_max):
    return np.maximum(REL_FLOOR * lam_max, ABS_FLOOR)


def cov_to_scale_rot(cov6):
    """-> (log_scale [P,3] descending, quat [P,4]) in float64; a non-finite row gives the
    identity quaternion and the floor scale."""
    ok = finite_rows(cov6)
    c = np.where(ok[:, None], np.asarray(cov6, np.float64), 0.0)
    lam, V = np.linalg.eigh(sym3(c))
    lam, V = lam[:, ::-1], V[:, :, ::-1].copy()
    V[:, :, 2] *= np.where(np.linalg.det(V) < 0, -1.0, 1.0)[:, None]
    lam = np.maximum(lam, floor_of(lam[:, :1]))
    quat = rot_to_quat(V)
    quat[~ok] = [1.0, 0.0, 0.0, 0.0]
    return 0.5 * np.log(lam), quat


def reconstruct(log_scale, quat):
    """R(quat) diag(exp(2 log_scale)) R(quat)^T in float64, [P,3,3]."""
    R = quat_to_rot(quat)
    L = R * np.exp(np.asarray(log_scale, np.float64))[:, None, :]
    return L @ L.transpose(0, 2, 1)


def cov_error(cov6, log_scale, quat):
    """Per row ||R S^2 R^T - Sigma||_max / ||Sigma||_F; nan for non-finite and zero rows
    (the zero matrix has its own check: it reconstructs to the absolute floor)."""
    S = sym3(np.where(finite_rows(cov6)[:, None], cov6, 0.0))
    err = np.abs(reconstruct(log_scale, quat) - S).max(axis=(1, 2))
    nrm = np.linalg.norm(S, axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = err / nrm
    e[(nrm == 0) | ~finite_rows(cov6)] = np.nan
    return e


def _axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _compose(R, lam):
    R = np.asarray(R, np.float64)
    return (R * np.asarray(lam, np.float64)[None, :]) @ R.T


def special_covariances(seed=0):
    """The finite special rows of the issue's input set, float32 [S,6]."""
    rng = np.random.default_rng(seed)
    rot = lambda: random_rotations(rng, 1)[0]
    rows = [_compose(rot(), [0.7, 0.7, 0.7]),                       # isotropic
            _compose(rot(), [2.0, 2.0, 0.3]), _compose(rot(), [2.0, 0.3, 0.3])]  # two equal eigenvalues
    for perm in ([0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):  # diagonal, six axis orders
        rows.append(np.diag(np.array([3.0, 2.0, 1.0])[perm]))
    rows.append(np.array([[1.0, 0.25, 0.0], [0.25, 1.0, 0.0], [0.0, 0.0, 0.5]]))      # 45 degree Jacobi corner
    rows.append(np.array([[1.0, 0.25, 0.125], [0.25, 1.0, 0.0625], [0.125, 0.0625, 1.0]]))
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]):                         # exact 180 degree turns
        rows.append(_compose(_axis_angle(axis, np.pi), [3.0, 2.0, 1.0]))
    rows.append(_compose(rot(), [1.5, 0.5, 0.0]))                   # rank 2
    rows.append(_compose(rot(), [1.5, 0.0, 0.0]))                   # rank 1
    rows.append(np.zeros((3, 3)))                                   # zero
    for mag in (1e-12, 1.0, 1e6):
        for ratio in (1.0, 1e3, 1e6, 1e9, 1e12):
            rows.append(_compose(rot(), mag * np.array([1.0, ratio ** -0.5, 1.0 / ratio])))
    for mag in (1e-12, 1.0, 1e6):                                   # the ratios again, exactly representable
        rows.append(np.diag(mag * np.array([1e-12, 1.0, 1e-6])))
    while True:                                                     # PSD in f64, indefinite once rounded to f32
        v = rng.normal(size=3)
        S = np.outer(v, v)
        if np.linalg.eigvalsh(S.astype(np.float32).astype(np.float64))[0] < 0:
            rows.append(S)
            break
    return cov6_of(np.stack(rows)).astype(np.float32)


def covariance_inputs(P, seed=0):
    """float32 [P,6]: the special rows first, then random R diag(lambda) R^T (log-uniform
    eigenvalue ratios up to 1e8 and magnitudes 1e-8..1e2); for P >= 3 one row with a NaN (at
    P // 3) and one with an Inf (the last) are among them.  Returns (cov6, bad_rows)."""
    sp = special_covariances(seed)
    rng = np.random.default_rng(seed + 1)
    n = max(P, N_MAX)  # one pool whatever P: a smaller set is a prefix of the larger ones
    R = random_rotations(rng, n)
    lam = 10.0 ** rng.uniform(-8, 2, size=(n, 1)) * 10.0 ** -np.sort(rng.uniform(0, 8, size=(n, 3)), axis=1)
    rnd = cov6_of((R * lam[:, None, :]) @ R.transpose(0, 2, 1)).astype(np.float32)
    fin = np.concatenate([sp, rnd])
    if P < 3:
        return fin[:P].copy(), []
    nan_row = np.array([[1.0, 0.0, 0.0, 1.0, np.nan, 1.0]], np.float32)
    inf_row = np.array([[np.inf, 0.0, 0.0, 1.0, 0.0, 1.0]], np.float32)
    cov = np.concatenate([fin[:P // 3], nan_row, fin[P // 3:P - 2], inf_row])
    return np.ascontiguousarray(cov), [P // 3, P - 1]


# -------------------------------------------------------------------- SH --
def sh_basis(D, d):
    """Y_m(d) with the signs and constants of the rasterizer (sh = sum_m c_m Y_m + 0.5); [n,(D+1)^2]."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = [np.full_like(x, SH_C0)]
    if D > 0:
        Y += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if D > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        Y += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if D > 2:
        Y += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy),
              SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
    return np.stack(Y, axis=-1)


def sh_eval(D, shs, d):
    """sh(D, shs_p, d_p): shs [P,M,3], d [P,n,3] -> [P,n,3] (float64)."""
    K = (D + 1) ** 2
    return np.einsum("pnm,pmc->pnc", sh_basis(D, d), np.asarray(shs, np.float64)[:, :K]) + 0.5


def unit_directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


_FIT_DIRS = unit_directions(np.random.default_rng(777), 256)


def band_maps(D, Q):
    """Per Gaussian and band l <= D the least-squares X_l with Y_l(Q d) ~ Y_l(d) X_l; a list of [P,2l+1,2l+1]."""
    Q = np.asarray(Q, np.float64).reshape(-1, 3, 3)
    Yd = sh_basis(D, _FIT_DIRS)                                         # [n,K]
    Yq = sh_basis(D, np.einsum("pij,nj->pni", Q, _FIT_DIRS))            # [P,n,K]
    maps = []
    for l in range(1, D + 1):
        sl = slice(l * l, (l + 1) * (l + 1))
        maps.append(np.einsum("mn,pnk->pmk", np.linalg.pinv(Yd[:, sl]), Yq[:, :, sl]))
    return maps


def rotate_sh(shs, Q, D):
    """out with sh(D, out_p, d) = sh(D, shs_p, Q_p d); band 0 and the tail past (D+1)^2 unchanged."""
    out = np.array(shs, np.float64)
    for l, X in zip(range(1, D + 1), band_maps(D, Q)):
        sl = slice(l * l, (l + 1) * (l + 1))
        out[:, sl] = np.einsum("pmk,pkc->pmc", X, out[:, sl])
    return out


def sh_error(D, shs, Q, out, dirs):
    """max |sh(out, d) - sh(shs, Q d)| over the Gaussians and `dirs` [n,3], relative to max |shs|."""
    Q = np.asarray(Q, np.float64).reshape(-1, 3, 3)
    P = Q.shape[0]
    d = np.broadcast_to(dirs, (P,) + dirs.shape)
    want = sh_eval(D, shs, np.einsum("pij,nj->pni", Q, dirs))
    return float(np.abs(sh_eval(D, out, d) - want).max() / np.abs(np.asarray(shs, np.float64)).max())


def simulator_rotations():
    """float32 [512,3,3]: Simulator.sh_rotations() of a sheared jelly block after 20 substeps, as
    test_gpu_export.py::sheared_block_rotations produces it (tests/golden/export_sim_Q.npy is one
    recorded output): rotations with the orthogonality defect of the f32 polar decomposition."""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_sim_Q.npy"))


def orthogonality_defect(Q):
    Q = np.asarray(Q, np.float64).reshape(-1, 3, 3)
    return float(np.abs(Q.transpose(0, 2, 1) @ Q - np.eye(3)).max())


def rotation_inputs(P, seed=0):
    """float32 [P,3,3]: the identity, the 180 degree turns about x, y, z and (1,1,0), then random
    proper rotations; every third random one is a float32 product of two float32 rotations, i.e.
    off orthogonal by f32 rounding.  A smaller set is a prefix of the larger ones."""
    rng = np.random.default_rng(seed + 2)
    n = max(P, N_MAX)
    fixed = [np.eye(3)] + [_axis_angle(a, np.pi) for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0])]
    R = random_rotations(rng, n).astype(np.float32)
    R2 = random_rotations(rng, n).astype(np.float32)
    R[::3] = np.einsum("pij,pjk->pik", R[::3], R2[::3], dtype=np.float32)
    Q = np.concatenate([np.stack(fixed).astype(np.float32), R])
    return np.ascontiguousarray(Q[:P])


def sh_inputs(P, M, seed=0):
    """float32 [P,M,3] like a trained model's: dc ~ N(0.5, 0.5), the rest ~ N(0, 0.05), every
    seventh row ten times that.  Row 0 holds the largest entry (4.0, a saturated dc), so that
    max |shs|, which sh_error is relative to, is the same for every P."""
    rng = np.random.default_rng(seed + 3)
    n = max(P, N_MAX)
    shs = rng.normal(0.0, 0.05, size=(n, M, 3))
    shs[:, 0] = np.clip(rng.normal(0.5, 0.5, size=(n, 3)), -3.0, 3.0)
    shs[::7, 1:] *= 10.0
    shs = np.clip(shs, -3.5, 3.5)
    shs[0, 0, 0] = 4.0
    return np.ascontiguousarray(shs[:P].astype(np.float32))


# -------------------------------------------- the reference's own error --
_ERRORS = {}


def check_directions():
    """The 64 random unit directions both test files evaluate SH at."""
    return unit_directions(np.random.default_rng(64), 64)


def reference_errors():
    """{"e_cov": ..., "e_sh": {D: ...}}: the error of this reference once its outputs are rounded
    to f32, over covariance_inputs(N_MAX) and over sh_inputs(N_MAX) with rotation_inputs(N_MAX)
    followed by simulator_rotations().  The GPU bounds are 4x these (test_gpu_export.py)."""
    if not _ERRORS:
        cov, _ = covariance_inputs(N_MAX)
        ls, q = cov_to_scale_rot(cov)
        _ERRORS["e_cov"] = float(np.nanmax(cov_error(cov, ls.astype(np.float32), q.astype(np.float32))))
        Q = np.concatenate([rotation_inputs(N_MAX), simulator_rotations()])
        shs = sh_inputs(len(Q), 16)
        _ERRORS["e_sh"] = {D: sh_error(D, shs, Q, rotate_sh(shs, Q, D).astype(np.float32), check_directions())
                           for D in (1, 2, 3)}
        _ERRORS["e_sh"][0] = 0.0
    return _ERRORS
