"""Float64 reference of the constitutive step, the input classes and the error
measures shared by test_constitutive_ref.py (CPU) and
test_gpu_constitutive_ref.py (GPU).

Plain numpy, vectorised over rows, no project code.  Every function is written
from the reference's formulas (mpm_solver/constitutive_models.py and
mpm_solver/utils.py:13-54, line numbers cited at each step) around
np.linalg.svd, not from the device or the oracle sources, so a transcription
error shared by those two does not reach it.

Material codes are gsmpm_constitutive's: 0 jelly as written (zero stress),
1 metal, 2 sand, 3 foam, 4 jelly with FCR, 5 fluid.  The constants are the ones
that entry hard-codes: friction angle 25 degrees, plastic viscosity 0.008,
hardening = 1, xi = 1.
"""
import functools
import math

import numpy as np

SIN_PHI = math.sin(25.0 / 180.0 * math.pi)
ALPHA = math.sqrt(2.0 / 3.0) * 2.0 * SIN_PHI / (3.0 - SIN_PHI)
PVISC = 0.008
XI = 1.0
DT = 1e-4

MATERIALS = {0: "jelly", 1: "metal", 2: "sand", 3: "foam", 4: "fcr", 5: "fluid"}
CLASSES = ("moderate", "near_id", "tiny", "pair", "triple", "large", "clamp", "reflect")
N_ROWS = 2048 + 37  # the last block and the last wave are ragged

# branch codes
KEPT, PLASTIC, ROTATION = 0, 1, 2

# Foam: a plastic row is compared only with a singular-value gap
# of at least FOAM_GAP and every foam row sits FOAM_MARGIN (strain units) away
# from its yield surface, ~100 times the f32 log-strain error.
FOAM_GAP = 0.05
FOAM_MARGIN = 1e-3
FOAM_SPLIT = ("moderate", "large", "clamp", "reflect")  # the other classes: every foam row elastic
FOAM_DROP_CAP = 0.05
# Rows at least this far (strain units) inside a branch must take that branch
# on any f32 implementation: the discriminants are sums of three f32 logs of
# singular values whose own error is ~1e-6 (the oracle's sigma column), so 1e-5
# is ten times what rounding can move them.  Used by the bit-exact row-copy
# checks; the error bounds hold for every row regardless (the maps are
# continuous across their surfaces).
BRANCH_MARGIN = 1e-5


# ------------------------------------------------------------------ helpers --
def _diag(v):
    out = np.zeros(v.shape + (3,), np.float64)
    for d in range(3):
        out[..., d, d] = v[..., d]
    return out


def _T(A):
    return np.swapaxes(A, -1, -2)


def _sym(A):
    return (A + _T(A)) / 2.0


def svd_taichi(F):
    """ti.svd's convention from np.linalg.svd: sigma1 >= sigma2 >= |sigma3|,
    U and V rotations, the sign of det F on sigma3."""
    F = np.asarray(F, np.float64)
    U, s, Vh = np.linalg.svd(F)
    V = _T(Vh).copy()
    U = U.copy()
    s = s.copy()
    du = np.sign(np.linalg.det(U))
    dv = np.sign(np.linalg.det(V))
    U[..., :, 2] *= du[..., None]
    V[..., :, 2] *= dv[..., None]
    s[..., 2] *= du * dv
    return U, s, V


def _col(a):
    return np.asarray(a, np.float64)[..., None]


class Result:
    """F: returned F (n,3,3); tau: symmetrised stress; yld: yield after the
    step; branch: KEPT / PLASTIC / ROTATION; disc: the branch discriminant in
    strain units (> 0: not kept); tr: sand's second discriminant (log-strain
    trace), 0 elsewhere; s_trial: Taichi-convention singular values of F_trial."""

    def __init__(self, F, tau, yld, branch, disc, s_trial, tr=None):
        self.F, self.tau, self.yld, self.branch, self.disc, self.s_trial = F, tau, yld, branch, disc, s_trial
        self.tr = np.zeros_like(disc) if tr is None else tr


# ----------------------------------------------------------------- stresses --
def stress_fcr(F, mu, lam):
    """kirchoff_stress_FCR, constitutive_models.py:10-20; J, U, V of utils.py:31-33."""
    U, _, V = svd_taichi(F)
    R = U @ _T(V)
    J = np.linalg.det(F)
    return 2.0 * _col(mu)[..., None] * (F - R) @ _T(F) + np.eye(3) * (lam * J * (J - 1.0))[..., None, None]


def stress_stvk(F, U, s, V, mu, lam):
    """kirchoff_stress_StVK, constitutive_models.py:23-38."""
    eps = np.log(np.maximum(s, 0.01))
    tau = 2.0 * _col(mu) * eps + _col(lam) * eps.sum(-1, keepdims=True)
    return U @ _diag(tau) @ _T(V) @ _T(F)


def stress_dp(F, U, s, V, mu, lam):
    """kirchoff_stress_Drucker_Prager, constitutive_models.py:41-58 (the log of a
    negative sigma is NaN, as in the reference)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ls = np.log(s)
        c = 2.0 * _col(mu) * ls / s + _col(lam) * ls.sum(-1, keepdims=True) / s
    return U @ _diag(c) @ _T(V) @ _T(F)


# -------------------------------------------------------------- the 6 codes --
def _prep(F, mu, lam, yld):
    F = np.asarray(F, np.float64)
    n = F.shape[0]
    b = lambda a: np.broadcast_to(np.asarray(a, np.float64), (n,)).copy()
    return F, b(mu), b(lam), b(yld)


def jelly(F, mu, lam, yld, dt=DT):
    """Code 0.  utils.py:28-29 keeps F_trial; `model.material == 0` at utils.py:37
    compares the field, not the entry, so no stress branch fires: zero stress."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    _, s, _ = svd_taichi(F)
    z = np.zeros(len(F))
    return Result(F.copy(), np.zeros_like(F), yld, z.astype(int), z - 1.0, s)


def jelly_fcr(F, mu, lam, yld, dt=DT):
    """Code 4.  utils.py:28-29 keeps F_trial; stress by utils.py:38 as intended."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    _, s, _ = svd_taichi(F)
    z = np.zeros(len(F))
    return Result(F.copy(), _sym(stress_fcr(F, mu, lam)), yld, z.astype(int), z - 1.0, s)


def metal_cond_norm(F, mu, lam):
    """||dev tau|| of constitutive_models.py:64-79, the quantity compared with the yield at :82."""
    _, s, _ = svd_taichi(F)
    eps = np.log(np.maximum(s, 0.01))                                   # :67-70
    tau = 2.0 * _col(mu) * eps + _col(lam) * eps.sum(-1, keepdims=True)   # :75
    cond = tau - tau.sum(-1, keepdims=True) / 3.0                       # :78-79
    return np.linalg.norm(cond, axis=-1)


def metal(F, mu, lam, yld, dt=DT):
    """Code 1.  von_mises_return_mapping, constitutive_models.py:62-103, then
    StVK stress of the returned F (utils.py:31-41, 52)."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    U, s, V = svd_taichi(F)                                             # :64
    eps = np.log(np.maximum(s, 0.01))                                   # :67-70
    temp = eps.sum(-1) / 3.0                                            # :71
    cn = metal_cond_norm(F, mu, lam)
    plastic = cn > yld                                                  # :82
    eh = eps - temp[:, None]                                            # :83
    ehn = np.linalg.norm(eh, axis=-1) + 1e-6                            # :84
    dg = ehn - yld / (2.0 * mu)                                         # :85
    eps_new = eps - (dg / ehn)[:, None] * eh                            # :86
    with np.errstate(over="ignore", invalid="ignore"):  # lanes that stay elastic (a huge yield) are discarded
        Fp = U @ _diag(np.exp(eps_new)) @ _T(V)                         # :88-95
    Fn = np.where(plastic[:, None, None], Fp, F)                        # :100-102
    yn = np.where(plastic, yld + 2.0 * mu * XI * dg, yld)               # :97-98, hardening == 1
    U2, s2, V2 = svd_taichi(Fn)                                         # utils.py:33
    tau = _sym(stress_stvk(Fn, U2, s2, V2, mu, lam))                    # utils.py:40-41, 52
    return Result(Fn, tau, yn, plastic.astype(int), (cn - yld) / (2.0 * mu), s)


def sand(F, mu, lam, yld, dt=DT):
    """Code 2.  sand_return_mapping, constitutive_models.py:105-140, then the
    Drucker-Prager stress (utils.py:43-46, 52)."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    U, s, V = svd_taichi(F)                                             # :107
    eps = np.log(np.maximum(np.abs(s), 1e-14))                          # :110-114
    tr = eps.sum(-1)                                                    # :116
    eh = eps - tr[:, None] / 3.0                                        # :117
    ehn = np.linalg.norm(eh, axis=-1)                                   # :118
    dg = ehn + (3.0 * lam + 2.0 * mu) / (2.0 * mu) * tr * ALPHA         # :119-125
    with np.errstate(invalid="ignore", divide="ignore"):
        H = eps - eh * (dg / ehn)[:, None]                              # :135
    Fproj = U @ _diag(np.exp(H)) @ _T(V)                                # :137-139
    Frot = U @ _T(V)                                                    # :132
    branch = np.where(dg <= 0, KEPT, np.where(tr > 0, ROTATION, PLASTIC))
    Fn = np.where((branch == KEPT)[:, None, None], F, np.where((branch == ROTATION)[:, None, None], Frot, Fproj))
    U2, s2, V2 = svd_taichi(Fn)                                         # utils.py:33
    tau = _sym(stress_dp(Fn, U2, s2, V2, mu, lam))
    return Result(Fn, tau, yld, branch, dg, s, tr)


def foam(F, mu, lam, yld, dt=DT):
    """Code 3.  viscoplasticity_return_mapping_with_StVK, constitutive_models.py:216-259
    (the element-wise product at :256), then StVK stress (utils.py:47-50, 52)."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    U, s, V = svd_taichi(F)                                             # :218
    sg = np.maximum(s, 0.01)                                            # :224
    eps = np.log(sg)                                                    # :228
    tr = eps.sum(-1)                                                    # :229
    st = 2.0 * mu[:, None] * (eps - tr[:, None] / 3.0)                  # :233-234
    stn = np.linalg.norm(st, axis=-1)                                   # :235
    y = stn - 0.8 * math.sqrt(2.0 / 3.0) * yld                          # :236
    plastic = y > 0                                                     # :238
    mu_hat = mu * (sg ** 2).sum(-1) / 3.0                               # :239
    snn = stn - y / (1.0 + PVISC * 2 / (2.0 * mu_hat * dt))             # :240-242
    with np.errstate(invalid="ignore", divide="ignore"):
        s_new = (snn / stn)[:, None] * st                               # :243
    eps_new = 1.0 / (2.0 * mu[:, None]) * s_new + tr[:, None] / 3.0     # :244
    with np.errstate(over="ignore", invalid="ignore"):  # lanes that stay elastic (a huge yield) are discarded
        Fp = U * _diag(np.exp(eps_new)) * _T(V)                         # :245-256, element-wise
    Fn = np.where(plastic[:, None, None], Fp, F)
    U2, s2, V2 = svd_taichi(Fn)
    tau = _sym(stress_stvk(Fn, U2, s2, V2, mu, lam))
    return Result(Fn, tau, yld, plastic.astype(int), y / (2.0 * mu), s)


def fluid(F, mu, lam, yld, dt=DT):
    """Code 5.  fluid_return_mapping, constitutive_models.py:142-213 (a true
    matrix product at :208), paired with the StVK stress as material 3."""
    F, mu, lam, yld = _prep(F, mu, lam, yld)
    U, s, V = svd_taichi(F)                                             # :158
    eps = np.log(np.maximum(np.abs(s), 0.01))                           # :162-166
    tr = eps.sum(-1)                                                    # :167
    st = 2.0 * mu[:, None] * (eps - tr[:, None] / 3.0)                  # :168-171
    stn = np.linalg.norm(st, axis=-1)                                   # :172
    y = stn - math.sqrt(2.0 / 3.0) * yld                                # :176
    plastic = y > 0                                                     # :182
    mu_hat = mu * (s ** 2).sum(-1) / 3.0                                # :184
    pf = 1.0 + PVISC / (2.0 * mu_hat * dt)                              # :185
    snn = stn - y / pf                                                  # :188
    with np.errstate(invalid="ignore", divide="ignore"):
        s_new = (snn / stn)[:, None] * st                               # :189
    eps_new = (1.0 / (2.0 * mu[:, None])) * s_new + tr[:, None] / 3.0   # :192
    with np.errstate(over="ignore", invalid="ignore"):  # as in metal
        Fp = U @ _diag(np.exp(eps_new)) @ _T(V)                         # :195-208
    Fn = np.where(plastic[:, None, None], Fp, F)                        # :209-211
    U2, s2, V2 = svd_taichi(Fn)
    tau = _sym(stress_stvk(Fn, U2, s2, V2, mu, lam))
    return Result(Fn, tau, yld, plastic.astype(int), y / (2.0 * mu), s)


REFERENCE = {0: jelly, 1: metal, 2: sand, 3: foam, 4: jelly_fcr, 5: fluid}


# ------------------------------------------------------------------- inputs --
def haar(rng, n):
    """n Haar-distributed rotations."""
    Q, R = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    Q = Q * np.sign(np.diagonal(R, axis1=-2, axis2=-1))[:, None, :]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def _stretches(cls, rng, n):
    u = rng.uniform
    if cls in ("moderate", "reflect"):
        s = np.stack([u(1.1, 1.3, n), u(0.9, 1.05, n), u(0.7, 0.85, n)], 1)
        if cls == "reflect":
            s[:, 2] *= -1.0
        return s
    if cls == "near_id":
        return 1.0 + 1e-4 * rng.standard_normal((n, 3))
    if cls == "tiny":
        return 1.0 + 1e-6 * rng.standard_normal((n, 3))
    if cls == "pair":
        a = u(0.8, 1.2, n)
        return np.stack([a, a, u(0.6, 0.75, n)], 1)
    if cls == "triple":
        return np.repeat(u(0.7, 1.3, n)[:, None], 3, 1)
    if cls == "large":
        return np.exp(u(-1.2, 1.2, (n, 3)))
    if cls == "clamp":
        return np.stack([u(0.9, 1.1, n), u(0.5, 0.8, n), u(0.002, 0.03, n)], 1)
    raise KeyError(cls)


TINY_IDENTITY = slice(0, 64)     # `tiny`: F = I exactly
TINY_ROTATION = slice(64, 128)   # `tiny`: F a pure rotation (rounded to f32)


@functools.lru_cache(maxsize=None)
def inputs(cls):
    """(F, mu, lam) of a class, f32, read-only: F = R1 diag(s) R2^T with Haar
    rotations, E log-uniform in [1e4, 1e7], nu uniform in [0.1, 0.45]."""
    n = N_ROWS
    rng = np.random.default_rng(1000 + CLASSES.index(cls))
    R1, R2 = haar(rng, n), haar(rng, n)
    s = _stretches(cls, rng, n)
    if cls == "tiny":
        s[TINY_IDENTITY] = 1.0
        s[TINY_ROTATION] = 1.0
        R2[TINY_IDENTITY] = R1[TINY_IDENTITY]
    F = ((R1 * s[:, None, :]) @ _T(R2)).astype(np.float32)
    if cls == "tiny":
        F[TINY_IDENTITY] = np.eye(3, dtype=np.float32)
    E = np.exp(rng.uniform(math.log(1e4), math.log(1e7), n)).astype(np.float32)
    nu = rng.uniform(0.1, 0.45, n).astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    mu = E / (two * (one + nu))
    lam = E * nu / ((one + nu) * (one - two * nu))
    assert mu.dtype == np.float32 and lam.dtype == np.float32
    for a in (F, mu, lam):
        a.setflags(write=False)
    return F, mu, lam


def singular_gap(s):
    return np.minimum(s[:, 0] - s[:, 1], s[:, 1] - np.abs(s[:, 2]))


@functools.lru_cache(maxsize=None)
def yields(code, cls):
    """The per-row f32 yield of (material, class), from the reference's own
    discriminant so that both branches hold rows: even rows plastic
    (factor U[0.2, 0.99]), odd rows elastic (U[1.01, 3])."""
    F, mu, lam = inputs(cls)
    n = len(F)
    if code not in (1, 3, 5):
        y = np.full(n, 0.005, np.float32)  # not read by these materials
        y.setflags(write=False)
        return y
    rng = np.random.default_rng(2000 + 10 * CLASSES.index(cls) + code)
    fac = np.where(np.arange(n) % 2 == 0, rng.uniform(0.2, 0.99, n), rng.uniform(1.01, 3.0, n))
    # c: the yield at which the row sits on its surface (the discriminant at yield 0, rescaled)
    if code == 1:
        c = metal_cond_norm(F, mu, lam)                                   # :82
    elif code == 5:
        c = fluid(F, mu, lam, 0.0).disc * 2.0 * mu / math.sqrt(2.0 / 3.0)  # :176
    else:
        c = foam(F, mu, lam, 0.0).disc * 2.0 * mu / (0.8 * math.sqrt(2.0 / 3.0))  # :236
    y = (c * fac).astype(np.float32)
    if code == 3:
        if cls not in FOAM_SPLIT:
            y[:] = 1e30
        else:
            r = foam(F, mu, lam, y)
            bad = (np.abs(r.disc) < FOAM_MARGIN) | ((r.branch == PLASTIC) & (singular_gap(r.s_trial) < FOAM_GAP))
            y[bad] = 1e30  # elastic instead of dropped
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def expected(code, cls):
    """The float64 reference result of (material, class) on inputs() and yields()."""
    F, mu, lam = inputs(cls)
    return REFERENCE[code](F, mu, lam, yields(code, cls))


def compare_masks(code, res):
    """(rows whose F is compared, rows whose tau is compared).  Everything,
    except foam's plastic rows under the gap or the margin, and the stress of
    sand rows whose reference stress is not finite (kept F with a negative sigma)."""
    n = len(res.F)
    mF = np.ones(n, bool)
    if code == 3:
        mF = ~((res.branch == PLASTIC) & (singular_gap(res.s_trial) < FOAM_GAP)) & (np.abs(res.disc) >= FOAM_MARGIN)
    mT = mF & np.isfinite(res.tau).all((1, 2))
    return mF, mT


def branch_margin(code, res):
    """Distance (strain units) of each row from the nearest branch surface."""
    m = np.abs(res.disc)
    if code == 2:
        m = np.where(res.disc > 0, np.minimum(m, np.abs(res.tr)), m)
    return m


# ----------------------------------------------------------------- measures --
def _amax(A):
    return np.abs(A).reshape(len(A), -1).max(1)


def err_F(F, F_ref):
    """Per row: max|dF| / max(1, max|F_ref|)."""
    F_ref = np.asarray(F_ref, np.float64).reshape(-1, 9)
    return _amax(np.asarray(F, np.float64).reshape(-1, 9) - F_ref) / np.maximum(1.0, _amax(F_ref))


def err_tau(code, tau, tau_ref, F_ref, mu, lam):
    """Per row: max|dtau| / ((2 mu + 3 lam) max(1, max|F_ref|)^p k), p = 2 for FCR
    and 1 otherwise, k = max(1, 1 / min|sigma(F_ref)|) for sand and 1 otherwise."""
    F_ref = np.asarray(F_ref, np.float64).reshape(-1, 3, 3)
    mu, lam = np.asarray(mu, np.float64), np.asarray(lam, np.float64)
    scale = (2.0 * mu + 3.0 * lam) * np.maximum(1.0, _amax(F_ref)) ** (2 if code == 4 else 1)
    if code == 2:
        scale = scale * np.maximum(1.0, 1.0 / np.linalg.svd(F_ref, compute_uv=False).min(-1))
    d = np.asarray(tau, np.float64).reshape(-1, 9) - np.asarray(tau_ref, np.float64).reshape(-1, 9)
    return _amax(d) / scale


def err_yield(y, y_ref, mu):
    return np.abs(np.asarray(y, np.float64) - np.asarray(y_ref, np.float64)) / (2.0 * np.asarray(mu, np.float64))


def measures(code, cls, F_out, tau_out, y_out, res=None, mu=None, lam=None):
    """The three maxima (F, tau, yield) of an implementation's outputs against
    the reference over the compared rows, and finiteness wherever compared."""
    if res is None:
        res = expected(code, cls)
        _, mu, lam = inputs(cls)
    mF, mT = compare_masks(code, res)
    F_out = np.asarray(F_out).reshape(-1, 3, 3)
    tau_out = np.asarray(tau_out).reshape(-1, 3, 3)
    assert np.isfinite(F_out[mF]).all() and np.isfinite(tau_out[mT]).all() and np.isfinite(y_out).all()
    eF = err_F(F_out[mF], res.F[mF]).max() if mF.any() else 0.0
    eT = err_tau(code, tau_out[mT], res.tau[mT], res.F[mT], mu[mT], lam[mT]).max() if mT.any() else 0.0
    eY = err_yield(y_out, res.yld, mu).max()
    return float(eF), float(eT), float(eY)


# ---------------------------------------------------------------- SVD checks --
SVD_FAMILIES = CLASSES + ("random",)


@functools.lru_cache(maxsize=None)
def svd_inputs(family):
    """The eight classes plus test_gpu_constitutive.py's random family
    (I + 0.05 N and plain N(0,1) matrices)."""
    if family != "random":
        return inputs(family)[0]
    rng = np.random.default_rng(0)
    A = (np.eye(3)[None] + 0.05 * rng.standard_normal((N_ROWS, 3, 3))).astype(np.float32)
    A[:512] = rng.standard_normal((512, 3, 3))
    A.setflags(write=False)
    return A


SVD_MEASURES = ("sigma", "orth", "det", "recon")


def svd_measures(A, U, S, V):
    """Per-row maxima of an f32 SVD against np.linalg.svd in float64:
    sigma: |sigma - sigma_ref| / max(1, sigma1); orth: max(|U^T U - I|, |V^T V - I|);
    det: max(|det U - 1|, |det V - 1|); recon: |U S V^T - A| / max(1, |A|)."""
    A = np.asarray(A, np.float64).reshape(-1, 3, 3)
    U = np.asarray(U, np.float64).reshape(-1, 3, 3)
    V = np.asarray(V, np.float64).reshape(-1, 3, 3)
    S = np.asarray(S, np.float64).reshape(-1, 3)
    _, s_ref, _ = svd_taichi(A)
    I = np.eye(3)
    out = {
        "sigma": (np.abs(S - s_ref).max(1) / np.maximum(1.0, s_ref[:, 0])).max(),
        "orth": max(_amax(_T(U) @ U - I).max(), _amax(_T(V) @ V - I).max()),
        "det": max(np.abs(np.linalg.det(U) - 1.0).max(), np.abs(np.linalg.det(V) - 1.0).max()),
        "recon": (_amax(U @ _diag(S) @ _T(V) - A) / np.maximum(1.0, _amax(A))).max(),
    }
    return {k: float(v) for k, v in out.items()}
