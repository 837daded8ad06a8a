"""CPU: the float64 constitutive reference (constitutive_ref.py) pinned by
algebra that never touches the oracle, then the f32 oracle pinned to that
reference on eight input classes x six materials, per row, in strain units.

ORACLE_BOUNDS / ORACLE_SVD_BOUNDS below are the yardstick of
test_gpu_constitutive_ref.py: each entry is twice the oracle-versus-float64
maximum measured on the CPU, rounded up to one digit.
`pytest -s tests/test_constitutive_ref.py` prints the measured values.
"""
import ctypes
import math

import numpy as np
import pytest

import oracle as O
import constitutive_ref as R
from constitutive_ref import CLASSES, KEPT, PLASTIC, ROTATION

CODES = (0, 1, 2, 3, 4, 5)

# (F, tau, yield) bounds per material code and class: 2 x the oracle's measured
# maximum against float64, rounded up to one digit; 0 where the oracle is exact
# (row copies, the zero stress of jelly as written, an untouched yield).
ORACLE_BOUNDS = {
    0: {  # jelly
        'moderate': (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'near_id' : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'tiny'    : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'pair'    : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'triple'  : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'large'   : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'clamp'   : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
        'reflect' : (0e+00, 0e+00, 0e+00),  # measured 0.00e+00 0.00e+00 0.00e+00
    },
    1: {  # metal
        'moderate': (2e-06, 2e-06, 7e-07),  # measured 7.42e-07 9.37e-07 3.16e-07
        'near_id' : (2e-06, 3e-06, 3e-06),  # measured 8.07e-07 1.04e-06 1.18e-06
        'tiny'    : (2e-06, 3e-06, 3e-06),  # measured 9.25e-07 1.10e-06 1.48e-06
        'pair'    : (2e-06, 2e-06, 2e-06),  # measured 9.07e-07 8.13e-07 6.03e-07
        'triple'  : (2e-06, 3e-06, 3e-06),  # measured 9.54e-07 1.42e-06 1.44e-06
        'large'   : (2e-05, 4e-06, 8e-07),  # measured 5.55e-06 1.57e-06 3.69e-07
        'clamp'   : (2e-06, 2e-06, 4e-06),  # measured 6.40e-07 6.65e-07 1.68e-06
        'reflect' : (2e-06, 8e-06, 2e-06),  # measured 8.54e-07 3.67e-06 5.89e-07
    },
    2: {  # sand
        'moderate': (4e-06, 2e-06, 0e+00),  # measured 1.51e-06 9.92e-07 0.00e+00
        'near_id' : (4e-06, 2e-06, 0e+00),  # measured 1.53e-06 8.66e-07 0.00e+00
        'tiny'    : (3e-06, 3e-06, 0e+00),  # measured 1.01e-06 1.01e-06 0.00e+00
        'pair'    : (3e-06, 2e-06, 0e+00),  # measured 1.40e-06 8.92e-07 0.00e+00
        'triple'  : (2e-06, 2e-06, 0e+00),  # measured 5.67e-07 6.95e-07 0.00e+00
        'large'   : (2e-05, 2e-06, 0e+00),  # measured 7.80e-06 7.13e-07 0.00e+00
        'clamp'   : (9e-07, 9e-07, 0e+00),  # measured 4.04e-07 4.01e-07 0.00e+00
        'reflect' : (6e-06, 2e-06, 0e+00),  # measured 2.80e-06 9.15e-07 0.00e+00
    },
    3: {  # foam
        'moderate': (6e-06, 9e-06, 0e+00),  # measured 2.67e-06 4.32e-06 0.00e+00
        'near_id' : (0e+00, 1e-06, 0e+00),  # measured 0.00e+00 4.74e-07 0.00e+00
        'tiny'    : (0e+00, 2e-06, 0e+00),  # measured 0.00e+00 5.41e-07 0.00e+00
        'pair'    : (0e+00, 2e-06, 0e+00),  # measured 0.00e+00 5.37e-07 0.00e+00
        'triple'  : (0e+00, 2e-06, 0e+00),  # measured 0.00e+00 7.79e-07 0.00e+00
        'large'   : (2e-05, 4e-05, 0e+00),  # measured 5.94e-06 1.55e-05 0.00e+00
        'clamp'   : (8e-07, 2e-06, 0e+00),  # measured 3.85e-07 7.37e-07 0.00e+00
        'reflect' : (2e-06, 8e-06, 0e+00),  # measured 5.98e-07 3.67e-06 0.00e+00
    },
    4: {  # fcr
        'moderate': (0e+00, 6e-07, 0e+00),  # measured 0.00e+00 2.81e-07 0.00e+00
        'near_id' : (0e+00, 8e-07, 0e+00),  # measured 0.00e+00 3.61e-07 0.00e+00
        'tiny'    : (0e+00, 9e-07, 0e+00),  # measured 0.00e+00 4.21e-07 0.00e+00
        'pair'    : (0e+00, 1e-06, 0e+00),  # measured 0.00e+00 4.77e-07 0.00e+00
        'triple'  : (0e+00, 8e-07, 0e+00),  # measured 0.00e+00 3.52e-07 0.00e+00
        'large'   : (0e+00, 6e-06, 0e+00),  # measured 0.00e+00 2.72e-06 0.00e+00
        'clamp'   : (0e+00, 5e-07, 0e+00),  # measured 0.00e+00 2.50e-07 0.00e+00
        'reflect' : (0e+00, 2e-06, 0e+00),  # measured 0.00e+00 9.50e-07 0.00e+00
    },
    5: {  # fluid
        'moderate': (2e-06, 2e-06, 0e+00),  # measured 8.17e-07 9.56e-07 0.00e+00
        'near_id' : (2e-06, 2e-06, 0e+00),  # measured 8.68e-07 8.64e-07 0.00e+00
        'tiny'    : (2e-06, 3e-06, 0e+00),  # measured 9.62e-07 1.10e-06 0.00e+00
        'pair'    : (2e-06, 2e-06, 0e+00),  # measured 8.53e-07 9.39e-07 0.00e+00
        'triple'  : (2e-06, 3e-06, 0e+00),  # measured 9.58e-07 1.42e-06 0.00e+00
        'large'   : (7e-06, 3e-06, 0e+00),  # measured 3.18e-06 1.28e-06 0.00e+00
        'clamp'   : (2e-06, 2e-06, 0e+00),  # measured 6.88e-07 9.64e-07 0.00e+00
        'reflect' : (5e-06, 8e-06, 0e+00),  # measured 2.26e-06 3.67e-06 0.00e+00
    },
}

# (sigma, orth, det, recon) of O.svd3 against np.linalg.svd, same rule.
ORACLE_SVD_BOUNDS = {
    'moderate': (1e-06, 2e-06, 2e-06, 2e-06),  # measured 4.87e-07 9.25e-07 9.57e-07 9.05e-07
    'near_id' : (2e-06, 2e-06, 3e-06, 2e-06),  # measured 5.10e-07 9.66e-07 1.11e-06 9.29e-07
    'tiny'    : (2e-06, 3e-06, 3e-06, 3e-06),  # measured 7.04e-07 1.13e-06 1.11e-06 1.12e-06
    'pair'    : (2e-06, 3e-06, 3e-06, 3e-06),  # measured 6.55e-07 1.00e-06 1.22e-06 1.17e-06
    'triple'  : (2e-06, 3e-06, 3e-06, 3e-06),  # measured 6.35e-07 1.01e-06 1.24e-06 1.10e-06
    'large'   : (2e-06, 2e-06, 3e-06, 2e-05),  # measured 5.36e-07 9.02e-07 1.05e-06 6.44e-06
    'clamp'   : (1e-06, 3e-06, 3e-06, 2e-06),  # measured 4.99e-07 1.07e-06 1.21e-06 8.14e-07
    'reflect' : (1e-06, 2e-06, 3e-06, 2e-06),  # measured 4.79e-07 9.03e-07 1.06e-06 9.65e-07
    'random'  : (2e-06, 2e-06, 3e-06, 7e-06),  # measured 5.26e-07 8.90e-07 1.05e-06 3.28e-06
}


def round_up_1(x):
    """x rounded up to one significant digit (0 stays 0)."""
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x))
    m = math.ceil(x / 10.0 ** e - 1e-9)
    return float(f"{m}e{e}")


# ---------------------------------------------------------- oracle drivers --
def oracle_constitutive(code, F, mu, lam, yld, dt=R.DT):
    """The oracle's entry points on n rows: om_stress through OracleMPM for
    codes 0-4, O.fluid_return_mapping for 5.  Returns F, tau, yield (f32)."""
    n = len(F)
    F = np.ascontiguousarray(F, np.float32).reshape(n, 9)
    if code == 5:
        Fo, To = O.fluid_return_mapping(F, mu, lam, yld, dt, R.PVISC)
        return Fo.reshape(n, 9), To.reshape(n, 9), np.array(yld, np.float32)
    material = {0: "jelly", 1: "metal", 2: "sand", 3: "foam", 4: "jelly"}[code]
    s = O.OracleMPM(np.full((n, 3), 1.0, np.float32), np.zeros((n, 6), np.float32), np.ones(n, np.float32),
                    n_grid=8, material=material, jelly_quirk=code != 4)
    s.F_trial[:] = F
    s.mu[:], s.lam[:], s.yield_stress[:] = mu, lam, yld
    with np.errstate(all="ignore"):
        O.lib().om_stress(ctypes.byref(s._st), ctypes.c_float(dt))
    return s.F.copy(), s.stress.copy(), s.yield_stress.copy()


def oracle_svd(A):
    out = [O.svd3(a) for a in A]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


# ------------------------------------------------ (a) the reference's algebra --
def _dev_tau_norm(F, mu, lam):
    return R.metal_cond_norm(F, mu, lam)


@pytest.mark.parametrize("cls", CLASSES)
def test_ref_metal_plastic_lands_on_yield_surface(cls):
    F, mu, lam = R.inputs(cls)
    yld = R.yields(1, cls).astype(np.float64)
    r = R.expected(1, cls)
    p = r.branch == PLASTIC
    mu64 = mu.astype(np.float64)
    # ||dev tau(F_new)|| = yld_old up to the 1e-6 of constitutive_models.py:84 (2 mu 1e-6 in stress)
    cn = _dev_tau_norm(r.F[p], mu[p], lam[p])
    assert np.all(np.abs(cn - yld[p]) / (2 * mu64[p]) <= 1e-6 * (1 + 1e-6) + 1e-12)
    # tr eps kept: the flow is deviatoric
    tr = lambda A: np.log(np.maximum(R.svd_taichi(A)[1], 0.01)).sum(-1)
    assert np.abs(tr(r.F[p]) - tr(F[p].astype(np.float64))).max() < 1e-12
    # hardening: yld + 2 mu xi dgamma, dgamma = ||eps_hat|| + 1e-6 - yld / 2mu  (:84-85, :98)
    eps = np.log(np.maximum(R.svd_taichi(F[p])[1], 0.01))
    ehn = np.linalg.norm(eps - eps.mean(-1, keepdims=True), axis=-1) + 1e-6
    dg = ehn - yld[p] / (2 * mu64[p])
    assert np.all(dg > 0)
    np.testing.assert_allclose(r.yld[p], yld[p] + 2 * mu64[p] * dg, rtol=1e-13)
    # elastic rows: F and the yield unchanged
    assert np.array_equal(r.F[~p], F[~p].astype(np.float64)) and np.array_equal(r.yld[~p], yld[~p])


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("cls", CLASSES)
def test_ref_kept_rows_return_F(code, cls):
    F, _, _ = R.inputs(cls)
    r = R.expected(code, cls)
    k = r.branch == KEPT
    assert np.array_equal(r.F[k], F[k].astype(np.float64))
    if code != 1:
        assert np.array_equal(r.yld, R.yields(code, cls).astype(np.float64))


@pytest.mark.parametrize("cls", CLASSES)
def test_ref_sand_cone_and_tension(cls):
    F, mu, lam = R.inputs(cls)
    r = R.expected(2, cls)
    p = r.branch == PLASTIC
    if p.any():  # projected onto the cone: a second pass finds dgamma = 0
        again = R.sand(r.F[p], mu[p], lam[p], 0.0)
        assert np.abs(again.disc).max() < 1e-12
    t = r.branch == ROTATION
    if t.any():  # tr > 0: a rotation, zero stress
        Ft = r.F[t]
        assert np.abs(np.swapaxes(Ft, 1, 2) @ Ft - np.eye(3)).max() < 1e-13
        assert np.abs(np.linalg.det(Ft) - 1.0).max() < 1e-13  # U, V rotations, also where det F < 0
        scale = (2.0 * mu[t] + 3.0 * lam[t]).astype(np.float64)
        assert (np.abs(r.tau[t]).reshape(t.sum(), -1).max(1) / scale).max() < 1e-13


def test_ref_stress_vanishes_at_rotation():
    rng = np.random.default_rng(3)
    Q = R.haar(rng, 64)
    mu, lam = np.full(64, 8.3e4), np.full(64, 5.6e4)
    for fn in (R.jelly_fcr, R.metal, R.foam, R.fluid):
        r = fn(Q, mu, lam, 1e30)
        assert np.abs(r.tau).max() / (2 * 8.3e4 + 3 * 5.6e4) < 1e-13, fn.__name__


def test_ref_small_strain_limit():
    """F = I + eps E, E symmetric: FCR and StVK reduce to 2 mu eps E + lam eps tr(E) I to O(eps^2)."""
    rng = np.random.default_rng(4)
    E = rng.standard_normal((64, 3, 3))
    E = (E + np.swapaxes(E, 1, 2)) / 2
    e = 1e-6
    mu, lam = np.full(64, 8.3e4), np.full(64, 5.6e4)
    lin = 2 * 8.3e4 * e * E + 5.6e4 * e * np.trace(E, axis1=1, axis2=2)[:, None, None] * np.eye(3)
    for fn in (R.jelly_fcr, R.metal, R.foam, R.fluid):
        r = fn(np.eye(3) + e * E, mu, lam, 1e30)
        # the O(eps^2) term, with |E| up to ~4: a few tens of eps^2 (2 mu + 3 lam)
        assert np.abs(r.tau - lin).max() / (2 * 8.3e4 + 3 * 5.6e4) < 100 * e * e, fn.__name__


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("cls", ["moderate", "large", "clamp", "reflect", "near_id"])
def test_ref_objectivity(code, cls):
    """tau(QF) = Q tau(F) Q^T and F_new(QF) = Q F_new(F); foam's plastic rows excepted (F13)."""
    F, mu, lam = R.inputs(cls)
    yld = R.yields(code, cls)
    r = R.expected(code, cls)
    Q = R.haar(np.random.default_rng(5), len(F))
    rq = R.REFERENCE[code](Q @ F.astype(np.float64), mu, lam, yld)
    # rows a rounding away from a branch surface may change branch under Q
    ok = R.branch_margin(code, r) > 1e-9
    if code == 3:
        ok &= r.branch == KEPT
    assert ok.mean() > 0.4
    assert np.array_equal(rq.branch[ok], r.branch[ok])
    assert R.err_F(rq.F[ok], Q[ok] @ r.F[ok]).max() < 1e-12
    fin = ok & np.isfinite(r.tau).all((1, 2))
    want = Q[fin] @ r.tau[fin] @ np.swapaxes(Q[fin], 1, 2)
    assert R.err_tau(code, rq.tau[fin], want, r.F[fin], mu[fin], lam[fin]).max() < 1e-11
    np.testing.assert_allclose(rq.yld[ok], r.yld[ok], rtol=1e-10)


def test_ref_svd_convention():
    for cls in CLASSES:
        A = R.inputs(cls)[0].astype(np.float64)
        U, s, V = R.svd_taichi(A)
        assert np.all(s[:, 0] >= s[:, 1]) and np.all(s[:, 1] >= np.abs(s[:, 2]))
        assert np.abs(np.linalg.det(U) - 1).max() < 1e-12 and np.abs(np.linalg.det(V) - 1).max() < 1e-12
        assert np.array_equal(np.sign(s[:, 2]), np.sign(np.linalg.det(A)))
        assert np.abs(U @ R._diag(s) @ np.swapaxes(V, 1, 2) - A).max() < 1e-13


# ------------------------------------------------------ (c) caps and branches --
@pytest.mark.parametrize("cls", CLASSES)
def test_exclusion_caps(cls):
    """Conditions, not measurements: nothing is excluded for metal, sand, FCR,
    fluid and jelly except the stress of sand's kept rows with det F < 0; foam
    drops at most 5% of a class."""
    for code in CODES:
        r = R.expected(code, cls)
        mF, mT = R.compare_masks(code, r)
        if code == 3:
            assert (~mF).mean() <= R.FOAM_DROP_CAP and (~mT).mean() <= R.FOAM_DROP_CAP
        elif code == 2 and cls == "reflect":
            assert mF.all()
            assert np.array_equal(~mT, r.branch == KEPT)
        else:
            assert mF.all() and mT.all(), code


# the classes built to hold every branch of a material
BRANCH_CLASSES = {1: CLASSES, 5: CLASSES, 3: R.FOAM_SPLIT, 2: ("large",)}


def test_branch_coverage():
    for code, classes in BRANCH_CLASSES.items():
        for cls in classes:
            r = R.expected(code, cls)
            for b in ((KEPT, PLASTIC, ROTATION) if code == 2 else (KEPT, PLASTIC)):
                assert (r.branch == b).mean() >= 0.05, (code, cls, b)
    for cls in CLASSES:  # foam elsewhere: every row elastic
        if cls not in R.FOAM_SPLIT:
            assert (R.expected(3, cls).branch == KEPT).all()
    # foam's compared plastic rows are clear of the surface and of a repeated sigma
    for cls in R.FOAM_SPLIT:
        r = R.expected(3, cls)
        p = r.branch == PLASTIC
        assert R.singular_gap(r.s_trial)[p].min() >= R.FOAM_GAP
        assert np.abs(r.disc).min() >= R.FOAM_MARGIN


# ------------------------------------------- (b) the oracle against float64 --
@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("cls", CLASSES)
def test_oracle_vs_float64(code, cls):
    F, mu, lam = R.inputs(cls)
    yld = R.yields(code, cls)
    r = R.expected(code, cls)
    Fo, To, yo = oracle_constitutive(code, F, mu, lam, yld.copy())
    got = R.measures(code, cls, Fo, To, yo)
    print(f"oracle vs f64 {R.MATERIALS[code]:6s} {cls:9s} F {got[0]:.2e} tau {got[1]:.2e} yield {got[2]:.2e}")
    bound = ORACLE_BOUNDS[code][cls]
    assert all(g <= b for g, b in zip(got, bound)), (got, bound)
    # rows clear of a branch surface: kept rows are copies, bit for bit
    k = (r.branch == KEPT) & (R.branch_margin(code, r) >= R.BRANCH_MARGIN)
    assert np.array_equal(Fo.reshape(-1, 9)[k].view(np.uint32), F.reshape(-1, 9)[k].view(np.uint32))
    assert np.array_equal(yo[k].view(np.uint32), yld[k].view(np.uint32))
    if code != 1:
        assert np.array_equal(yo.view(np.uint32), yld.view(np.uint32))


@pytest.mark.parametrize("family", R.SVD_FAMILIES)
def test_oracle_svd_vs_float64(family):
    A = R.svd_inputs(family)
    U, S, V = oracle_svd(A)
    got = R.svd_measures(A, U, S, V)
    print(f"oracle svd vs f64 {family:9s} " + " ".join(f"{k} {got[k]:.2e}" for k in R.SVD_MEASURES))
    bound = ORACLE_SVD_BOUNDS[family]
    assert all(got[k] <= b for k, b in zip(R.SVD_MEASURES, bound)), (got, bound)


def test_bounds_rule():
    """Every committed bound is one significant digit (2 x measured, rounded up)."""
    for tab in (ORACLE_BOUNDS, ORACLE_SVD_BOUNDS):
        for row in tab.values():
            for b in (row.values() if isinstance(row, dict) else [row]):
                assert all(x == round_up_1(x) for x in b)
