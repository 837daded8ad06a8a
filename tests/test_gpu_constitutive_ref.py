"""GPU: gsmpm_constitutive, gsmpm_constitutive_mixed and gsmpm_svd3 against the
float64 reference of constitutive_ref.py, per row, on eight input classes.

The yardstick is the f32 oracle's own distance from float64
(test_constitutive_ref.py: ORACLE_BOUNDS, ORACLE_SVD_BOUNDS, measured on the
CPU).  A device bound is FACTOR x the oracle's entry, never above CEILING, or an
entry of WIDENED with its cause named; none is derived from device output.
`pytest -s` prints the measured device maxima (recorded in DESIGN.md 3.8).
"""
import numpy as np
import pytest

import constitutive_ref as R
from constitutive_ref import CLASSES, KEPT
from mixed_oracle import material_codes
from test_constitutive_ref import BRANCH_CLASSES, CODES, ORACLE_BOUNDS, ORACLE_SVD_BOUNDS

pytestmark = pytest.mark.gpu

# Device against oracle, each of rounding size: the NR-refined rsqrt / sqrt of
# the fast SVD (~0.5 ulp) against correctly rounded, device logf / expf at
# 1-2 ulp, and U, s, V reused in place of a fresh SVD of the rounded product.
FACTOR = 4.0
CEILING = 1e-4  # the project's per-element parity bound, same units
# (code, class) -> (F, tau, yield): entries wider than FACTOR x the oracle's,
# each with its cause (a documented shortcut), none past CEILING.
WIDENED = {}
WIDENED_SVD = {}


def device_bound(code, cls):
    if (code, cls) in WIDENED:
        b = WIDENED[(code, cls)]
        assert all(x <= CEILING for x in b)
        return b
    return tuple(min(FACTOR * b, CEILING) for b in ORACLE_BOUNDS[code][cls])


def device_svd_bound(family):
    if family in WIDENED_SVD:
        b = WIDENED_SVD[family]
        assert all(x <= CEILING for x in b)
        return b
    return tuple(min(FACTOR * b, CEILING) for b in ORACLE_SVD_BOUNDS[family])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(dev, code, n, F, mu, lam, yld, ids=None, jelly_fcr=0, Fo=None, To=None):
    """One launch on the first n rows of the given host arrays; returns F, tau, yield as numpy."""
    import torch
    from gsmpm._lib import LIB, check, ptr, stream_of
    t = lambda a: torch.from_numpy(np.array(a, np.float32)).to(dev)  # a copy: the shared inputs are read-only
    Ft, tm, tl, ty = t(np.reshape(F, (-1, 9))), t(mu), t(lam), t(yld)
    Fg = torch.empty_like(Ft) if Fo is None else t(Fo)
    Tg = torch.empty_like(Ft) if To is None else t(To)
    if ids is None:
        check(LIB.gsmpm_constitutive(code, ptr(Ft), n, ptr(tm), ptr(tl), ptr(ty), R.DT, ptr(Fg), ptr(Tg),
                                     stream_of(dev)))
    else:
        tid = t(ids)
        check(LIB.gsmpm_constitutive_mixed(ptr(tid), ptr(Ft), n, ptr(tm), ptr(tl), ptr(ty), R.DT, jelly_fcr, ptr(Fg),
                                           ptr(Tg), stream_of(dev)))
    return Fg.cpu().numpy(), Tg.cpu().numpy(), ty.cpu().numpy()


def _check_rows(code, cls, rows, Fg, Tg, yg, yld, tag):
    """The three measures, finiteness and the bit-exact copies of the given
    rows (a bool mask) of one material against its float64 reference."""
    F, mu, lam = R.inputs(cls)
    r = R.expected(code, cls)
    mF, mT = R.compare_masks(code, r)
    mF, mT = mF & rows, mT & rows
    Fg3, Tg3 = Fg.reshape(-1, 3, 3), Tg.reshape(-1, 3, 3)
    assert np.isfinite(Fg3[mF]).all() and np.isfinite(Tg3[mT]).all() and np.isfinite(yg[rows]).all()
    eF = R.err_F(Fg3[mF], r.F[mF]).max() if mF.any() else 0.0
    eT = R.err_tau(code, Tg3[mT], r.tau[mT], r.F[mT], mu[mT], lam[mT]).max() if mT.any() else 0.0
    eY = R.err_yield(yg[rows], r.yld[rows], mu[rows]).max()
    bound = device_bound(code, cls)
    print(f"{tag} {R.MATERIALS[code]:6s} {cls:9s} F {eF:.2e} tau {eT:.2e} yield {eY:.2e}  bound "
          + " ".join(f"{b:.0e}" for b in bound))
    assert eF <= bound[0] and eT <= bound[1] and eY <= bound[2], ((eF, eT, eY), bound)
    # kept rows clear of the branch surface are copies of F_trial, their yield untouched
    k = rows & (r.branch == KEPT) & (R.branch_margin(code, r) >= R.BRANCH_MARGIN)
    assert np.array_equal(_bits(Fg)[k], _bits(F.reshape(-1, 9))[k])
    assert np.array_equal(_bits(yg)[k], _bits(yld)[k])
    if code != 1:
        assert np.array_equal(_bits(yg)[rows], _bits(yld)[rows])
    if code == 2:  # a kept row with det F < 0 has no finite reference stress: only F, bit for bit
        nf = rows & ~np.isfinite(r.tau).all((1, 2))
        assert np.array_equal(_bits(Fg)[nf], _bits(F.reshape(-1, 9))[nf])
    return k


_WIDE = ("moderate", "pair", "large", "clamp", "reflect")
COPY_CLASSES = {0: CLASSES, 1: _WIDE, 2: ("moderate", "large", "reflect"), 3: CLASSES, 5: _WIDE}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("code", CODES)
def test_constitutive_vs_float64(dev, code, cls):
    F, mu, lam = R.inputs(cls)
    yld = R.yields(code, cls)
    n = len(F)
    Fg, Tg, yg = _launch(dev, code, n, F, mu, lam, yld)
    assert np.isfinite(Fg).all()  # the reference's F is finite on every row
    k = _check_rows(code, cls, np.ones(n, bool), Fg, Tg, yg, yld, "device vs f64")
    # the copy check is not vacuous where the class spreads its rows wider than
    # BRANCH_MARGIN around the surface (near_id, tiny and triple do not, by construction)
    if code in COPY_CLASSES and cls in COPY_CLASSES[code]:
        assert k.mean() >= 0.04, k.mean()


def test_branch_coverage():
    """Both branches of metal, foam and fluid and all three of sand hold at
    least 5% of the rows in the classes built for them (the reference's output)."""
    for code, classes in BRANCH_CLASSES.items():
        for cls in classes:
            b = R.expected(code, cls).branch
            for v in range(3 if code == 2 else 2):
                assert (b == v).mean() >= 0.05, (code, cls, v)


SENTINEL = np.uint32(0x7FC12345)  # a NaN payload no kernel produces


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("n", [0, 1])
def test_degenerate_sizes(dev, code, n):
    """n = 1 and n = 0 through the same entry: rows from n on keep their bits."""
    cls = "moderate"
    F, mu, lam = R.inputs(cls)
    yld = R.yields(code, cls)
    m = 4
    fill = np.full((m, 9), SENTINEL, np.uint32).view(np.float32)
    for ids in (None, np.full(m, code if code < 4 else 0, np.float32)):
        if ids is not None and code == 5:
            continue  # the mixed entry has no fluid
        Fg, Tg, yg = _launch(dev, code, n, F[:m], mu[:m], lam[:m], yld[:m], ids=ids, jelly_fcr=int(code == 4),
                             Fo=fill, To=fill)
        assert (_bits(Fg)[n:] == SENTINEL).all() and (_bits(Tg)[n:] == SENTINEL).all()
        assert np.array_equal(_bits(yg)[n:], _bits(yld[:m])[n:])
        if n == 1:
            r = R.expected(code, cls)
            bound = device_bound(code, cls)
            assert R.err_F(Fg[:1].reshape(1, 3, 3), r.F[:1])[0] <= bound[0]
            assert R.err_tau(code, Tg[:1], r.tau[:1], r.F[:1], mu[:1], lam[:1])[0] <= bound[1]
            assert R.err_yield(yg[:1], r.yld[:1], mu[:1])[0] <= bound[2]


# ------------------------------------------------------------ mixed dispatch --
ODD_IDS = np.array([7.0, -1.0, 0.5, np.nan], np.float32)  # the reference's `else` branch


def _ids(layout, n):
    rng = np.random.default_rng(31)
    if layout == "runs":  # runs of 64 equal ids: wave-uniform waves
        return (np.arange(n) // 64 % 4).astype(np.float32)
    ids = rng.integers(0, 4, n).astype(np.float32)  # a random id per row: divergent waves
    if layout == "odd":
        at = rng.choice(n, n // 8, replace=False)
        ids[at] = ODD_IDS[rng.integers(0, 4, len(at))]
    return ids


def _mixed_yields(cls, code):
    y = np.empty(len(code), np.float32)
    for c in np.unique(code):
        y[code == c] = R.yields(int(c), cls)[code == c]
    return y


@pytest.mark.parametrize("jelly_fcr", [0, 1])
@pytest.mark.parametrize("layout", ["runs", "random", "odd"])
@pytest.mark.parametrize("cls", CLASSES)
def test_mixed_vs_float64(dev, cls, layout, jelly_fcr):
    """Every row against the float64 reference of its own material, foam rows
    included; metal's body here is the EXACT form."""
    F, mu, lam = R.inputs(cls)
    n = len(F)
    ids = _ids(layout, n)
    code = material_codes(ids)
    code[code == 0] = 4 if jelly_fcr else 0
    yld = _mixed_yields(cls, code)
    Fg, Tg, yg = _launch(dev, -1, n, F, mu, lam, yld, ids=ids, jelly_fcr=jelly_fcr)
    assert np.isfinite(Fg).all()
    for c in np.unique(code):
        assert (code == c).sum() > n // 8
        _check_rows(int(c), cls, code == c, Fg, Tg, yg, yld, f"mixed {layout:6s} fcr {jelly_fcr}")


@pytest.mark.parametrize("cls", ["moderate", "tiny", "large", "reflect"])
def test_mixed_result_independent_of_wave_neighbours(dev, cls):
    """A particle's result does not depend on which other particles share its
    wave (constitutive.h): the same rows in another order give the same bits."""
    F, mu, lam = R.inputs(cls)
    n = len(F)
    ids = _ids("odd", n)
    code = material_codes(ids)
    code[code == 0] = 4
    yld = _mixed_yields(cls, code)
    a = _launch(dev, -1, n, F, mu, lam, yld, ids=ids, jelly_fcr=1)
    perm = np.random.default_rng(32).permutation(n)
    b = _launch(dev, -1, n, F[perm], mu[perm], lam[perm], yld[perm], ids=ids[perm], jelly_fcr=1)
    for x, y in zip(a, b):
        back = np.empty_like(y)
        back[perm] = y
        assert np.array_equal(_bits(x), _bits(back))


# ----------------------------------------------------------------------- SVD --
@pytest.mark.parametrize("family", R.SVD_FAMILIES)
def test_svd_vs_float64(dev, family):
    import torch
    from gsmpm._lib import LIB, check, ptr, stream_of
    A = R.svd_inputs(family)
    n = len(A)
    At = torch.from_numpy(np.array(A.reshape(n, 9))).to(dev)
    U, V = torch.empty_like(At), torch.empty_like(At)
    S = torch.empty(n, 3, device=dev)
    check(LIB.gsmpm_svd3(ptr(At), n, ptr(U), ptr(S), ptr(V), stream_of(dev)))
    U, S, V = U.cpu().numpy(), S.cpu().numpy().astype(np.float64), V.cpu().numpy()
    assert np.isfinite(U).all() and np.isfinite(S).all() and np.isfinite(V).all()
    got = R.svd_measures(A, U, S, V)
    bound = device_svd_bound(family)
    print(f"device svd vs f64 {family:9s} " + " ".join(f"{k} {got[k]:.2e}" for k in R.SVD_MEASURES)
          + "  bound " + " ".join(f"{b:.0e}" for b in bound))
    assert all(got[k] <= b for k, b in zip(R.SVD_MEASURES, bound)), (got, bound)
    # descending order with the sign on sigma3, up to the sigma bound
    tol = bound[0] * np.maximum(1.0, S[:, 0])
    assert np.all(S[:, 0] - S[:, 1] >= -tol) and np.all(S[:, 1] - np.abs(S[:, 2]) >= -tol)
    # sign(sigma3) = sign(det A) wherever det A resolves it: |det A| > bound max(1, sigma1)^3
    # gives |sigma3| = |det A| / (sigma1 sigma2) > bound max(1, sigma1), the sigma bound of the row
    det = np.linalg.det(A.astype(np.float64))
    sure = np.abs(det) > bound[0] * np.maximum(1.0, S[:, 0]) ** 3
    assert sure.mean() > 0.9
    assert np.array_equal(np.sign(S[sure, 2]), np.sign(det[sure]))
