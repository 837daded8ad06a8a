"""The f32 differentiable-MPM oracle (oracle/diff_oracle.c, default mode: the
one the GPU implements) against the float64 autograd reference of
tests/fit_ref.py, one substep at a time, on the input classes of fit_ref.

ORACLE_FIT_BOUNDS[case][field] = (field_err, elem_err) is the oracle's measured
distance from float64, rounded up to two digits: the yardstick of
test_gpu_fit_ref.py.  print_bounds() prints the table from a fresh measurement
(from tests/: python -c "import conftest, test_fit_ref_oracle as t; t.print_bounds()");
`pytest -s` prints each case's maxima.

The mutation checks prove that the classes see what they were built for: the
reference with one behaviour flipped (a mass adjoint, a cube that blocks the
adjoint, a dJ term under the |J| clamp, grid adjoints cleared every substep)
leaves the recorded bound by a factor of 100 at the least.
"""
import math

import numpy as np
import pytest

import fit_ref as R
import oracle as O

F32 = np.float32
N176 = dict(n=3000, n_grid=176, lo=0.95, hi=1.05, dt=1e-4)  # test_gpu_fit.test_fit_binning_paths' large shape


class OracleSim:
    """OracleDiff behind the method names the drivers of fit_ref use."""
    GRID = {"mass": "gm", "v_in": "gv_in", "v_out": "gv_out", "v_in_grad": "g_gv_in", "v_out_grad": "g_gv_out"}

    def __init__(self, c, levels=2, **kw):
        self.o = O.OracleDiff(c.x, c.cov, c.vol, n_grid=c.n_grid, grid_extent=R.EXT, gravity=R.GRAV, init_v=c.v,
                              levels=levels, ground_only=True, **R.MAT, **kw)
        self.n = c.n
        for k in ("mu_lam", "postprocess_forward", "postprocess_backward", "set_grads", "learn", "cycle_init",
                  "clear_grads"):
            setattr(self, k, getattr(self.o, k))
        self.forward, self.backward = self.o.p2g2p_forward, self.o.p2g2p_backward

    def set(self, field, a, level=0):
        arr = getattr(self.o, field)
        dst = arr[level] if arr.ndim == 3 else arr
        dst[...] = np.asarray(a, F32).reshape(dst.shape)

    def get(self, field, level=0):
        arr = getattr(self.o, field)
        if arr.ndim == 3:
            return arr[level].copy()
        return arr.reshape(self.n, 6).copy() if arr.size == 6 * self.n and field.endswith("cov") else arr.copy()

    def grid_field(self, which):
        return getattr(self.o, self.GRID[which]).copy()


def round_up_2(x):
    """x rounded up to two significant digits (0 stays 0)."""
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f"{math.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e:.1e}")


# ----------------------------------------------------------- measurement --
def assert_no_mass_on_the_edge(m):
    m = np.asarray(m)
    assert not ((m >= 1e-16) & (m <= 1e-14)).any(), "a node mass within a decade of the 1e-15 threshold"


def _non_vacuous(c, ref):
    """Each class's own condition, on the reference's data."""
    G = ref.G
    m = ref.m.numpy()
    assert_no_mass_on_the_edge(m)
    base = G.base(ref.x[0]).numpy()
    assert base.min() >= 3 and base.max() + 2 <= c.n_grid - 4  # >= 3 cells from every face
    name = c.name
    if name == "box":
        inc = G.in_cube(np.arange(c.n_grid ** 3)).numpy()
        assert int((inc & (m > 1e-15)).sum()) >= 20
    elif name == "clamp":
        J = np.linalg.det(c.F.astype(np.float64).reshape(-1, 3, 3))
        assert (np.abs(np.abs(J) / 1e-2 - 1.0) >= 0.05).all()
        assert ((J > 0) & (J < 1e-2)).mean() >= 0.25 and ((J < 0) & (J > -1e-2)).mean() >= 0.25
        assert (np.abs(J) > 0.5).mean() >= 0.25
    elif name == "face":
        fx = c.x.astype(np.float64) * G.inv_dx - base
        d = np.minimum(np.abs(fx - 0.5), np.abs(fx - 1.5))
        assert (((d >= 1e-3 * 0.99) & (d <= 1e-2 * 1.01)).sum(1) >= 1).mean() >= 0.33
        live = m[m > 1e-15]
        assert int((live < 1e-4 * np.median(live)).sum()) >= 10  # lone light nodes
    elif name == "dense":
        t = base >> 3
        assert c.n >= 600 and (t == t[0]).all() and base.max() <= c.n_grid - 3
        for k in ("gx", "gv", "gF", "gC"):
            a = np.abs(c[k]).max(1)
            assert a.max() / a.min() >= 1e5
    elif name == "corner":
        t = base >> 3
        assert len(np.unique((t[:, 0] * 4 + t[:, 1]) * 4 + t[:, 2])) == 8
        assert set(np.unique(base)) == {7, 8}


def measure_class(name, n_grid=None, **flags):
    c = R.make_case(name, n_grid)
    ref, orc = R.new_ref(c, **flags), OracleSim(c)
    rf, rb = R.one_substep(ref, c)
    of, ob = R.one_substep(orc, c)
    _non_vacuous(c, ref)
    e = R.compare(of, rf)
    e.update(R.compare(ob, rb, ref.grid_adjoint("g_v_out_scale")))
    return e


def measure_three(through_set_grads=False, **flags):
    c = R.make_case("interior")
    ref, orc = R.new_ref(c, levels=4, **flags), OracleSim(c, levels=4)
    rf, rs = R.three_substeps(ref, c, through_set_grads)
    of, os_ = R.three_substeps(orc, c, through_set_grads)
    assert_no_mass_on_the_edge(ref.m.numpy())
    # glogE grows triangularly: gmu is added again every substep (the final value is not the sum of increments)
    assert np.abs(rs[2]["glogE"]).max() > 1.5 * np.abs(rs[0]["glogE"]).max()
    errs = [R.compare(of, rf)]
    errs += [R.compare(o, r, ref.grid_adjoint("g_v_out_scale")) for o, r in zip(os_, rs)]
    return R.worst(errs)


def measure_accumulation():
    c = R.make_case("interior")
    ref, orc = R.new_ref(c), OracleSim(c)
    rs, os_ = R.accumulation(ref, c), R.accumulation(orc, c)
    return R.worst([R.compare(o, r, ref.grid_adjoint("g_v_out_scale")) for o, r in zip(os_, rs)])


def measure_postprocess():
    c = R.make_case("box")
    ref, orc = R.new_ref(c), OracleSim(c)
    rf, rb = R.postprocess_path(ref, c)
    of, ob = R.postprocess_path(orc, c)
    e = R.compare(of, rf)
    e.update(R.compare(ob, rb, ref.grid_adjoint("g_v_out_scale")))
    return e


def case_176():
    """3,000 particles in a 176^3 grid (22^3 tiles: the k_scan + k_place binning), dt 1e-4."""
    rng = np.random.default_rng(176)
    n, ng = N176["n"], N176["n_grid"]
    x = rng.uniform(N176["lo"], N176["hi"], (n, 3)).astype(F32)
    N = lambda *s: rng.standard_normal(s)
    c = R.Case(name="big176", n_grid=ng, n=n, x=x, v=(0.05 * N(n, 3)).astype(F32), C=(0.5 * N(n, 9)).astype(F32),
               F=(np.eye(3).reshape(1, 9) + 0.05 * N(n, 9)).astype(F32),
               cov=np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], F32), (n, 1)), vol=R.volumes(x, ng),
               logE=(5.0 + rng.uniform(-0.5, 0.5, n)).astype(F32), y=rng.uniform(-0.5, 0.5, n).astype(F32))
    for k, w in (("gx", 3), ("gv", 3), ("gF", 9), ("gC", 9)):
        c[k] = N(n, w).astype(F32)
    return c


def run_176(sim, c, nodes=None):
    """One substep at dt 1e-4; grid fields on `nodes` only."""
    R.seed_state(sim, c)
    sim.forward(N176["dt"], 0)
    sim.clear_grads()
    R.seed_cotangents(sim, c, 1)
    sim.backward(N176["dt"], 0)
    out = R.backward_fields(sim, (0,))
    out.update({k + "1": sim.get(k, 1) for k in ("x", "v", "C", "F")})
    if nodes is not None:
        for k in ("v_in_grad", "v_out_grad"):
            assert np.count_nonzero(out[k]) == np.count_nonzero(out[k][nodes])  # nothing off the touched nodes
            out[k] = out[k][nodes]
    return out


def measure_176():
    c = case_176()
    ref = R.FitRef(c.x, c.cov, c.vol, n_grid=c.n_grid, grid_extent=R.EXT, gravity=R.GRAV, init_v=c.v, levels=2,
                   ground_only=True, sparse=True, **R.MAT)
    r = run_176(ref, c)
    assert_no_mass_on_the_edge(ref.m.numpy())
    o = run_176(OracleSim(c), c, ref.nodes.numpy())
    return R.compare(o, r, ref.grid_adjoint("g_v_out_scale"))


MEASURES = {name: (lambda name=name: measure_class(name)) for name in R.CLASSES}
MEASURES.update({
    "dense20": lambda: measure_class("dense", 20),
    "corner20": lambda: measure_class("corner", 20),
    "three": measure_three,
    "three_post": lambda: measure_three(True),
    "accumulate": measure_accumulation,
    "post": measure_postprocess,
    "big176": measure_176,
})

# Measured on the CPU (oracle built with -ffp-contract=off), rounded up to two digits.
ORACLE_FIT_BOUNDS = {
    'interior': {
        'x1': (4.3e-08, 5.9e-08),  # measured 4.26e-08 5.86e-08
        'v1': (4.1e-07, 6.8e-05),  # measured 4.01e-07 6.79e-05
        'C1': (5.1e-07, 7.0e-05),  # measured 5.10e-07 6.95e-05
        'F1': (1.6e-07, 3.0e-07),  # measured 1.54e-07 2.95e-07
        'stress': (6.0e-07, 7.4e-05),  # measured 5.91e-07 7.32e-05
        'mass': (3.2e-07, 4.5e-07),  # measured 3.13e-07 4.43e-07
        'v_in': (3.2e-07, 8.8e-06),  # measured 3.17e-07 8.77e-06
        'v_out': (7.6e-07, 5.2e-06),  # measured 7.53e-07 5.10e-06
        'mu': (9.4e-08, 1.2e-07),  # measured 9.32e-08 1.15e-07
        'lam': (2.7e-07, 3.2e-07),  # measured 2.61e-07 3.18e-07
        'gx': (3.7e-07, 5.1e-05),  # measured 3.64e-07 5.02e-05
        'gv': (2.8e-07, 2.6e-05),  # measured 2.80e-07 2.55e-05
        'gC': (2.5e-07, 3.4e-05),  # measured 2.40e-07 3.32e-05
        'gF': (3.1e-07, 3.7e-05),  # measured 3.04e-07 3.62e-05
        'gstress': (2.0e-07, 3.4e-05),  # measured 1.92e-07 3.31e-05
        'gmu': (4.8e-07, 1.8e-05),  # measured 4.76e-07 1.75e-05
        'glam': (1.3e-07, 2.2e-05),  # measured 1.24e-07 2.17e-05
        'glogE': (4.5e-07, 6.7e-05),  # measured 4.41e-07 6.68e-05
        'gy': (3.6e-07, 9.4e-05),  # measured 3.55e-07 9.32e-05
        'v_in_grad': (1.2e-07, 6.9e-06),  # measured 1.19e-07 6.85e-06
        'v_out_grad': (3.5e-07, 2.5e-07),  # measured 3.50e-07 2.47e-07
    },
    'box': {
        'x1': (5.0e-08, 5.8e-08),  # measured 4.96e-08 5.76e-08
        'v1': (1.5e-07, 4.0e-05),  # measured 1.43e-07 3.90e-05
        'C1': (3.1e-07, 5.7e-05),  # measured 3.06e-07 5.66e-05
        'F1': (1.6e-07, 9.9e-07),  # measured 1.60e-07 9.81e-07
        'stress': (3.7e-07, 6.1e-05),  # measured 3.68e-07 6.02e-05
        'mass': (1.8e-07, 2.6e-07),  # measured 1.72e-07 2.55e-07
        'v_in': (3.8e-07, 2.6e-05),  # measured 3.77e-07 2.52e-05
        'v_out': (9.6e-07, 8.7e-06),  # measured 9.51e-07 8.61e-06
        'mu': (8.9e-08, 1.3e-07),  # measured 8.88e-08 1.25e-07
        'lam': (2.3e-07, 3.1e-07),  # measured 2.28e-07 3.06e-07
        'gx': (5.0e-07, 2.8e-05),  # measured 4.96e-07 2.73e-05
        'gv': (2.3e-07, 3.6e-05),  # measured 2.22e-07 3.54e-05
        'gC': (1.7e-07, 1.9e-05),  # measured 1.61e-07 1.87e-05
        'gF': (3.0e-07, 1.6e-05),  # measured 2.91e-07 1.51e-05
        'gstress': (1.6e-07, 1.6e-05),  # measured 1.51e-07 1.56e-05
        'gmu': (3.7e-07, 3.9e-05),  # measured 3.68e-07 3.82e-05
        'glam': (4.5e-07, 2.4e-05),  # measured 4.47e-07 2.38e-05
        'glogE': (3.9e-07, 1.8e-05),  # measured 3.82e-07 1.74e-05
        'gy': (4.4e-07, 1.6e-05),  # measured 4.32e-07 1.54e-05
        'v_in_grad': (8.7e-08, 1.1e-05),  # measured 8.66e-08 1.01e-05
        'v_out_grad': (2.1e-07, 5.9e-07),  # measured 2.02e-07 5.87e-07
    },
    'clamp': {
        'x1': (4.4e-08, 5.9e-08),  # measured 4.36e-08 5.82e-08
        'v1': (2.6e-07, 4.6e-05),  # measured 2.52e-07 4.55e-05
        'C1': (2.9e-07, 4.2e-05),  # measured 2.87e-07 4.19e-05
        'F1': (1.6e-07, 8.0e-06),  # measured 1.52e-07 7.95e-06
        'stress': (3.1e-07, 8.5e-06),  # measured 3.06e-07 8.47e-06
        'mass': (2.5e-07, 3.4e-07),  # measured 2.45e-07 3.37e-07
        'v_in': (3.0e-07, 6.6e-05),  # measured 2.91e-07 6.51e-05
        'v_out': (2.0e-07, 2.0e-06),  # measured 1.96e-07 1.97e-06
        'mu': (7.0e-08, 1.2e-07),  # measured 6.94e-08 1.19e-07
        'lam': (2.7e-07, 3.7e-07),  # measured 2.64e-07 3.66e-07
        'gx': (3.1e-07, 3.5e-05),  # measured 3.06e-07 3.40e-05
        'gv': (5.1e-07, 2.2e-05),  # measured 5.10e-07 2.13e-05
        'gC': (1.6e-07, 1.7e-05),  # measured 1.51e-07 1.67e-05
        'gF': (2.4e-07, 6.5e-05),  # measured 2.34e-07 6.47e-05
        'gstress': (2.2e-07, 2.3e-05),  # measured 2.12e-07 2.20e-05
        'gmu': (3.6e-07, 3.3e-05),  # measured 3.53e-07 3.21e-05
        'glam': (2.5e-07, 1.3e-05),  # measured 2.46e-07 1.23e-05
        'glogE': (4.3e-07, 1.3e-05),  # measured 4.26e-07 1.25e-05
        'gy': (4.6e-07, 1.3e-05),  # measured 4.57e-07 1.25e-05
        'v_in_grad': (9.7e-08, 5.1e-06),  # measured 9.64e-08 5.08e-06
        'v_out_grad': (3.0e-07, 2.1e-07),  # measured 2.91e-07 2.02e-07
    },
    'face': {
        'x1': (4.6e-08, 5.9e-08),  # measured 4.52e-08 5.89e-08
        'v1': (1.7e-07, 2.4e-05),  # measured 1.61e-07 2.36e-05
        'C1': (3.6e-07, 5.2e-05),  # measured 3.54e-07 5.12e-05
        'F1': (1.7e-07, 5.1e-07),  # measured 1.69e-07 5.08e-07
        'stress': (5.0e-07, 9.3e-05),  # measured 4.93e-07 9.25e-05
        'mass': (3.7e-07, 4.9e-07),  # measured 3.66e-07 4.81e-07
        'v_in': (4.5e-07, 2.2e-05),  # measured 4.45e-07 2.13e-05
        'v_out': (5.7e-07, 2.2e-05),  # measured 5.70e-07 2.14e-05
        'mu': (9.1e-08, 1.3e-07),  # measured 9.09e-08 1.26e-07
        'lam': (2.5e-07, 3.6e-07),  # measured 2.42e-07 3.51e-07
        'gx': (4.3e-07, 4.1e-05),  # measured 4.21e-07 4.08e-05
        'gv': (2.6e-07, 2.7e-05),  # measured 2.59e-07 2.66e-05
        'gC': (2.9e-07, 2.7e-05),  # measured 2.87e-07 2.68e-05
        'gF': (1.2e-07, 1.2e-05),  # measured 1.13e-07 1.16e-05
        'gstress': (2.2e-07, 2.1e-05),  # measured 2.17e-07 2.01e-05
        'gmu': (8.7e-07, 5.0e-05),  # measured 8.69e-07 5.00e-05
        'glam': (3.6e-07, 2.0e-05),  # measured 3.53e-07 1.93e-05
        'glogE': (4.5e-07, 2.6e-05),  # measured 4.45e-07 2.51e-05
        'gy': (6.5e-07, 2.0e-05),  # measured 6.49e-07 1.90e-05
        'v_in_grad': (1.3e-07, 4.7e-06),  # measured 1.21e-07 4.66e-06
        'v_out_grad': (3.4e-07, 5.0e-07),  # measured 3.30e-07 4.93e-07
    },
    'dense': {
        'x1': (4.0e-08, 4.7e-08),  # measured 3.97e-08 4.69e-08
        'v1': (2.6e-07, 2.9e-05),  # measured 2.54e-07 2.83e-05
        'C1': (3.4e-07, 2.1e-05),  # measured 3.40e-07 2.07e-05
        'F1': (1.5e-07, 2.1e-07),  # measured 1.47e-07 2.08e-07
        'stress': (4.1e-07, 1.1e-04),  # measured 4.04e-07 1.08e-04
        'mass': (2.7e-07, 4.8e-07),  # measured 2.66e-07 4.79e-07
        'v_in': (6.7e-07, 1.5e-05),  # measured 6.68e-07 1.43e-05
        'v_out': (2.8e-07, 1.5e-05),  # measured 2.77e-07 1.49e-05
        'mu': (9.3e-08, 1.3e-07),  # measured 9.21e-08 1.27e-07
        'lam': (2.0e-07, 3.7e-07),  # measured 1.90e-07 3.63e-07
        'gx': (4.6e-07, 2.5e-04),  # measured 4.54e-07 2.46e-04
        'gv': (5.0e-07, 3.8e-05),  # measured 4.96e-07 3.77e-05
        'gC': (7.6e-07, 7.5e-05),  # measured 7.58e-07 7.49e-05
        'gF': (4.2e-07, 1.7e-05),  # measured 4.12e-07 1.68e-05
        'gstress': (6.6e-07, 2.1e-04),  # measured 6.55e-07 2.06e-04
        'gmu': (3.6e-07, 1.1e-04),  # measured 3.55e-07 1.07e-04
        'glam': (4.7e-07, 6.4e-05),  # measured 4.67e-07 6.33e-05
        'glogE': (3.6e-07, 6.9e-05),  # measured 3.54e-07 6.85e-05
        'gy': (3.3e-07, 2.7e-05),  # measured 3.21e-07 2.69e-05
        'v_in_grad': (1.6e-07, 3.2e-06),  # measured 1.52e-07 3.15e-06
        'v_out_grad': (6.6e-07, 7.6e-07),  # measured 6.58e-07 7.55e-07
    },
    'corner': {
        'x1': (5.1e-08, 5.9e-08),  # measured 5.02e-08 5.82e-08
        'v1': (1.9e-07, 9.4e-06),  # measured 1.88e-07 9.31e-06
        'C1': (4.5e-07, 3.5e-05),  # measured 4.47e-07 3.48e-05
        'F1': (1.6e-07, 6.9e-07),  # measured 1.54e-07 6.88e-07
        'stress': (3.9e-07, 2.6e-05),  # measured 3.83e-07 2.58e-05
        'mass': (4.1e-07, 4.4e-07),  # measured 4.08e-07 4.37e-07
        'v_in': (3.3e-07, 2.3e-05),  # measured 3.20e-07 2.28e-05
        'v_out': (4.3e-07, 2.3e-05),  # measured 4.29e-07 2.26e-05
        'mu': (1.2e-07, 1.4e-07),  # measured 1.18e-07 1.31e-07
        'lam': (2.0e-07, 2.7e-07),  # measured 1.93e-07 2.63e-07
        'gx': (3.2e-07, 5.5e-05),  # measured 3.15e-07 5.49e-05
        'gv': (1.9e-07, 2.0e-05),  # measured 1.87e-07 1.91e-05
        'gC': (2.0e-07, 4.9e-05),  # measured 2.00e-07 4.81e-05
        'gF': (3.3e-07, 5.1e-05),  # measured 3.28e-07 5.02e-05
        'gstress': (3.6e-07, 1.8e-05),  # measured 3.51e-07 1.78e-05
        'gmu': (3.8e-07, 5.8e-05),  # measured 3.76e-07 5.74e-05
        'glam': (3.3e-07, 1.8e-05),  # measured 3.25e-07 1.80e-05
        'glogE': (2.7e-07, 1.0e-05),  # measured 2.65e-07 9.93e-06
        'gy': (3.5e-07, 8.2e-06),  # measured 3.42e-07 8.12e-06
        'v_in_grad': (3.4e-07, 4.4e-05),  # measured 3.38e-07 4.39e-05
        'v_out_grad': (2.2e-07, 2.6e-07),  # measured 2.19e-07 2.51e-07
    },
    'ragged1': {
        'x1': (4.2e-08, 4.7e-08),  # measured 4.12e-08 4.67e-08
        'v1': (8.1e-08, 2.5e-07),  # measured 8.00e-08 2.48e-07
        'C1': (4.8e-07, 2.3e-06),  # measured 4.70e-07 2.27e-06
        'F1': (3.3e-08, 1.1e-07),  # measured 3.21e-08 1.05e-07
        'stress': (7.4e-07, 6.2e-05),  # measured 7.34e-07 6.12e-05
        'mass': (6.9e-08, 1.4e-07),  # measured 6.85e-08 1.35e-07
        'v_in': (1.9e-07, 2.0e-05),  # measured 1.80e-07 1.94e-05
        'v_out': (7.1e-07, 4.7e-06),  # measured 7.02e-07 4.66e-06
        'mu': (3.1e-08, 3.1e-08),  # measured 3.07e-08 3.06e-08
        'lam': (1.3e-07, 1.3e-07),  # measured 1.29e-07 1.29e-07
        'gx': (1.2e-07, 1.2e-07),  # measured 1.12e-07 1.17e-07
        'gv': (2.2e-06, 1.1e-05),  # measured 2.13e-06 1.04e-05
        'gC': (3.9e-08, 1.8e-07),  # measured 3.87e-08 1.75e-07
        'gF': (1.8e-07, 5.5e-07),  # measured 1.76e-07 5.49e-07
        'gstress': (9.3e-08, 2.5e-07),  # measured 9.27e-08 2.49e-07
        'gmu': (3.1e-08, 3.1e-08),  # measured 3.02e-08 3.02e-08
        'glam': (2.5e-06, 2.5e-06),  # measured 2.48e-06 2.48e-06
        'glogE': (2.6e-07, 2.6e-07),  # measured 2.58e-07 2.57e-07
        'gy': (7.8e-06, 7.8e-06),  # measured 7.72e-06 7.71e-06
        'v_in_grad': (4.7e-08, 1.1e-06),  # measured 4.70e-08 1.05e-06
        'v_out_grad': (5.5e-08, 1.3e-06),  # measured 5.44e-08 1.21e-06
    },
    'ragged257': {
        'x1': (4.3e-08, 5.8e-08),  # measured 4.24e-08 5.71e-08
        'v1': (2.5e-07, 3.0e-05),  # measured 2.45e-07 2.99e-05
        'C1': (4.9e-07, 2.8e-05),  # measured 4.85e-07 2.76e-05
        'F1': (1.3e-07, 2.6e-07),  # measured 1.29e-07 2.60e-07
        'stress': (6.0e-07, 6.0e-05),  # measured 5.97e-07 5.92e-05
        'mass': (2.2e-07, 3.9e-07),  # measured 2.15e-07 3.83e-07
        'v_in': (1.9e-07, 2.3e-05),  # measured 1.80e-07 2.21e-05
        'v_out': (2.2e-07, 1.8e-05),  # measured 2.11e-07 1.71e-05
        'mu': (8.8e-08, 1.3e-07),  # measured 8.70e-08 1.27e-07
        'lam': (2.8e-07, 3.1e-07),  # measured 2.75e-07 3.07e-07
        'gx': (3.3e-07, 1.1e-04),  # measured 3.23e-07 1.03e-04
        'gv': (3.7e-07, 2.3e-05),  # measured 3.60e-07 2.26e-05
        'gC': (2.1e-07, 2.6e-05),  # measured 2.00e-07 2.59e-05
        'gF': (1.6e-07, 1.7e-05),  # measured 1.53e-07 1.69e-05
        'gstress': (2.2e-07, 1.8e-05),  # measured 2.20e-07 1.77e-05
        'gmu': (4.4e-07, 2.3e-05),  # measured 4.34e-07 2.29e-05
        'glam': (3.6e-07, 3.6e-05),  # measured 3.58e-07 3.52e-05
        'glogE': (4.9e-07, 2.3e-05),  # measured 4.85e-07 2.21e-05
        'gy': (6.5e-07, 1.5e-05),  # measured 6.43e-07 1.42e-05
        'v_in_grad': (8.2e-08, 2.4e-05),  # measured 8.19e-08 2.35e-05
        'v_out_grad': (3.4e-07, 2.3e-07),  # measured 3.31e-07 2.22e-07
    },
    'ragged1003': {
        'x1': (4.3e-08, 5.9e-08),  # measured 4.26e-08 5.88e-08
        'v1': (4.8e-07, 3.6e-05),  # measured 4.78e-07 3.55e-05
        'C1': (6.1e-07, 1.4e-04),  # measured 6.07e-07 1.34e-04
        'F1': (1.7e-07, 3.4e-07),  # measured 1.69e-07 3.30e-07
        'stress': (6.9e-07, 1.2e-04),  # measured 6.87e-07 1.16e-04
        'mass': (4.5e-07, 6.9e-07),  # measured 4.41e-07 6.84e-07
        'v_in': (2.2e-07, 1.2e-05),  # measured 2.13e-07 1.12e-05
        'v_out': (8.4e-07, 1.5e-05),  # measured 8.34e-07 1.42e-05
        'mu': (9.3e-08, 1.2e-07),  # measured 9.22e-08 1.20e-07
        'lam': (2.8e-07, 3.6e-07),  # measured 2.79e-07 3.54e-07
        'gx': (2.4e-07, 2.9e-05),  # measured 2.37e-07 2.80e-05
        'gv': (2.3e-07, 3.8e-05),  # measured 2.24e-07 3.70e-05
        'gC': (2.0e-07, 3.9e-05),  # measured 1.96e-07 3.88e-05
        'gF': (5.6e-07, 2.5e-05),  # measured 5.50e-07 2.49e-05
        'gstress': (2.2e-07, 1.9e-04),  # measured 2.13e-07 1.84e-04
        'gmu': (2.4e-07, 3.2e-05),  # measured 2.39e-07 3.17e-05
        'glam': (5.0e-07, 7.3e-05),  # measured 4.94e-07 7.30e-05
        'glogE': (3.9e-07, 5.8e-05),  # measured 3.85e-07 5.74e-05
        'gy': (6.6e-07, 3.5e-05),  # measured 6.59e-07 3.50e-05
        'v_in_grad': (1.3e-07, 1.4e-05),  # measured 1.21e-07 1.32e-05
        'v_out_grad': (4.4e-07, 2.0e-07),  # measured 4.38e-07 2.00e-07
    },
    'dense20': {
        'x1': (5.0e-08, 5.9e-08),  # measured 4.97e-08 5.89e-08
        'v1': (1.4e-06, 2.4e-04),  # measured 1.38e-06 2.30e-04
        'C1': (1.7e-06, 3.4e-04),  # measured 1.68e-06 3.31e-04
        'F1': (1.5e-07, 9.4e-07),  # measured 1.45e-07 9.38e-07
        'stress': (6.1e-07, 1.2e-04),  # measured 6.09e-07 1.11e-04
        'mass': (4.9e-07, 6.2e-07),  # measured 4.86e-07 6.18e-07
        'v_in': (8.0e-07, 2.4e-05),  # measured 7.91e-07 2.39e-05
        'v_out': (4.0e-06, 5.4e-05),  # measured 3.97e-06 5.39e-05
        'mu': (9.2e-08, 1.3e-07),  # measured 9.15e-08 1.27e-07
        'lam': (2.4e-07, 3.4e-07),  # measured 2.35e-07 3.35e-07
        'gx': (2.2e-06, 8.1e-05),  # measured 2.18e-06 8.01e-05
        'gv': (8.6e-07, 1.7e-04),  # measured 8.52e-07 1.65e-04
        'gC': (2.0e-06, 5.8e-05),  # measured 1.91e-06 5.73e-05
        'gF': (1.5e-06, 1.6e-05),  # measured 1.41e-06 1.52e-05
        'gstress': (1.8e-06, 1.6e-04),  # measured 1.73e-06 1.58e-04
        'gmu': (5.4e-07, 8.0e-05),  # measured 5.36e-07 7.97e-05
        'glam': (8.8e-07, 1.0e-04),  # measured 8.78e-07 9.99e-05
        'glogE': (1.2e-06, 7.4e-05),  # measured 1.17e-06 7.32e-05
        'gy': (1.1e-06, 4.5e-05),  # measured 1.05e-06 4.46e-05
        'v_in_grad': (8.9e-07, 1.5e-05),  # measured 8.82e-07 1.41e-05
        'v_out_grad': (7.0e-07, 2.7e-06),  # measured 6.95e-07 2.69e-06
    },
    'corner20': {
        'x1': (3.2e-08, 4.0e-08),  # measured 3.14e-08 3.91e-08
        'v1': (6.9e-07, 1.8e-04),  # measured 6.80e-07 1.78e-04
        'C1': (1.2e-06, 4.7e-04),  # measured 1.16e-06 4.68e-04
        'F1': (1.8e-07, 8.1e-07),  # measured 1.75e-07 8.01e-07
        'stress': (6.1e-07, 1.1e-04),  # measured 6.04e-07 1.10e-04
        'mass': (4.8e-07, 8.0e-07),  # measured 4.71e-07 7.92e-07
        'v_in': (3.9e-07, 4.7e-05),  # measured 3.88e-07 4.62e-05
        'v_out': (7.9e-07, 1.2e-04),  # measured 7.89e-07 1.12e-04
        'mu': (9.7e-08, 1.3e-07),  # measured 9.61e-08 1.23e-07
        'lam': (2.2e-07, 3.3e-07),  # measured 2.18e-07 3.25e-07
        'gx': (7.8e-07, 1.2e-04),  # measured 7.79e-07 1.16e-04
        'gv': (1.4e-06, 2.7e-04),  # measured 1.36e-06 2.70e-04
        'gC': (6.4e-07, 2.4e-04),  # measured 6.38e-07 2.39e-04
        'gF': (2.1e-06, 1.7e-04),  # measured 2.01e-06 1.70e-04
        'gstress': (8.6e-07, 1.1e-04),  # measured 8.54e-07 1.09e-04
        'gmu': (8.4e-07, 1.2e-04),  # measured 8.34e-07 1.15e-04
        'glam': (8.5e-07, 8.1e-05),  # measured 8.42e-07 8.06e-05
        'glogE': (2.7e-06, 2.1e-04),  # measured 2.61e-06 2.01e-04
        'gy': (3.2e-06, 1.3e-04),  # measured 3.17e-06 1.27e-04
        'v_in_grad': (5.8e-07, 1.3e-04),  # measured 5.76e-07 1.21e-04
        'v_out_grad': (1.2e-06, 1.1e-06),  # measured 1.18e-06 1.04e-06
    },
    'three': {
        'x3': (1.2e-07, 1.6e-07),  # measured 1.15e-07 1.53e-07
        'v3': (1.2e-06, 1.9e-04),  # measured 1.12e-06 1.85e-04
        'C3': (1.4e-06, 3.0e-04),  # measured 1.32e-06 2.91e-04
        'F3': (3.1e-07, 2.3e-06),  # measured 3.05e-07 2.29e-06
        'gx': (4.1e-06, 2.7e-04),  # measured 4.01e-06 2.68e-04
        'gv': (1.5e-06, 1.2e-04),  # measured 1.44e-06 1.12e-04
        'gC': (9.2e-07, 1.7e-04),  # measured 9.15e-07 1.64e-04
        'gF': (1.1e-06, 2.0e-04),  # measured 1.00e-06 1.97e-04
        'gstress': (1.3e-06, 2.0e-04),  # measured 1.20e-06 1.90e-04
        'gmu': (3.8e-06, 1.5e-04),  # measured 3.78e-06 1.48e-04
        'glam': (1.1e-06, 2.6e-04),  # measured 1.09e-06 2.53e-04
        'glogE': (3.1e-06, 1.6e-04),  # measured 3.10e-06 1.60e-04
        'gy': (1.6e-06, 1.3e-04),  # measured 1.59e-06 1.28e-04
        'v_in_grad': (1.7e-05, 1.7e-03),  # measured 1.66e-05 1.65e-03
        'v_out_grad': (1.6e-06, 3.5e-06),  # measured 1.53e-06 3.43e-06
    },
    'three_post': {
        'x3': (1.2e-07, 1.6e-07),  # measured 1.15e-07 1.53e-07
        'v3': (1.2e-06, 1.9e-04),  # measured 1.12e-06 1.85e-04
        'C3': (1.4e-06, 3.0e-04),  # measured 1.32e-06 2.91e-04
        'F3': (3.1e-07, 2.3e-06),  # measured 3.05e-07 2.29e-06
        'cov': (5.7e-07, 1.2e-05),  # measured 5.63e-07 1.19e-05
        'gx': (4.4e-07, 3.8e-05),  # measured 4.35e-07 3.71e-05
        'gv': (1.1e-06, 2.8e-04),  # measured 1.07e-06 2.76e-04
        'gC': (1.2e-06, 3.1e-04),  # measured 1.12e-06 3.07e-04
        'gF': (2.3e-07, 3.0e-05),  # measured 2.23e-07 2.91e-05
        'gstress': (3.3e-06, 4.5e-04),  # measured 3.27e-06 4.46e-04
        'gmu': (2.1e-06, 1.9e-04),  # measured 2.09e-06 1.86e-04
        'glam': (2.8e-06, 4.7e-04),  # measured 2.71e-06 4.68e-04
        'glogE': (2.3e-06, 1.4e-04),  # measured 2.25e-06 1.39e-04
        'gy': (3.0e-06, 1.9e-04),  # measured 2.91e-06 1.85e-04
        'v_in_grad': (8.2e-06, 4.0e-04),  # measured 8.18e-06 4.00e-04
        'v_out_grad': (9.9e-07, 3.1e-06),  # measured 9.80e-07 3.03e-06
    },
    'accumulate': {
        'gx': (3.6e-07, 4.4e-05),  # measured 3.52e-07 4.33e-05
        'gv': (2.9e-07, 3.6e-05),  # measured 2.86e-07 3.58e-05
        'gC': (3.0e-07, 1.7e-05),  # measured 2.91e-07 1.64e-05
        'gF': (4.0e-07, 1.2e-05),  # measured 3.97e-07 1.17e-05
        'gstress': (4.0e-07, 8.4e-07),  # measured 3.94e-07 8.37e-07
        'gmu': (3.3e-07, 2.9e-05),  # measured 3.20e-07 2.80e-05
        'glam': (4.8e-07, 4.1e-05),  # measured 4.80e-07 4.08e-05
        'glogE': (6.0e-07, 2.6e-05),  # measured 5.97e-07 2.50e-05
        'gy': (5.3e-07, 3.2e-05),  # measured 5.26e-07 3.13e-05
        'v_in_grad': (1.2e-07, 6.9e-06),  # measured 1.19e-07 6.87e-06
        'v_out_grad': (3.9e-07, 2.5e-07),  # measured 3.89e-07 2.44e-07
    },
    'post': {
        'x1': (5.0e-08, 5.8e-08),  # measured 4.96e-08 5.76e-08
        'v1': (1.5e-07, 4.0e-05),  # measured 1.43e-07 3.90e-05
        'C1': (3.1e-07, 5.7e-05),  # measured 3.06e-07 5.66e-05
        'F1': (1.6e-07, 9.9e-07),  # measured 1.60e-07 9.81e-07
        'stress': (3.7e-07, 6.1e-05),  # measured 3.68e-07 6.02e-05
        'mass': (1.8e-07, 2.6e-07),  # measured 1.72e-07 2.55e-07
        'v_in': (3.8e-07, 2.6e-05),  # measured 3.77e-07 2.52e-05
        'v_out': (9.6e-07, 8.7e-06),  # measured 9.51e-07 8.61e-06
        'mu': (8.9e-08, 1.3e-07),  # measured 8.88e-08 1.25e-07
        'lam': (2.3e-07, 3.1e-07),  # measured 2.28e-07 3.06e-07
        'cov': (3.4e-07, 5.1e-06),  # measured 3.31e-07 5.08e-06
        'gx': (4.1e-07, 6.3e-05),  # measured 4.08e-07 6.29e-05
        'gv': (1.5e-07, 3.8e-05),  # measured 1.41e-07 3.76e-05
        'gC': (2.6e-07, 4.0e-05),  # measured 2.59e-07 3.99e-05
        'gF': (1.5e-07, 5.2e-06),  # measured 1.49e-07 5.10e-06
        'gstress': (2.0e-07, 4.2e-05),  # measured 1.91e-07 4.12e-05
        'gmu': (5.0e-07, 1.5e-04),  # measured 4.91e-07 1.42e-04
        'glam': (4.1e-07, 3.1e-05),  # measured 4.00e-07 3.04e-05
        'glogE': (3.7e-07, 3.1e-05),  # measured 3.63e-07 3.08e-05
        'gy': (3.3e-07, 4.8e-05),  # measured 3.20e-07 4.78e-05
        'v_in_grad': (1.5e-07, 4.9e-06),  # measured 1.45e-07 4.88e-06
        'v_out_grad': (2.5e-07, 6.9e-07),  # measured 2.49e-07 6.84e-07
        'gF1': (1.2e-07, 5.6e-06),  # measured 1.15e-07 5.55e-06
    },
    'big176': {
        'gx': (8.4e-06, 9.7e-04),  # measured 8.37e-06 9.65e-04
        'gv': (8.0e-06, 1.7e-03),  # measured 7.90e-06 1.61e-03
        'gC': (9.1e-06, 1.9e-03),  # measured 9.01e-06 1.86e-03
        'gF': (6.2e-06, 1.2e-03),  # measured 6.10e-06 1.20e-03
        'gstress': (8.8e-06, 1.6e-03),  # measured 8.78e-06 1.53e-03
        'gmu': (1.1e-05, 2.6e-03),  # measured 1.07e-05 2.59e-03
        'glam': (8.9e-06, 8.3e-04),  # measured 8.87e-06 8.28e-04
        'glogE': (6.7e-06, 6.7e-04),  # measured 6.68e-06 6.64e-04
        'gy': (7.7e-06, 5.7e-04),  # measured 7.69e-06 5.69e-04
        'v_in_grad': (1.6e-05, 1.7e-03),  # measured 1.58e-05 1.61e-03
        'v_out_grad': (7.8e-06, 2.3e-05),  # measured 7.78e-06 2.24e-05
        'x1': (5.7e-08, 6.0e-08),  # measured 5.68e-08 5.93e-08
        'v1': (7.1e-06, 1.4e-03),  # measured 7.04e-06 1.35e-03
        'C1': (6.8e-06, 1.8e-03),  # measured 6.72e-06 1.71e-03
        'F1': (1.9e-07, 6.0e-06),  # measured 1.83e-07 5.95e-06
    },
}


@pytest.mark.parametrize("case", list(MEASURES))
def test_oracle_within_recorded_bounds(case):
    got = MEASURES[case]()
    bounds = ORACLE_FIT_BOUNDS[case]
    print(f"oracle vs f64 {case:10s} " + " ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in got.items()))
    assert set(got) == set(bounds)
    assert not R.within(got, bounds), R.within(got, bounds)


def test_bounds_are_two_digits():
    for row in ORACLE_FIT_BOUNDS.values():
        for b in row.values():
            assert all(x == round_up_2(x) for x in b), b


# -------------------------------------------------------------- mutations --
MUTATION_FACTOR = 100.0


@pytest.mark.parametrize("flag, case, fields", [
    ("mass_adjoint", "interior", ("gx",)),
    ("bc_blocks_adjoint", "box", ("v_in_grad", "gv")),
    ("clamp_has_dJ", "clamp", ("gF",)),
    ("clear_grid_adjoints_each_substep", "three", ("v_out_grad", "v_in_grad", "gv")),
])
def test_flipped_reference_leaves_the_bound(flag, case, fields):
    """The oracle against the reference with one behaviour flipped: beyond
    100 x the recorded field_err, so the class sees the behaviour and the
    bound is not slack."""
    got = measure_three(**{flag: True}) if case == "three" else measure_class(case, **{flag: True})
    for f in fields:
        need = MUTATION_FACTOR * ORACLE_FIT_BOUNDS[case][f][0]
        print(f"{flag} on {case}: {f} field_err {got[f][0]:.2e}, needs > {need:.2e}")
        assert got[f][0] > need, (flag, f, got[f][0], need)


def test_mass_adjoint_flag_is_the_oracles_exact_mode():
    """The flipped mass behaviour is the oracle's test-only exact_mass_grad
    mode (the one test_oracle_diff.py checks by finite differences)."""
    c = R.make_case("interior")
    _, rb = R.one_substep(R.new_ref(c, mass_adjoint=True), c)
    _, ob = R.one_substep(OracleSim(c, exact_mass_grad=True), c)
    assert R.field_err(ob["gx"], rb["gx"]) <= 10 * ORACLE_FIT_BOUNDS["interior"]["gx"][0]


# ------------------------------------------------------------ small ones --
LEARN_GRADS = np.array([-3.0, -1.0 - 2.0 ** -23, -1.0, -1.0 + 2.0 ** -24, -0.5, -1e-8, 0.0, 1e-8, 0.5, 1.0 - 2.0 ** -24,
                        1.0, 1.0 + 2.0 ** -23, 3.0, 1e10, -1e10, 0.999], F32)


def learn_inputs(n):
    reps = -(-n // len(LEARN_GRADS))
    return np.tile(LEARN_GRADS, reps)[:n], np.tile(LEARN_GRADS[::-1], reps)[:n]


def ulps(a, want64, operand):
    """|a - want| in units of the f32 spacing at max(|want|, |operand|)."""
    at = np.maximum(np.abs(np.asarray(want64, np.float64)), np.abs(np.asarray(operand, np.float64))).astype(F32)
    return np.abs(np.asarray(a, np.float64) - np.asarray(want64, np.float64)) / np.spacing(at).astype(np.float64)


def check_learn(sim, ref, c):
    """learn() with adjoints straddling the clip: the f32 rounding of the
    float64 result bit for bit where the adjoint is clipped (lr * 1 is
    exact: one rounding), within 1 ulp elsewhere (lr * g rounds at the
    spacing of lr * g, the difference at the spacing of the result: half an
    ulp each of the larger of the two, or one rounding with an FMA)."""
    ga, gb = learn_inputs(c.n)
    for s in (sim, ref):
        R.seed_state(s, c)
        s.clear_grads()
        s.set("glogE", ga)
        s.set("gy", gb)
        s.learn()
    for k, g, lr in (("logE", ga, 0.8), ("y", gb, 1.6)):
        got, want = sim.get(k), ref.get(k)
        assert (ulps(got, want, lr * np.clip(g.astype(np.float64), -1, 1)) <= 1.0).all(), k
        clipped = np.abs(g) >= 1.0
        assert clipped.any() and (np.abs(g) == 1.0).any()
        assert np.array_equal(got[clipped], want.astype(F32)[clipped]), k


def test_learn_at_the_clip():
    c = R.make_case("ragged257")
    check_learn(OracleSim(c), R.new_ref(c), c)


def check_cycle_init(sim, c):
    R.seed_state(sim, c)
    sim.forward(R.DT, 0)
    sim.forward(R.DT, 1)
    last = {k: sim.get(k, 2) for k in R.LEVELED}
    first = {k: sim.get(k, 1) for k in R.LEVELED}
    sim.cycle_init()
    for k in R.LEVELED:
        assert np.array_equal(sim.get(k, 0), last[k]), k
        assert np.array_equal(sim.get(k, 1), first[k]) and np.array_equal(sim.get(k, 2), last[k]), k
    assert np.abs(last["x"] - first["x"]).max() > 0


def test_cycle_init_copies_the_last_level():
    c = R.make_case("interior")
    check_cycle_init(OracleSim(c, levels=3), c)
    check_cycle_init(R.new_ref(c, levels=3), c)


def check_dead_grid(sim, c):
    """Every node mass below the threshold: nothing moves, and the only
    adjoint path left is x1 = x0 (+ dt * 0) and F1 = F0."""
    R.seed_state(sim, c)
    sim.set("mass", np.full(c.n, 1e-21, F32))
    sim.forward(R.DT, 0)
    assert sim.grid_field("mass").max() < 1e-16
    assert not sim.get("v", 1).any() and not sim.get("C", 1).any() and not sim.grid_field("v_out").any()
    assert np.array_equal(sim.get("F", 1), sim.get("F", 0)) and np.array_equal(sim.get("x", 1), sim.get("x", 0))
    sim.clear_grads()
    R.seed_cotangents(sim, c, 1)
    sim.backward(R.DT, 0)
    for k in ("gv", "gC", "gstress"):
        assert not sim.get(k, 0).any(), k
    assert not sim.grid_field("v_in_grad").any()
    assert np.array_equal(sim.get("gx", 0), sim.get("gx", 1))
    assert np.array_equal(sim.get("gF", 0), sim.get("gF", 1))
    for k in R.MODEL_ADJ:
        assert not sim.get(k).any(), k


def test_dead_grid_known_answers():
    c = R.make_case("interior")
    check_dead_grid(OracleSim(c), c)
    check_dead_grid(R.new_ref(c), c)


def print_bounds():
    """The table above from a fresh measurement."""
    print("ORACLE_FIT_BOUNDS = {")
    for case, fn in MEASURES.items():
        print(f"    {case!r}: {{")
        for k, (a, b) in fn().items():
            print(f"        {k!r}: ({round_up_2(a):.1e}, {round_up_2(b):.1e}),  # measured {a:.2e} {b:.2e}")
        print("    },")
    print("}")
