"""GPU: the differentiable MPM (csrc/fit.hip through gsmpm/fit.py) against the
float64 autograd reference of fit_ref.py, one substep at a time, on the input
classes of fit_ref: every forward field, all nine particle and model adjoints
and both grid adjoint fields per node.

The yardstick is the f32 oracle's own distance from float64
(test_fit_ref_oracle.py: ORACLE_FIT_BOUNDS, measured on the CPU).  A device
bound is FACTOR x the oracle's entry, its field_err never above CEILING, or an
entry of WIDENED with its cause named; none is derived from device output.
`pytest -s` prints the measured device maxima (recorded in DESIGN.md 4.2).
"""
import numpy as np
import pytest

import fit_ref as R
import test_fit_ref_oracle as T
from test_fit_ref_oracle import ORACLE_FIT_BOUNDS

pytestmark = pytest.mark.gpu

F32 = np.float32
# Device against oracle, each of rounding size: FMA contraction on the device
# against -ffp-contract=off in the oracle; device powf / expf at 1-2 ulp; window
# sums exact in fixed point, then f32 sums of <= 8 windows in a fixed order,
# against the oracle's serial f32 order.
FACTOR = 4.0
CEILING = 1e-4  # on field_err: the project's parity bound
# (case, field) -> (field_err, elem_err): entries wider than FACTOR x the oracle's, each with its cause.
WIDENED = {}


def device_bounds(case):
    out = {}
    for k, (fe, ee) in ORACLE_FIT_BOUNDS[case].items():
        out[k] = WIDENED.get((case, k), (min(FACTOR * fe, CEILING), FACTOR * ee))
        assert out[k][0] <= CEILING
    return out


class DeviceSim:
    """FitSimulator behind the method names the drivers of fit_ref use."""

    def __init__(self, dev, c, levels=2):
        import torch
        from gsmpm.fit import FitSimulator
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32)).to(dev)
        self.g = g = FitSimulator(c.n, n_grid=c.n_grid, grid_extent=R.EXT, levels=levels, gravity=R.GRAV, **R.MAT)
        g.set_particles(self.t(c.x), self.t(c.cov), self.t(c.vol), self.t(c.v))
        g.set_bc_ground_only()
        self.n, self.nn = c.n, c.n_grid ** 3
        for k in ("mu_lam", "forward", "backward", "postprocess_forward", "postprocess_backward", "learn", "cycle_init",
                  "clear_grads"):
            setattr(self, k, getattr(g, k))

    def set(self, field, a, level=0):
        self.g.set(field, self.t(a), level)

    def get(self, field, level=0):
        return self.g.get(field, level).cpu().numpy()

    def set_grads(self, xyz_grad, cov_grad):
        self.g.set_grads(self.t(xyz_grad), self.t(np.reshape(cov_grad, -1)))

    def grid_field(self, which):
        a = self.g.get_grid(which).cpu().numpy()
        return a.reshape(self.nn) if which == "mass" else a.reshape(self.nn, 3)


def _report(case, got, bounds):
    assert set(got) == set(bounds)
    for k, e in got.items():
        assert np.isfinite(e).all(), (k, e)
    print(f"device vs f64 {case:10s} " + " ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in got.items()))
    bad = R.within(got, bounds)
    assert not bad, bad


ONE_SUBSTEP = {name: (name, None) for name in R.CLASSES}
ONE_SUBSTEP.update(dense20=("dense", 20), corner20=("corner", 20))


@pytest.mark.parametrize("case", list(ONE_SUBSTEP))
def test_one_substep_vs_float64(dev, case):
    """The cotangents go in through `set`, which drops the grid the forward
    pass stored: backward recomputes it (k_p2g<true>)."""
    name, ng = ONE_SUBSTEP[case]
    c = R.make_case(name, ng)
    ref = R.new_ref(c)
    rf, rb = R.one_substep(ref, c)
    df, db = R.one_substep(DeviceSim(dev, c), c)
    e = R.compare(df, rf)
    e.update(R.compare(db, rb, ref.grid_adjoint("g_v_out_scale")))
    _report(case, e, device_bounds(case))


def test_postprocess_path_vs_float64(dev):
    """set_grads + postprocess_backward + backward with levels = 2: k_cov,
    k_cov_bwd and the backward pass on the grid its forward pass stored."""
    c = R.make_case("box")
    ref = R.new_ref(c)
    rf, rb = R.postprocess_path(ref, c)
    df, db = R.postprocess_path(DeviceSim(dev, c), c)
    e = R.compare(df, rf)
    e.update(R.compare(db, rb, ref.grid_adjoint("g_v_out_scale")))
    _report("post", e, device_bounds("post"))


@pytest.mark.parametrize("case", ["three", "three_post"])
def test_three_substeps_vs_float64(dev, case):
    """levels = 4, every level's adjoints, the model adjoints and both grid
    adjoint fields after each backward: the grid adjoints persist and glogE /
    gy grow triangularly.  `three` seeds through `set` (recomputed grids),
    `three_post` through set_grads (stored grids)."""
    c = R.make_case("interior")
    ref = R.new_ref(c, levels=4)
    rf, rs = R.three_substeps(ref, c, case == "three_post")
    df, ds = R.three_substeps(DeviceSim(dev, c, levels=4), c, case == "three_post")
    errs = [R.compare(df, rf)] + [R.compare(d, r, ref.grid_adjoint("g_v_out_scale")) for d, r in zip(ds, rs)]
    _report(case, R.worst(errs), device_bounds(case))


def test_accumulation_vs_float64(dev):
    """Adjoints present before backward(s) are added to, not overwritten, and
    a second backward(s) without clear_grads adds again."""
    c = R.make_case("interior")
    ref = R.new_ref(c)
    rs, ds = R.accumulation(ref, c), R.accumulation(DeviceSim(dev, c), c)
    errs = [R.compare(d, r, ref.grid_adjoint("g_v_out_scale")) for d, r in zip(ds, rs)]
    _report("accumulate", R.worst(errs), device_bounds("accumulate"))


def test_dead_grid_known_answers(dev):
    c = R.make_case("interior")
    T.check_dead_grid(DeviceSim(dev, c), c)


def test_learn_at_the_clip(dev):
    c = R.make_case("ragged257")
    T.check_learn(DeviceSim(dev, c), R.new_ref(c), c)


def test_cycle_init_copies_the_last_level(dev):
    c = R.make_case("interior")
    T.check_cycle_init(DeviceSim(dev, c, levels=3), c)


def test_large_grid_binning_backward_vs_float64(dev):
    """One backward on a grid of more than 8,192 tiles (k_scan + k_place);
    the reference lives on the nodes the particles touch, and the device's
    grid adjoints are zero everywhere else."""
    c = T.case_176()
    ref = R.FitRef(c.x, c.cov, c.vol, n_grid=c.n_grid, grid_extent=R.EXT, gravity=R.GRAV, init_v=c.v, levels=2,
                   ground_only=True, sparse=True, **R.MAT)
    r = T.run_176(ref, c)
    d = T.run_176(DeviceSim(dev, c), c, ref.nodes.numpy())
    _report("big176", R.compare(d, r, ref.grid_adjoint("g_v_out_scale")), device_bounds("big176"))


SENTINEL = np.uint32(0x7FC12345)  # a NaN payload no kernel produces


def test_get_writes_n_rows_only(dev):
    """n = 257 (np = 512 planes inside): after a forward and a backward pass,
    `get` of every field writes rows 0..256 of the output and leaves rows
    257..511 alone."""
    import torch
    from gsmpm import _lib
    from gsmpm._lib import LIB, check, ptr, stream_of
    c = R.make_case("ragged257")
    sim = DeviceSim(dev, c)
    R.one_substep(sim, c)
    sim.postprocess_forward()
    rows = 512
    for field, fid in _lib.FIT_FIELD.items():
        w = LIB.gsmpm_fit_field_width(fid)
        for level in ((0, 1) if field in R.LEVELED or field[1:] in R.LEVELED else (0,)):
            out = torch.from_numpy(np.full((rows, w), SENTINEL, np.uint32).view(F32)).to(dev)
            check(LIB.gsmpm_fit_get(sim.g._h, fid, level, ptr(out), stream_of(dev)))
            bits = out.cpu().numpy().view(np.uint32)
            assert (bits[c.n:] == SENTINEL).all(), (field, level)
            assert (bits[:c.n] != SENTINEL).all(), (field, level)
            assert np.array_equal(out.cpu().numpy()[:c.n].reshape(sim.get(field, level).shape), sim.get(field, level))
