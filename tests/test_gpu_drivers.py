"""Particle drivers on the device (gsmpm_mpm_add_driver): the driver entry
points of the P2G kernels against the oracle composition of
tests/driver_ref.py, under test_gpu_mixed.py's bounds (x 1e-4, v 2e-3,
C 5e-3, F_trial 1e-4), on lego_problem(4000, 48) over 30 substeps.
"""
import os

import numpy as np
import pytest

import driver_ref as D
from conftest import rel_err
from scenarios import build_oracle_sim
from test_driver_ref import (RIGID_STEPS, RIGID_W, STEPS, layout, oracle_drivers, parity_oracle, parity_records,
                             rigid_distances, rigid_error, rigid_problem, scene, undriven_oracle)
from test_gpu_mixed import BOUNDS, PIPES, _check, _run

pytestmark = pytest.mark.gpu

CODE = {"jelly": 0.0, "metal": 1.0, "sand": 2.0}


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _dropin(prob, dev, pipe, material, records=(), **over):
    """The drop-in on `prob` with `records` appended to its bc list."""
    from gpu_helpers import dropin_sim
    p = dict(prob)
    p["cfg"] = dict(prob["cfg"], boundary_conditions=list(prob["cfg"]["boundary_conditions"]) + list(records))
    s, args = dropin_sim(p, dev, material=material, phased=pipe == "phased", **over)
    if pipe.startswith("fused_r"):
        s._sim.set_rebin_interval(int(pipe[len("fused_r"):]))
    assert s._sim.pipeline == ("phased" if pipe == "phased" else "fused")
    return s


def _ids(prob, material, ids):
    return np.full(len(prob["x"]), CODE[material], np.float32) if ids is None else ids


# ------------------------------------------------------ 1. trajectory parity --
@pytest.mark.parametrize("case", ["jelly", "metal", "sand", "regions"])
@pytest.mark.parametrize("pipe", PIPES)
def test_driver_trajectory_parity(dev, pipe, case):
    """A twist of the top fifth (substeps 5-24), a translation of a salted
    10 % mask (0-11) and a masked impulse on their union (8-19), given as time
    windows to the drop-in, whose clock decides the substep each one flips on."""
    prob = scene()
    material, ids_name = ("metal", "regions") if case == "regions" else (case, None)
    ref, ids = parity_oracle(material, ids_name)
    und = undriven_oracle(material, ids_name)
    # what makes the comparison mean something: the drivers moved the body far more than the bound
    assert rel_err(ref.x, und.x) > 100 * BOUNDS["x"]
    s = _dropin(prob, dev, pipe, material, parity_records(prob))
    if ids is not None:
        s._sim.set("material", _t(dev, ids))
        assert s._sim.material_mode == 1
    assert [bc.type for bc in s.particle_preprocess] == [r["type"] for r in parity_records(prob)]
    _run(s, prob)
    _check(s, ref, _ids(prob, material, ids), f"drivers {case} {pipe}")


# ------------------------------------------------------------- 2. selection --
@pytest.mark.parametrize("pipe", ["fused", "phased"])
def test_selection_is_fixed(dev, pipe):
    prob = scene()
    recs = parity_records(prob)
    drv = oracle_drivers(prob, recs)
    ref, _ = parity_oracle("metal")
    # on the oracle side some box rows leave the box during the run, and stay driven
    assert (drv[0].sel & ~D.box_selection(ref.x, recs[0]["center"], recs[0]["size"])).sum() > 0
    s = _dropin(prob, dev, pipe, "metal", recs)
    bits = [bc.bit for bc in s.particle_preprocess]
    sel = lambda: [s._sim.driver_selection(b).cpu().numpy() for b in bits]
    want = [d.sel for d in drv]
    assert want[0].sum() == D.box_selection(prob["x"], recs[0]["center"], recs[0]["size"]).sum() > 100
    for got, w in zip(sel(), want):
        assert got.dtype == bool and np.array_equal(got, w)
    _run(s, prob, STEPS // 2)
    s.flush()
    s._sim.resort()
    for got, w in zip(sel(), want):
        assert np.array_equal(got, w)
    _run(s, prob, STEPS - STEPS // 2)
    for got, w in zip(sel(), want):
        assert np.array_equal(got, w)
    _check(s, ref, _ids(prob, "metal", None), f"drivers with a resort, {pipe}")
    from gsmpm import _lib
    out = _t(dev, np.zeros(len(prob["x"]), np.uint8))
    rc = _lib.LIB.gsmpm_mpm_get_driver_selection(s._sim._h, 31, _lib.ptr(out), None)
    assert rc == _lib.GSMPM_EINVAL and "no driver" in _lib.last_error()


# ----------------------------------------------------------- 3. permutation --
@pytest.mark.parametrize("pipe", ["fused", "phased"])
def test_permuted_rows(dev, pipe):
    """The particle rows permuted, and the masks with them: the caller-order result within the bounds."""
    prob = scene()
    ref, _ = parity_oracle("sand")
    perm = np.random.default_rng(11).permutation(len(prob["x"]))
    p2 = dict(prob, x=prob["x"][perm], cov=prob["cov"][perm], vol=prob["vol"][perm])
    recs = parity_records(prob)
    for r in recs:
        if r.get("mask") is not None:
            r["mask"] = r["mask"][perm]
    s = _dropin(p2, dev, pipe, "sand", recs)
    _run(s, prob)

    class Back:  # the oracle's fields in the permuted order
        x, v, C, F_trial, yield_stress = (getattr(ref, k)[perm] for k in ("x", "v", "C", "F_trial", "yield_stress"))
    _check(s, Back, _ids(prob, "sand", None), f"drivers, permuted rows, {pipe}")
    got = s._sim.driver_selection(s.particle_preprocess[0].bit).cpu().numpy()
    assert np.array_equal(got, oracle_drivers(prob, recs[:1])[0].sel[perm])


# ----------------------------------------------------- 4. rigid translation --
@pytest.mark.parametrize("material", ["jelly", "metal"])
@pytest.mark.parametrize("pipe", ["fused", "phased"])
def test_rigid_translation_on_the_device(dev, pipe, material):
    """Every particle driven with w, gravity 0, no other record, against the
    analytic v = w, x = x0 + k dt w, C = 0, F = I; tolerance: ten times the
    oracle's own distance from that answer (the margin the float64-reference
    tests give the GPU over the oracle), at least 1e-6 absolute."""
    prob = rigid_problem()
    s = _dropin(prob, dev, pipe, material, with_collider=False)
    bc = s.enforce_particle_translation(RIGID_W, mask=np.ones(len(prob["x"]), bool))
    assert bc.bit == 0 and bc.isActive(0.0)
    _run(s, prob, RIGID_STEPS)
    st = s.mpm_state
    g = lambda f: f.to_torch().cpu().numpy().astype(np.float64)
    e = rigid_error(prob, g(st.particle_xyz), g(st.particle_vel), g(st.particle_C), g(st.particle_F_trial))
    o = rigid_distances(material)
    tol = {k: max(10.0 * o[k], 1e-6) for k in o}
    print(f"rigid translation {material} {pipe}: device", {k: f"{v:.2e}" for k, v in e.items()},
          "oracle", {k: f"{v:.2e}" for k, v in o.items()})
    for k in e:
        assert e[k] <= tol[k], (k, e[k], tol[k])


# ------------------------------------------------ 5. uniform scenes untouched --
def _bare(prob, dev, material="metal", **kw):
    from gsmpm.sim import Simulator
    cfg = prob["cfg"]
    sim = Simulator(len(prob["x"]), n_grid=prob["n_grid"], grid_extent=cfg["grid_extent"], material=material,
                    E=cfg["E"], nu=cfg["nu"], density=cfg["density"], gravity=cfg["gravity"], **kw)
    sim.set_particles(_t(dev, prob["x"]), _t(dev, prob["cov"]), _t(dev, prob["vol"]))
    return sim


@pytest.mark.parametrize("phased", [False, True])
def test_a_handle_without_active_drivers_is_the_plain_handle(dev, phased):
    """Two fresh handles, one of which holds a driver with an empty selection
    that is never activated (it launches the driver entry points): x, v, C and
    F_trial bit for bit over 30 substeps; device_bytes grows by 4 * np with the
    first driver, once, and not at all without one."""
    prob = scene()
    n = len(prob["x"])
    np_ = (n + 255) // 256 * 256  # the handle's row capacity: the particle count rounded up to 256
    dt = prob["cfg"]["substep_dt"]
    plain, drv = _bare(prob, dev, phased=phased), _bare(prob, dev, phased=phased)
    cube = [p.add_fixed_cube([1.0, 1.2, 0.5], [1.0, 0.8, 0.3]) for p in (plain, drv)]
    base = drv.device_bytes()
    assert base == plain.device_bytes()
    bit = drv.add_driver("enforce_particle_translation", mask=np.zeros(n, bool), velocity=[9.0, 9.0, 9.0])
    assert bit == 1 and not drv.driver_selection(bit).any()
    assert drv.device_bytes() == {**base, "total": base["total"] + 4 * np_}
    drv.add_driver("particle_impulse", center=[5.0, 5.0, 5.0], size=[0.1, 0.1, 0.1], force=[1.0, 0.0, 0.0],
                   substep_dt=dt)
    assert drv.device_bytes()["total"] == base["total"] + 4 * np_  # only once
    for p in (plain, drv):
        p.step(dt, [1 << cube[0]] * STEPS)
    assert plain.device_bytes() == base
    for k in ("x", "v", "C", "F_trial"):
        a, b = plain.get(k).cpu().numpy(), drv.get(k).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, rel_err(a, b))
    assert np.abs(plain.get("x").cpu().numpy() - prob["x"]).max() > 1e-4
    # an empty selection that IS active changes nothing either
    drv.step(dt, [(1 << cube[0]) | (1 << bit)] * 4)
    plain.step(dt, [1 << cube[0]] * 4)
    assert np.array_equal(plain.get("v").cpu().numpy().view(np.uint32), drv.get("v").cpu().numpy().view(np.uint32))


def test_a_driver_added_after_a_step_takes_effect(dev):
    """The cached graphs baked the plain entry points: they are dropped, as for a collider added late."""
    prob = scene()
    dt = prob["cfg"]["substep_dt"]
    sim = _bare(prob, dev)
    assert sim.graph_count() == 0
    sim.step(dt, [0] * 10)
    assert sim.graph_count() >= 1
    bit = sim.add_driver("enforce_particle_translation", center=[1.0, 1.0, 1.0], size=[2.0, 2.0, 2.0],
                         velocity=[0.0, 0.0, 7.0])
    assert sim.graph_count() == 0 and sim.driver_selection(bit).all()
    sim.step(dt, [1 << bit] * 10)
    assert sim.graph_count() >= 1
    v = sim.get("v").cpu().numpy()
    assert np.abs(v - np.array([0.0, 0.0, 7.0], np.float32)).max() < 0.05  # one substep of gravity: dt * 100
    counts = []
    for _ in range(3):
        sim.step(dt, [1 << bit] * 10)
        counts.append(sim.graph_count())
    assert all(c == counts[0] for c in counts), counts  # and the new graphs are reused


# ------------------------------------------------------------- 6. refusals --
def _raw_add(sim, dev, mask=None, **kw):
    from gsmpm import _lib
    d = _lib.Driver()
    d.kind = kw.pop("kind", 1)
    d.center[:], d.size[:] = kw.pop("center", [1.0, 1.0, 1.0]), kw.pop("size", [0.5, 0.5, 0.5])
    d.velocity[:] = kw.pop("velocity", [1.0, 0.0, 0.0])
    d.force[:], d.substep_dt = kw.pop("force", [1.0, 0.0, 0.0]), kw.pop("substep_dt", 1e-4)
    d.point[:], d.axis[:] = kw.pop("point", [1.0, 1.0, 1.0]), kw.pop("axis", [0.0, 0.0, 1.0])
    d.omega, d.along = kw.pop("omega", 1.0), kw.pop("along", 0.0)
    assert not kw
    import ctypes
    rc = _lib.LIB.gsmpm_mpm_add_driver(sim._h, ctypes.byref(d), None if mask is None else _lib.ptr(mask),
                                       _lib.stream_of(dev))
    return rc, _lib.last_error()


def test_slab_and_fold_handles_refuse(dev):
    from gsmpm import _lib
    from gsmpm.sim import Simulator
    prob = scene()
    n = len(prob["x"])
    slab = Simulator(n, n_grid=48, material="metal")
    slab.slab_init(0, 1, 0, 48)
    rc, msg = _raw_add(slab, dev)
    assert rc == _lib.GSMPM_ESTATE and "slab" in msg
    assert slab.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0  # no id was taken
    # the other order: slab_init on a handle that holds a driver; it stays an ordinary handle that steps
    sim = _bare(prob, dev)
    bit = sim.add_driver("enforce_particle_translation", center=[1, 1, 1], size=[2, 2, 2], velocity=[0, 0, 1])
    rc = _lib.LIB.gsmpm_mpm_slab_init(sim._h, 0, 1, 0, 48, 2, 10)
    assert rc == _lib.GSMPM_ESTATE and "particle drivers" in _lib.last_error()
    sim.step(1e-4, [1 << bit] * 2)
    assert np.isfinite(sim.get("v").cpu().numpy()).all()
    old = os.environ.get("GSMPM_FOLD")
    os.environ["GSMPM_FOLD"] = "1"
    try:
        fold = _bare(prob, dev)
    finally:
        if old is None:
            os.environ.pop("GSMPM_FOLD")
        else:
            os.environ["GSMPM_FOLD"] = old
    assert fold.folded
    before = fold.device_bytes()
    rc, msg = _raw_add(fold, dev)
    assert rc == _lib.GSMPM_ESTATE and "GSMPM_FOLD" in msg
    assert fold.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == 0 and fold.device_bytes() == before


def test_bad_arguments(dev):
    from gsmpm import _lib
    from gsmpm.sim import Simulator
    prob = scene()
    n = len(prob["x"])
    fresh = Simulator(n, n_grid=48, material="metal")
    rc, msg = _raw_add(fresh, dev)
    assert rc == _lib.GSMPM_ESTATE and "particles not set" in msg
    sim = _bare(prob, dev)
    before = sim.device_bytes()
    nan, inf = float("nan"), float("inf")
    bad = [dict(kind=3), dict(kind=-1), dict(kind=0, force=[nan, 0, 0]), dict(kind=0, substep_dt=inf),
           dict(kind=1, velocity=[0, inf, 0]), dict(kind=2, axis=[0, 0, 0]), dict(kind=2, axis=[0, nan, 1]),
           dict(kind=2, point=[nan, 0, 0]), dict(kind=2, omega=nan), dict(kind=2, along=inf),
           dict(size=[0.5, 0.0, 0.5]), dict(size=[0.5, -1.0, 0.5]), dict(size=[0.5, nan, 0.5]),
           dict(center=[inf, 1, 1])]
    for kw in bad:
        rc, msg = _raw_add(sim, dev, **kw)
        assert rc == _lib.GSMPM_EINVAL and "gsmpm_mpm_add_driver" in msg, (kw, rc, msg)
    assert _lib.LIB.gsmpm_mpm_add_driver(sim._h, None, None, None) == _lib.GSMPM_EINVAL
    # nothing was taken: the first good record gets id 0, and a mask makes the box irrelevant
    assert sim.device_bytes() == before
    rc, msg = _raw_add(sim, dev, mask=_t(dev, np.ones(n, np.uint8)), size=[0.0, 0.0, 0.0])
    assert rc == 0, msg
    assert sim.driver_selection(0).all()
    with pytest.raises(ValueError, match="unknown kind"):
        sim.add_driver("pull", mask=np.ones(n, bool))
    with pytest.raises(TypeError, match="missing"):
        sim.add_driver("enforce_particle_rotation", mask=np.ones(n, bool), point=[1, 1, 1])
    with pytest.raises(TypeError, match="unexpected"):
        sim.add_driver("enforce_particle_translation", mask=np.ones(n, bool), velocity=[1, 0, 0], force=[1, 0, 0])
    with pytest.raises(TypeError, match="center and size, or as mask"):
        sim.add_driver("enforce_particle_translation", velocity=[1, 0, 0])
    with pytest.raises(ValueError, match="entries"):
        sim.add_driver("enforce_particle_translation", velocity=[1, 0, 0], mask=np.ones(n - 1, bool))
    assert sim.add_driver("enforce_particle_translation", velocity=[1, 0, 0], center=[1, 1, 1], size=[1, 1, 1]) == 1


def test_the_33rd_id_is_refused(dev):
    from gsmpm import _lib
    prob = scene()
    sim = _bare(prob, dev)
    for b in range(32):
        if b % 4 == 0:
            assert sim.add_fixed_cube([1.0, 1.0, 1.0], [0.1, 0.1, 0.1]) == b
        else:
            assert sim.add_driver("enforce_particle_translation", center=[1, 1, 1], size=[0.2, 0.2, 0.2],
                                  velocity=[0, 0, 0]) == b
    rc, msg = _raw_add(sim, dev)
    assert rc == _lib.GSMPM_EINVAL and "too many boundary conditions (max 32)" in msg
    sim.step(1e-4, [0xFFFFFFFF] * 2)  # 24 drivers, all active
    assert np.isfinite(sim.get("v").cpu().numpy()).all()


def test_fitting_refuses_driver_records(dev):
    from gpu_helpers import dropin_sim
    from scenarios import lego_problem
    prob = lego_problem(500, 32)
    prob["cfg"] = dict(prob["cfg"], boundary_conditions=[])
    sim, args = dropin_sim(prob, dev, with_collider=False, fitting=True)
    rec = dict(type="enforce_particle_translation", velocity=[1, 0, 0], center=[1, 1, 1], size=[1, 1, 1])
    with pytest.raises(TypeError, match="fitting"):
        sim.set_boundary_conditions([rec], args)
    for call in (lambda: sim.add_particle_impulse([1, 0, 0], center=[1, 1, 1], size=[1, 1, 1], substep_dt=1e-4),
                 lambda: sim.enforce_particle_translation([1, 0, 0], center=[1, 1, 1], size=[1, 1, 1]),
                 lambda: sim.enforce_particle_rotation([1, 1, 1], [0, 0, 1], 1.0, center=[1, 1, 1], size=[1, 1, 1])):
        with pytest.raises(TypeError, match="fitting"):
            call()
    assert sim.particle_preprocess == []


# -------------------------------------------------------------- 7. drop-in --
def test_dropin_lego_wring(dev):
    """configs/lego-wring.json's bc list through set_boundary_conditions at this size, against driver_run."""
    from scenarios import lego_problem
    prob = lego_problem(4000, 48, config="lego-wring.json")
    cfg = prob["cfg"]
    recs = [r for r in cfg["boundary_conditions"] if r["type"] == "enforce_particle_rotation"]
    ref, imps, ops = build_oracle_sim(prob)  # the fixed cube and the ground plane
    drv = oracle_drivers(prob, recs)
    assert len(drv) == 1 and drv[0].sel.sum() > 300
    D.driver_run(ref, drv, imps, ops, cfg["substep_dt"], STEPS)
    und, imps, ops = build_oracle_sim(prob)
    D.driver_run(und, [], imps, ops, cfg["substep_dt"], STEPS)
    assert rel_err(ref.x, und.x) > 10 * BOUNDS["x"]
    s = _dropin(dict(prob, cfg=dict(cfg)), dev, "fused", cfg["material"])
    (bc,) = s.particle_preprocess
    assert bc.type == "enforce_particle_rotation" and np.array_equal(
        s._sim.driver_selection(bc.bit).cpu().numpy(), drv[0].sel)
    _run(s, prob)
    _check(s, ref, _ids(prob, "jelly", None), "lego-wring drop-in")
