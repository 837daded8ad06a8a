"""The fluid material (GSMPM_MAT_FLUID = 5: fluid_return_mapping,
constitutive_models.py:142-213, with the StVK Kirchhoff stress) as a uniform
handle, as a per-particle id and as a region, against the CPU oracle's phase
composition with a fifth code (tests/fluid_oracle.py).

Every trajectory case is test_gpu_mixed.py's scene (lego_problem(4000, 48), the
impulse moved to t = 0) for 30 substeps on the pipes `fused`, `phased` and
`fused_r1`, under test_gpu_mixed.BOUNDS: x 1e-4, v 2e-3, C 5e-3, F_trial 1e-4
(2e-2 on foam rows), metal yield 5e-3.  The fluid forms a true
matrix product (U diag V^T), so it takes the non-foam F_trial bound; it never
hardens, so its yield plane keeps the bits it was given.
"""
import copy
import json
import os

import numpy as np
import pytest

import oracle as O
from conftest import rel_err
from fluid_oracle import codes5, fluid_run, region_mask
from scenarios import CONFIGS, build_oracle_sim
from test_gpu_mixed import BOUNDS, PIPES, STEPS, _deformed_F, _problem

pytestmark = pytest.mark.gpu

FLUID_CASES = [(0.005, 0.008), (2000.0, 0.008), (2000.0, 50.0)]  # (yield_stress, plastic_viscosity)
_CACHE = {}


def _scene():
    if "prob" not in _CACHE:
        _CACHE["prob"] = _problem()
    return _CACHE["prob"]


def _layout(prob, name):
    x = prob["x"][:, 0]
    five = np.array([0.0, 1.0, 2.0, 3.0, 5.0], np.float32)
    if name == "fluid":
        return np.full(len(x), 5.0, np.float32)
    if name == "regions5":  # a fifth of the body's x extent each: jelly, metal, sand, foam, fluid
        q = np.floor(5.0 * (x - x.min()) / (x.max() - x.min())).astype(np.int64)
        return five[np.clip(q, 0, 4)]
    if name == "salt5":
        return np.random.default_rng(5).choice(five, size=len(x)).astype(np.float32)
    raise KeyError(name)


def _oracle(name, yld=0.005, pv=0.008):
    """The helper's oracle after STEPS substeps (computed once, never modified)."""
    key = ("oracle", name, yld, pv)
    if key not in _CACHE:
        prob = _scene()
        ref, imps, ops = build_oracle_sim(prob, material="metal")
        ref.yield_stress[:] = np.float32(yld)
        ids = _layout(prob, name)
        fluid_run(ref, ids, imps, ops, prob["cfg"]["substep_dt"], STEPS, pv)
        assert np.abs(ref.x - prob["x"]).max() > 1e-4 and np.isfinite(ref.x).all()
        _CACHE[key] = (ref, ids)
    return _CACHE[key]


def _gpu_sim(prob, dev, pipe, material, **over):
    from gpu_helpers import dropin_sim
    s, _ = dropin_sim(prob, dev, material=material, phased=pipe == "phased", **over)
    if pipe.startswith("fused_r"):
        s._sim.set_rebin_interval(int(pipe[len("fused_r"):]))
    assert s._sim.pipeline == ("phased" if pipe == "phased" else "fused")
    return s


def _run(s, prob, steps=STEPS):
    dt = prob["cfg"]["substep_dt"]
    for _ in range(steps):
        s.p2g2p(dt)


def _state(s):
    st = s.mpm_state
    return {"x": st.particle_xyz.to_torch().cpu().numpy(), "v": st.particle_vel.to_torch().cpu().numpy(),
            "C": st.particle_C.to_torch().cpu().numpy().reshape(-1, 9),
            "F_trial": st.particle_F_trial.to_torch().cpu().numpy().reshape(-1, 9),
            "yield": s.mpm_model.yield_stress.to_torch().cpu().numpy()}


def _errors(g, ref, ids, yield0):
    """Errors per field; `yield0`: the yield plane as it was set (kept bit for bit outside metal rows)."""
    code = codes5(ids)
    foam, metal = code == 3, code == 1
    e = {"x": rel_err(g["x"], ref.x), "v": rel_err(g["v"], ref.v), "C": rel_err(g["C"], ref.C),
         "F_trial": rel_err(g["F_trial"][~foam], ref.F_trial[~foam]) if (~foam).any() else 0.0,
         "F_trial_foam": rel_err(g["F_trial"][foam], ref.F_trial[foam]) if foam.any() else 0.0,
         "yield": rel_err(g["yield"][metal], ref.yield_stress[metal]) if metal.any() else 0.0}
    kept = bool(np.array_equal(g["yield"][~metal].view(np.uint32), yield0[~metal].view(np.uint32)))
    return e, kept


def _check(g, ref, ids, yield0, label, bounds=BOUNDS):
    e, kept = _errors(g, ref, ids, yield0)
    print(label, {k: f"{v:.2e}" for k, v in e.items()}, "non-metal yield kept:", kept)
    for k in g:
        assert np.isfinite(g[k]).all(), f"{label}: non-finite {k}"
    for k, v in e.items():
        assert v < bounds[k], f"{label} {k}: rel err {v:.3e} > {bounds[k]} (all: {e})"
    assert kept, f"{label}: the yield of a non-metal row changed"
    return e


# ---------------------------------------------------- 1. the handle exists --
def test_fluid_handle(dev):
    """gsmpm_mpm_create accepts GSMPM_MAT_FLUID (it was GSMPM_EINVAL): a uniform handle of code 5."""
    import torch
    from gsmpm.sim import MATERIALS, Simulator
    assert MATERIALS["fluid"] == 5
    prob = _scene()
    n = len(prob["x"])
    sim = Simulator(n, n_grid=48, material="fluid", yield_stress=3.5, plastic_viscosity=0.25)
    assert sim.material_mode == 0
    assert np.array_equal(sim.get("material").cpu().numpy(), np.full(n, 5.0, np.float32))
    t = lambda a: torch.from_numpy(a).to(dev)
    sim.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
    assert np.array_equal(sim.get("yield_stress").cpu().numpy(), np.full(n, 3.5, np.float32))
    sim.step(1e-4, [0] * 4)
    assert sim.material_mode == 0
    assert np.array_equal(sim.get("material").cpu().numpy(), np.full(n, 5.0, np.float32))
    assert np.array_equal(sim.get("yield_stress").cpu().numpy(), np.full(n, 3.5, np.float32))
    assert np.isfinite(sim.get("x").cpu().numpy()).all()
    by_code = Simulator(n, n_grid=48, material=5)
    assert np.array_equal(by_code.get("material").cpu().numpy(), np.full(n, 5.0, np.float32))


# ------------------------------------------------- 2. uniform trajectories --
@pytest.mark.parametrize("yld,pv", FLUID_CASES)
@pytest.mark.parametrize("pipe", PIPES)
def test_uniform_fluid_trajectory_parity(dev, pipe, yld, pv):
    """A handle created as fluid, through the drop-in with the two constants it
    lives on taken from the arguments, against fluid_run with every id 5.
    (0.005, 0.008): the defaults, nearly every row yields every substep;
    (2000, 0.008): both branches (a quarter of the rows yield by substep 29);
    (2000, 50): the viscosity slows the return (pf = 4 instead of 1.0005)."""
    prob = _scene()
    ref, ids = _oracle("fluid", yld, pv)
    s = _gpu_sim(prob, dev, pipe, "fluid", yield_stress=yld, plastic_viscosity=pv)
    assert s._sim.material_mode == 0 and s.mpm_model.material_code == 5
    _run(s, prob)
    g = _state(s)
    _check(g, ref, ids, np.full(len(ids), yld, np.float32), f"uniform fluid {pipe} yield {yld} pv {pv}")
    assert s._sim.material_mode == 0
    _CACHE[("gpu", pipe, yld, pv)] = g["F_trial"]


def test_viscosity_reaches_the_kernel(dev):
    """plastic_viscosity is an argument of the handle, not a constant of the
    build: at yield 2000 the runs at 50 and at 0.008 part by more than 1e-3
    on F_trial (the oracle's two runs part by 1.3e-2)."""
    prob = _scene()
    out = {}
    for pv in (0.008, 50.0):
        key = ("gpu", "fused", 2000.0, pv)
        if key not in _CACHE:
            s = _gpu_sim(prob, dev, "fused", "fluid", yield_stress=2000.0, plastic_viscosity=pv)
            _run(s, prob)
            _CACHE[key] = _state(s)["F_trial"]
        out[pv] = _CACHE[key]
    d = rel_err(out[50.0], out[0.008])
    do = rel_err(_oracle("fluid", 2000.0, 50.0)[0].F_trial, _oracle("fluid", 2000.0, 0.008)[0].F_trial)
    print("F_trial, plastic_viscosity 50 against 0.008: gpu", d, "oracle", do)
    assert d > 1e-3


# --------------------------------------------------- 3./4. mixed layouts --
def _permuted_spread(name, runs=3):
    """test_gpu_mixed._permuted_spread on this helper's oracle: max rel err of
    non-foam F_trial over `runs` permuted particle orders."""
    prob = _scene()
    ref, ids = _oracle(name)
    nonfoam = codes5(ids) != 3
    spread = 0.0
    for r in range(runs):
        perm = np.random.default_rng(100 + r).permutation(len(ids))
        p2 = dict(prob, x=prob["x"][perm], cov=prob["cov"][perm], vol=prob["vol"][perm])
        o, imps, ops = build_oracle_sim(p2, material="metal")
        fluid_run(o, ids[perm], imps, ops, prob["cfg"]["substep_dt"], STEPS)
        back = np.empty_like(o.F_trial)
        back[perm] = o.F_trial
        spread = max(spread, rel_err(back[nonfoam], ref.F_trial[nonfoam]))
    return spread


@pytest.mark.parametrize("layout", ["regions5", "salt5"])
@pytest.mark.parametrize("pipe", PIPES)
def test_mixed_five_codes_trajectory_parity(dev, pipe, layout):
    """Created as metal, a material id per particle out of {0, 1, 2, 3, 5}.
    `regions5`: fifths of the x extent (746-851 rows each); `salt5`: a random
    code per particle, where alone the F_trial bound may widen by
    test_mixed_trajectory_parity's rule (3x the oracle's own permuted-order
    spread, capped at 1e-3; the spread measured on the CPU is 1.05e-5, so the
    rule should not bite)."""
    import torch
    prob = _scene()
    ref, ids = _oracle(layout)
    code = codes5(ids)
    assert min(int((code == c).sum()) for c in (0, 1, 2, 3, 5)) >= 500
    s = _gpu_sim(prob, dev, pipe, "metal")
    assert s._sim.material_mode == 0
    s._sim.set("material", torch.from_numpy(ids).to(dev))
    assert s._sim.material_mode == 1
    _run(s, prob)
    g = _state(s)
    yield0 = np.full(len(ids), 0.005, np.float32)
    bounds = dict(BOUNDS)
    e, _ = _errors(g, ref, ids, yield0)
    if layout == "salt5":
        spread = _CACHE.setdefault("spread_salt5", _permuted_spread("salt5"))
        print("salt5", pipe, "F_trial", e["F_trial"], "permuted-order oracle spread", spread)
        if e["F_trial"] >= BOUNDS["F_trial"]:
            bounds["F_trial"] = min(max(BOUNDS["F_trial"], 3.0 * spread), 1e-3)
            print("salt5: F_trial bound ->", bounds["F_trial"])
    _check(g, ref, ids, yield0, f"mixed {layout} {pipe}", bounds)
    assert np.array_equal(s._sim.get("material").cpu().numpy(), ids)  # stored as given, in caller order


# ------------------------------------------------ 5. constitutive dispatch --
@pytest.mark.parametrize("jelly_fcr", [0, 1])
def test_constitutive_mixed_fluid_rows(dev, jelly_fcr):
    """test_constitutive_mixed_vs_oracle's id layout with 5 mixed in: runs of 128
    equal ids (wave-uniform waves) and a random id per row (divergent waves).
    The id-5 rows are within 1e-4 of O.fluid_return_mapping, keep their yield's
    bits, and -- bit 5 of GSMPM_MIXED_EXACT being clear in this build -- equal
    gsmpm_constitutive(5, ...) on the same inputs bit for bit."""
    import torch
    from gsmpm._lib import LIB, check, ptr, stream_of
    n = 5000
    F = _deformed_F(n, 1).reshape(n, 9)
    rng = np.random.default_rng(11)
    five = np.array([0.0, 1.0, 2.0, 3.0, 5.0], np.float32)
    ids = rng.choice(five, size=n).astype(np.float32)
    ids[:2560] = np.repeat(five[np.arange(20) % 5], 128)
    ids[[2570, 3001, 4999]] = np.array([4.0, 7.0, np.nan], np.float32)  # still the `else` branch
    mu = np.full(n, 8.3e4, np.float32)
    lam = np.full(n, 5.6e4, np.float32)
    # 2 mu |dev log s| is 1e4 - 5e4 on these F: the low yield returns every row, the high one none
    yld = np.where(rng.random(n) < 0.5, 0.005, 1e5).astype(np.float32)
    dt = 1e-4
    fl = ids == 5.0
    assert fl.sum() > 500
    Fo, To = O.fluid_return_mapping(F[fl], mu[fl], lam[fl], yld[fl], dt)
    Fo, To = Fo.reshape(-1, 9), To.reshape(-1, 9)
    moved = (Fo != F[fl]).any(axis=1)
    assert 0.1 * fl.sum() < moved.sum() < 0.9 * fl.sum()  # both branches
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ft, tm, tl, ty, tid = t(F), t(mu), t(lam), t(yld.copy()), t(ids)
    Fg, Tg = torch.empty_like(Ft), torch.empty_like(Ft)
    check(LIB.gsmpm_constitutive_mixed(ptr(tid), ptr(Ft), n, ptr(tm), ptr(tl), ptr(ty), dt, jelly_fcr, ptr(Fg),
                                       ptr(Tg), stream_of(dev)))
    Fg, Tg, yg = Fg.cpu().numpy(), Tg.cpu().numpy(), ty.cpu().numpy()
    assert np.isfinite(Fg).all() and np.isfinite(Tg).all()
    eF, eT = rel_err(Fg[fl], Fo), rel_err(Tg[fl], To)
    print("constitutive mixed, fluid rows, jelly_fcr", jelly_fcr, "F", eF, "tau", eT)
    assert eF < 1e-4 and eT < 1e-4
    assert np.array_equal(yg[fl].view(np.uint32), yld[fl].view(np.uint32))
    # codes 4, 7, NaN keep F_trial (the `else` branch), as 0 does
    other = np.isin(np.arange(n), [2570, 3001, 4999])
    assert np.array_equal(Fg[other], F[other])
    # the uniform kernel's body on the same rows
    nf = int(fl.sum())
    Fu_in, mu_u, lam_u, y_u = t(F[fl]), t(mu[fl]), t(lam[fl]), t(yld[fl].copy())
    Fu, Tu = torch.empty_like(Fu_in), torch.empty_like(Fu_in)
    check(LIB.gsmpm_constitutive(5, ptr(Fu_in), nf, ptr(mu_u), ptr(lam_u), ptr(y_u), dt, ptr(Fu), ptr(Tu),
                                 stream_of(dev)))
    Fu, Tu = Fu.cpu().numpy(), Tu.cpu().numpy()
    assert np.array_equal(Fg[fl].view(np.uint32), Fu.view(np.uint32))
    assert np.array_equal(Tg[fl].view(np.uint32), Tu.view(np.uint32))
    assert np.array_equal(y_u.cpu().numpy().view(np.uint32), yld[fl].view(np.uint32))


# --------------------------------------------------------------- 6. drop-in --
def test_dropin_fluid_records(dev):
    """A config with material "fluid", yield_stress and plastic_viscosity, a
    modify_material record that names the fluid and an additional_params record
    with a yield_stress: ids and yield plane as the records say (the strict
    f32 box test), and 30 substeps in parity with the helper."""
    from gpu_helpers import dropin_sim
    prob = dict(_scene())
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    y0, pv, y1 = 2000.0, 0.05, 50.0
    prob["cfg"].update(material="fluid", yield_stress=y0, plastic_viscosity=pv)
    E2, nu2, d2 = 2e5, 0.3, 200.0
    big = 10 ** 12
    box = lambda c, s: {"center": [c, 1.0, 1.0], "size": [s, 2.0, 2.0], "start_time": 0, "num_dt": big}
    recs = [dict(box(0.75, 0.25), id=10, type="modify_material", material=1),           # metal 0.5 < x < 1.0
            dict(box(0.625, 0.125), id=11, type="modify_material", material="fluid"),   # fluid again 0.5 < x < 0.75
            dict(box(0.625, 0.125), id=12, type="additional_params", E=E2, nu=nu2, density=d2, mu=1000,
                 yield_stress=y1)]
    prob["cfg"]["boundary_conditions"] = prob["cfg"]["boundary_conditions"] + recs
    x = prob["x"]
    ids = np.full(len(x), 5.0, np.float32)
    ids[region_mask(x, recs[0]["center"], recs[0]["size"])] = 1.0
    inp = region_mask(x, recs[1]["center"], recs[1]["size"])
    ids[inp] = 5.0
    assert (ids == 1.0).sum() > 300 and inp.sum() > 300 and (ids == 5.0).sum() > inp.sum() + 300
    yield0 = np.full(len(x), y0, np.float32)
    yield0[inp] = y1
    ref, imps, ops = build_oracle_sim(prob, material="metal")
    mo, lo = O.mu_lam(E2, nu2, 1)
    ref.mu[inp], ref.lam[inp] = mo[0], lo[0]
    ref.mass[inp] = np.float32(d2) * ref.vol[inp]
    ref.yield_stress[:] = yield0
    fluid_run(ref, ids, imps, ops, prob["cfg"]["substep_dt"], STEPS, pv)
    s, args = dropin_sim(prob, dev)
    assert s.mpm_model.material_code == 5 and s.mpm_model.plastic_viscosity == pv
    assert s._sim.material_mode == 1
    assert np.array_equal(s.mpm_model.material.to_torch().cpu().numpy(), ids)
    assert np.array_equal(s.mpm_model.yield_stress.to_torch().cpu().numpy(), yield0)
    assert rel_err(s.mpm_model.lam.to_torch().cpu().numpy(), ref.lam) < 1e-6
    _run(s, prob)
    _check(_state(s), ref, ids, yield0, "drop-in fluid records")


def test_lego_melt_config(dev, tmp_path):
    """configs/lego-melt.json: the lego as written with a fluid upper half; two frames of main.py."""
    from PIL import Image

    import main as drv
    with open(os.path.join(CONFIGS, "lego-melt.json")) as f:
        melt = json.load(f)
    with open(os.path.join(CONFIGS, "lego.json")) as f:
        plain = json.load(f)
    recs = melt["mpm"]["boundary_conditions"]
    assert recs[:len(plain["mpm"]["boundary_conditions"])] == plain["mpm"]["boundary_conditions"]
    assert {k: v for k, v in melt["mpm"].items() if k not in ("boundary_conditions", "plastic_viscosity")} == \
        {k: v for k, v in plain["mpm"].items() if k != "boundary_conditions"}
    mod = [r for r in recs if r["type"] == "modify_material"]
    par = [r for r in recs if r["type"] == "additional_params"]
    assert len(mod) == 1 and mod[0]["material"] == "fluid" and len(par) == 1 and "yield_stress" in par[0]
    assert (mod[0]["center"], mod[0]["size"]) == (par[0]["center"], par[0]["size"])
    assert "plastic_viscosity" in melt["mpm"]
    # the mpm group through the drop-in: the upper half is fluid with its own yield, and two frames stay finite
    from gpu_helpers import dropin_sim
    from scenarios import lego_problem
    prob = lego_problem(4000, 48, config="lego-melt.json")
    s, args = dropin_sim(prob, dev)
    assert args.plastic_viscosity == melt["mpm"]["plastic_viscosity"] == s._sim.params.plastic_viscosity
    up = region_mask(prob["x"], mod[0]["center"], mod[0]["size"])
    assert 0.25 * len(up) < up.sum() < 0.75 * len(up)
    assert np.array_equal(s.mpm_model.material.to_torch().cpu().numpy(), np.where(up, 5.0, 0.0).astype(np.float32))
    assert np.array_equal(s.mpm_model.yield_stress.to_torch().cpu().numpy(),
                          np.where(up, par[0]["yield_stress"], 0.005).astype(np.float32))
    _run(s, prob, 2 * args.steps_per_frame)
    s._sim.check_finite()
    g = _state(s)
    assert all(np.isfinite(g[k]).all() for k in g) and np.abs(g["x"] - prob["x"]).max() > 1e-4
    out = str(tmp_path / "melt")
    drv.main(["--config_path", os.path.join(CONFIGS, "lego-melt.json"), "--synthetic", "4000", "--n_grid", "48",
              "--num_frames", "2", "--output_path", out])
    for f in range(3):
        img = np.asarray(Image.open(os.path.join(out, "images", f"{f:04d}.png")))
        assert img.shape == (800, 800, 3) and img.dtype == np.uint8
    assert (np.asarray(Image.open(os.path.join(out, "images", "0002.png"))) > 0).any()


# ----------------------------------------------------------------- 7. refusals --
def test_refusals(dev):
    import ctypes

    import torch
    from gsmpm import _lib
    from gsmpm._lib import LIB
    from gsmpm.sim import Simulator
    from gpu_helpers import sim_args_from_cfg
    from mpm_solver.solver import MPM_Simulator
    prob = _scene()
    n = len(prob["x"])
    p = Simulator(n, n_grid=48, material="fluid").params  # a parameter block create accepts
    for code in (4, 6, 7, -1):  # 4 stays private (jelly + FCR)
        p.material = code
        h = ctypes.c_void_p()
        rc = LIB.gsmpm_mpm_create(ctypes.byref(p), ctypes.byref(h))
        assert rc == _lib.GSMPM_EINVAL and "Material not supported yet" in _lib.last_error(), code
        with pytest.raises(TypeError, match="Material not supported yet"):
            Simulator(n, n_grid=48, material=code)
    with pytest.raises(TypeError, match="Material not supported yet"):
        Simulator(n, n_grid=48, material="plasticine")
    # the differentiable simulator stays single-material and has no fluid
    args = sim_args_from_cfg(prob["cfg"], 48, material="fluid", fitting=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with pytest.raises(TypeError, match="Material not supported yet"):
        MPM_Simulator(t(prob["x"]), t(prob["cov"]), t(prob["vol"]), args)
    torch.cuda.synchronize()
