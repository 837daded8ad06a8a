"""Mixed-material scenes: the per-particle material field, the mixed dispatch
of the P2G kernels and the two region records (additional_params,
modify_material), against the CPU oracle's per-particle dispatch
(tests/mixed_oracle.py).

Bounds are test_gpu_mpm.py's test_materials_parity bounds: x 1e-4, v 2e-3,
C 5e-3, F_trial 1e-4 (2e-2 on foam rows), metal yield 5e-3; the
yield of every other row stays exactly the 0.005 it was created with.
"""
import copy

import numpy as np
import pytest

import oracle as O
from conftest import rel_err
from mixed_oracle import material_codes, mixed_run, mixed_stress, region_mask
from scenarios import build_oracle_sim, lego_problem, oracle_run

pytestmark = pytest.mark.gpu

STEPS = 30
PIPES = ["fused", "phased", "fused_r1"]
BOUNDS = {"x": 1e-4, "v": 2e-3, "C": 5e-3, "F_trial": 1e-4, "F_trial_foam": 2e-2, "yield": 5e-3}


# ------------------------------------------------------------ the scene --
def _problem():
    """lego_problem(4000, 48) with the config's impulse moved into the horizon (test_impulse_window)."""
    prob = lego_problem(4000, 48)
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    for d in prob["cfg"]["boundary_conditions"]:
        if d["type"] == "impulse":
            d["start_time"] = 0
            d["force"] = [-80.0, 0.0, 30.0]
    return prob


def _layout(prob, name):
    x = prob["x"][:, 0]
    if name == "regions":  # a quarter of the body's x extent each: jelly, metal, sand, foam
        q = np.floor(4.0 * (x - x.min()) / (x.max() - x.min())).astype(np.int64)
        return np.clip(q, 0, 3).astype(np.float32)
    if name == "salt":
        return np.random.default_rng(5).integers(0, 4, size=len(x)).astype(np.float32)
    if name == "metal":
        return np.full(len(x), 1.0, np.float32)
    raise KeyError(name)


_CACHE = {}


def _scene():
    if "prob" not in _CACHE:
        _CACHE["prob"] = _problem()
    return _CACHE["prob"]


def _oracle(name):
    """The helper's oracle after STEPS substeps of layout `name` (computed once, never modified)."""
    key = ("oracle", name)
    if key not in _CACHE:
        prob = _scene()
        ref, imps, ops = build_oracle_sim(prob, material="metal")
        ids = _layout(prob, name)
        mixed_run(ref, ids, imps, ops, prob["cfg"]["substep_dt"], STEPS)
        assert np.abs(ref.x - prob["x"]).max() > 1e-4 and np.isfinite(ref.x).all()
        _CACHE[key] = (ref, ids)
    return _CACHE[key]


def _gpu_sim(prob, dev, pipe, **over):
    from gpu_helpers import dropin_sim
    s, _ = dropin_sim(prob, dev, material="metal", phased=pipe == "phased", **over)
    if pipe.startswith("fused_r"):
        s._sim.set_rebin_interval(int(pipe[len("fused_r"):]))
    assert s._sim.pipeline == ("phased" if pipe == "phased" else "fused")
    return s


def _run(s, prob, steps=STEPS):
    dt = prob["cfg"]["substep_dt"]
    for _ in range(steps):
        s.p2g2p(dt)


def _errors(s, ref, ids):
    st = s.mpm_state
    code = material_codes(ids)
    foam, metal = code == 3, code == 1
    g = {"x": st.particle_xyz.to_torch().cpu().numpy(), "v": st.particle_vel.to_torch().cpu().numpy(),
         "C": st.particle_C.to_torch().cpu().numpy().reshape(-1, 9),
         "F_trial": st.particle_F_trial.to_torch().cpu().numpy().reshape(-1, 9)}
    y = s.mpm_model.yield_stress.to_torch().cpu().numpy()
    e = {"x": rel_err(g["x"], ref.x), "v": rel_err(g["v"], ref.v), "C": rel_err(g["C"], ref.C),
         "F_trial": rel_err(g["F_trial"][~foam], ref.F_trial[~foam]) if (~foam).any() else 0.0,
         "F_trial_foam": rel_err(g["F_trial"][foam], ref.F_trial[foam]) if foam.any() else 0.0,
         "yield": rel_err(y[metal], ref.yield_stress[metal]) if metal.any() else 0.0}
    other_yield_kept = bool(np.array_equal(y[~metal], np.full((~metal).sum(), 0.005, np.float32)))
    return e, other_yield_kept, g


def _check(s, ref, ids, label, bounds=BOUNDS):
    e, kept, g = _errors(s, ref, ids)
    print(label, {k: f"{v:.2e}" for k, v in e.items()}, "non-metal yield kept:", kept)
    for k, v in e.items():
        assert v < bounds[k], f"{label} {k}: rel err {v:.3e} > {bounds[k]} (all: {e})"
    assert kept, f"{label}: the yield of a non-metal row changed"
    return e, g


def _permuted_spread(name, runs=3):
    """Spread of the helper's oracle itself over permuted particle orders (the
    f32 summation order of P2G): max rel err of non-foam F_trial over `runs` orders."""
    prob = _scene()
    ref, ids = _oracle(name)
    nonfoam = material_codes(ids) != 3
    spread = 0.0
    for r in range(runs):
        perm = np.random.default_rng(100 + r).permutation(len(ids))
        p2 = dict(prob, x=prob["x"][perm], cov=prob["cov"][perm], vol=prob["vol"][perm])
        o, imps, ops = build_oracle_sim(p2, material="metal")
        mixed_run(o, ids[perm], imps, ops, prob["cfg"]["substep_dt"], STEPS)
        back = np.empty_like(o.F_trial)
        back[perm] = o.F_trial
        spread = max(spread, rel_err(back[nonfoam], ref.F_trial[nonfoam]))
    return spread


# ------------------------------------------------- 1. constitutive dispatch --
def _deformed_F(n, seed):
    """test_gpu_constitutive.py's moderately deformed F (rotation * stretch * rotation)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    Q *= np.sign(np.linalg.det(Q))[:, None, None]
    st = np.stack([rng.uniform(0.9, 1.1, n), rng.uniform(0.8, 1.2, n), rng.uniform(0.7, 1.3, n)], 1)
    F = (Q * st[:, None, :] @ np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]).astype(np.float32)
    F *= np.sign(np.linalg.det(F))[:, None, None]
    return F


@pytest.mark.parametrize("jelly_fcr", [0, 1])
def test_constitutive_mixed_vs_oracle(dev, jelly_fcr):
    import torch
    from gsmpm._lib import LIB, check, ptr, stream_of
    n = 5000
    F = _deformed_F(n, 1)
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 4, size=n).astype(np.float32)          # a random id per row: divergent waves
    ids[:2048] = np.repeat(np.arange(16) % 4, 128)               # runs of 128 equal ids: wave-uniform waves
    odd = np.array([7.0, -1.0, 0.5, np.nan], np.float32)         # the reference's `else` branch
    ids[[2050, 2117, 3001, 4999]] = odd                          # inside divergent waves
    ids[100:104] = odd                                           # and inside otherwise uniform ones
    mu = np.full(n, 8.3e4, np.float32)
    lam = np.full(n, 5.6e4, np.float32)
    yld = np.full(n, 0.005, np.float32)
    dt = 1e-4
    ref = O.OracleMPM(np.full((n, 3), 1.0, np.float32), np.zeros((n, 6), np.float32), np.ones(n, np.float32),
                      n_grid=8, material="metal", jelly_quirk=not jelly_fcr)
    ref.F_trial[:] = F.reshape(n, 9)
    ref.mu[:], ref.lam[:], ref.yield_stress[:] = mu, lam, yld
    mixed_stress(ref, ids, dt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ft, tm, tl, ty, tid = t(F.reshape(n, 9)), t(mu), t(lam), t(yld.copy()), t(ids)
    Fg, Tg = torch.empty_like(Ft), torch.empty_like(Ft)
    check(LIB.gsmpm_constitutive_mixed(ptr(tid), ptr(Ft), n, ptr(tm), ptr(tl), ptr(ty), dt, jelly_fcr, ptr(Fg),
                                       ptr(Tg), stream_of(dev)))
    Fg, Tg, yg = Fg.cpu().numpy(), Tg.cpu().numpy(), ty.cpu().numpy()
    code = material_codes(ids)
    assert [int((code == c).sum()) > 500 for c in range(4)] == [True] * 4
    keep = code != 3  # foam's element-wise F depends on the SVD basis itself (F13), as test_constitutive_vs_oracle
    eF, eT = rel_err(Fg[keep], ref.F[keep]), rel_err(Tg[keep], ref.stress[keep])
    ey = rel_err(yg, ref.yield_stress)
    print("constitutive mixed, jelly_fcr", jelly_fcr, "F", eF, "tau", eT, "yield", ey)
    assert np.isfinite(Fg).all() and np.isfinite(Tg).all()
    assert eF < 1e-4 and eT < 1e-4 and ey < 1e-4
    # row by row, each material's rows against its own scale
    for c in (0, 1, 2):
        r = code == c
        assert rel_err(Fg[r], ref.F[r]) < 1e-4, c
        if np.abs(ref.stress[r]).max() > 0:
            assert rel_err(Tg[r], ref.stress[r]) < 1e-4, c
        else:
            assert not Tg[r].any(), c  # jelly as written: zero stress
    assert np.array_equal(Fg[code == 0], F.reshape(n, 9)[code == 0])  # the else branch keeps F_trial
    assert (yg[code == 1] != np.float32(0.005)).any()  # metal hardened
    assert np.array_equal(yg[code != 1].view(np.uint32), yld[code != 1].view(np.uint32))  # bit for bit


# ------------------------------------------------------ 2. trajectory parity --
@pytest.mark.parametrize("layout", ["regions", "salt"])
@pytest.mark.parametrize("pipe", PIPES)
def test_mixed_trajectory_parity(dev, pipe, layout):
    """30 substeps of the impulse scene, created as metal, with a material id per
    particle, against the helper's oracle.  `fused_r1` re-bins every substep, so
    the id has to follow its particle through every permutation.

    Measured on an MI355X, all three pipes inside every bound: `salt` fused
    x 8.7e-7, v 5.5e-5, C 2.2e-4, F_trial 5.5e-5, foam F_trial 3.8e-3, yield
    5.5e-5 (phased F_trial 8.9e-5).  Metal's mixed body uses the
    reference-exact SVD arithmetic (constitutive.h EXACT, GSMPM_MIXED_EXACT):
    with the uniform kernels' fast SVD and SVD reuse in it, `salt` gave
    F_trial 3.24e-4 / 4.60e-4, over the 1.99e-4 its widened bound allows
    (DESIGN.md 3.6)."""
    import torch
    prob = _scene()
    ref, ids = _oracle(layout)
    s = _gpu_sim(prob, dev, pipe)
    assert s._sim.material_mode == 0
    s._sim.set("material", torch.from_numpy(ids).to(dev))
    assert s._sim.material_mode == 1
    _run(s, prob)
    bounds = dict(BOUNDS)
    e, kept, _ = _errors(s, ref, ids)
    if layout == "salt" and e["F_trial"] >= BOUNDS["F_trial"]:
        # the oracle's own spread over particle order, measured here; the
        # comparison stays against the helper's oracle
        spread = _CACHE.setdefault("spread_salt", _permuted_spread("salt"))
        bounds["F_trial"] = min(max(BOUNDS["F_trial"], 3.0 * spread), 1e-3)
        print("salt: permuted-order oracle spread", spread, "-> F_trial bound", bounds["F_trial"])
    _check(s, ref, ids, f"mixed {layout} {pipe}", bounds)
    assert np.array_equal(s._sim.get("material").cpu().numpy(), ids)  # stored as given, in caller order


# ------------------------------------- 3. uniform ids through the mixed kernel --
@pytest.mark.parametrize("pipe", PIPES)
def test_uniform_ids_through_mixed_kernel(dev, pipe):
    import torch
    prob = _scene()
    key = ("plain", "metal")
    if key not in _CACHE:
        ref, imps, ops = build_oracle_sim(prob, material="metal")
        oracle_run(ref, imps, ops, prob["cfg"]["substep_dt"], STEPS)
        _CACHE[key] = ref
    ref = _CACHE[key]
    ids = _layout(prob, "metal")
    s = _gpu_sim(prob, dev, pipe)
    s._sim.set("material", torch.from_numpy(ids).to(dev))
    assert s._sim.material_mode == 1
    _run(s, prob)
    _, g = _check(s, ref, ids, f"uniform ids, mixed kernel, {pipe}")
    u = _gpu_sim(prob, dev, pipe)  # the untouched uniform simulator
    _run(u, prob)
    assert u._sim.material_mode == 0
    _, _, gu = _errors(u, ref, ids)
    same = {k: bool(np.array_equal(g[k], gu[k])) for k in g}
    print(f"uniform ids through the mixed kernel ({pipe}): bit-identical to the uniform simulator:", same)


# -------------------------------------------------- 4. an untouched simulator --
@pytest.mark.parametrize("material,code", [("jelly", 0.0), ("sand", 2.0)])
def test_untouched_simulator_is_uniform(dev, material, code):
    import torch
    from gsmpm.sim import Simulator
    prob = _scene()
    n = len(prob["x"])
    sim = Simulator(n, n_grid=48, material=material)
    t = lambda a: torch.from_numpy(a).to(dev)
    assert sim.material_mode == 0
    assert np.array_equal(sim.get("material").cpu().numpy(), np.full(n, code, np.float32))
    sim.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
    sim.step(1e-4, [0] * 4)
    assert sim.material_mode == 0
    assert np.array_equal(sim.get("material").cpu().numpy(), np.full(n, code, np.float32))
    # mixed mode ends at set_particles, which resets the ids with mu / lam / yield
    sim.set("material", t(np.full(n, 3.0, np.float32)))
    assert sim.material_mode == 1
    sim.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
    assert sim.material_mode == 0
    assert np.array_equal(sim.get("material").cpu().numpy(), np.full(n, code, np.float32))


# ------------------------------------------------------------ 5. region calls --
def test_region_calls(dev):
    import torch
    from gsmpm.sim import Simulator
    rng = np.random.default_rng(3)
    n, ng = 3000, 32
    x = rng.uniform(0.6, 1.4, size=(n, 3)).astype(np.float32)
    x[0] = [1.25, 1.0, 1.0]                                     # exactly on the box face: excluded
    x[1] = [np.nextafter(np.float32(1.25), np.float32(0)), 1.0, 1.0]  # one ulp inside: included
    cov = np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32), (n, 1))
    vol = O.particle_volume(x, ng, 2.0)
    E0, nu0, d0 = 2e5, 0.3, 200.0
    sim = Simulator(n, n_grid=ng, material="metal", E=E0, nu=nu0, density=d0)
    t = lambda a: torch.from_numpy(a).to(dev)
    sim.set_particles(t(x), t(cov), t(vol))
    g = lambda k: sim.get(k).cpu().numpy()
    mu0, lam0, m0 = g("mu"), g("lam"), g("mass")
    c1, s1 = [1.0, 1.0, 1.0], [0.25, 0.5, 0.5]
    # the create-time E, nu and density reproduce the create-time values bit for bit
    sim.set_region_params(c1, s1, E0, nu0, d0)
    assert sim.material_mode == 0  # a params call alone does not enter mixed mode
    for k, a in (("mu", mu0), ("lam", lam0), ("mass", m0)):
        assert np.array_equal(g(k).view(np.uint32), a.view(np.uint32)), k
    in1 = region_mask(x, c1, s1)
    assert not in1[0] and in1[1] and 100 < in1.sum() < n - 100
    E1, nu1, d1 = 5e4, 0.25, 350.0
    sim.set_region_material(c1, s1, "sand")
    assert sim.material_mode == 1
    sim.set_region_params(c1, s1, E1, nu1, d1)  # mu = 1000: the sentinel, no override
    c2, s2 = [1.15, 1.1, 1.0], [0.2, 0.2, 0.6]   # overlaps the first box and reaches past it: it wins
    in2 = region_mask(x, c2, s2)
    assert (in1 & in2).sum() > 20 and (in2 & ~in1).sum() > 20 and (in1 & ~in2).sum() > 20
    E2, nu2, d2, muo = 8e5, 0.35, 90.0, 123.5
    sim.set_region_material(c2, s2, 3)
    sim.set_region_params(c2, s2, E2, nu2, d2, mu=muo)
    ids = np.full(n, 1.0, np.float32)
    ids[in1] = 2.0
    ids[in2] = 3.0
    assert np.array_equal(g("material"), ids)
    mu, lam, mass = mu0.copy(), lam0.copy(), m0.copy()
    m1, l1 = O.mu_lam(E1, nu1, 1)
    m2, l2 = O.mu_lam(E2, nu2, 1)
    mu[in1], lam[in1], mass[in1] = m1[0], l1[0], np.float32(d1) * vol[in1]
    mu[in2], lam[in2], mass[in2] = np.float32(muo), l2[0], np.float32(d2) * vol[in2]
    gm, gl, gmass = g("mu"), g("lam"), g("mass")
    out = ~(in1 | in2)
    assert np.array_equal(gm[out].view(np.uint32), mu0[out].view(np.uint32))  # rows outside: untouched
    assert np.array_equal(gl[out].view(np.uint32), lam0[out].view(np.uint32))
    # mu / lam through the device's powf / expf: a few ulp of the oracle's f32 path
    assert rel_err(gm, mu) < 1e-6 and rel_err(gl, lam) < 1e-6
    assert np.array_equal(gm[in2], np.full(in2.sum(), np.float32(muo)))
    assert np.array_equal(gmass, mass)  # f32(density) * vol: one exact f32 product
    assert np.array_equal(g("yield_stress"), np.full(n, 0.005, np.float32))
    with pytest.raises(TypeError, match="Material not supported yet"):
        sim.set_region_material(c1, s1, "plasticine")


# ------------------------------------------------- 6. drop-in on the lego scene --
def test_dropin_region_records(dev):
    from gpu_helpers import dropin_sim
    from mpm_solver.boundary_conditions import MaterialTypeModifier
    prob = dict(_scene())
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    E2, nu2, d2 = 2e5, 0.3, 200.0
    big = 10 ** 12
    box = lambda c, s: {"center": [c, 1.0, 1.0], "size": [s, 2.0, 2.0], "start_time": 0, "num_dt": big}
    recs = [dict(box(0.5, 0.5), id=10, type="additional_params", E=E2, nu=nu2, density=d2, mu=1000),  # x < 1.0
            dict(box(0.625, 0.125), id=11, type="modify_material", material=0),        # jelly 0.5 < x < 0.75
            dict(box(1.125, 0.125), id=12, type="modify_material", material="sand"),   # sand  1.0 < x < 1.25
            dict(box(1.375, 0.125), id=13, type="modify_material", material=3)]        # foam  1.25 < x < 1.5
    prob["cfg"]["boundary_conditions"] = prob["cfg"]["boundary_conditions"] + recs
    x = prob["x"]
    ids = np.full(len(x), 1.0, np.float32)
    for r in recs[1:]:
        code = {"sand": 2}.get(r["material"], r["material"])
        ids[region_mask(x, r["center"], r["size"])] = code
    assert [int((ids == c).sum()) > 300 for c in range(4)] == [True] * 4
    inp = region_mask(x, recs[0]["center"], recs[0]["size"])
    ref, imps, ops = build_oracle_sim(prob, material="metal")
    mo, lo = O.mu_lam(E2, nu2, 1)
    ref.mu[inp], ref.lam[inp] = mo[0], lo[0]
    ref.mass[inp] = np.float32(d2) * ref.vol[inp]
    mixed_run(ref, ids, imps, ops, prob["cfg"]["substep_dt"], STEPS)
    s, args = dropin_sim(prob, dev, material="metal")  # no raise
    assert s._sim.material_mode == 1
    assert np.array_equal(s.mpm_model.material.to_torch().cpu().numpy(), ids)
    dens = s.mpm_state.particle_density.to_torch().cpu().numpy()
    exp = np.full(len(x), np.float32(prob["cfg"]["density"]), np.float32)
    exp[inp] = d2
    assert np.array_equal(dens, exp)
    assert rel_err(s.mpm_model.lam.to_torch().cpu().numpy(), ref.lam) < 1e-6
    _run(s, prob)
    _check(s, ref, ids, "drop-in records")
    with pytest.raises(TypeError, match="Material not supported yet"):
        MaterialTypeModifier(len(x), dict(box(1.0, 0.1), id=14, type="modify_material", material="plasticine"), args)
    # model.material is writable: back to all metal
    import torch
    s.mpm_model.material.from_torch(torch.full((len(x),), 1.0))
    assert not (s.mpm_model.material.to_torch().cpu().numpy() != 1.0).any()


# --------------------------------------------- 7. udon with its own two records --
def test_udon_with_its_override_records(dev):
    """udon.json's records 9 and 10 (the metal udon's softer, lighter sand
    region), which the existing udon test drops on both sides.  The scene barely
    moves over 100 substeps: a does-it-run check at the existing test's 1e-4."""
    from gpu_helpers import dropin_sim
    from scenarios import world2grid_np
    from test_gpu_udon import UDON_MPM, _model
    g = _model(dev)
    xyz = g.get_xyz.detach().float().cpu().numpy()
    cov = g.get_covariance().detach().float().cpu().numpy()
    cfg = copy.deepcopy(UDON_MPM)
    over = [{"id": 9, "type": "additional_params", "center": [0.96, 0.82, 0.9], "size": [0.12, 0.12, 0.25],
             "start_time": 0, "num_dt": 100000000000000, "E": 2e5, "nu": 0.1, "density": 20.0, "mu": 1000},
            {"id": 10, "type": "modify_material", "center": [0.96, 0.84, 0.9], "size": [0.12, 0.12, 0.25],
             "start_time": 0, "num_dt": 100000000000000, "material": 2}]
    cfg["boundary_conditions"] = cfg["boundary_conditions"] + over
    xg, c, s = world2grid_np(xyz, cfg["grid_extent"])
    covg = (cov * (s * s)).astype(np.float32)
    ng = cfg["n_grid"]
    vol = O.particle_volume(xg, ng, cfg["grid_extent"])
    prob = dict(x=xg, cov=covg, vol=vol, cfg=cfg, n_grid=ng)
    inp, inm = region_mask(xg, over[0]["center"], over[0]["size"]), region_mask(xg, over[1]["center"], over[1]["size"])
    print("udon: particles inside the params / material boxes:", int(inp.sum()), int(inm.sum()))
    assert (int(inp.sum()), int(inm.sum())) == (205, 220)
    ref, imps, ops = build_oracle_sim(prob)
    mo, lo = O.mu_lam(over[0]["E"], over[0]["nu"], 1)
    ref.mu[inp], ref.lam[inp] = mo[0], lo[0]
    ref.mass[inp] = np.float32(over[0]["density"]) * ref.vol[inp]
    ids = np.full(len(xg), 1.0, np.float32)
    ids[inm] = 2.0
    sim, args = dropin_sim(prob, dev)
    assert sim._sim.material_mode == 1
    assert np.array_equal(sim.mpm_model.material.to_torch().cpu().numpy(), ids)
    dt, steps = cfg["substep_dt"], 100
    mixed_run(ref, ids, imps, ops, dt, steps)
    for _ in range(steps):
        sim.p2g2p(dt)
    x = sim.mpm_state.particle_xyz.to_torch().cpu().numpy()
    assert np.isfinite(ref.x).all()
    ex = rel_err(x, ref.x)
    sim.postprocess()
    ref.postprocess()
    gc = sim.mpm_state.particle_cov.to_torch().cpu().numpy().reshape(-1, 6)
    ec = rel_err(gc, ref.cov)
    print("udon with overrides: x", ex, "cov", ec)
    assert ex < 1e-4 and ec < 1e-4, (ex, ec)


# ----------------------------------------------------------------- 8. refusals --
def test_refusals(dev):
    import torch
    from gsmpm import _lib
    from gsmpm._lib import LIB, ptr, stream_of
    from gsmpm.sim import Simulator, _d3
    prob = _scene()
    n = len(prob["x"])
    t = lambda a: torch.from_numpy(a).to(dev)
    ids = t(np.full(n, 2.0, np.float32))
    slab = Simulator(n, n_grid=48, material="metal")
    slab.slab_init(0, 1, 0, 48)
    rc = LIB.gsmpm_mpm_set(slab._h, _lib.FIELD["material"], ptr(ids), stream_of(dev))
    assert rc == _lib.GSMPM_ESTATE and "slab" in _lib.last_error()
    rc = LIB.gsmpm_mpm_set_region_material(slab._h, _d3([1, 1, 1]), _d3([1, 1, 1]), 2, stream_of(dev))
    assert rc == _lib.GSMPM_ESTATE and "slab" in _lib.last_error()
    assert slab.material_mode == 0
    mixed = Simulator(n, n_grid=48, material="metal")
    mixed.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
    rc = LIB.gsmpm_mpm_set_region_material(mixed._h, _d3([1, 1, 1]), _d3([1, 1, 1]), 4, stream_of(dev))
    assert rc == _lib.GSMPM_EINVAL and mixed.material_mode == 0
    mixed.set("material", ids)
    assert mixed.material_mode == 1
    rc = LIB.gsmpm_mpm_slab_init(mixed._h, 0, 1, 0, 48, 2, 10)
    assert rc == _lib.GSMPM_ESTATE and "per-particle materials" in _lib.last_error()
    torch.cuda.synchronize()
