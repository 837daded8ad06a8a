"""Particle drivers on the CPU: the oracle composition (tests/driver_ref.py)
against known answers, its own invariants and the analytic rigid translation,
and the pieces of the feature that need no GPU (the exported symbols, the
header and bindings, the drop-in's descriptors, configs/lego-wring.json).
"""
from __future__ import annotations

import copy
import ctypes
import functools
import json
import os
import re
import types

import numpy as np
import pytest

import driver_ref as D
from conftest import PKG, ROOT, rel_err
from scenarios import build_oracle_sim, lego_problem, oracle_run

f32 = np.float32
STEPS = 30
# test_gpu_mixed.BOUNDS (that module is GPU-marked as a whole; the values are its own)
BOUNDS = {"x": 1e-4, "v": 2e-3, "C": 5e-3, "F_trial": 1e-4}


# ------------------------------------------------------------ the scene --
@functools.lru_cache(maxsize=None)
def scene():
    """lego_problem(4000, 48) with the config's own impulse off (its window never opens in the horizon)."""
    prob = lego_problem(4000, 48)
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    prob["cfg"]["boundary_conditions"] = [d for d in prob["cfg"]["boundary_conditions"] if d["type"] != "impulse"]
    return prob


def parity_records(prob):
    """The three overlapping records of the parity scene, as keyword dicts
    shared by the oracle side and the drop-in side: a twist of the top fifth
    (substeps 5-24), a translation of a salted 10 % mask (0-11) and a masked
    impulse on the union (8-19).  Windows as times, half a substep off the
    flips so the f64 clock decides them without a tie."""
    x = prob["x"]
    dt = prob["cfg"]["substep_dt"]
    zmax, z80 = float(x[:, 2].max()), float(np.quantile(x[:, 2], 0.8))
    box = dict(center=[1.0, 1.0, zmax], size=[0.3, 0.3, zmax - z80])
    salt = np.random.default_rng(7).random(len(x)) < 0.1
    twist_sel = D.box_selection(x, box["center"], box["size"])
    w = lambda a, b: dict(start_time=(a - 0.5) * dt, end_time=(b + 0.5) * dt)
    return [
        dict(type="enforce_particle_rotation", **box, point=[1.0, 1.0, 1.0], axis=[0.0, 0.0, 1.0], omega=40.0,
             along=1.0, **w(5, 24)),
        dict(type="enforce_particle_translation", mask=salt, velocity=[3.0, 0.0, 1.5], **w(0, 11)),
        dict(type="particle_impulse", mask=twist_sel | salt, force=[-80.0, 0.0, 30.0], **w(8, 19)),
    ]


def oracle_drivers(prob, recs, x=None):
    """driver_ref.Driver records of bc dicts (box selections on x, default the scene's positions)."""
    x = prob["x"] if x is None else x
    out = []
    for r in recs:
        sel = r["mask"] if r.get("mask") is not None else D.box_selection(x, r["center"], r["size"])
        kw = {k: r[k] for k in ("force", "velocity", "point", "axis", "omega", "along") if k in r}
        if r["type"] == "particle_impulse":
            kw["substep_dt"] = prob["cfg"]["substep_dt"]
        out.append(D.Driver(r["type"], sel, start=r.get("start_time", 0.0), end=r.get("end_time", 999.0), **kw))
    return out


_CACHE = {}


def parity_oracle(material, ids_name=None):
    """The oracle after STEPS substeps of the parity scene (computed once, never modified): (ref, ids)."""
    key = (material, ids_name)
    if key not in _CACHE:
        prob = scene()
        ref, imps, ops = build_oracle_sim(prob, material=material)
        ids = layout(prob, ids_name)
        D.driver_run(ref, oracle_drivers(prob, parity_records(prob)), imps, ops, prob["cfg"]["substep_dt"], STEPS,
                     material=ids)
        assert np.isfinite(ref.x).all()
        _CACHE[key] = (ref, ids)
    return _CACHE[key]


def undriven_oracle(material, ids_name=None):
    key = ("undriven", material, ids_name)
    if key not in _CACHE:
        prob = scene()
        ref, imps, ops = build_oracle_sim(prob, material=material)
        D.driver_run(ref, [], imps, ops, prob["cfg"]["substep_dt"], STEPS, material=layout(prob, ids_name))
        _CACHE[key] = ref
    return _CACHE[key]


def layout(prob, name):
    """test_gpu_mixed's `regions` layout: a quarter of the body's x extent each, jelly, metal, sand, foam."""
    if name is None:
        return None
    assert name == "regions"
    x = prob["x"][:, 0]
    q = np.floor(4.0 * (x - x.min()) / (x.max() - x.min())).astype(np.int64)
    return np.clip(q, 0, 3).astype(f32)


def rigid_problem():
    """Every particle selected, gravity 0, no other record: a rigid translation."""
    prob = dict(scene())
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    prob["cfg"]["gravity"] = [0.0, 0.0, 0.0]
    prob["cfg"]["boundary_conditions"] = []
    return prob


RIGID_W = (3.0, -2.0, 1.5)
RIGID_STEPS = 10


def rigid_distances(material):
    """The oracle's distance from v = w, x = x0 + k dt w, C = 0, F = I after
    RIGID_STEPS substeps: {x, v, C, F} max abs."""
    key = ("rigid", material)
    if key not in _CACHE:
        prob = rigid_problem()
        ref, imps, ops = build_oracle_sim(prob, material=material, with_collider=False)
        d = D.Driver("enforce_particle_translation", np.ones(len(prob["x"]), bool), velocity=RIGID_W)
        D.driver_run(ref, [d], imps, ops, prob["cfg"]["substep_dt"], RIGID_STEPS)
        _CACHE[key] = rigid_error(prob, ref.x, ref.v, ref.C, ref.F_trial)
    return _CACHE[key]


def rigid_error(prob, x, v, C, F):
    w = np.asarray(RIGID_W, np.float64)
    xa = prob["x"].astype(np.float64) + RIGID_STEPS * prob["cfg"]["substep_dt"] * w
    eye = np.eye(3).reshape(1, 9)
    return {"x": float(np.abs(x - xa).max()), "v": float(np.abs(v - w).max()),
            "C": float(np.abs(np.asarray(C).reshape(-1, 9)).max()),
            "F": float(np.abs(np.asarray(F).reshape(-1, 9) - eye).max())}


# ----------------------------------------------------- 1. known answers --
def _rows():
    x = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.25], [0.75, 1.25, 0.5], [1.0, 0.5, 1.5]], f32)
    v = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-1.0, 0.5, 0.25], [4.0, 4.0, 4.0]], f32)
    m = np.array([0.5, 0.25, 2.0, 1.0], f32)
    return x, v, m


def test_known_answer_impulse():
    x, v, m = _rows()
    d = D.Driver("particle_impulse", [True, True, False, True], force=[1.0, -2.0, 0.5], substep_dt=0.5)
    D.apply_driver(d, x, v, m)
    # v + f / m * 0.5: every value a dyadic rational, exact in f32
    exp = np.array([[1.0, -2.0, 0.5], [3.0, -2.0, 4.0], [-1.0, 0.5, 0.25], [4.5, 3.0, 4.25]], f32)
    assert np.array_equal(v, exp)


def test_known_answer_translation():
    x, v, m = _rows()
    w = [0.1, -0.2, 0.3]  # not representable: the f32 of the doubles, bit for bit
    d = D.Driver("enforce_particle_translation", [False, True, True, False], velocity=w)
    v0 = v.copy()
    D.apply_driver(d, x, v, m)
    assert np.array_equal(v[[1, 2]], np.tile(np.asarray(w, np.float64).astype(f32), (2, 1)))
    assert np.array_equal(v[[0, 3]], v0[[0, 3]])


def test_known_answer_rotation():
    x, v, m = _rows()
    # axis (0, 0, 2) normalises to z; omega 2, along 0.5, about the line through (1, 1, .)
    d = D.Driver("enforce_particle_rotation", [True, True, True, False], point=[1.0, 1.0, 0.0], axis=[0.0, 0.0, 2.0],
                 omega=2.0, along=0.5)
    assert np.array_equal(d.axis, np.array([0, 0, 1], f32))
    D.apply_driver(d, x, v, m)
    # omega * (-ry, rx, 0) + along * z
    exp = np.array([[0.0, 0.0, 0.5], [0.0, 1.0, 0.5], [-0.5, -0.5, 0.5], [4.0, 4.0, 4.0]], f32)
    assert np.array_equal(v, exp)
    # a tilted axis: v is perpendicular to the arm and to the axis but for `along`, and |v_perp| = omega * distance
    a = np.array([1.0, 2.0, -2.0])
    d = D.Driver("enforce_particle_rotation", [True] * 4, point=[0.5, 0.25, 1.0], axis=a, omega=3.0, along=0.0)
    x, v, m = _rows()
    D.apply_driver(d, x, v, m)
    ah = a / 3.0
    r = x.astype(np.float64) - np.array([0.5, 0.25, 1.0])
    assert np.abs(v @ ah).max() < 1e-6 and np.abs((v * r).sum(1)).max() < 1e-6
    dist = np.linalg.norm(r - np.outer(r @ ah, ah), axis=1)
    assert np.allclose(np.linalg.norm(v, axis=1), 3.0 * dist, rtol=1e-6)


def test_empty_selection_is_a_no_op():
    x, v, m = _rows()
    v0 = v.copy()
    for kind, kw in (("particle_impulse", dict(force=[1, 1, 1], substep_dt=1.0)),
                     ("enforce_particle_translation", dict(velocity=[1, 1, 1])),
                     ("enforce_particle_rotation", dict(point=[0, 0, 0], axis=[0, 1, 0], omega=1.0))):
        D.apply_driver(D.Driver(kind, [False] * 4, **kw), x, v, m)
    assert np.array_equal(v, v0)


# ------------------------------------------------------ 2. order matters --
def test_order_matters():
    x, v, m = _rows()
    imp = D.Driver("particle_impulse", [True, True, False, False], force=[1.0, 0.0, 0.0], substep_dt=1.0)
    tr = D.Driver("enforce_particle_translation", [False, True, True, False], velocity=[7.0, 7.0, 7.0])
    a, b = v.copy(), v.copy()
    for d in (imp, tr):
        D.apply_driver(d, x, a, m)
    for d in (tr, imp):
        D.apply_driver(d, x, b, m)
    # row 1 is in both: a later enforce overrides the kick, a later kick adds to the enforce
    assert np.array_equal(a[1], np.array([7, 7, 7], f32)) and np.array_equal(b[1], np.array([11, 7, 7], f32))
    assert np.array_equal(a[[0, 2, 3]], b[[0, 2, 3]])


# --------------------------------------------- 3. no driver: the oracle --
@pytest.mark.parametrize("material", ["jelly", "metal"])
def test_no_driver_is_oracle_run(material):
    prob = dict(scene())
    prob["cfg"] = copy.deepcopy(prob["cfg"])
    prob["cfg"]["boundary_conditions"].append(  # an impulse in the horizon: the impulse phase is exercised
        {"id": 2, "type": "impulse", "center": [1.0, 0.65, 1.22], "size": [1.4, 0.18, 0.27],
         "force": [-80.0, 0.0, 30.0], "start_time": 0, "num_dt": 10})
    dt = prob["cfg"]["substep_dt"]
    a, imps, ops = build_oracle_sim(prob, material=material)
    oracle_run(a, imps, ops, dt, 12)
    b, imps, ops = build_oracle_sim(prob, material=material)
    D.driver_run(b, [], imps, ops, dt, 12)
    for k in ("x", "v", "C", "F_trial", "F", "yield_stress"):
        assert np.array_equal(getattr(a, k).view(np.uint32), getattr(b, k).view(np.uint32)), k


# ------------------------------------------------- 4. rigid translation --
@pytest.mark.parametrize("material", ["jelly", "metal"])
def test_rigid_translation(material):
    """Every particle driven with one velocity, no gravity, no other record:
    the grid velocity is w wherever there is mass, so G2P returns v = w, C = 0
    and F stays I.  Measured: jelly |v - w| 1.2e-6, |C| 3.7e-5; metal |v - w|
    5.9e-6, |C| 4.2e-4 (f32 rounding of the normalisation m v / m)."""
    e = rigid_distances(material)
    print("rigid translation", material, {k: f"{v:.2e}" for k, v in e.items()})
    # v: the f32 rounding of (sum w_i m w) / (sum w_i m) over 27 nodes and of G2P's 27-term sum, allowed 64 ulp
    # of |w|'s largest component (3: ulp 2^-22); C = 4 inv_dx sum w_i v_i dpos_i^T carries that error times
    # 4 inv_dx (|dpos| < 1.5 dx, the weights sum to 1); x adds dt * the v error and half an ulp of x (2^-24 * 2)
    # a substep; F_trial = (I + dt C) F adds dt * the C error a substep, and metal's return map a few ulp of 1
    prob = rigid_problem()
    ev = 64 * 2.0 ** -22
    eC = 4 * (prob["n_grid"] / prob["cfg"]["grid_extent"]) * ev
    ex = RIGID_STEPS * (prob["cfg"]["substep_dt"] * ev + 2.0 ** -24)
    eF = RIGID_STEPS * (prob["cfg"]["substep_dt"] * eC + 8 * 2.0 ** -23)
    assert e["v"] < ev and e["C"] < eC and e["x"] < ex and e["F"] < eF, (e, ev, eC, ex, eF)


# -------------------------------------------- 5. permuted-order spread --
def test_permuted_order_spread():
    """The oracle's own spread over three permuted particle orders (the f32
    summation order of P2G) on the parity scene, metal and sand, stays ten
    times or more inside the bounds the GPU is held to.  Measured: x 2.4e-7,
    v 5.3e-6, C 2.5e-5, F_trial 9.8e-6."""
    prob = scene()
    dt = prob["cfg"]["substep_dt"]
    recs = parity_records(prob)
    worst = {k: 0.0 for k in BOUNDS}
    for material in ("metal", "sand"):
        ref, _ = parity_oracle(material)
        for r in range(3):
            perm = np.random.default_rng(100 + r).permutation(len(prob["x"]))
            p2 = dict(prob, x=prob["x"][perm], cov=prob["cov"][perm], vol=prob["vol"][perm])
            o, imps, ops = build_oracle_sim(p2, material=material)
            drv = oracle_drivers(prob, recs)
            for d in drv:
                d.sel = d.sel[perm]
            D.driver_run(o, drv, imps, ops, dt, STEPS)
            for k in BOUNDS:
                back = np.empty_like(getattr(o, k))
                back[perm] = getattr(o, k)
                worst[k] = max(worst[k], rel_err(back, getattr(ref, k)))
    print("permuted-order spread", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, b in BOUNDS.items():
        assert worst[k] * 10.0 <= b, (k, worst[k], b)


def test_parity_scene_means_something():
    """The driven and undriven oracle runs differ in x by more than 100x the x
    bound, the box record selects rows that leave the box while driven, and
    the three selections overlap."""
    prob = scene()
    recs = parity_records(prob)
    drv = oracle_drivers(prob, recs)
    ref, _ = parity_oracle("metal")
    und = undriven_oracle("metal")
    diff = rel_err(ref.x, und.x)
    left = int((drv[0].sel & ~D.box_selection(ref.x, recs[0]["center"], recs[0]["size"])).sum())
    print("driven vs undriven x:", diff, "box rows:", int(drv[0].sel.sum()), "left the box:", left)
    assert diff > 100 * BOUNDS["x"]
    assert drv[0].sel.sum() > 100 and left > 0
    assert (drv[0].sel & drv[1].sel).sum() > 0 and np.array_equal(drv[2].sel, drv[0].sel | drv[1].sel)


# ------------------------------------------ 6. the library and bindings --
def test_library_exports_the_entries():
    from gsmpm import _lib  # binds every entry of _SIGS at import: a missing symbol raises there
    for name in ("gsmpm_mpm_add_driver", "gsmpm_mpm_get_driver_selection"):
        assert name in _lib._SIGS and getattr(_lib.LIB, name) is not None
    with open(os.path.join(ROOT, "include", "gsmpm.h")) as f:
        h = f.read()
    for name in ("gsmpm_mpm_add_driver", "gsmpm_mpm_get_driver_selection"):
        assert re.search(r"\bint %s\(" % name, h)
    m = re.search(r"typedef struct \{([^}]*)\} gsmpm_driver;", h)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip().split("[")[0] for decl in re.findall(r"(?:int32_t|double) ([^;]+);", body)
             for n in decl.split(",")]
    assert names == [n for n, _ in _lib.Driver._fields_]
    assert ctypes.sizeof(_lib.Driver) == 8 + 8 * (3 * 6 + 3)
    for kind, code in _lib.DRIVER.items():
        assert re.search(r"#define GSMPM_DRIVER_\w+ %d\b" % code, h), kind


# -------------------------------------------------- 7. the descriptors --
def test_descriptors():
    from mpm_solver import boundary_conditions as B
    args = types.SimpleNamespace(substep_dt=1e-4)
    box = dict(center=[1, 1, 1.4], size=[0.3, 0.3, 0.1])
    for name in B.driver_bc:
        assert B.boundaryConditionTypeCallBacks[name] is B.ParticleDriverBC
        assert name not in B.preprocess_bc and name not in B.postprocess_bc and name not in B.collider_bc
    assert B.preprocess_bc == "impulse" and len(B.driver_bc) == 3
    bc = B.ParticleDriverBC(10, dict(type="enforce_particle_rotation", id=4, point=[1, 1, 1], axis=[0, 0, 1],
                                     omega=2.0, **box), args)
    assert (bc.start_time, bc.end_time) == (0.0, 999.0) and bc.mask is None and bc.center == box["center"]
    assert bc.params == dict(point=[1, 1, 1], axis=[0, 0, 1], omega=2.0, along=0.0)
    assert bc.isActive(0.0) and bc.isActive(998.9) and not bc.isActive(999.0) and not bc.isCollide
    bc = B.ParticleDriverBC(10, dict(type="enforce_particle_translation", velocity=[1, 0, 0], end_time=None,
                                     num_dt=None, **box), args)
    assert (bc.start_time, bc.end_time) == (0.0, 999.0)  # None: the default, as the solver's methods pass it
    # num_dt: the reference's f64 window arithmetic
    bc = B.ParticleDriverBC(10, dict(type="particle_impulse", force=[1, 2, 3, 4], start_time=0.3, num_dt=7, **box),
                            args)
    assert bc.end_time == 0.3 + 1e-4 * 7 and bc.params == dict(force=[1, 2, 3], substep_dt=1e-4)
    assert bc.isActive(0.3) and not bc.isActive(bc.end_time) and not bc.isActive(0.29999)
    mask = np.arange(10) % 2 == 0
    bc = B.ParticleDriverBC(10, dict(type="enforce_particle_translation", velocity=[1, 0, 0], mask=mask,
                                     start_time=0.1, end_time=0.2), args)
    assert bc.mask is mask and bc.center is None and (bc.start_time, bc.end_time) == (0.1, 0.2)
    with pytest.raises(TypeError, match="center and size, or as mask"):
        B.ParticleDriverBC(10, dict(type="enforce_particle_translation", velocity=[1, 0, 0]), args)
    with pytest.raises(TypeError, match="center and size, or as mask"):
        B.ParticleDriverBC(10, dict(type="enforce_particle_translation", velocity=[1, 0, 0], mask=mask, **box), args)
    with pytest.raises(TypeError, match="end_time or num_dt"):
        B.ParticleDriverBC(10, dict(type="enforce_particle_translation", velocity=[1, 0, 0], end_time=1.0, num_dt=3,
                                    **box), args)
    with pytest.raises(KeyError, match="axis"):
        B.ParticleDriverBC(10, dict(type="enforce_particle_rotation", point=[1, 1, 1], **box), args)


def test_lego_wring_config():
    """The lego's base held by lego.json's fixed cube, the top fifth of its
    height turned about the vertical axis through the grid centre, with a
    small lift along it."""
    from mpm_solver import boundary_conditions as B
    with open(os.path.join(PKG, "configs", "lego-wring.json")) as f:
        cfg = json.load(f)["mpm"]
    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        lego = json.load(f)["mpm"]
    recs = cfg["boundary_conditions"]
    cubes = [r for r in recs if r["type"] == "fixed_cube"]
    assert cubes == [lego["boundary_conditions"][0]]
    (rot,) = [r for r in recs if r["type"] == "enforce_particle_rotation"]
    assert rot["axis"] == [0.0, 0.0, 1.0] and rot["point"][:2] == [1.0, 1.0] and rot["omega"] != 0
    assert 0 < abs(rot["along"]) < 0.1 * abs(rot["omega"])
    args = types.SimpleNamespace(substep_dt=cfg["substep_dt"])
    for r in recs:
        B.boundaryConditionTypeCallBacks[r["type"]](100, r, args)
    # the top fifth of the synthetic lego's height, and clear of the fixed cube
    prob = lego_problem(4000, 48, config="lego-wring.json")
    z = prob["x"][:, 2]
    sel = D.box_selection(prob["x"], rot["center"], rot["size"])
    top = z > z.max() - 0.2 * (z.max() - z.min())
    assert abs(int(sel.sum()) - int(top.sum())) <= 0.02 * top.sum() and not (sel & ~top).any()
    assert z[sel].min() > cubes[0]["center"][2] + cubes[0]["size"][2] + 0.1
