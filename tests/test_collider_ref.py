"""The extended colliders' reference (tests/collider_ref.py) against its own
laws, the geometry lists' counts on scene S, the host side that needs no GPU
(bc.py's windowed kind, the lego-ball config, the solver's descriptors), and
the C-ABI's declaration and export.  CPU only.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

import collider_ref as CR
import grid_ref as G
from conftest import PKG, ROOT

SURF = (("sticky", 0.0), ("slip", 0.5), ("separate", 0.5))


@functools.lru_cache(maxsize=None)
def _sums():
    S = G.scene()
    m, mv, _ = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    return S, m, mv


def _update(ops, active):
    S, m, mv = _sums()
    return CR.node_update_ref(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops, active)


def _free():
    return _update([], [])[0]


def _normals(op):
    """[(hit & massive, n [nn, 3])] of an ext op on scene S."""
    S, m, _ = _sums()
    live = m > 1e-15
    hits, _ = CR._inside_and_normals(CR.node_positions32(S["n_grid"], S["dx32"]), op)
    return [(h & live, n if n.ndim == 2 else np.broadcast_to(n, (len(h), 3))) for h, n in hits]


# ------------------------------------------------------------- counts --
@pytest.mark.parametrize("name", list(CR.GEOMETRY))
def test_counts_of_scene_S(name):
    S, m, mv = _sums()
    op = CR.ext(name, "slip", 0.5, **CR.GEOMETRY[name])
    inside, acting, multi = CR.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], op)
    _, amb = _update([op], [1])
    assert (inside, acting) == CR.COUNTS[name]
    assert acting >= CR.MIN_ACTING
    assert not (amb & (m > 1e-15)).any()
    if name == "walls":
        assert multi == CR.WALLS_MULTI
    if name == "ball":
        p = CR.node_positions32(S["n_grid"], S["dx32"])
        L = np.sqrt(((p - G.f32(CR.GEOMETRY["ball"]["center"])) ** 2).sum(1))
        assert 0.03 < L[m > 1e-15].min() < 0.031
    if name == "box":  # no tie between two penetration depths
        p = CR.node_positions32(S["n_grid"], S["dx32"])
        q = np.sort(G.f32(CR.GEOMETRY["box"]["half"]) - np.abs(p - G.f32(CR.GEOMETRY["box"]["center"])), 1)
        ins = (q[:, 0] > 0) & (m > 1e-15)
        assert (q[ins, 1] - q[ins, 0]).min() > G.AMBIG


# --------------------------------------------------------------- laws --
@pytest.mark.parametrize("name", list(CR.GEOMETRY))
def test_sticky_zeroes_and_leaves_the_rest(name):
    op = CR.ext(name, "sticky", **CR.GEOMETRY[name])
    v, v0 = _update([op], [1])[0], _free()
    hit = np.logical_or.reduce([h for h, _ in _normals(op)])
    assert hit.sum() == CR.COUNTS[name][0]
    assert np.all(v[hit] == 0) and np.array_equal(v[~hit], v0[~hit])


@pytest.mark.parametrize("name", list(CR.GEOMETRY))
def test_slip_removes_and_separate_bounds_the_normal_component(name):
    v0 = _free()
    scale = np.sqrt((v0 * v0).sum(1)).max()
    for surface in ("slip", "separate"):
        op = CR.ext(name, surface, 0.0, **CR.GEOMETRY[name])
        v = _update([op], [1])[0]
        for hit, n in _normals(op):
            vn = (v[hit] * n[hit]).sum(1)
            if surface == "slip":
                assert np.abs(vn).max() <= 1e-13 * scale
            else:
                assert vn.min() >= -1e-13 * scale
                # a node moving out of the collider keeps its velocity (one normal: ball, box)
                if name != "walls":
                    away = hit & ((v0 * n).sum(1) >= 0)
                    assert away.sum() > 100 and np.array_equal(v[away], v0[away])


@pytest.mark.parametrize("name", ["ball", "box"])
@pytest.mark.parametrize("surface", ["slip", "separate"])
def test_friction_shortens_the_tangential_speed(name, surface):
    v0 = _free()
    (hit, n), = _normals(CR.ext(name, surface, 0.0, **CR.GEOMETRY[name]))
    nc = (v0 * n).sum(1)
    tang = v0 - nc[:, None] * n
    t0 = np.sqrt((tang * tang).sum(1))
    clamped = 0
    for mu in (0.5, 3.0):
        v = _update([CR.ext(name, surface, mu, **CR.GEOMETRY[name])], [1])[0]
        act = hit & (nc < 0)
        assert act.sum() == CR.COUNTS[name][1]
        t1 = np.sqrt((v[act] * v[act]).sum(1))  # no normal component is left on an acting node
        want = np.maximum(0.0, t0[act] - float(np.float32(mu)) * np.abs(nc[act]))
        assert np.abs(t1 - want).max() <= 1e-12 * t0.max()
        clamped += int((want == 0).sum())
        # direction kept
        keep = want > 0
        cosang = (v[act][keep] * tang[act][keep]).sum(1) / (t1[keep] * t0[act][keep])
        assert cosang.min() > 1 - 1e-12
    assert clamped > 100  # friction 3 stops nodes


def test_walls_corner_nodes_lose_every_outward_component():
    S, m, _ = _sums()
    for surface in ("slip", "separate"):
        op = CR.ext("walls", surface, 0.5, 0.9, **CR.GEOMETRY["walls"])
        v = _update([op], [1])[0]
        hits = _normals(op)
        count = np.sum([h for h, _ in hits], 0)
        assert (count >= 2).sum() == CR.WALLS_MULTI and (count == 3).sum() > 0
        scale = np.abs(_free()).max()
        for hit, n in hits:
            corner = hit & (count >= 2)
            vn = (v[corner] * n[corner]).sum(1)  # n points into the box: outward is vn < 0
            assert vn.min() >= -1e-13 * scale
            if surface == "slip":
                assert np.abs(vn).max() <= 1e-13 * scale


def test_damping_once_per_record():
    v0 = _free()
    for name in CR.GEOMETRY:
        a = _update([CR.ext(name, "slip", 0.5, 1.0, **CR.GEOMETRY[name])], [1])[0]
        b = _update([CR.ext(name, "slip", 0.5, 0.9, **CR.GEOMETRY[name])], [1])[0]
        hit = np.logical_or.reduce([h for h, _ in _normals(CR.ext(name, "slip", **CR.GEOMETRY[name]))])
        assert np.abs(b[hit] - a[hit] * float(np.float32(0.9))).max() <= 1e-15 * np.abs(v0).max()
        assert np.array_equal(b[~hit], v0[~hit])


def test_inactive_record_is_the_identity():
    v0 = _free()
    for name in CR.GEOMETRY:
        for surface, mu in SURF:
            op = CR.ext(name, surface, mu, 0.9, **CR.GEOMETRY[name])
            assert np.array_equal(_update([op], [0])[0], v0)
            assert not np.array_equal(_update([op], [1])[0], v0)
    # between two other operators, in both forms
    S, m, mv = _sums()
    ops = [G.CUBE, CR.ext("ball", "slip", 0.5, **CR.GEOMETRY["ball"]), G.OP_LISTS["b"][0][0]]
    assert np.array_equal(_update(ops, [1, 0, 1])[0], _update([ops[0], ops[2]], [1, 1])[0])
    a32 = CR.node_update_f32(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops, [1, 0, 1])
    b32 = CR.node_update_f32(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], [ops[0], ops[2]], [1, 1])
    assert np.array_equal(a32, b32)


@pytest.mark.parametrize("name", list("abc"))
def test_plane_separate_099_is_the_legacy_collider(name):
    """Exactly, in both forms; and the f32 transcription of the legacy list
    equals the oracle-checked expression order (same results as the ext form)."""
    S, m, mv = _sums()
    ops, act = G.OP_LISTS[name]
    eops = [CR.ext("plane", "separate", o[3], float(np.float32(0.99)), point=o[1], normal=o[2]) for o in ops]
    legacy, amb = G.node_update_ref(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops, act)
    mine, amb2 = _update(eops, act)
    assert not amb.any() and not amb2.any()
    assert np.array_equal(legacy, mine)
    assert G.acting_nodes(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops) >= CR.MIN_ACTING
    a32 = CR.node_update_f32(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], ops, act)
    b32 = CR.node_update_f32(mv, m, S["n_grid"], S["dx32"], S["dt_g32"], eops, act)
    assert np.array_equal(a32, b32)


def test_f32_transcription_is_close_to_float64():
    """On every list of the GPU test: a few EPS of ||v_in / m|| + ||dt g||."""
    S, m, mv = _sums()
    m32, mv32 = m.astype(np.float32), mv.astype(np.float32)
    live = m32 > np.float32(1e-15)
    scale = np.zeros(len(m))
    scale[live] = np.sqrt(((mv32[live].astype(np.float64) / m32[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum())
    for name in CR.GEOMETRY:
        for surface, mu in SURF:
            op = CR.ext(name, surface, mu, 0.9, **CR.GEOMETRY[name])
            ref, amb = CR.node_update_ref(mv32, m32, S["n_grid"], S["dx32"], S["dt_g32"], [op], [1])
            v32 = CR.node_update_f32(mv32, m32, S["n_grid"], S["dx32"], S["dt_g32"], [op], [1])
            e = (np.abs(v32 - ref).max(1) / scale)[~amb].max()
            assert e <= 4 * G.EPS, (name, surface, e / G.EPS)
            assert np.all(v32[~live] == 0)


# ------------------------------------------------------------ host side --
def test_windowed_kind_follows_the_float64_clock():
    from gsmpm.bc import BCSpec, substep_masks, windowed_collider
    dt = 1e-4
    # as lego's impulse: 8000 additions of 1e-4 stay below 0.8, so the window
    # [0.8, 0.801) opens one substep late -- on substep 8001, not 8000 -- and stays open 10
    late = windowed_collider(3, 0.8, 0.8 + dt * 10)
    exact = windowed_collider(5, 0.25, 0.5)
    legacy = BCSpec("collider", 7)
    dflt = windowed_collider(9)
    assert (dflt.start_time, dflt.end_time) == (0.0, 999.0)
    masks, t_end = substep_masks([late, exact, legacy, dflt], 0.0, dt, 8100)
    t, clock = 0.0, []
    for _ in range(8100):
        clock.append(t)
        t += dt
    assert t_end == t
    on = [s for s, mk in enumerate(masks) if mk >> 3 & 1]
    assert on == list(range(8001, 8011))
    assert on == [s for s, tt in enumerate(clock) if 0.8 <= tt < 0.8 + dt * 10]
    assert [s for s, mk in enumerate(masks) if mk >> 5 & 1] == [s for s, tt in enumerate(clock) if 0.25 <= tt < 0.5]
    assert all(mk >> 9 & 1 for mk in masks)
    assert not any(mk >> 7 & 1 for mk in masks)  # the legacy plane ignores its bit: none is set for it
    assert legacy.is_active(1e9) and not late.is_active(0.7)


def test_lego_ball_config_parses_into_the_expected_records():
    from mpm_solver.boundary_conditions import ColliderBC, boundaryConditionTypeCallBacks, collider_bc
    with open(os.path.join(PKG, "configs", "lego-ball.json")) as f:
        ball = json.load(f)
    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        lego = json.load(f)
    bcs, base = ball["mpm"]["boundary_conditions"], lego["mpm"]["boundary_conditions"]
    assert bcs[:len(base)] == base and len(bcs) == len(base) + 2
    assert {k: v for k, v in ball["mpm"].items() if k != "boundary_conditions"} == \
           {k: v for k, v in lego["mpm"].items() if k != "boundary_conditions"}
    recs = [boundaryConditionTypeCallBacks[b["type"]](10, b, None) for b in bcs[len(base):]]
    assert all(isinstance(r, ColliderBC) and r.type in collider_bc and not r.isCollide for r in recs)
    walls, ballc = recs
    ext = ball["mpm"]["grid_extent"]
    dx = ext / ball["mpm"]["n_grid"]
    assert (walls.shape, walls.surface, walls.friction, walls.damping) == ("walls", "slip", 0.0, 1.0)
    assert (walls.start_time, walls.end_time) == (0.0, 999.0)
    lo = [c - h for c, h in zip(walls.geometry["center"], walls.geometry["half"])]
    hi = [c + h for c, h in zip(walls.geometry["center"], walls.geometry["half"])]
    assert all(2 * dx <= a <= 4 * dx for a in lo) and all(2 * dx <= ext - b <= 4 * dx for b in hi)  # just inside the grid
    assert (ballc.shape, ballc.surface, ballc.friction, ballc.damping) == ("ball", "separate", 0.3, 0.99)
    assert set(ballc.geometry) == {"center", "radius"} and ballc.geometry["radius"] > 0
    assert ballc.geometry["center"][2] + ballc.geometry["radius"] < 1.0  # under the model's centre
    assert ballc.isActive(0.0) and ballc.isActive(998.0) and not ballc.isActive(999.0)
    with pytest.raises(KeyError):
        ColliderBC(10, {"type": "collider", "shape": "ball", "center": [1, 1, 1]})
    with pytest.raises(ValueError):
        ColliderBC(10, {"type": "collider", "shape": "torus"})


def test_header_declares_and_library_exports_add_collider():
    with open(os.path.join(ROOT, "include", "gsmpm.h")) as f:
        h = f.read()
    assert re.search(r"int\s+gsmpm_mpm_add_collider\s*\(\s*gsmpm_mpm\s*\*\s*\w+\s*,\s*const\s+gsmpm_collider\s*\*", h)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*gsmpm_collider\s*;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == \
        "int32_t shape, surface; double a[3], b[3]; double friction; double damping;"
    vals = {k: int(v) for k, v in re.findall(r"#define\s+GSMPM_(SHAPE_\w+|SURF_\w+)\s+(\d+)", h)}
    assert set(vals) == {"SHAPE_PLANE", "SHAPE_BALL", "SHAPE_BOX", "SHAPE_WALLS", "SURF_STICKY", "SURF_SLIP",
                         "SURF_SEPARATE"}
    lib = ctypes.CDLL(os.path.join(PKG, "libgsmpm.so"))
    assert hasattr(lib, "gsmpm_mpm_add_collider")
    from gsmpm import _lib
    assert {f"SHAPE_{k.upper()}": v for k, v in _lib.SHAPE.items()} == {k: v for k, v in vals.items() if "SHAPE" in k}
    assert {f"SURF_{k.upper()}": v for k, v in _lib.SURFACE.items()} == {k: v for k, v in vals.items() if "SURF" in k}
    assert ctypes.sizeof(_lib.Collider) == 8 + 8 * 8
    # NULL arguments are refused before anything is touched
    _lib.LIB.gsmpm_mpm_add_collider.argtypes = [ctypes.c_void_p, ctypes.POINTER(_lib.Collider)]
    assert _lib.LIB.gsmpm_mpm_add_collider(None, None) == _lib.GSMPM_EINVAL
    assert "gsmpm_mpm_add_collider" in _lib.last_error()
