"""The moving colliders' reference (tests/moving_ref.py) against its own laws,
the shared constants' counts on scene S, the host side that needs no GPU
(bc.substep_times, the lego-press config, the solver's descriptors) and the
C-ABI's declarations and exports.  CPU only.
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
import moving_ref as M
from conftest import PKG, ROOT

SURF = (("sticky", 0.0), ("slip", 0.5), ("separate", 0.5))
PLANE = G.OP_LISTS["b"][0][0]  # the oblique plane of list b
SHAPES = ("plane", "ball", "box", "walls")


def _geo(name):
    return dict(point=PLANE[1], normal=PLANE[2]) if name == "plane" else CR.GEOMETRY[name]


@functools.lru_cache(maxsize=None)
def _sums():
    S = G.scene()
    m, mv, _ = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    return S, m, mv


def _args():
    S, m, mv = _sums()
    return mv, m, S["n_grid"], S["dx32"], S["dt_g32"]


def _normals(op, t):
    """[(hit & massive, n [nn, 3])] of a moving op on scene S at time t."""
    S, m, _ = _sums()
    live = m > 1e-15
    hits, _ = CR._inside_and_normals(CR.node_positions32(S["n_grid"], S["dx32"]), M.static_at(op, t))
    return [(h & live, n if n.ndim == 2 else np.broadcast_to(n, (len(h), 3))) for h, n in hits]


# ------------------------------------------------------------- counts --
@pytest.mark.parametrize("name", SHAPES)
def test_counts_of_scene_S(name):
    """At each of the twelve shape x time pairs (and the plane's four): no
    massive node ambiguous, the acting nodes as recorded and >= MIN_ACTING."""
    S, m, mv = _sums()
    assert len(S["x"]) == 4000 and S["n_grid"] == 32 and int((m > 1e-15).sum()) == 5883
    op = M.mov(CR.ext(name, "slip", 0.5, **_geo(name)))
    for i, t in enumerate(M.T):
        _, acting = M.acting_nodes(*_args(), op, t)
        _, amb = M.node_update_ref(*_args(), [op], [1], t)
        assert not (amb & (m > 1e-15)).any(), (name, t)
        assert acting >= CR.MIN_ACTING, (name, t, acting)
        if name != "plane":
            assert acting == M.ACTING[name][i], (name, t, acting)
    assert M.ACTING[name][0] == CR.COUNTS[name][1] if name != "plane" else True


def test_placement_follows_the_three_phases():
    op = M.mov(CR.ext("ball", **CR.GEOMETRY["ball"]))
    a, w = np.asarray(CR.CENTRE, np.float32), np.asarray(M.W, np.float32)
    t0, t1 = np.float32(M.WINDOW[0]), np.float32(M.WINDOW[1])
    c, wc, tau = M.placement32(op, 0.0)
    assert np.array_equal(c, a) and np.all(wc == 0) and tau == 0
    c, wc, tau = M.placement32(op, 0.0507)
    assert tau == np.float32(np.float32(0.0507) - t0) and np.array_equal(wc, w)
    assert np.array_equal(c, (a + (w * tau).astype(np.float32)).astype(np.float32))
    end = (a + (w * np.float32(t1 - t0)).astype(np.float32)).astype(np.float32)
    for t in (M.WINDOW[1], 0.1, 5.0):
        c, wc, _ = M.placement32(op, t)
        assert np.array_equal(c, end) and np.all(wc == 0)
    c, wc, _ = M.placement32(op, float(np.nextafter(t1, np.float32(0))))
    assert np.array_equal(wc, w)  # the window is half open: the last f32 below t1 still moves
    inf = M.mov(CR.ext("ball", **CR.GEOMETRY["ball"]), M.W, 0.0, float("inf"))
    c, wc, tau = M.placement32(inf, 7.0)
    assert tau == np.float32(7.0) and np.array_equal(wc, w)


# ----------------------------------------------------- the reference's laws --
@pytest.mark.parametrize("name", SHAPES)
def test_laws_on_hit_nodes(name):
    """sticky: v == wc exactly; slip: (v - wc) . n = 0 before damping;
    separate: (v - wc) . n >= 0; untouched nodes keep v bit for bit."""
    t = M.T[2]
    free = M.node_update_ref(*_args(), [], [])[0]
    for surface, mu in SURF:
        op = M.mov(CR.ext(name, surface, mu, 1.0, **_geo(name)))
        wc = M.placement32(op, t)[1].astype(np.float64)
        assert np.array_equal(wc, G.f32(M.W))
        v, _ = M.node_update_ref(*_args(), [op], [1], t)
        hits = _normals(op, t)
        any_hit = np.zeros(len(v), bool)
        for h, n in hits:
            any_hit |= h
        assert any_hit.sum() >= CR.MIN_ACTING
        assert np.array_equal(v[~any_hit], free[~any_hit])
        if surface == "sticky":
            assert np.all(v[any_hit] == wc[None, :])
            continue
        # the axis normals and the ball's are unit to float64 rounding; the plane's is the f32 of a unit
        # vector, so |n|^2 - 1 is up to 2 * 2^-24 and that share of (v - wc) . n is left over
        tol = (2.0 ** -23 if name == "plane" else 1e-12) * max(1.0, np.abs(free).max() + np.abs(wc).max())
        for h, n in hits:
            rel = ((v[h] - wc[None, :]) * n[h]).sum(1)
            if surface == "slip":
                assert np.abs(rel).max() <= tol
            else:
                assert rel.min() >= -tol


@pytest.mark.parametrize("name", SHAPES)
def test_galilean_identity(name):
    """ref(v, moving w) == ref_static(v - w) + w on the nodes the record
    hits, v elsewhere: to 1e-12, damping 1, inside the window."""
    S, m, mv = _sums()
    t = M.T[2]
    live = m > 1e-15
    free = M.node_update_ref(*_args(), [], [])[0]
    w = G.f32(M.W)
    for surface, mu in SURF:
        op = M.mov(CR.ext(name, surface, mu, 1.0, **_geo(name)))
        got, _ = M.node_update_ref(*_args(), [op], [1], t)
        # the static record at the same placement, fed v - w: (mv - m w) / m + dt g = v - w
        mv_rel = mv - m[:, None] * w[None, :]
        stat, _ = CR.node_update_ref(mv_rel, m, S["n_grid"], S["dx32"], S["dt_g32"], [M.static_at(op, t)], [1])
        hit = M.hit_nodes(S["n_grid"], S["dx32"], op, t) & live
        want = free.copy()
        want[hit] = stat[hit] + w[None, :]
        scale = max(1.0, np.abs(free).max())
        assert np.abs(got - want).max() <= 1e-12 * scale, (name, surface)


@pytest.mark.parametrize("name", SHAPES)
def test_standing_phases_are_the_static_record(name):
    """w = 0, t < t0 and t >= t1 reproduce collider_ref.node_update_ref at
    the corresponding static centre exactly, in both forms."""
    S, m, mv = _sums()
    a = _args()
    for surface, mu in SURF:
        e = CR.ext(name, surface, mu, 0.9, **_geo(name))
        cases = [(M.mov(e, (0.0, 0.0, 0.0)), M.T[2]), (M.mov(e), 0.0), (M.mov(e), 0.0100), (M.mov(e), M.WINDOW[1]),
                 (M.mov(e), 0.1)]
        for op, t in cases:
            static = M.static_at(op, t)
            if t < M.WINDOW[0] or op[2] == (0.0, 0.0, 0.0):
                assert static == e[:3] + (tuple(float(x) for x in np.asarray(e[3], np.float32)),) + e[4:]
            got, amb = M.node_update_ref(*a, [op], [1], t)
            want, amb_w = CR.node_update_ref(*a, [static], [1])
            assert np.array_equal(got, want) and np.array_equal(amb, amb_w), (name, surface, t)
            assert np.array_equal(M.node_update_f32(*a, [op], [1], t), CR.node_update_f32(*a, [static], [1]))


def test_static_lists_are_collider_refs():
    a = _args()
    for name in CR.GEOMETRY:
        ops = [G.CUBE, PLANE, CR.ext(name, "separate", 0.5, 0.9, **CR.GEOMETRY[name])]
        for act in ([1, 1, 1], [0, 1, 0]):
            r1, r2 = CR.node_update_ref(*a, ops, act), M.node_update_ref(*a, ops, act, 0.3)
            assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
            assert np.array_equal(CR.node_update_f32(*a, ops, act), M.node_update_f32(*a, ops, act, 0.3))


def test_inactive_record_is_skipped_and_its_clock_runs():
    a = _args()
    op = M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"]))
    free = M.node_update_ref(*a, [], [])[0]
    assert np.array_equal(M.node_update_ref(*a, [op], [0], M.T[2])[0], free)
    # switched on late, it is where its own clock put it, not at the start
    late = M.node_update_ref(*a, [op], [1], M.T[2])[0]
    start = CR.node_update_ref(*a, [op[1]], [1])[0]
    assert (np.abs(late - start).max(1) > 1e-3).sum() >= 100


def test_f32_transcription_is_close_to_float64():
    """The response runs on u = v - wc, so its roundings scale with
    ||v_in / m|| + ||dt g|| + ||wc||: collider_ref's 4 EPS for the chain, plus
    1 EPS for the two roundings the moving form adds (v - wc and u + wc, half
    an EPS each)."""
    S, m, mv = _sums()
    m32, mv32 = m.astype(np.float32), mv.astype(np.float32)
    live = m32 > np.float32(1e-15)
    scale = np.zeros(len(m))
    scale[live] = np.sqrt(((mv32[live].astype(np.float64) / m32[live, None]) ** 2).sum(1))
    scale += np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum()) + np.sqrt((G.f32(M.W) ** 2).sum())
    a = (mv32, m32, S["n_grid"], S["dx32"], S["dt_g32"])
    for name in SHAPES:
        for surface, mu in SURF:
            op = M.mov(CR.ext(name, surface, mu, 0.9, **_geo(name)))
            ref, amb = M.node_update_ref(*a, [op], [1], M.T[2])
            v32 = M.node_update_f32(*a, [op], [1], M.T[2])
            e = (np.abs(v32 - ref).max(1) / scale)[~amb].max()
            print(f"MOVING transcription {name} {surface}: {e / G.EPS:.2f} EPS")
            assert e <= 5 * G.EPS, (name, surface, e / G.EPS)
            assert np.all(v32[~live] == 0)


# ------------------------------------------------------------ host side --
def test_substep_times_is_the_clock_of_substep_masks():
    from gsmpm.bc import substep_masks, substep_times, windowed_collider
    dt = 1e-4
    times, t_end = substep_times(0.0, dt, 8100)
    spec = windowed_collider(3, 0.8, 0.8 + dt * 10)
    masks, t_end_m = substep_masks([spec], 0.0, dt, 8100)
    assert t_end == t_end_m and len(times) == 8100
    t = 0.0
    for s in range(8100):
        assert times[s] == t  # value for value
        t += dt
    assert [s for s, mk in enumerate(masks) if mk >> 3 & 1] == [s for s, tt in enumerate(times) if spec.is_active(tt)]
    # a motion window opening at 0.8 with dt 1e-4 opens on substep 8001 of this clock (8000 additions stay below 0.8)
    assert min(s for s, tt in enumerate(times) if tt >= 0.8) == 8001
    # a call that starts later continues the same clock
    more, _ = substep_times(times[100], dt, 50)
    assert more == times[100:150]


def test_lego_press_config_parses_into_the_expected_records():
    from mpm_solver.boundary_conditions import ColliderBC, boundaryConditionTypeCallBacks, collider_bc
    load = lambda n: json.load(open(os.path.join(PKG, "configs", n)))
    press, lego, ballcfg = load("lego-press.json"), load("lego.json"), load("lego-ball.json")
    bcs, base = press["mpm"]["boundary_conditions"], lego["mpm"]["boundary_conditions"]
    assert bcs[:len(base)] == base and len(bcs) == len(base) + 3
    assert {k: v for k, v in press["mpm"].items() if k != "boundary_conditions"} == \
           {k: v for k, v in lego["mpm"].items() if k != "boundary_conditions"}
    assert bcs[len(base)] == ballcfg["mpm"]["boundary_conditions"][len(base)]  # lego-ball's slip walls
    recs = [boundaryConditionTypeCallBacks[b["type"]](10, b, None) for b in bcs[len(base):]]
    assert all(isinstance(r, ColliderBC) and r.type in collider_bc and not r.isCollide for r in recs)
    walls, ball, box = recs
    assert (walls.shape, walls.surface) == ("walls", "slip") and walls.velocity is None and walls.motion == {}
    clip = press["render"]["num_frames"] * press["mpm"]["frame_dt"]
    assert (ball.shape, ball.surface) == ("ball", "separate") and ball.friction > 0
    assert any(ball.motion["velocity"]) and 0.0 <= ball.move_start < ball.move_end < clip  # it flies, then stops
    assert (box.shape, box.surface, box.friction) == ("box", "sticky", 0.0)
    assert box.motion["velocity"][2] < 0 and box.move_end < clip  # it descends, then holds
    lo = [c - h for c, h in zip(walls.geometry["center"], walls.geometry["half"])]
    hi = [c + h for c, h in zip(walls.geometry["center"], walls.geometry["half"])]
    for r, reach in ((ball, [ball.geometry["radius"]] * 3), (box, box.geometry["half"])):
        for c0 in (r.geometry["center"],
                   [c + w * (r.move_end - r.move_start) for c, w in zip(r.geometry["center"], r.motion["velocity"])]):
            assert all(l <= c - h and c + h <= u for l, u, c, h in zip(lo, hi, c0, reach))  # inside the walls
    # the motion window defaults to the activity window
    d = ColliderBC(10, dict(type="collider", shape="ball", center=[1, 1, 1], radius=0.1, velocity=[1, 0, 0],
                            start_time=0.25, end_time=0.5))
    assert d.motion == dict(velocity=[1.0, 0.0, 0.0], move_start=0.25, move_end=0.5)
    with pytest.raises(TypeError):
        ColliderBC(10, dict(type="collider", shape="ball", center=[1, 1, 1], radius=0.1, move_start=0.1))


def test_header_declares_and_library_exports_the_moving_api():
    with open(os.path.join(ROOT, "include", "gsmpm.h")) as f:
        h = f.read()
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*gsmpm_collider_motion\s*;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "double velocity[3]; double t_start, t_end;"
    assert re.search(r"int\s+gsmpm_mpm_add_moving_collider\s*\(\s*gsmpm_mpm\s*\*\s*\w+\s*,\s*const\s+gsmpm_collider\s*\*"
                     r"\s*\w+\s*,\s*const\s+gsmpm_collider_motion\s*\*", h)
    assert re.search(r"int\s+gsmpm_mpm_step_timed\s*\(\s*gsmpm_mpm\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*void\s*\*", h)
    assert re.search(r"int\s+gsmpm_mpm_graph_count\s*\(\s*gsmpm_mpm\s*\*", h)
    # additive: the static record and the untimed step keep their declarations
    assert re.search(r"int\s+gsmpm_mpm_step\s*\(gsmpm_mpm\*\s*h,\s*float dt,\s*int32_t n_substeps,\s*"
                     r"const uint32_t\*\s*bc_active,\s*void\*\s*stream\);", h)
    lib = ctypes.CDLL(os.path.join(PKG, "libgsmpm.so"))
    for name in ("gsmpm_mpm_add_moving_collider", "gsmpm_mpm_step_timed", "gsmpm_mpm_graph_count"):
        assert hasattr(lib, name), name
    from gsmpm import _lib
    assert ctypes.sizeof(_lib.ColliderMotion) == 5 * 8
    assert _lib.LIB.gsmpm_mpm_add_moving_collider(None, None, None) == _lib.GSMPM_EINVAL
    assert "gsmpm_mpm_add_moving_collider" in _lib.last_error()
    assert _lib.LIB.gsmpm_mpm_step_timed(None, ctypes.c_float(1e-4), 1, None, None, None) == _lib.GSMPM_EINVAL
    assert "gsmpm_mpm_step_timed" in _lib.last_error()
