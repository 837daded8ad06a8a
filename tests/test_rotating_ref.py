"""The rotating colliders' reference (tests/rotating_ref.py) against its own
laws, the shared constants' counts on scene S, and the host side that needs no
GPU (the solver's descriptors, the lego-twist config, the C-ABI's
declarations).  CPU only.
"""
from __future__ import annotations

import functools
import json
import os
import re

import numpy as np
import pytest

import collider_ref as CR
import grid_ref as G
import moving_ref as M
import rotating_ref as R
from conftest import PKG, ROOT

SURF = (("sticky", 0.0), ("slip", 0.5), ("separate", 0.5))
SHAPES = ("plane", "ball", "box", "walls")


@functools.lru_cache(maxsize=None)
def _sums():
    S = G.scene()
    m, mv, _ = G.p2g_ref(S["x"], S["v"], S["C"], S["mass"], S["n_grid"], S["dx32"], S["inv_dx32"])
    return S, m, mv


def _args():
    S, m, mv = _sums()
    return mv, m, S["n_grid"], S["dx32"], S["dt_g32"]


def _scale():
    """||v|| + ||dt g|| per node, the unit of the grid-level bounds."""
    S, m, mv = _sums()
    live = m.reshape(-1) > 1e-15
    s = np.zeros(len(live))
    s[live] = np.sqrt(((mv.reshape(-1, 3)[live] / m.reshape(-1)[live, None]) ** 2).sum(1))
    return s + np.sqrt((S["dt_g32"].astype(np.float64) ** 2).sum()), live


# ------------------------------------- 1. lists without a rotating record --
def test_a_list_without_rotating_records_is_moving_ref():
    ops = [G.CUBE, R.PLANE, M.mov(CR.ext("ball", "slip", 0.5, 0.9, **CR.GEOMETRY["ball"])),
           CR.ext("box", "separate", 0.5, 0.9, **CR.GEOMETRY["box"]),
           M.mov(CR.ext("walls", "sticky", **CR.GEOMETRY["walls"]))]
    for active in ([1] * 5, [1, 1, 0, 1, 0], [0, 1, 1, 0, 1]):
        for t in M.T:
            a, amb_a = R.node_update_ref(*_args(), ops, active, t)
            b, amb_b = M.node_update_ref(*_args(), ops, active, t)
            assert np.array_equal(a, b) and np.array_equal(amb_a, amb_b)
            assert np.array_equal(R.node_update_f32(*_args(), ops, active, t),
                                  M.node_update_f32(*_args(), ops, active, t))


# ----------------------------------------------- 2. body against world --
@pytest.mark.parametrize("surface,mu", SURF)
@pytest.mark.parametrize("name", SHAPES)
def test_body_and_world_frame_agree(name, surface, mu):
    """Both float64 forms on the unrounded pose (an orthogonal R): 1e-12 of the node scale, on every node that is
    not ambiguous (at an ambiguous one the two may pick different faces)."""
    scale, live = _scale()
    op = R.rot(CR.ext(name, surface, mu, 0.9, **R.geo(name)))
    for t in R.T[name]:
        poses = {0: R.pose16(op, t)}
        body, amb = R.node_update_ref(*_args(), [op], [1], t, poses)
        world = R.node_update_world(*_args(), [op], [1], t, poses)
        err = (np.abs(body - world).max(1) / scale)[~amb].max()
        assert not (amb & live).any() and err <= 1e-12, (t, err)
        free, _ = R.node_update_ref(*_args(), [], [])
        assert (np.abs(body - free).max(1) > 1e-3 * scale)[live].sum() >= CR.MIN_ACTING  # the record acted


def test_the_stored_rotation_is_orthogonal_to_f32_only():
    """Why the check above takes the unrounded pose: R of pose32 misses orthogonality by a few 2^-24."""
    op = R.rot(CR.ext("box", **CR.GEOMETRY["box"]))
    R32 = R.pose32(op, R.T_IN)[:9].reshape(3, 3).astype(np.float64)
    R64 = R.pose64(op, R.T_IN)["R"]
    assert np.abs(R64 @ R64.T - np.eye(3)).max() < 1e-15
    assert 1e-9 < np.abs(R32 @ R32.T - np.eye(3)).max() < 4 * 2.0 ** -24
    assert np.abs(R32 - R64).max() <= 2.0 ** -24  # one rounding of entries below 1
    ang = np.degrees(np.arccos((np.trace(R64) - 1) / 2))
    assert abs(ang - 31.7) < 0.05


# ------------------------------------------------------------ 3. sticky --
@pytest.mark.parametrize("name", SHAPES)
def test_sticky_nodes_take_the_colliders_velocity(name):
    S = _sums()[0]
    op = R.rot(CR.ext(name, "sticky", **R.geo(name)))
    p = CR.node_positions32(S["n_grid"], S["dx32"])
    _, live = _scale()
    for t in R.T[name]:
        v, _ = R.node_update_ref(*_args(), [op], [1], t)
        hit = R.hit_nodes(S["n_grid"], S["dx32"], op, t) & live
        o = R.pose32(op, t)[12:15]
        wc = R.wc64(op, t, p, o)
        assert hit.sum() >= CR.MIN_ACTING and np.array_equal(v[hit], wc[hit])
        inside = M.WINDOW[0] <= t < M.WINDOW[1]
        assert (np.abs(wc[hit]).max() > 1.0) == inside  # it stands outside the window
        free, _ = R.node_update_ref(*_args(), [], [])
        assert np.array_equal(v[~hit], free[~hit])


# ---------------------------------------- 4. a ball centred on its pivot --
def test_a_ball_on_its_pivot_keeps_its_hit_set():
    """With the pivot at the centre and no translation c = a at every time:
    the hit set is that of t = 0, only the collider's velocity changes."""
    S = _sums()[0]
    geo = CR.GEOMETRY["ball"]
    op = R.rot(CR.ext("ball", "slip", 0.5, 0.9, **geo), pivot=geo["center"], velocity=(0.0, 0.0, 0.0))
    sets, outs = [], []
    for t in M.T:
        P = R.pose32(op, t)
        assert np.array_equal(P[9:12], np.asarray(geo["center"], np.float32)) and np.array_equal(P[9:12], P[12:15])
        sets.append(R.hit_nodes(S["n_grid"], S["dx32"], op, t))
        v, amb = R.node_update_ref(*_args(), [op], [1], t)
        assert not (amb & _scale()[1]).any()
        outs.append(v)
    assert all(np.array_equal(sets[0], s) for s in sets[1:]) and sets[0].sum() >= CR.MIN_ACTING
    static, _ = CR.node_update_ref(*_args(), [op[1]], [1])
    for t, v in zip(M.T, outs):  # outside the window it is the static ball, up to the rotation there and back
        if not M.WINDOW[0] <= t < M.WINDOW[1]:
            assert np.abs(v - static).max() < 1e-6
    # inside it the surface drags material, and a ball looks the same at every angle: one answer at both times
    assert np.abs(outs[2] - static).max() > 1e-2 and np.abs(outs[1] - outs[2]).max() < 1e-6


# ------------------------------------------------------------ 5. counts --
@pytest.mark.parametrize("name", SHAPES)
def test_counts_of_scene_S(name):
    """At each shape x time pair: no massive node ambiguous, the acting nodes as recorded and >= MIN_ACTING."""
    S, m, _ = _sums()
    assert len(S["x"]) == 4000 and S["n_grid"] == 32 and int((m > 1e-15).sum()) == 5883
    op = R.rot(CR.ext(name, "slip", 0.5, **R.geo(name)))
    got = []
    for t in R.T[name]:
        inside, acting, amb = R.acting_nodes(*_args(), op, t)
        _, amb_ref = R.node_update_ref(*_args(), [op], [1], t)
        assert amb == 0 and not (amb_ref & _scale()[1]).any(), (name, t, amb)
        assert acting >= CR.MIN_ACTING
        got.append(acting)
    assert tuple(got) == R.ACTING[name]
    if name != "plane":
        assert R.T[name] == M.T and (CR.acting_nodes(*_args(), op[1])[:2] ==
                                     R.acting_nodes(*_args(), op, 0.0)[:2] == CR.COUNTS[name])


def test_the_transcription_stays_close_to_the_reference():
    """node_update_f32 against node_update_ref on the same f32 pose: a few EPS of the node's scale (the rotation
    there and back costs some; the GPU tests take 4 x this figure as their bound)."""
    scale, _ = _scale()
    for name in SHAPES:
        op = R.rot(CR.ext(name, "slip", 0.5, 0.9, **R.geo(name)))
        ref, amb = R.node_update_ref(*_args(), [op], [1], R.T_IN)
        t32 = R.node_update_f32(*_args(), [op], [1], R.T_IN)
        e32 = (np.abs(t32 - ref).max(1) / scale)[~amb].max()
        assert e32 < 64 * G.EPS, (name, e32 / G.EPS)


# ------------------------------------------------- host side, no GPU --
def test_pose_of_the_window_edges():
    """Before the window the pose of t0 (R = I, c = a), from its end on the pose of t1."""
    op = R.rot(CR.ext("box", **CR.GEOMETRY["box"]))
    P0 = R.pose32(op, 0.0)
    assert np.array_equal(P0[:9].reshape(3, 3), np.eye(3, dtype=np.float32))
    assert np.array_equal(P0[12:15], np.asarray(R.PIVOT, np.float32))
    assert np.abs(P0[9:12] - np.asarray(CR.GEOMETRY["box"]["center"], np.float32)).max() <= 2.0 ** -23
    assert np.array_equal(R.pose32(op, 0.1), R.pose32(op, M.WINDOW[1])) and np.array_equal(
        R.pose32(op, 5.0), R.pose32(op, 0.1))
    assert not np.array_equal(R.pose32(op, 0.05), R.pose32(op, 0.06))


def test_collider_descriptor_takes_the_spin():
    from mpm_solver.boundary_conditions import ColliderBC
    geo = CR.GEOMETRY["box"]
    bc = ColliderBC(10, dict(type="collider", shape="box", start_time=0.25, end_time=0.5,
                             angular_velocity=[0.0, 0.0, 2.0], **geo))
    assert bc.motion == dict(angular_velocity=[0.0, 0.0, 2.0], move_start=0.25, move_end=0.5)
    bc = ColliderBC(10, dict(type="collider", shape="box", angular_velocity=[0, 1, 0], pivot=[1, 1, 1],
                             velocity=[0, 0, -1], move_start=0.1, move_end=0.2, **geo))
    assert bc.motion == dict(angular_velocity=[0.0, 1.0, 0.0], pivot=[1.0, 1.0, 1.0], velocity=[0.0, 0.0, -1.0],
                             move_start=0.1, move_end=0.2)
    # all zeros: today's records
    assert ColliderBC(10, dict(type="collider", shape="box", angular_velocity=[0, 0, 0], **geo)).motion == {}
    bc = ColliderBC(10, dict(type="collider", shape="box", angular_velocity=[0, 0, 0], velocity=[1, 0, 0], **geo))
    assert bc.motion == dict(velocity=[1.0, 0.0, 0.0], move_start=0.0, move_end=999.0)
    with pytest.raises(TypeError, match="pivot"):
        ColliderBC(10, dict(type="collider", shape="box", pivot=[1, 1, 1], **geo))


def test_lego_twist_config():
    """Two sticky boxes round the two ends of the model's long axis, counter-rotating about it for a window."""
    with open(os.path.join(PKG, "configs", "lego-twist.json")) as f:
        full = json.load(f)
    with open(os.path.join(PKG, "configs", "lego-press.json")) as f:
        press = json.load(f)["mpm"]
    cfg = full["mpm"]
    recs = [b for b in cfg["boundary_conditions"] if b["type"] == "collider" and "angular_velocity" in b]
    assert len(recs) == 2 and all(b["shape"] == "box" and b["surface"] == "sticky" for b in recs)
    a, b = recs
    assert np.array_equal(np.asarray(a["angular_velocity"]), -np.asarray(b["angular_velocity"]))
    axis = np.nonzero(a["angular_velocity"])[0]
    assert len(axis) == 1  # about one coordinate axis, the long one
    ax = int(axis[0])
    others = [d for d in range(3) if d != ax]
    assert a["center"][ax] != b["center"][ax] and all(a["center"][d] == b["center"][d] for d in others)
    assert all(r["pivot"][d] == r["center"][d] for r in recs for d in others)  # the axis runs through both
    assert all(r["move_start"] == a["move_start"] and r["move_end"] == a["move_end"] == r["end_time"] for r in recs)
    assert a["move_end"] < cfg["frame_dt"] * full["render"]["num_frames"]  # released before the end
    for k in ("material", "n_grid", "grid_extent", "sim_area", "substep_dt", "frame_dt", "E", "nu", "density", "gravity"):
        assert cfg[k] == press[k], k


def test_header_and_bindings_declare_the_entries():
    from gsmpm import _lib
    with open(os.path.join(ROOT, "include", "gsmpm.h")) as f:
        h = f.read()
    for name in ("gsmpm_mpm_add_rotating_collider", "gsmpm_mpm_get_poses"):
        assert re.search(r"\bint %s\(" % name, h) and name in _lib._SIGS
    m = re.search(r"typedef struct \{([^}]*)\} gsmpm_collider_spin;", h)
    fields = re.findall(r"double (\w+)(?:\[3\])?(?:, (\w+))?;", m.group(1))
    assert [n for pair in fields for n in pair if n] == [n for n, _ in _lib.ColliderSpin._fields_]
    import ctypes
    assert ctypes.sizeof(_lib.ColliderSpin) == 11 * 8
