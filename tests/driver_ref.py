"""A substep with particle drivers, built from the oracle's own phase
functions (test infrastructure only; oracle/ is unchanged).

particle_preprocess (solver.py:41-42) with the drivers after the impulses:
grid reset, om_impulses, the drivers in the order they were added, the stress
(per material id when ids are given, mixed_oracle.mixed_stress), P2G, then the
oracle's substep_end -- the composition of mixed_oracle.mixed_substep with one
phase more.  The three kinds are plain f32 numpy on ``ref.v``, one operation
per rounding, in the order the library documents (include/gsmpm.h).  With no
driver the substep is ``OracleMPM.substep`` bit for bit
(tests/test_driver_ref.py).
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from mixed_oracle import mixed_stress, region_mask

KINDS = ("particle_impulse", "enforce_particle_translation", "enforce_particle_rotation")
f32 = np.float32


class Driver:
    """One record: ``sel`` the fixed boolean selection (caller rows), the
    kind's parameters, and the window [start, end) on the host's f64 clock."""

    def __init__(self, kind, sel, *, force=None, substep_dt=None, velocity=None, point=None, axis=None, omega=0.0,
                 along=0.0, start=0.0, end=999.0):
        assert kind in KINDS, kind
        self.kind = kind
        self.sel = np.asarray(sel, bool).copy()
        self.start, self.end = start, end
        if kind == "particle_impulse":
            self.force = np.asarray(force, np.float64).astype(f32)
            self.sdt = f32(substep_dt)
        elif kind == "enforce_particle_translation":
            self.velocity = np.asarray(velocity, np.float64).astype(f32)
        else:
            a = np.asarray(axis, np.float64)
            self.axis = (a * (1.0 / np.sqrt((a * a).sum()))).astype(f32)  # normalised in f64, rounded once
            self.point = np.asarray(point, np.float64).astype(f32)
            self.omega, self.along = f32(omega), f32(along)

    def active(self, t):
        return self.start <= t < self.end


def box_selection(x, center, size):
    """The selection of a box record: the region records' strict f32 test on the positions given."""
    return region_mask(x, center, size)


def apply_driver(d, x, v, mass):
    """One driver on v (in place), f32, unfused, left to right."""
    r = d.sel
    if not r.any():
        return
    if d.kind == "particle_impulse":
        v[r] = (v[r] + d.force[None, :] / mass[r, None] * d.sdt).astype(f32)
    elif d.kind == "enforce_particle_translation":
        v[r] = d.velocity
    else:
        q = (x[r] - d.point).astype(f32)
        a = d.axis
        c = np.stack([a[1] * q[:, 2] - a[2] * q[:, 1], a[2] * q[:, 0] - a[0] * q[:, 2],
                      a[0] * q[:, 1] - a[1] * q[:, 0]], 1).astype(f32)
        v[r] = (d.omega * c + (d.along * a)[None, :]).astype(f32)


def driver_substep(ref, drivers, dt, imp_active=None, op_active=None, drv_active=None, material=None):
    """solver.py:27-52 with the drivers between the impulses and the stress."""
    imps, ia, _, _ = ref._tables(imp_active, None)
    ref.gm[:] = 0
    ref.gv_in[:] = 0
    ref.gv_out[:] = 0
    L, st = ref._L, ctypes.byref(ref._st)
    L.om_impulses(st, ctypes.c_int(len(ref.impulses)), imps, O._p(ia))
    for j, d in enumerate(drivers):
        if drv_active is None or drv_active[j]:
            apply_driver(d, ref.x, ref.v, ref.mass)
    if material is None:
        L.om_stress(st, ctypes.c_float(dt))
    else:
        mixed_stress(ref, material, dt)
    L.om_p2g(st, ctypes.c_float(dt))
    ref.substep_end(dt, op_active)


def driver_run(ref, drivers, imps, ops, dt, n, t0=0.0, material=None):
    """scenarios.oracle_run with the driver substep; the activity of every
    record from the host clock, as the drop-in decides it."""
    t = t0
    for _ in range(n):
        ia = [int(b.active(t)) for b in imps]
        oa = [1 if b is None else int(b.active(t)) for b in ops]
        da = [int(d.active(t)) for d in drivers]
        driver_substep(ref, drivers, dt, ia, oa, da, material)
        t += dt
    return t
