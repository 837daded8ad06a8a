"""A mixed-material substep built from the oracle's own phase functions
(test infrastructure only; oracle/ is unchanged).

The reference dispatches compute_stress_from_F_trial per particle on
``model.material[p]`` (utils.py:13-54).  ``om_stress`` is independent per
particle and reads one material for the whole state, so running it once per
material id present, on a compacted copy of that id's rows, is exactly the
reference's per-particle dispatch.  With uniform ids the substep below is
``OracleMPM.substep`` bit for bit (tests/test_mixed_oracle.py).
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O


def material_codes(material):
    """The reference's comparisons on the stored f32 value: == 1 metal, == 2
    sand, == 3 foam, anything else (NaN and non-integers included) the `else`
    branch, jelly (0)."""
    m = np.asarray(material, np.float32)
    code = np.zeros(m.shape, np.int32)
    for c in (1, 2, 3):
        code[m == np.float32(c)] = c
    return code


def mixed_stress(ref, material, dt):
    """om_stress per material id on compacted rows; F, stress and yield_stress scattered back."""
    code = material_codes(material)
    L = ref._L
    for c in np.unique(code):
        rows = np.nonzero(code == c)[0]
        sub = {k: np.ascontiguousarray(getattr(ref, k)[rows]) for k in
               ("F_trial", "F", "stress", "mu", "lam", "yield_stress")}
        st = O._State()
        ctypes.memmove(ctypes.byref(st), ctypes.byref(ref._st), ctypes.sizeof(O._State))
        st.n = len(rows)
        st.material = int(c)
        for k, a in sub.items():
            setattr(st, k, O._p(a))
        L.om_stress(ctypes.byref(st), ctypes.c_float(dt))
        for k in ("F", "stress", "yield_stress"):
            getattr(ref, k)[rows] = sub[k]


def mixed_substep(ref, material, dt, imp_active=None, op_active=None):
    """solver.py:27-52 with the per-particle material dispatch: grid reset,
    impulses, stress per id, P2G, then the oracle's substep_end."""
    imps, ia, _, _ = ref._tables(imp_active, None)
    ref.gm[:] = 0
    ref.gv_in[:] = 0
    ref.gv_out[:] = 0
    L, st = ref._L, ctypes.byref(ref._st)
    L.om_impulses(st, ctypes.c_int(len(ref.impulses)), imps, O._p(ia))
    mixed_stress(ref, material, dt)
    L.om_p2g(st, ctypes.c_float(dt))
    ref.substep_end(dt, op_active)


def mixed_run(ref, material, imps, ops, dt, n, t0=0.0):
    """scenarios.oracle_run with the mixed substep."""
    t = t0
    for _ in range(n):
        ia = [int(b.active(t)) for b in imps]
        oa = [1 if b is None else int(b.active(t)) for b in ops]
        mixed_substep(ref, material, dt, ia, oa)
        t += dt
    return t


def region_mask(x, center, size):
    """The region records' box test (boundary_conditions.py:44, 60, 84) in f32, strict."""
    x = np.asarray(x, np.float32)
    c = np.asarray(center, np.float32)
    s = np.asarray(size, np.float32)
    return np.all(np.abs(x - c) < s, axis=1)
