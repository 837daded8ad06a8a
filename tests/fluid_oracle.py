"""tests/mixed_oracle.py's phase composition with a fifth code, the fluid
(test infrastructure only; oracle/ is unchanged).

The substep is the same sequence -- grid reset, ``om_impulses``, stress,
``om_p2g``, ``substep_end`` -- and the stress of the rows with codes 0-3 is
``om_stress`` per id on compacted rows, exactly as ``mixed_oracle.mixed_stress``
does it.  Rows whose stored value is == 5 take
``oracle.fluid_return_mapping(F_trial, mu, lam, yield, dt, plastic_viscosity)``
(``om_fluid``: fluid_return_mapping, constitutive_models.py:142-213, with the
StVK Kirchhoff stress), written to ``F`` and ``stress``; their yield is never
written.  With ids 0-3 only, ``fluid_run`` is ``mixed_run`` bit for bit
(tests/test_fluid_oracle.py).
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from mixed_oracle import region_mask  # noqa: F401  (re-exported)

FLUID = 5


def codes5(material):
    """mixed_oracle.material_codes plus == 5 fluid: the stored f32 value by the
    reference's comparisons (== 1 metal, == 2 sand, == 3 foam), == 5 the
    fluid, anything else (4, 7, non-integers, NaN) the `else` branch, jelly (0)."""
    m = np.asarray(material, np.float32)
    code = np.zeros(m.shape, np.int32)
    for c in (1, 2, 3, FLUID):
        code[m == np.float32(c)] = c
    return code


def fluid_stress(ref, material, dt, pv=0.008):
    """The stress phase per id on compacted rows; F, stress (and for codes 0-3
    yield_stress) scattered back.  Returns the fluid rows that yielded
    (F != F_trial), a bool array over all rows."""
    code = codes5(material)
    L = ref._L
    yielded = np.zeros(len(code), bool)
    for c in np.unique(code):
        rows = np.nonzero(code == c)[0]
        if c == FLUID:
            Fo, tau = O.fluid_return_mapping(ref.F_trial[rows], ref.mu[rows], ref.lam[rows], ref.yield_stress[rows],
                                             dt, pv)
            ref.F[rows] = Fo.reshape(-1, 9)
            ref.stress[rows] = tau.reshape(-1, 9)
            yielded[rows] = (ref.F[rows] != ref.F_trial[rows]).any(axis=1)
            continue
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
    return yielded


def fluid_substep(ref, material, dt, imp_active=None, op_active=None, pv=0.008):
    """mixed_oracle.mixed_substep with the five-code stress phase; returns fluid_stress's mask."""
    imps, ia, _, _ = ref._tables(imp_active, None)
    ref.gm[:] = 0
    ref.gv_in[:] = 0
    ref.gv_out[:] = 0
    L, st = ref._L, ctypes.byref(ref._st)
    L.om_impulses(st, ctypes.c_int(len(ref.impulses)), imps, O._p(ia))
    yielded = fluid_stress(ref, material, dt, pv)
    L.om_p2g(st, ctypes.c_float(dt))
    ref.substep_end(dt, op_active)
    return yielded


def fluid_run(ref, ids, imps, ops, dt, n, pv=0.008, t0=0.0, yielded=None):
    """mixed_oracle.mixed_run with the five-code substep.  ``yielded``: a list
    that receives each substep's count of yielded fluid rows."""
    t = t0
    for _ in range(n):
        ia = [int(b.active(t)) for b in imps]
        oa = [1 if b is None else int(b.active(t)) for b in ops]
        y = fluid_substep(ref, ids, dt, ia, oa, pv)
        if yielded is not None:
            yielded.append(int(y.sum()))
        t += dt
    return t
