"""gsmpm_raster_backward_aux at the C-ABI, without a GPU: declared in
include/gsmpm.h, exported by libgsmpm.so, bound in gsmpm/_lib.py with the
signature the header states, and its argument validation runs before any HIP
call."""
from __future__ import annotations

import ctypes
import os
import re

from conftest import ROOT

NAME = "gsmpm_raster_backward_aux"


def test_declared_exported_and_bound():
    from gsmpm import _lib  # loads libgsmpm.so (no HIP call is made)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsmpm.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{NAME} is not declared in include/gsmpm.h"
    params = [p.strip() for p in m.group(1).split(",")]
    names = [re.findall(r"\w+", p)[-1] for p in params]
    assert names == ["r", "a", "radii", "dL_dcolor", "dL_ddepth", "dL_dalpha", "dL_dmeans2D", "dL_dcolors",
                     "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
                     "dL_dsh_rotations", "stream"]
    assert all(p.startswith("const float*") for p in params[3:6])
    fn = getattr(_lib.LIB, NAME)
    assert isinstance(fn, ctypes._CFuncPtr)
    restype, argtypes = _lib._SIGS[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params)
    # two more pointers than the call it extends
    assert len(argtypes) == len(_lib._SIGS["gsmpm_raster_backward_rot"][1]) + 2


def test_null_arguments_are_refused_before_any_hip_call():
    from gsmpm import _lib
    a = _lib.RasterArgs()
    a.P, a.W, a.H = 10, 64, 64
    rc = getattr(_lib.LIB, NAME)(None, ctypes.byref(a), *([None] * 14))
    assert rc == _lib.GSMPM_EINVAL
    assert "null argument" in _lib.last_error()
