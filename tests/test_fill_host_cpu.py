"""The interior-filling entry points validate their arguments before any HIP
call, so the refusals can be checked without a GPU (tests/test_gpu_fill.py
repeats them on the device and follows them with a valid call)."""
from __future__ import annotations

import ctypes
import json
import os

import pytest

from conftest import PKG
from test_gpu_fill import bad_argument_cases, good_params, refused


def test_fill_entry_points_refuse_bad_arguments_without_a_gpu():
    from gsmpm import _lib
    L = _lib.LIB
    nb = ctypes.c_uint64(0)
    assert L.gsmpm_fill_workspace_size(ctypes.byref(good_params()), ctypes.byref(nb)) == 0
    # 8^3 cells: two u64 grids, one u32, u16 + 2 u8, three line masks, the scan's block totals, a counter
    assert 8 ** 3 * (8 + 8 + 4 + 2 + 1 + 1) + 3 * 64 * 8 <= nb.value <= 2 * 8 ** 3 * 24 + 4096
    fake = 0x1000  # never dereferenced: validation fails first
    tot, skp = ctypes.c_int64(0), ctypes.c_int64(0)
    for field, value in bad_argument_cases():
        p = good_params()
        setattr(p, field, value)
        assert refused(L.gsmpm_fill_workspace_size(ctypes.byref(p), ctypes.byref(nb))), field
        assert refused(L.gsmpm_fill_interior(ctypes.byref(p), fake, fake, fake, 1, fake, 1 << 30, ctypes.byref(tot),
                                             ctypes.byref(skp), None), field), field
    p = good_params()
    assert refused(L.gsmpm_fill_interior(ctypes.byref(p), None, fake, fake, 1, fake, 1 << 30, ctypes.byref(tot),
                                         ctypes.byref(skp), None), "null")
    assert refused(L.gsmpm_fill_interior(ctypes.byref(p), fake, fake, fake, -3, fake, 1 << 30, ctypes.byref(tot),
                                         ctypes.byref(skp), None), "count")
    assert L.gsmpm_fill_interior(ctypes.byref(p), fake, fake, fake, 1, fake, 16, ctypes.byref(tot),
                                 ctypes.byref(skp), None) == _lib.GSMPM_ESPACE
    assert refused(L.gsmpm_fill_nearest(fake, 1, None, 1, fake, None), "null")


def test_particle_filling_record_in_arguments_and_config():
    from arguments import FillingParams
    assert FillingParams(None).extract() is None
    rec = FillingParams({"n_grid": 64, "boundary": [0, 2, 0, 2, 0.4, 2]}).extract()
    assert rec["n_grid"] == 64 and rec["min_hits"] == 6 and rec["parity_dir"] == -1 and rec["per_cell"] == 1
    assert set(rec) == {"n_grid", "density_threshold", "support", "min_hits", "parity_dir", "per_cell", "seed",
                        "max_particles", "boundary"}
    with pytest.raises(ValueError):
        FillingParams({"n_grids": 64})
    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        plain = json.load(f)
    with open(os.path.join(PKG, "configs", "lego-filled.json")) as f:
        filled = json.load(f)
    assert "particle_filling" not in plain
    assert FillingParams(filled["particle_filling"]).extract()["n_grid"] == 128
    assert filled["mpm"] == plain["mpm"] and filled["model"] == plain["model"]
