"""Interior particle filling (csrc/fill.hip) -- thin wrappers over gsmpm_fill_*.

    f = Filler(n_grid=128, grid_extent=2.0, density_threshold=0.5)
    total, skipped = f.interior(x, cov6, opacity)   # grid-space x [N,3], cov6 [N,6], opacity [N]
    new_x = f.emit()                                 # [min(total, capacity), 3]
    idx = nearest(new_x, x)                          # nearest source Gaussian of each

Tensors in, tensors out, on the tensors' device and current stream.  The
workspace is one torch buffer owned by the Filler.  DESIGN.md "Interior
filling" defines every step.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import LIB, FillParams, check, ptr, stream_of

GRID = {"density": (0, torch.float32), "occupied": (1, torch.uint8), "interior": (2, torch.uint8),
        "bits": (3, torch.int16), "density_fixed": (4, torch.int64)}
QUANTUM = 2.0 ** -24
DIRECTIONS = ("+x", "-x", "+y", "-y", "+z", "-z")


class Filler:
    def __init__(self, n_grid, grid_extent, density_threshold, support=4, min_hits=6, parity_dir=-1, per_cell=1,
                 seed=0, box=None, capacity=None):
        p = FillParams()
        p.n_grid, p.grid_extent, p.density_threshold = int(n_grid), float(grid_extent), float(density_threshold)
        p.support, p.min_hits, p.parity_dir, p.per_cell = int(support), int(min_hits), int(parity_dir), int(per_cell)
        p.seed = int(seed) & 0xFFFFFFFF
        if box is not None:
            lo, hi = box
            p.use_box = 1
            p.lo[:] = [float(v) for v in lo]
            p.hi[:] = [float(v) for v in hi]
        # default capacity: every cell interior
        p.capacity = int(n_grid) ** 3 * int(per_cell) if capacity is None else int(capacity)
        self.params = p
        nb = ctypes.c_uint64(0)
        check(LIB.gsmpm_fill_workspace_size(ctypes.byref(p), ctypes.byref(nb)), "gsmpm_fill_workspace_size")
        self.ws_bytes = nb.value
        self.ws = None
        self.total = None

    def _workspace(self, device):
        if self.ws is None or self.ws.device != device:
            self.ws = torch.empty(self.ws_bytes + 256, dtype=torch.uint8, device=device)
            self._off = (-self.ws.data_ptr()) % 256
        return self.ws.data_ptr() + self._off

    def interior(self, x, cov6, opacity):
        """-> (total, skipped).  The grids stay in the workspace for emit() / grid()."""
        x = x.detach().to(torch.float32).contiguous()
        cov6 = cov6.detach().to(torch.float32).contiguous()
        opacity = opacity.detach().to(torch.float32).reshape(-1).contiguous()
        n = x.shape[0]
        if x.shape != (n, 3) or cov6.shape != (n, 6) or opacity.shape != (n,):
            raise ValueError("expected x [N,3], cov6 [N,6], opacity [N]")
        self.device = x.device
        total, skipped = ctypes.c_int64(0), ctypes.c_int64(0)
        with torch.cuda.device(x.device):
            check(LIB.gsmpm_fill_interior(ctypes.byref(self.params), ptr(x), ptr(cov6), ptr(opacity), n,
                                          self._workspace(x.device), self.ws_bytes, ctypes.byref(total),
                                          ctypes.byref(skipped), stream_of(x.device)), "gsmpm_fill_interior")
        self.total = total.value
        return total.value, skipped.value

    def emit(self, out=None):
        """The first min(total, capacity) particles, [M,3]; `out` (at least that many rows) is written in place."""
        if self.total is None:
            raise RuntimeError("emit() before interior()")
        m = min(self.total, self.params.capacity)
        if out is None:
            out = torch.empty((m, 3), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 3 or out.shape[0] < m:
            raise ValueError("out must be float32 [>= min(total, capacity), 3]")
        if out.shape[0]:
            with torch.cuda.device(self.device):
                check(LIB.gsmpm_fill_emit(ctypes.byref(self.params), self._workspace(self.device), self.ws_bytes,
                                          ptr(out), stream_of(self.device)), "gsmpm_fill_emit")
        return out

    def grid(self, which):
        """density / occupied / interior / bits / density_fixed as an [n,n,n] tensor."""
        if self.total is None:
            raise RuntimeError("grid() before interior()")
        gid, dtype = GRID[which]
        n = self.params.n_grid
        out = torch.empty((n, n, n), dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            check(LIB.gsmpm_fill_get_grid(ctypes.byref(self.params), self._workspace(self.device), self.ws_bytes, gid,
                                          ptr(out), stream_of(self.device)), "gsmpm_fill_get_grid")
        return out


def nearest(query, source):
    """int32 [Q]: for each query row the nearest source row (exact, lowest index on ties)."""
    query = query.detach().to(torch.float32).contiguous()
    source = source.detach().to(torch.float32).contiguous()
    idx = torch.empty(query.shape[0], dtype=torch.int32, device=query.device)
    with torch.cuda.device(query.device):
        check(LIB.gsmpm_fill_nearest(ptr(query), query.shape[0], ptr(source), source.shape[0], ptr(idx),
                                     stream_of(query.device)), "gsmpm_fill_nearest")
    return idx
