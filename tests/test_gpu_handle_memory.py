"""What device memory an MPM handle holds (gsmpm_mpm_device_bytes): a handle
allocates the buffers of the pipeline it runs only -- the per-phase set, the
fused set, and the FOLD set on top of the fused one when GSMPM_FOLD=1 -- and
the buffers allocated on first use appear when they are first used.  The
figures are the sizes requested from hipMalloc, so they follow exactly from
the shapes: n = 3000 particles (np = 3072 rows) on a 32^3 grid is 4 x 4 x 5 =
80 fused tiles (8 x 8 x 7 cells) with max_chunks = 11 + 81 + 1 = 93, and 64
per-phase tiles (8^3 cells) with max_chunks = 11 + 65 + 1 = 77.  No test
reads the device's free memory: other processes move it.

That allocating by pipeline changed no result is
test_gpu_mpm.py::test_fused_single_chunk_deterministic (two independently
created default handles agree bit for bit) and the rest of the GPU suite.

No reference counterpart: memory accounting is this library's own."""
import os

import numpy as np
import pytest

from scenarios import lego_problem

pytestmark = pytest.mark.gpu

N, NG, NP = 3000, 32, 3072
KEYS = {"total", "phased", "fused", "fold"}


def _sim(fold=False, **kw):
    """A Simulator of the lego-like scene's parameters, created with GSMPM_FOLD set around the create only."""
    from gsmpm.sim import Simulator
    cfg = lego_problem(N, NG)["cfg"]
    old = os.environ.get("GSMPM_FOLD")
    os.environ["GSMPM_FOLD"] = "1" if fold else "0"
    try:
        return Simulator(N, n_grid=NG, grid_extent=cfg["grid_extent"], E=cfg["E"], nu=cfg["nu"],
                         density=cfg["density"], gravity=cfg["gravity"], **kw)
    finally:
        if old is None:
            os.environ.pop("GSMPM_FOLD")
        else:
            os.environ["GSMPM_FOLD"] = old


def _set_lego(sim, dev):
    import torch
    prob = lego_problem(N, NG)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    sim.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))


def _fused_tile_depth(sim, dev):
    """Cells of a fused tile along z (GSMPM_FT2 of the build): one column of
    cells 2..29 with 107 particles a cell (the 4 left over in cell 2), so the
    fullest tile holds 107 x depth particles for any depth up to 13."""
    import torch
    dx = sim.grid_extent / NG
    cell = np.concatenate([np.repeat(np.arange(2, 30), 107), np.full(N - 28 * 107, 2)])
    x = np.stack([np.full(N, 16.75 * dx), np.full(N, 16.75 * dx), (cell + 0.75) * dx], axis=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    sim.set_particles(t(x), t(np.tile([1e-4, 0, 0, 1e-4, 0, 1e-4], (N, 1))), t(np.full(N, dx ** 3 / 8)))
    st = sim.debug_stats()
    assert st["outside"] == 0 and st["binned"] == N and st["max_per_tile"] % 107 == 0, st
    return st["max_per_tile"] // 107


def test_default_handle_holds_the_fused_buffers_only(dev):
    sim = _sim()
    assert sim.pipeline == "fused" and not sim.folded
    m = sim.device_bytes()
    assert set(m) == KEYS
    assert m["phased"] == 0 and m["fold"] == 0 and m["fused"] > 0
    assert m["total"] >= m["fused"]


def test_phased_handle_holds_the_phased_buffers_only(dev):
    sim = _sim(phased=True)
    assert sim.pipeline == "phased" and not sim.folded
    m = sim.device_bytes()
    assert m["fused"] == 0 and m["fold"] == 0
    assert m["phased"] >= 16 * 78 * 1000  # its window slots alone: (max_chunks + 1) x kWin float4
    assert m["total"] >= m["phased"]


def test_fold_handle_adds_exactly_the_fold_buffers(dev):
    base = _sim().device_bytes()
    sim = _sim(fold=True)
    assert sim.pipeline == "fused" and sim.folded
    m = sim.device_bytes()  # before the probe below: set_particles allocates nothing (the test after this one)
    assert m["phased"] == 0
    assert m["fused"] == base["fused"]
    assert m["total"] - m["fold"] == base["total"]
    depth = _fused_tile_depth(sim, dev)
    if depth != 7:
        pytest.skip(f"the library was built with GSMPM_FT2 = {depth}, not its default 7: the tile count differs")
    # slots2 [93 + 1][1584] float4 + two 32^3 float4 grids + esc_nodes [3072][27] float4 + two tbox2 [80] int
    assert m["fold"] == 16 * 94 * 1584 + 2 * 16 * 32 ** 3 + 16 * 27 * NP + 2 * 4 * 80


def test_lazy_buffers_and_lifetime(dev):
    import torch
    first = _sim()
    total = first.device_bytes()["total"]
    _set_lego(first, dev)
    first.step(1e-4, [0] * 20)
    torch.cuda.synchronize()
    assert first.device_bytes()["total"] == total  # nothing is allocated by set_particles or a step
    first.set("material", torch.zeros(N, device=dev))
    assert first.material_mode == 1
    assert first.device_bytes()["total"] == total + 4 * NP  # mat_ids, on entering mixed mode
    first.set("material", torch.ones(N, device=dev))
    assert first.device_bytes()["total"] == total + 4 * NP  # and only once
    for _ in range(10):
        _sim().close()
    last = _sim()
    assert last.device_bytes() == {**first.device_bytes(), "total": total}
