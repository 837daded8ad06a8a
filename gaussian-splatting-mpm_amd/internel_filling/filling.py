"""Internal filling and particle volumes (internel_filling/filling.py) on the GPU.

fill_particles / init_filled_particles: new particles inside a hollow shell of
Gaussians, and their covariance, SH and opacity from the nearest source
Gaussian (libgsmpm.so's gsmpm_fill_*; DESIGN.md "Interior filling").

get_particle_volume: vol_p = dx^3 / (number of particles in p's cell),
cell = floor(x / dx), counted with i32 atomics in libgsmpm.so (k_fill_count /
k_fill_vol).
"""
import torch

from arguments import FillingParams
from gsmpm.fill import Filler, nearest
from gsmpm.sim import particle_volume

FILL_DEFAULTS = {**FillingParams.DEFAULTS, "grid_extent": 2.0}


def fill_particles(pos: torch.Tensor, cov: torch.Tensor, opacity: torch.Tensor, fill_args) -> torch.Tensor:
    """Grid-space pos [N,3], cov [N,6], opacity [N] or [N,1] -> filled_pos [M,3].

    fill_args: the config's ``particle_filling`` record (a dict; missing keys take
    FILL_DEFAULTS).  ``boundary`` = [x0, x1, y0, y1, z0, z1] in grid space keeps
    the filling inside that box; ``max_particles`` caps the count (the first ones
    in cell order are kept)."""
    unknown = set(fill_args) - set(FILL_DEFAULTS)
    if unknown:
        raise ValueError(f"particle_filling: unknown keys {sorted(unknown)}")
    a = {**FILL_DEFAULTS, **fill_args}
    box = None
    if a["boundary"] is not None:
        b = [float(v) for v in a["boundary"]]
        if len(b) != 6:
            raise ValueError("particle_filling.boundary must be [x0, x1, y0, y1, z0, z1]")
        box = (b[0::2], b[1::2])
    f = Filler(a["n_grid"], a["grid_extent"], a["density_threshold"], support=a["support"], min_hits=a["min_hits"],
               parity_dir=a["parity_dir"], per_cell=a["per_cell"], seed=a["seed"], box=box,
               capacity=a["max_particles"])
    f.interior(pos, cov, opacity)
    return f.emit()


def init_filled_particles(pos, shs, cov, opacity, new_pos):
    """(shs, opacity, cov) extended by one row per new_pos row: the values of its nearest source Gaussian."""
    if new_pos.shape[0] == 0:
        return shs, opacity, cov
    idx = nearest(new_pos, pos).long()
    return (torch.cat([shs, shs[idx]], dim=0), torch.cat([opacity, opacity[idx]], dim=0),
            torch.cat([cov, cov[idx]], dim=0))


def get_particle_volume(pos: torch.Tensor, args, uniform: bool = False):
    vol = particle_volume(pos, args.n_grid, args.grid_extent)
    if uniform:  # same volume for all particles (filling.py:39-40)
        return torch.mean(vol).repeat(pos.shape[0])
    return vol
