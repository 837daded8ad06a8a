"""Torch-facing wrapper of the MPM C-ABI (gsmpm_mpm_*).

All tensors live on the current HIP device; every call is asynchronous on
torch's current stream.  This is plumbing: the math runs in libgsmpm.so.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import LIB, check, ptr, stream_of

# mpm_solver/utils.py:5-10, plus the fluid (GSMPM_MAT_FLUID: fluid_return_mapping, which the reference never dispatches)
MATERIALS = {"jelly": 0, "metal": 1, "sand": 2, "foam": 3, "fluid": 5}
_CODES = (0, 1, 2, 3, 5)  # 4 is private to the library (jelly + FCR: jelly_fcr=True)

_WIDTH = {"x": 3, "v": 3, "C": 9, "F_trial": 9, "cov": 6, "init_cov": 6, "R": 9, "mass": 1, "vol": 1, "mu": 1,
          "lam": 1, "yield_stress": 1, "material": 1}


def _d3(v):
    return (ctypes.c_double * 3)(*[float(a) for a in v])


class Simulator:
    """One MPM domain: particle state + dense n^3 grid on one GPU."""

    def __init__(self, n_particles: int, *, n_grid: int, grid_extent: float = 2.0, material: str | int = "jelly",
                 E: float = 2e6, nu: float = 0.4, density: float = 1000.0, gravity=(0.0, -9.81, 0.0),
                 yield_stress: float = 0.005, hardening: float = 1.0, xi: float = 1.0,
                 plastic_viscosity: float = 0.008, friction_angle: float = 25.0, jelly_fcr: bool = False,
                 keep_grid: bool = False, use_graph: bool = True, sort: bool = True, phased: bool = False,
                 device=None):
        code = MATERIALS.get(material, -1) if isinstance(material, str) else int(material)
        if code not in _CODES:
            raise TypeError("Material not supported yet")  # model.py:27-30
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.n = int(n_particles)
        self.n_grid = int(n_grid)
        self.grid_extent = float(grid_extent)
        p = _lib.MpmParams()
        p.n_particles = self.n
        p.n_grid = self.n_grid
        p.grid_extent = self.grid_extent
        p.material = code
        p.E, p.nu, p.density = float(E), float(nu), float(density)
        p.gravity[:] = [float(g) for g in gravity]
        p.yield_stress, p.hardening, p.xi = float(yield_stress), float(hardening), float(xi)
        p.plastic_viscosity, p.friction_angle_deg = float(plastic_viscosity), float(friction_angle)
        flags = 0
        if jelly_fcr:
            flags |= _lib.FLAG_JELLY_FCR
        if keep_grid:
            flags |= _lib.FLAG_KEEP_GRID
        if not use_graph:
            flags |= _lib.FLAG_NO_GRAPH
        if not sort:
            flags |= _lib.FLAG_NO_SORT
        if phased:
            flags |= _lib.FLAG_PHASED
        p.flags = flags
        self.params = p
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(LIB.gsmpm_mpm_create(ctypes.byref(p), ctypes.byref(h)), "gsmpm_mpm_create")
        self._h = h

    # -------------------------------------------------------------- setup --
    def set_particles(self, x, cov6, vol, v=None):
        f = lambda t: None if t is None else t.detach().to(self.device, torch.float32).contiguous()
        x, cov6, vol, v = f(x), f(cov6), f(vol), f(v)
        assert x.numel() == 3 * self.n and cov6.numel() == 6 * self.n and vol.numel() == self.n
        assert v is None or v.numel() == 3 * self.n
        check(LIB.gsmpm_mpm_set_particles(self._h, ptr(x), ptr(cov6), ptr(vol), ptr(v), stream_of(self.device)),
              "gsmpm_mpm_set_particles")

    def add_fixed_cube(self, center, size) -> int:
        return check(LIB.gsmpm_mpm_add_fixed_cube(self._h, _d3(center), _d3(size)), "add_fixed_cube")

    def add_impulse(self, center, size, force, substep_dt) -> int:
        return check(LIB.gsmpm_mpm_add_impulse(self._h, _d3(center), _d3(size), _d3(force), float(substep_dt)),
                     "add_impulse")

    def add_plane_collider(self, point, normal, friction=0.0) -> int:
        return check(LIB.gsmpm_mpm_add_plane_collider(self._h, _d3(point), _d3(normal), float(friction)),
                     "add_plane_collider")

    def add_collider(self, shape, surface="separate", friction=0.0, damping=1.0, *, point=None, normal=None,
                     center=None, radius=None, half=None, velocity=None, move_start=None, move_end=None,
                     angular_velocity=None, pivot=None) -> int:
        """An extended collider (gsmpm_mpm_add_collider; no reference counterpart):
        ``shape`` "plane" (point, normal), "ball" (center, radius), "box" or
        "walls" (center, half: a solid box / everything outside it), ``surface``
        "sticky", "slip" or "separate".  Returns its bit of the activity mask,
        which -- unlike the legacy plane collider's -- it honours.

        ``velocity`` (three components) makes it a moving record
        (gsmpm_mpm_add_moving_collider): it translates with that velocity
        while move_start <= time < move_end (defaults 0 and +inf) on the
        clock the caller hands ``step`` as ``times``, stands at its placement
        before and where it arrived after, and acts on the velocity relative
        to its own.

        ``angular_velocity`` (a vector, radians per unit of that clock) makes
        it a rotating record (gsmpm_mpm_add_rotating_collider): inside the
        same window it also turns about ``pivot``, a point of the axis that
        travels with the body (default: the record's point or centre, so the
        body spins in place); ``velocity`` may be combined with it and
        defaults to zero.  None or all zeros routes to the entries above."""
        if shape not in _lib.SHAPE:
            raise ValueError(f"add_collider: unknown shape {shape!r} (one of {sorted(_lib.SHAPE)})")
        if surface not in _lib.SURFACE:
            raise ValueError(f"add_collider: unknown surface {surface!r} (one of {sorted(_lib.SURFACE)})")
        want = {"plane": ("point", "normal"), "ball": ("center", "radius")}.get(shape, ("center", "half"))
        given = {"point": point, "normal": normal, "center": center, "radius": radius, "half": half}
        extra = [k for k, v in given.items() if v is not None and k not in want]
        missing = [k for k in want if given[k] is None]
        if extra or missing:
            raise TypeError(f"add_collider: a {shape} takes {want[0]} and {want[1]}"
                            + (f"; missing {missing}" if missing else "") + (f"; unexpected {extra}" if extra else ""))
        c = _lib.Collider()
        c.shape, c.surface = _lib.SHAPE[shape], _lib.SURFACE[surface]
        c.a[:] = [float(a) for a in given[want[0]]]
        c.b[:] = [float(radius), 0.0, 0.0] if shape == "ball" else [float(a) for a in given[want[1]]]
        c.friction, c.damping = float(friction), float(damping)
        spins = angular_velocity is not None and any(float(a) != 0.0 for a in angular_velocity)
        if pivot is not None and angular_velocity is None:
            raise TypeError("add_collider: a pivot needs an angular_velocity")
        if spins:
            sp = _lib.ColliderSpin()
            sp.velocity[:] = [0.0, 0.0, 0.0] if velocity is None else [float(a) for a in velocity]
            sp.t_start = 0.0 if move_start is None else float(move_start)
            sp.t_end = float("inf") if move_end is None else float(move_end)
            sp.omega[:] = [float(a) for a in angular_velocity]
            sp.pivot[:] = list(c.a) if pivot is None else [float(a) for a in pivot]
            bit = check(LIB.gsmpm_mpm_add_rotating_collider(self._h, ctypes.byref(c), ctypes.byref(sp)),
                        "add_collider")
            self._n_rot = getattr(self, "_n_rot", 0) + 1  # the width of poses()
            return bit
        if velocity is None:
            if move_start is not None or move_end is not None:
                raise TypeError("add_collider: move_start / move_end need a velocity")
            return check(LIB.gsmpm_mpm_add_collider(self._h, ctypes.byref(c)), "add_collider")
        m = _lib.ColliderMotion()
        m.velocity[:] = [float(a) for a in velocity]
        m.t_start = 0.0 if move_start is None else float(move_start)
        m.t_end = float("inf") if move_end is None else float(move_end)
        return check(LIB.gsmpm_mpm_add_moving_collider(self._h, ctypes.byref(c), ctypes.byref(m)), "add_collider")

    def poses(self, n: int):
        """The poses of the rotating colliders on the first n substeps of the
        last step call, a float32 array [n, rotating records, 16]: R (9, row
        major), c, o, 0 (gsmpm_mpm_get_poses; diagnostics, waits for the stream)."""
        import numpy as np
        n, n_rot = int(n), getattr(self, "_n_rot", 0)
        buf = (ctypes.c_float * max(16 * n_rot * n, 1))()
        check(LIB.gsmpm_mpm_get_poses(self._h, n, buf, stream_of(self.device)), "gsmpm_mpm_get_poses")
        return np.frombuffer(buf, dtype=np.float32, count=16 * n_rot * n).reshape(n, n_rot, 16).copy()

    def add_driver(self, kind, *, center=None, size=None, mask=None, force=None, substep_dt=None, velocity=None,
                   point=None, axis=None, omega=0.0, along=0.0) -> int:
        """A particle driver (gsmpm_mpm_add_driver): a record on a selection of
        particles that is chosen now and never changes -- the rows inside the
        box ``center`` / ``size`` at this moment (strict f32 |x - c| < s), or
        the rows of ``mask`` (n booleans, caller order).  ``kind``:
        "particle_impulse" (``force``, ``substep_dt``: v += force / m *
        substep_dt), "enforce_particle_translation" (``velocity``: v = velocity)
        or "enforce_particle_rotation" (``point``, ``axis``, ``omega``,
        ``along``: v = omega * cross(axis, x - point) + along * axis, the axis
        normalised).  Drivers act after the box impulses, in the order they
        were added, before the stress.  Returns the record's bit of the
        activity mask; the caller's clock decides its window."""
        if kind not in _lib.DRIVER:
            raise ValueError(f"add_driver: unknown kind {kind!r} (one of {sorted(_lib.DRIVER)})")
        want = {"particle_impulse": ("force", "substep_dt"), "enforce_particle_translation": ("velocity",),
                "enforce_particle_rotation": ("point", "axis")}[kind]
        given = {"force": force, "substep_dt": substep_dt, "velocity": velocity, "point": point, "axis": axis}
        extra = [k for k, v in given.items() if v is not None and k not in want]
        missing = [k for k in want if given[k] is None]
        if kind != "enforce_particle_rotation" and (float(omega) != 0.0 or float(along) != 0.0):
            extra.append("omega / along")
        if extra or missing:
            raise TypeError(f"add_driver: a {kind} takes {', '.join(want)}"
                            + (f"; missing {missing}" if missing else "") + (f"; unexpected {extra}" if extra else ""))
        if (center is None or size is None) if mask is None else (center is not None or size is not None):
            raise TypeError("add_driver: give the selection as center and size, or as mask")
        d = _lib.Driver()
        d.kind = _lib.DRIVER[kind]
        if mask is None:
            d.center[:] = [float(a) for a in center]
            d.size[:] = [float(a) for a in size]
        else:
            mask = torch.as_tensor(mask).to(self.device).reshape(-1).ne(0).to(torch.uint8).contiguous()
            if mask.numel() != self.n:
                raise ValueError(f"add_driver: the mask has {mask.numel()} entries for {self.n} particles")
        if kind == "particle_impulse":
            d.force[:] = [float(a) for a in force]
            d.substep_dt = float(substep_dt)
        elif kind == "enforce_particle_translation":
            d.velocity[:] = [float(a) for a in velocity]
        else:
            d.point[:] = [float(a) for a in point]
            d.axis[:] = [float(a) for a in axis]
            d.omega, d.along = float(omega), float(along)
        with torch.cuda.device(self.device):  # the first driver allocates the selection words
            return check(LIB.gsmpm_mpm_add_driver(self._h, ctypes.byref(d), ptr(mask), stream_of(self.device)),
                         "add_driver")

    def driver_selection(self, bit: int) -> torch.Tensor:
        """The selection of the driver with activity bit ``bit``: n booleans in
        caller order (gsmpm_mpm_get_driver_selection)."""
        out = torch.empty(self.n, dtype=torch.uint8, device=self.device)
        check(LIB.gsmpm_mpm_get_driver_selection(self._h, int(bit), ptr(out), stream_of(self.device)),
              "driver_selection")
        return out.bool()

    def graph_count(self) -> int:
        """Step graphs the handle caches now (gsmpm_mpm_graph_count; diagnostics)."""
        return check(LIB.gsmpm_mpm_graph_count(self._h), "graph_count")

    # ------------------------------------------------ per-particle materials --
    @property
    def material_mode(self) -> int:
        """0: one material (chosen at create); 1: mixed -- each particle's stress
        follows its own ``material`` value (gsmpm_mpm_material_mode).  Entered by
        ``set("material", t)`` or ``set_region_material``; lasts until
        ``set_particles``."""
        return check(LIB.gsmpm_mpm_material_mode(self._h), "gsmpm_mpm_material_mode")

    def set_region_material(self, center, size, material):
        """modify_material (boundary_conditions.py:74-85): the particles now
        inside the box |x - center| < size get `material` (a name or a code)."""
        code = MATERIALS.get(material, -1) if isinstance(material, str) else int(material)
        if code not in _CODES:
            raise TypeError("Material not supported yet")  # model.py:27-30
        check(LIB.gsmpm_mpm_set_region_material(self._h, _d3(center), _d3(size), code, stream_of(self.device)),
              "gsmpm_mpm_set_region_material")

    def set_region_params(self, center, size, E, nu, density, mu=1000):
        """additional_params (boundary_conditions.py:47-70): the particles now
        inside the box get mu / lam from E and nu, mass = density * vol, and
        mu = `mu` unless it is the reference's sentinel 1000."""
        check(LIB.gsmpm_mpm_set_region_params(self._h, _d3(center), _d3(size), float(E), float(nu), float(density),
                                              float(mu), stream_of(self.device)), "gsmpm_mpm_set_region_params")

    # ------------------------------------------------------------ stepping --
    def step(self, dt: float, masks, times=None):
        """len(masks) substeps.  ``times``: the caller's float64 clock at each
        substep (bc.substep_times), required once the simulator holds a moving
        collider -- the library then refuses the untimed call (RuntimeError)
        -- and ignored otherwise (gsmpm_mpm_step_timed)."""
        n = len(masks)
        if n == 0:
            return
        arr = (ctypes.c_uint32 * n)(*[int(m) & 0xFFFFFFFF for m in masks])
        if times is None:
            check(LIB.gsmpm_mpm_step(self._h, ctypes.c_float(dt), n, arr, stream_of(self.device)), "gsmpm_mpm_step")
            return
        if len(times) != n:
            raise ValueError(f"step: {n} masks but {len(times)} times")
        tarr = (ctypes.c_double * n)(*[float(t) for t in times])
        check(LIB.gsmpm_mpm_step_timed(self._h, ctypes.c_float(dt), n, arr, tarr, stream_of(self.device)),
              "gsmpm_mpm_step_timed")

    def check_finite(self, clear: bool = False):
        """SURVEY 5's per-frame NaN / Inf check: waits for the stream and
        raises RuntimeError if any substep so far produced non-finite particle
        state -- a position, or a P2G scatter input (mass, velocity, C,
        stress) -- (``step`` also raises, at the call after)."""
        check(LIB.gsmpm_mpm_check_finite(self._h, int(bool(clear)), stream_of(self.device)), "check_finite")

    # ---------------------------------------------------------- slab mode --
    def slab_init(self, rank: int, world: int, lo: int, hi: int, margin: int = 2, interval: int = 10):
        """Make this simulator (created with n_particles = capacity) rank `rank`
        of a `world`-slab domain owning grid planes [lo, hi) (csrc/slab.h)."""
        with torch.cuda.device(self.device):  # the slab's comm stream / buffers live on this device
            check(LIB.gsmpm_mpm_slab_init(self._h, int(rank), int(world), int(lo), int(hi), int(margin),
                                          int(interval)), "gsmpm_mpm_slab_init")

    def slab_set_particles(self, x, cov6, vol, gid, v=None):
        f = lambda t: None if t is None else t.detach().to(self.device, torch.float32).contiguous()
        x, cov6, vol, v = f(x), f(cov6), f(vol), f(v)
        gid = gid.detach().to(self.device, torch.int32).contiguous()
        n = int(gid.numel())
        assert x.numel() == 3 * n and cov6.numel() == 6 * n and vol.numel() == n
        check(LIB.gsmpm_mpm_slab_set_particles(self._h, n, ptr(x) if n else None, ptr(cov6) if n else None,
                                               ptr(vol) if n else None, ptr(v) if n and v is not None else None,
                                               ptr(gid) if n else None, stream_of(self.device)),
              "gsmpm_mpm_slab_set_particles")

    def slab_step(self, dt: float, masks, transport):
        """`len(masks)` substeps with the window exchange every substep and the
        particle migration every `interval` substeps through `transport`
        (gsmpm.dist.RcclTransport / CallbackTransport)."""
        n = len(masks)
        if n == 0:
            return
        arr = (ctypes.c_uint32 * n)(*[int(m) & 0xFFFFFFFF for m in masks])
        xp = None if transport is None else ctypes.byref(transport.struct)
        with torch.cuda.device(self.device):
            check(LIB.gsmpm_mpm_slab_step(self._h, ctypes.c_float(dt), n, arr, xp, stream_of(self.device)),
                  "gsmpm_mpm_slab_step")

    @property
    def count(self) -> int:
        """Particles this simulator holds now (a slab's count changes with migration)."""
        return check(LIB.gsmpm_mpm_count(self._h), "gsmpm_mpm_count")

    def get_gid(self) -> torch.Tensor:
        out = torch.empty(self.count, dtype=torch.int32, device=self.device)
        if out.numel():
            check(LIB.gsmpm_mpm_get_gid(self._h, ptr(out), stream_of(self.device)), "gsmpm_mpm_get_gid")
        return out

    def slab_stats(self):
        b = (ctypes.c_int64 * 12)()
        check(LIB.gsmpm_mpm_slab_stats(self._h, b), "gsmpm_mpm_slab_stats")
        keys = ("migrations", "migrated", "lo", "hi", "margin", "interval", "window_planes", "capacity", "deferred",
                "payload_capacity", "host_syncs", "step_calls")
        return dict(zip(keys, [int(v) for v in b]))

    def slab_rects(self):
        """The exchanged yz rect of the lower and upper window: [(y0, ny, z0, nz)] * 2."""
        b = (ctypes.c_int32 * 8)()
        check(LIB.gsmpm_mpm_slab_rects(self._h, b), "gsmpm_mpm_slab_rects")
        return [tuple(int(v) for v in b[4 * w:4 * w + 4]) for w in (0, 1)]

    def slab_set_rebalance(self, on: bool = True, tolerance: float = 0.05):
        """Re-cut the slabs at step-call boundaries when the most loaded one holds
        more than (1 + tolerance) x the mean (gsmpm_mpm_slab_set_rebalance)."""
        check(LIB.gsmpm_mpm_slab_set_rebalance(self._h, 1 if on else 0, ctypes.c_float(tolerance)),
              "gsmpm_mpm_slab_set_rebalance")

    def slab_set_weight(self, weight: float):
        """This rank's share weight in the re-cut (gsmpm_mpm_slab_set_weight)."""
        check(LIB.gsmpm_mpm_slab_set_weight(self._h, ctypes.c_float(weight)), "gsmpm_mpm_slab_set_weight")

    def slab_bounds(self, world: int):
        """(every slab's bounds [world + 1], re-cuts so far)."""
        b = (ctypes.c_int32 * (world + 1))()
        n = ctypes.c_int64(0)
        check(LIB.gsmpm_mpm_slab_bounds(self._h, b, world + 1, ctypes.byref(n)), "gsmpm_mpm_slab_bounds")
        return [int(v) for v in b], int(n.value)

    def profile(self, dt: float, masks):
        """Eager substeps with a hipEvent pair per kernel -> summed ms of
        (k_p2g, k_grid, k_g2p, binning); fused pipeline: (k_fused, k_grid_f,
        binning + the re-binning permute, number of k_grid_f launches)."""
        n = len(masks)
        arr = (ctypes.c_uint32 * max(1, n))(*[int(m) & 0xFFFFFFFF for m in masks])
        out = (ctypes.c_float * 4)()
        check(LIB.gsmpm_mpm_profile_substeps(self._h, ctypes.c_float(dt), n, arr, out, stream_of(self.device)),
              "gsmpm_mpm_profile_substeps")
        return tuple(float(v) for v in out)

    def time_kernels(self, dt: float, mask: int, reps: int = 20):
        """Per-launch ms of (k_p2g, k_grid, k_g2p, binning) -- fused pipeline:
        (k_fused, k_grid_f, binning, 0: the permute is not timed here and no
        launch is counted) -- from hipEvents around `reps` back-to-back
        launches of each on this stream; state restored."""
        out = (ctypes.c_float * 4)()
        check(LIB.gsmpm_mpm_time_kernels(self._h, ctypes.c_float(dt), int(mask) & 0xFFFFFFFF, int(reps), out,
                                         stream_of(self.device)), "gsmpm_mpm_time_kernels")
        return tuple(float(v) for v in out)

    def debug_stats(self):
        b = (ctypes.c_int32 * 8)()
        check(LIB.gsmpm_mpm_debug_stats(self._h, b, stream_of(self.device)), "gsmpm_mpm_debug_stats")
        keys = ("active_tiles", "max_per_tile", "outside", "chunks", "touched_tiles", "binned", "parity", "since_sort")
        return dict(zip(keys, list(b)))

    def live_box(self):
        b = (ctypes.c_int32 * 6)()
        check(LIB.gsmpm_mpm_live_box(self._h, b, stream_of(self.device)), "gsmpm_mpm_live_box")
        return list(b[:3]), list(b[3:])

    @property
    def pipeline(self) -> str:
        """'fused' (k_fused + k_grid_f per substep) or 'phased' (k_p2g, k_grid, k_g2p, binning)."""
        code = check(LIB.gsmpm_mpm_pipeline(self._h), "gsmpm_mpm_pipeline")
        return "fused" if code == _lib.PIPE_FUSED else "phased"

    @property
    def folded(self) -> bool:
        """True when each substep's grid update is folded into the next k_fused
        launch (gsmpm_mpm_folded; one launch per substep)."""
        return bool(check(LIB.gsmpm_mpm_folded(self._h), "gsmpm_mpm_folded"))

    def device_bytes(self) -> dict:
        """Device memory the handle holds, in requested bytes (gsmpm_mpm_device_bytes):
        'total' and its 'phased', 'fused' and 'fold' parts."""
        out = (ctypes.c_uint64 * 4)()
        check(LIB.gsmpm_mpm_device_bytes(self._h, out), "gsmpm_mpm_device_bytes")
        return dict(zip(("total", "phased", "fused", "fold"), (int(v) for v in out)))

    def escapes(self, clear: bool = False) -> int:
        """Particle scatters that left their chunk window since set_particles or
        the last clear (gsmpm_mpm_escapes; syncs the stream)."""
        out = ctypes.c_int64(0)
        check(LIB.gsmpm_mpm_escapes(self._h, int(bool(clear)), ctypes.byref(out), stream_of(self.device)),
              "gsmpm_mpm_escapes")
        return int(out.value)

    def rebin_state(self):
        """{interval, auto, rebins_last_call, vmax} (gsmpm_mpm_rebin_state): the
        longest spacing, whether the re-binnings adapt to the particles' speed,
        how many the last step call ran (0: from the interval) and the fastest
        velocity component seen."""
        b = (ctypes.c_int32 * 3)()
        v = ctypes.c_float(0.0)
        check(LIB.gsmpm_mpm_rebin_state(self._h, b, ctypes.byref(v)), "gsmpm_mpm_rebin_state")
        return {"interval": int(b[0]), "auto": bool(b[1]), "rebins_last_call": int(b[2]), "vmax": float(v.value)}

    def set_rebin_interval(self, substeps: int):
        """Fused pipeline: substeps between particle re-binnings (any value >= 1 is correct)."""
        check(LIB.gsmpm_mpm_set_rebin_interval(self._h, int(substeps)), "gsmpm_mpm_set_rebin_interval")

    def resort(self, interval: int = -1):
        """Re-sort storage into Morton order now; interval >= 0 sets the automatic period."""
        check(LIB.gsmpm_mpm_resort(self._h, int(interval), stream_of(self.device)), "gsmpm_mpm_resort")

    def postprocess(self):
        if self.count == 0:
            return
        check(LIB.gsmpm_mpm_postprocess(self._h, stream_of(self.device)), "gsmpm_mpm_postprocess")

    # ------------------------------------------------------------------ io --
    def get(self, name: str) -> torch.Tensor:
        w, n = _WIDTH[name], self.count
        out = torch.empty((n, w) if w > 1 else (n,), dtype=torch.float32, device=self.device)
        if n:
            check(LIB.gsmpm_mpm_get(self._h, _lib.FIELD[name], ptr(out), stream_of(self.device)), f"get {name}")
        return out

    def set(self, name: str, t: torch.Tensor):
        t = t.detach().to(self.device, torch.float32).contiguous()
        assert t.numel() == self.n * _WIDTH[name]
        check(LIB.gsmpm_mpm_set(self._h, _lib.FIELD[name], ptr(t), stream_of(self.device)), f"set {name}")

    def get_grid(self, which: str) -> torch.Tensor:
        code = {"mass": 0, "v_in": 1, "v_out": 2}[which]
        ng = self.n_grid
        shape = (ng, ng, ng) if code == 0 else (ng, ng, ng, 3)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        check(LIB.gsmpm_mpm_get_grid(self._h, code, ptr(out), stream_of(self.device)), f"get_grid {which}")
        return out

    def world_outputs(self, scale, center, render_space: bool, means_out=None, cov_out=None):
        """Fused grid2world (+ render shift) of x and cov, in caller order."""
        n = self.count
        means_out = torch.empty((n, 3), dtype=torch.float32, device=self.device) if means_out is None else means_out
        cov_out = torch.empty((n, 6), dtype=torch.float32, device=self.device) if cov_out is None else cov_out
        if n == 0:
            return means_out, cov_out
        c = (ctypes.c_float * 3)(*[float(a) for a in center])
        check(LIB.gsmpm_mpm_world_outputs(self._h, ctypes.c_float(float(scale)), c, int(bool(render_space)),
                                          ptr(means_out), ptr(cov_out), stream_of(self.device)), "world_outputs")
        return means_out, cov_out

    def sh_rotations(self, A=None, out=None):
        """gsmpm_mpm_sh_rotations: [N,3,3], the rasterizer's sh_rotations for the
        last postprocess, in caller order.  A is None: particle_R as stored
        (= R^T of the polar rotation R, the Q for world-space means).  A given
        (3x3, means_render = A means_world): A particle_R A^T."""
        n = self.count
        out = torch.empty((n, 3, 3), dtype=torch.float32, device=self.device) if out is None else out
        if n == 0:
            return out
        a = None
        if A is not None:
            vals = torch.as_tensor(A, dtype=torch.float64).reshape(-1).tolist()
            if len(vals) != 9:
                raise ValueError("sh_rotations: A must be 3x3")
            a = (ctypes.c_float * 9)(*vals)
        check(LIB.gsmpm_mpm_sh_rotations(self._h, a, ptr(out), stream_of(self.device)), "gsmpm_mpm_sh_rotations")
        return out

    def close(self):
        if getattr(self, "_h", None):
            LIB.gsmpm_mpm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def particle_volume(x: torch.Tensor, n_grid: int, grid_extent: float) -> torch.Tensor:
    """internel_filling/filling.py:27-42 on the GPU (i32 atomics, floor cells)."""
    x = x.detach().to(torch.float32).contiguous()
    n = x.shape[0]
    scratch = torch.empty(n_grid ** 3, dtype=torch.int32, device=x.device)
    vol = torch.empty(n, dtype=torch.float32, device=x.device)
    check(LIB.gsmpm_particle_volume(ptr(x), n, n_grid, float(grid_extent), ptr(scratch), ptr(vol),
                                    stream_of(x.device)), "gsmpm_particle_volume")
    return vol


def alpha_from_friction(friction_angle_deg: float) -> float:
    """model.py:48-51 (f64)."""
    s = math.sin(friction_angle_deg / 180.0 * 3.141592653589793)
    return math.sqrt(2.0 / 3.0) * 2.0 * s / (3.0 - s)
