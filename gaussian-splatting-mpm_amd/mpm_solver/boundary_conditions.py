"""Boundary-condition descriptors (mpm_solver/boundary_conditions.py:6-117).

Same constructor arguments, attributes, ``isActive`` windows and type
registries as the reference; the per-node / per-particle work runs inside the
fused HIP kernels (fixed cubes in k_grid, impulses in k_p2g).  The two
region records (additional_params, modify_material) are applied once, when
``set_boundary_conditions`` ends, through the library's region calls.
"""
from __future__ import annotations

from mpm_solver.utils import material_types


class BasicBC:
    """fixed_cube: zero v_out on nodes with |i*dx - center| < size (boundary_conditions.py:6-31)."""

    def __init__(self, n_particles, bc_args, sim_args):
        self.n_particles = n_particles
        self.substep_dt = sim_args.substep_dt
        self.id = bc_args["id"]
        self.type = bc_args["type"]
        self.start_time = bc_args["start_time"]
        # float64 on the host, as boundary_conditions.py:16
        self.end_time = bc_args["start_time"] + sim_args.substep_dt * bc_args["num_dt"]
        self.center = bc_args["center"]
        self.size = bc_args["size"]
        self.isCollide = False
        self.bit = None  # library bc id (bit of the activity mask)

    def isActive(self, time):
        return time >= self.start_time and time < self.end_time


class ImpulseBC(BasicBC):
    """impulse: v += force / m * substep_dt inside the box (boundary_conditions.py:34-45)."""

    def __init__(self, n_particles, bc_args, sim_args):
        self.force = list(bc_args["force"][:3])
        super().__init__(n_particles, bc_args, sim_args)


class MaterialParamsModifier(BasicBC):
    """additional_params (boundary_conditions.py:47-72).

    In the reference its apply() writes ``model.nu[p]`` / ``model.E[p]``,
    fields MPM_model never defines, so any config using it raises
    AttributeError before the record takes effect.  Here the
    record does what it plainly means: the particles inside the box get mu /
    lam from E and nu, mass from density, and ``applymu`` replaces mu unless
    it is the sentinel 1000 (gsmpm_mpm_set_region_params does all three).
    The fitting path only collects the record.
    """

    def __init__(self, n_particles, bc_args, sim_args):
        self.mu = bc_args["mu"]
        self.density = bc_args["density"]
        self.E = bc_args["E"]
        self.nu = bc_args["nu"]
        # optional, not in the reference: the yield of the rows inside the box (a
        # fluid region inside a metal body needs its own); absent: untouched
        self.yield_stress = bc_args.get("yield_stress")
        self.isMaterial = False
        super().__init__(n_particles, bc_args, sim_args)

    def apply(self, state, model):
        sim = _forward_sim(model, "additional_params")
        model._owner.flush()
        state._override_density(self.center, self.size, self.density)  # particle_density[p] = density (:63)
        sim.set_region_params(self.center, self.size, self.E, self.nu, self.density, self.mu)
        if self.yield_stress is not None:
            y = sim.get("yield_stress")
            y[_box_mask(sim.get("x"), self.center, self.size)] = float(self.yield_stress)
            sim.set("yield_stress", y)

    def applymu(self, state, model):
        """boundary_conditions.py:65-70 alone: mu inside the box, unless 1000.
        Kept for the reference's API shape only: apply() already took the
        override with E, nu and density in one region call, and
        set_boundary_conditions never calls this.  Called on its own it sets
        mu through the field views (a get and a set), not a kernel."""
        if self.mu == 1000:
            return
        sim = _forward_sim(model, "additional_params")
        model._owner.flush()
        mu = sim.get("mu")
        mu[_box_mask(sim.get("x"), self.center, self.size)] = float(self.mu)
        sim.set("mu", mu)


class MaterialTypeModifier(BasicBC):
    """modify_material (boundary_conditions.py:74-85): the particles inside the
    box take another material.  ``material`` is an int code, as the reference's
    configs give it, or a name from ``material_types``; an unknown name raises
    the reference's "Material not supported yet" TypeError (model.py:27-30).
    The simulator enters mixed mode (gsmpm_mpm_set_region_material)."""

    def __init__(self, n_particles, bc_args, sim_args):
        self.material = bc_args["material"]
        if isinstance(self.material, str):
            if self.material not in material_types:
                raise TypeError("Material not supported yet")
            self.material_code = material_types[self.material]
        else:
            self.material_code = int(self.material)
        self.isMaterial = True
        super().__init__(n_particles, bc_args, sim_args)

    def apply(self, state, model):
        sim = _forward_sim(model, "modify_material")
        model._owner.flush()
        sim.set_region_material(self.center, self.size, self.material_code)


def _box_mask(x, center, size):
    """The region records' box test (boundary_conditions.py:44, 60, 84): f32, strict."""
    import torch
    c = torch.tensor([float(v) for v in center], dtype=torch.float32, device=x.device)
    s = torch.tensor([float(v) for v in size], dtype=torch.float32, device=x.device)
    return ((x - c).abs() < s).all(dim=1)


def _forward_sim(model, what):
    owner = getattr(model, "_owner", None)
    sim = getattr(owner, "_sim", None)
    if sim is None:
        raise AttributeError(f"{what} applies to the forward-only simulator (the fitting path only collects it)")
    return sim


class StickyGroundBC(BasicBC):
    """sticky_ground (boundary_conditions.py:87-94): always-active fixed cube."""

    def __init__(self):
        self.center = [1.0, 0.6, 1.0]
        self.size = [1.0, 0.1, 1.0]
        self.type = "sticky_ground"
        self.isCollide = False
        self.start_time, self.end_time = 0.0, float("inf")
        self.bit = None

    def isActive(self, time):
        return True


class ColliderBC:
    """collider (not in the reference, whose add_surface_collider declares
    surface / start_time / end_time and never uses them, solver.py:140-147): an
    extended collider record -- shape "plane" (point, normal), "ball" (center,
    radius), "box" or "walls" (center, half), surface "sticky" / "slip" /
    "separate", friction, damping -- active while start_time <= time <
    end_time on the host's float64 clock.  The per-node work runs in the EXT
    grid kernels (gsmpm_mpm_add_collider).  isCollide stays False: unlike the
    legacy plane collider this one honours its window.  With a ``velocity``
    it is a moving record (gsmpm_mpm_add_moving_collider): it translates while
    move_start <= time < move_end (defaults: start_time, end_time).  With an
    ``angular_velocity`` it is a rotating record
    (gsmpm_mpm_add_rotating_collider): in the same window it also turns about
    ``pivot`` (default: its point or centre); ``velocity`` then defaults to
    zero."""

    _geometry = {"plane": ("point", "normal"), "ball": ("center", "radius"), "box": ("center", "half"),
                 "walls": ("center", "half")}

    def __init__(self, n_particles, bc_args, sim_args=None):
        self.n_particles = n_particles
        self.id = bc_args.get("id")
        self.type = "collider"
        self.shape = bc_args["shape"]
        if self.shape not in self._geometry:
            raise ValueError(f"collider: unknown shape {self.shape!r} (one of {sorted(self._geometry)})")
        self.surface = bc_args.get("surface", "separate")
        self.friction = float(bc_args.get("friction", 0.0))
        self.damping = float(bc_args.get("damping", 1.0))
        self.start_time = float(bc_args.get("start_time", 0.0))
        self.end_time = float(bc_args.get("end_time", 999.0))
        self.geometry = {k: bc_args[k] for k in self._geometry[self.shape]}  # KeyError names the missing one
        # a moving record: velocity, and the window of the motion (default: the activity window)
        self.velocity = bc_args.get("velocity")
        # a rotating record: angular velocity and pivot (default: the point or centre), in the same window
        self.angular_velocity = bc_args.get("angular_velocity")
        self.pivot = bc_args.get("pivot")
        if self.pivot is not None and self.angular_velocity is None:
            raise TypeError("collider: a pivot needs an angular_velocity")
        spins = self.angular_velocity is not None and any(float(a) != 0.0 for a in self.angular_velocity)
        self.motion = {}
        if self.velocity is not None or spins:
            ms, me = bc_args.get("move_start"), bc_args.get("move_end")
            self.move_start = self.start_time if ms is None else float(ms)
            self.move_end = self.end_time if me is None else float(me)
            self.motion = dict(move_start=self.move_start, move_end=self.move_end)
            if self.velocity is not None:
                self.motion["velocity"] = [float(a) for a in self.velocity]
            if spins:
                self.motion["angular_velocity"] = [float(a) for a in self.angular_velocity]
                if self.pivot is not None:
                    self.motion["pivot"] = [float(a) for a in self.pivot]
        elif bc_args.get("move_start") is not None or bc_args.get("move_end") is not None:
            raise TypeError("collider: move_start / move_end need a velocity or an angular_velocity")
        self.isCollide = False
        self.bit = None  # library bc id (bit of the activity mask)

    def isActive(self, time):
        return time >= self.start_time and time < self.end_time


class ParticleDriverBC:
    """particle_impulse / enforce_particle_translation /
    enforce_particle_rotation (not in the reference; ImpulseBC.apply's
    "#TODO: Need to replace this with a mask", boundary_conditions.py:43, asks
    for the first): a record on a selection of particles that is chosen once,
    when the record is added -- the rows inside ``center`` / ``size`` at that
    moment, or the rows of ``mask`` (n booleans, caller order) -- and never
    changes, wherever the particles go (gsmpm_mpm_add_driver).

      particle_impulse              force              v += force / m * substep_dt
      enforce_particle_translation  velocity           v = velocity
      enforce_particle_rotation     point, axis,       v = omega * cross(axis, x - point) + along * axis
                                    omega, along

    Active while start_time <= time < end_time on the host's float64 clock:
    ``start_time`` (default 0) with ``end_time`` (default 999.0) or ``num_dt``
    (end_time = start_time + substep_dt * num_dt in f64, as BasicBC).  Within
    a substep the drivers run after every box impulse, in the order they were
    added, before the stress: particle_preprocess with the drivers after the
    impulses."""

    _params = {"particle_impulse": ("force",), "enforce_particle_translation": ("velocity",),
               "enforce_particle_rotation": ("point", "axis")}

    def __init__(self, n_particles, bc_args, sim_args=None):
        self.n_particles = n_particles
        self.id = bc_args.get("id")
        self.type = bc_args["type"]
        if self.type not in self._params:
            raise ValueError(f"particle driver: unknown type {self.type!r} (one of {sorted(self._params)})")
        self.start_time = float(bc_args.get("start_time", 0.0))
        if bc_args.get("num_dt") is not None:
            if bc_args.get("end_time") is not None:
                raise TypeError(f"{self.type}: give end_time or num_dt, not both")
            self.end_time = self.start_time + sim_args.substep_dt * bc_args["num_dt"]  # f64, boundary_conditions.py:16
        else:
            end = bc_args.get("end_time")
            self.end_time = 999.0 if end is None else float(end)
        self.center, self.size, self.mask = bc_args.get("center"), bc_args.get("size"), bc_args.get("mask")
        if (self.center is None or self.size is None) if self.mask is None else (self.center is not None
                                                                                 or self.size is not None):
            raise TypeError(f"{self.type}: give the selection as center and size, or as mask")
        self.params = {k: bc_args[k] for k in self._params[self.type]}  # KeyError names the missing one
        if self.type == "particle_impulse":
            sdt = bc_args.get("substep_dt")
            self.params["substep_dt"] = float(sim_args.substep_dt if sdt is None else sdt)
            self.params["force"] = list(self.params["force"][:3])
        elif self.type == "enforce_particle_rotation":
            self.params["omega"] = float(bc_args.get("omega", 0.0))
            self.params["along"] = float(bc_args.get("along", 0.0))
        self.isCollide = False
        self.bit = None  # library bc id (bit of the activity mask)

    def isActive(self, time):
        return time >= self.start_time and time < self.end_time


# boundary_conditions.py:97-109 -- note preprocess_bc is a *string*, so
# ``type in preprocess_bc`` is a substring test exactly as in the reference
# (none of the driver names is a substring of it).
preprocess_bc = ("impulse")
postprocess_bc = ("fixed_cube", "sticky_ground")
init_bc = ("additional_params", "modify_material")
collider_bc = ("collider",)  # extended colliders: grid_postprocess entries with a window of their own
# particle drivers: particle_preprocess entries on a fixed selection, applied after the impulses
driver_bc = ("particle_impulse", "enforce_particle_translation", "enforce_particle_rotation")

boundaryConditionTypeCallBacks = {
    "fixed_cube": BasicBC,
    "impulse": ImpulseBC,
    "sticky_ground": StickyGroundBC,
    "additional_params": MaterialParamsModifier,
    "modify_material": MaterialTypeModifier,
    "collider": ColliderBC,
    "particle_impulse": ParticleDriverBC,
    "enforce_particle_translation": ParticleDriverBC,
    "enforce_particle_rotation": ParticleDriverBC,
}
