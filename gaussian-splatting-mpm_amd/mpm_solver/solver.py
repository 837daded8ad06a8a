"""``MPM_Simulator`` drop-in (mpm_solver/solver.py:9-177) over libgsmpm.so.

``p2g2p(dt)`` keeps the reference's per-substep call and float64 host clock
(solver.py:27-52) but does not launch per call: the substep's BC activity
mask is decided on the host (exactly as ``isActive`` at the current
``self.time``) and queued; the queue is flushed as one ``gsmpm_mpm_step`` --
a cached hipGraph of fused kernels -- when state is read, ``postprocess()``
runs, or ``flush()`` is called.  Results are identical to launching per call.

With ``args.fitting=True`` the simulator is the differentiable one
(MPM_state_opt, 31 state levels; gsmpm/fit.py over gsmpm_fit_*):
``p2g2p_forward / p2g2p_backward / postprocess_forward / _backward / learn /
clear_grads`` and ``mpm_state.set_grads / cycle_init`` as in the reference.
"""
from __future__ import annotations

import math

from gsmpm.fit import FitSimulator
from gsmpm.sim import Simulator
from mpm_solver.boundary_conditions import (ColliderBC, ParticleDriverBC, StickyGroundBC,
                                            boundaryConditionTypeCallBacks, collider_bc, driver_bc, init_bc,
                                            postprocess_bc, preprocess_bc)
from mpm_solver.collider import MPM_Collider, collideTypeCallBacks
from mpm_solver.model import MPM_model, MPM_state, MPM_state_opt

_MAX_QUEUE = 1 << 14


class MPM_Simulator:
    def __init__(self, xyzs, covs, volumes, args, init_v=None):
        self.n_particles = int(xyzs.shape[0])
        self.mpm_model = MPM_model(self.n_particles, args)
        self.fitting = bool(getattr(args, "fitting", False))
        self.time = 0.0
        self.collider_params = []
        self.particle_preprocess = []
        self.grid_postprocess = []
        self.init_particles = []
        self._queue = []
        self._queue_t = []  # the clock at each queued substep (moving colliders)
        self._queue_dt = None
        if self.fitting:  # MPM_state_opt (model.py:135-223) on gsmpm_fit_*
            self._sim = None
            self._fit = FitSimulator(self.n_particles, n_grid=args.n_grid, grid_extent=args.grid_extent, levels=31,
                                     E=args.E, nu=args.nu, density=args.density, gravity=args.gravity,
                                     device=xyzs.device if xyzs.is_cuda else None)
            self._fit.set_particles(xyzs.reshape(-1, 3), covs.reshape(-1, 6), volumes.reshape(-1), init_v)
            self._fit_bc = None
            self.mpm_model._bind_fit(self)
            self.mpm_state = MPM_state_opt(self, args)
            return
        m = self.mpm_model  # the material constants: the reference's, or the config's (MPMParams)
        self._sim = Simulator(
            self.n_particles, n_grid=args.n_grid, grid_extent=args.grid_extent, material=args.material, E=args.E,
            nu=args.nu, density=args.density, gravity=args.gravity, yield_stress=float(m.yield_stress_init),
            hardening=float(m.hardening), xi=float(m.xi), plastic_viscosity=float(m.plastic_viscosity),
            friction_angle=float(m.friction_angle), jelly_fcr=bool(getattr(args, "jelly_fcr", False)),
            keep_grid=bool(getattr(args, "keep_grid", False)), phased=bool(getattr(args, "phased", False)),
            device=xyzs.device if xyzs.is_cuda else None)
        self._sim.set_particles(xyzs.reshape(-1, 3), covs.reshape(-1, 6), volumes.reshape(-1), init_v)
        self.mpm_model._bind(self)
        self.mpm_state = MPM_state(self, args)

    # ------------------------------------------------------------ stepping --
    def _mask_now(self):
        m = 0
        for pp in self.particle_preprocess:
            if pp.isActive(self.time):
                m |= 1 << pp.bit
        for gp in self.grid_postprocess:
            if not gp.isCollide and gp.isActive(self.time):
                m |= 1 << gp.bit
        return m

    def p2g2p(self, dt, s=None):
        """One substep (solver.py:27-52); queued, see module docstring.

        With fitting=True, ``p2g2p(dt, s)`` runs ``p2g2p_forward(dt, s)``:
        extra.py:207 calls it that way although the reference's ``p2g2p``
        takes only ``dt``; the intended call is used."""
        if self.fitting:
            if s is None:
                raise TypeError("p2g2p(dt) steps the forward-only state; with fitting=True use p2g2p_forward(dt, s)")
            return self.p2g2p_forward(dt, s)
        if s is not None:
            raise TypeError("p2g2p() takes 2 positional arguments but 3 were given")  # solver.py:27
        if self._queue and dt != self._queue_dt:
            self.flush()
        self._queue_dt = dt
        self._queue.append(self._mask_now())
        self._queue_t.append(self.time)
        self.time += dt  # float64 host clock, solver.py:52
        if len(self._queue) >= _MAX_QUEUE:
            self.flush()

    def flush(self):
        if self.fitting:
            return
        if self._queue:
            q, self._queue = self._queue, []
            t, self._queue_t = self._queue_t, []
            self._sim.step(float(self._queue_dt), q, t)

    def postprocess(self):
        """compute_cov_from_F + compute_R_from_F (solver.py:135-137)."""
        if self.fitting:
            raise TypeError("postprocess() reads the forward-only state; with fitting=True use postprocess_forward()")
        self.flush()
        self._sim.postprocess()

    def sh_rotations(self, A=None):
        """[N,3,3] view-direction rotations for the rasterizer's sh_rotations from the
        last postprocess(): particle_R, or A particle_R A^T when the rendered means
        are A x the simulated ones (gsmpm_mpm_sh_rotations; not in the reference)."""
        if self.fitting:
            raise TypeError("sh_rotations() reads the forward-only state's particle_R; the fitting state has none")
        return self._sim.sh_rotations(A)

    # ----------------------------------------------------------------- BCs --
    def set_boundary_conditions(self, bc_args_arr, sim_args):
        if self.fitting:
            for bc_args in bc_args_arr:
                if bc_args["type"] in collider_bc:
                    raise TypeError("collider records apply to the forward-only simulator; the fitting path "
                                    "(MPM_state_opt) has no extended colliders")
                if bc_args["type"] in driver_bc:
                    raise TypeError("particle driver records apply to the forward-only simulator; the fitting path "
                                    "(MPM_state_opt) has no particle drivers")
                bc = boundaryConditionTypeCallBacks[bc_args["type"]](self.n_particles, bc_args, sim_args)
                if bc.type in postprocess_bc:
                    self.grid_postprocess.append(bc)
                elif bc.type in preprocess_bc or bc.type in init_bc:
                    # the _opt path never applies particle_preprocess / init_particles (solver.py:54-69)
                    (self.particle_preprocess if bc.type in preprocess_bc else self.init_particles).append(bc)
            return
        for bc_args in bc_args_arr:
            bc = boundaryConditionTypeCallBacks[bc_args["type"]](self.n_particles, bc_args, sim_args)
            if bc.type in preprocess_bc:
                bc.bit = self._sim.add_impulse(bc.center, bc.size, bc.force, bc.substep_dt)
                self.particle_preprocess.append(bc)
            if bc.type in postprocess_bc:
                bc.bit = self._sim.add_fixed_cube(bc.center, bc.size)
                self.grid_postprocess.append(bc)
            if bc.type in collider_bc:
                self._add_collider_bc(bc)
            if bc.type in driver_bc:
                self._add_driver_bc(bc)
            if bc.type in init_bc:
                self.init_particles.append(bc)
        # solver.py:125-129, in list order (a later box overrides an earlier one).  An
        # additional_params record's apply() covers the reference's three steps
        # (apply, compute_mu_lam_from_E_nu, applymu) in one region call.
        for pp in self.init_particles:
            pp.apply(self.mpm_state, self.mpm_model)

    def set_bc_ground_only(self):
        bc = StickyGroundBC()
        if self.fitting:
            self.grid_postprocess.append(bc)
            return
        bc.bit = self._sim.add_fixed_cube(bc.center, bc.size)
        self.grid_postprocess.append(bc)

    def add_surface_collider(self, point, normal, surface="sticky", friction=0.0, start_time=0.0, end_time=999.0):
        point = list(point)
        scale = 1.0 / math.sqrt(float(sum(x ** 2 for x in normal)))
        normal = [scale * x for x in normal]
        cp = MPM_Collider(point, normal, friction)
        self.collider_params.append(cp)
        cl = collideTypeCallBacks["ground"](cp.point, cp.normal, cp.friction)
        if self.fitting:  # only grid_postprocess[0] runs on the fitting path (solver.py:64)
            self.grid_postprocess.append(cl)
            return
        cl.bit = self._sim.add_plane_collider(point, normal, friction)
        self.grid_postprocess.append(cl)

    def add_collider(self, shape, surface="separate", friction=0.0, damping=1.0, start_time=0.0, end_time=999.0,
                     velocity=None, move_start=None, move_end=None, angular_velocity=None, pivot=None, **geometry):
        """An extended collider (not in the reference; add_surface_collider above
        stays the legacy plane): ``shape`` "plane" (point=, normal=), "ball"
        (center=, radius=), "box" or "walls" (center=, half=); ``surface``
        "sticky", "slip" or "separate"; active on the substeps where
        start_time <= time < end_time.  Returns the descriptor (its ``bit`` is
        the library's bc id).  Same record as a ``{"type": "collider", ...}``
        entry of set_boundary_conditions.  ``velocity`` makes it a moving
        record: it translates while move_start <= time < move_end (defaults:
        start_time, end_time) on the same clock, whether active or not.
        ``angular_velocity`` makes it a rotating record: in the same window it
        also turns about ``pivot`` (default: its point or centre)."""
        if self.fitting:
            raise TypeError("add_collider applies to the forward-only simulator; the fitting path (MPM_state_opt) "
                            "has no extended colliders")
        bc = ColliderBC(self.n_particles, dict(geometry, type="collider", shape=shape, surface=surface,
                                               friction=friction, damping=damping, start_time=start_time,
                                               end_time=end_time, velocity=velocity, move_start=move_start,
                                               move_end=move_end, angular_velocity=angular_velocity, pivot=pivot))
        self._add_collider_bc(bc)
        return bc

    def _add_collider_bc(self, bc):
        self.flush()  # substeps queued so far ran without it
        bc.bit = self._sim.add_collider(bc.shape, bc.surface, bc.friction, bc.damping, **bc.geometry, **bc.motion)
        self.grid_postprocess.append(bc)

    # ---------------------------------------------------- particle drivers --
    # Records on a selection of particles chosen at the call (the rows inside
    # center / size now, or the rows of mask) and fixed from then on
    # (gsmpm_mpm_add_driver); each returns its descriptor (``bit``: the
    # library's bc id) and is the same record as a set_boundary_conditions
    # entry of that type.  Within a substep they run after every box impulse,
    # in the order they were added, before the stress.
    def add_particle_impulse(self, force, *, center=None, size=None, mask=None, start_time=0.0, end_time=None,
                             num_dt=None, substep_dt=None):
        """v += force / m * substep_dt on the selection (ImpulseBC's arithmetic;
        substep_dt is needed here, there being no sim_args)."""
        if substep_dt is None:
            raise TypeError("add_particle_impulse: substep_dt is required")
        return self._new_driver("particle_impulse", dict(force=force, substep_dt=substep_dt), center, size, mask,
                                start_time, end_time, num_dt, substep_dt)

    def enforce_particle_translation(self, velocity, *, center=None, size=None, mask=None, start_time=0.0,
                                     end_time=None, num_dt=None, substep_dt=None):
        """v = velocity on the selection (num_dt needs substep_dt)."""
        return self._new_driver("enforce_particle_translation", dict(velocity=velocity), center, size, mask,
                                start_time, end_time, num_dt, substep_dt)

    def enforce_particle_rotation(self, point, axis, omega=0.0, along=0.0, *, center=None, size=None, mask=None,
                                  start_time=0.0, end_time=None, num_dt=None, substep_dt=None):
        """v = omega * cross(axis, x - point) + along * axis on the selection
        (the axis is normalised; num_dt needs substep_dt)."""
        return self._new_driver("enforce_particle_rotation", dict(point=point, axis=axis, omega=omega, along=along),
                                center, size, mask, start_time, end_time, num_dt, substep_dt)

    def _new_driver(self, kind, params, center, size, mask, start_time, end_time, num_dt, substep_dt):
        if self.fitting:
            raise TypeError("particle drivers apply to the forward-only simulator; the fitting path (MPM_state_opt) "
                            "has no particle drivers")
        if num_dt is not None and substep_dt is None:
            raise TypeError(f"{kind}: num_dt needs substep_dt")
        from types import SimpleNamespace
        bc = ParticleDriverBC(self.n_particles, dict(params, type=kind, center=center, size=size, mask=mask,
                                                     start_time=start_time, end_time=end_time, num_dt=num_dt),
                              SimpleNamespace(substep_dt=substep_dt))
        self._add_driver_bc(bc)
        return bc

    def _add_driver_bc(self, bc):
        self.flush()  # substeps queued so far ran without it, and a box selects the positions they lead to
        bc.bit = self._sim.add_driver(bc.type, center=bc.center, size=bc.size, mask=bc.mask, **bc.params)
        self.particle_preprocess.append(bc)

    # ------------------------------------------- differentiable (fitting) --
    def _need_fit(self, name):
        if not self.fitting:
            raise AttributeError(f"{name} needs args.fitting=True (MPM_state_opt)")
        if not self.grid_postprocess:
            raise IndexError("list index out of range")  # grid_postprocess[0], solver.py:64
        bc = self.grid_postprocess[0]
        if bc is not self._fit_bc:
            if getattr(bc, "isCollide", False) or not hasattr(bc, "center"):
                raise NotImplementedError("grid_postprocess[0] must be a fixed-cube BC on the fitting path")
            self._fit.set_fixed_cube(bc.center, bc.size)
            self._fit_bc = bc

    def p2g2p_forward(self, dt, s):
        """solver.py:54-69: stress, P2G, grid update, grid_postprocess[0], G2P; level s -> s+1."""
        self._need_fit("p2g2p_forward")
        self._fit.forward(float(dt), int(s))
        self.time += dt

    def p2g2p_backward(self, dt, s):
        """solver.py:71-90: redo P2G + grid of level s, then the adjoint chain."""
        self._need_fit("p2g2p_backward")
        self._fit.backward(float(dt), int(s))

    def learn(self):
        """solver.py:92-108: clipped SGD on logE (lr 0.8) and y (lr 1.6)."""
        self._need_fit("learn")
        self._fit.learn()

    def postprocess_forward(self):
        """solver.py:167-168: compute_cov_from_F_opt (covariances from F[30])."""
        self._need_fit("postprocess_forward")
        self._fit.postprocess_forward()

    def postprocess_backward(self):
        self._need_fit("postprocess_backward")
        self._fit.postprocess_backward()

    def clear_grads(self):
        """solver.py:173-175: MPM_model.clear_grad + MPM_state_opt.clear_grad."""
        if not self.fitting:
            raise AttributeError("clear_grads needs args.fitting=True")
        self._fit.clear_grads()
