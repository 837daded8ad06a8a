/*
 * gsmpm.h -- C-ABI of the MI355X-native PhysGaussian hot path (libgsmpm.so).
 *
 * Plain C types only: device pointers are `float*`/`int32_t*` allocated by
 * the caller (e.g. torch tensors' data_ptr()), streams are `void*`
 * (hipStream_t).  Every entry point returns 0 on success or a negative
 * status; gsmpm_last_error() then holds a thread-local message.
 *
 * Each declaration names the reference interface it replaces
 * (ranrandy/gaussian-splatting-mpm @ 2024-12-18, file:line).
 */
#ifndef GSMPM_H
#define GSMPM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSMPM_OK 0
#define GSMPM_EINVAL -1
#define GSMPM_EHIP -2
#define GSMPM_ESTATE -3
#define GSMPM_ESPACE -4  /* a caller-owned workspace is too small (gsmpm_raster_forward_ws) */

/* ------------------------------------------------------------ common --- */
const char* gsmpm_last_error(void);
int gsmpm_version(void);

/* --------------------------------------------------------------- MPM ---
 * Replaces mpm_solver.MPM_Simulator (mpm_solver/solver.py:9-177) with its
 * MPM_model / MPM_state (mpm_solver/model.py:6-132).
 */
typedef struct gsmpm_mpm gsmpm_mpm;

#define GSMPM_MAT_JELLY 0
#define GSMPM_MAT_METAL 1
#define GSMPM_MAT_SAND 2
#define GSMPM_MAT_FOAM 3
/* The cohesive fluid of fluid_return_mapping (constitutive_models.py:142-213,
 * which the reference defines and never dispatches) with the StVK stress foam
 * uses.  It lives on yield_stress (never written: the fluid does not harden)
 * and plastic_viscosity; at the default yield 0.005 nearly all deviatoric
 * stress is returned every substep and the bulk response is lam.  Code 4 stays
 * private (jelly + FCR, GSMPM_FLAG_JELLY_FCR); 4, 6, 7, ... are refused. */
#define GSMPM_MAT_FLUID 5

/* flags */
#define GSMPM_FLAG_JELLY_FCR 1u   /* fix SURVEY F3: run FCR elasticity for jelly (utils.py:37-38) */
#define GSMPM_FLAG_KEEP_GRID 2u   /* keep m / m*v of the last substep readable (debug, slower) */
#define GSMPM_FLAG_NO_GRAPH 4u    /* launch substeps eagerly instead of through a cached hipGraph */
#define GSMPM_FLAG_NO_SORT 8u     /* keep particles in input order (no spatial sort) */
#define GSMPM_FLAG_PHASED 16u     /* per-phase substep (P2G, grid, G2P, binning: 4 launches) instead of the
                                     fused G2P2G pipeline (2 launches); also implied by KEEP_GRID */

/* substep pipelines (gsmpm_mpm_pipeline) */
#define GSMPM_PIPE_PHASED 0
#define GSMPM_PIPE_FUSED 1

typedef struct {
  int32_t n_particles;
  int32_t n_grid;               /* MPMParams.n_grid (arguments/__init__.py:66) */
  double grid_extent;           /* MPMParams.grid_extent */
  int32_t material;             /* GSMPM_MAT_*; model.py:24-31 */
  double E, nu, density;        /* model.py:42-44, 100-102 */
  double gravity[3];            /* model.py:32 */
  double yield_stress;          /* 0.005, model.py:55-56 */
  double hardening, xi;         /* 1, 1, model.py:57-58 */
  double plastic_viscosity;     /* 0.008, model.py:59 */
  double friction_angle_deg;    /* 25, model.py:48 */
  uint32_t flags;
} gsmpm_mpm_params;

/* MPM_Simulator.__init__ -> MPM_model.__init__ (model.py:8-22) */
int gsmpm_mpm_create(const gsmpm_mpm_params* params, gsmpm_mpm** out);
int gsmpm_mpm_destroy(gsmpm_mpm* h);

/* MPM_state.__init__ (model.py:78-122): x [N,3] grid space, cov6 [N,6]
 * (becomes particle_init_cov and particle_cov), vol [N]; v [N,3] or NULL
 * (MPM_state_opt init_vel, model.py:160-167).  Device pointers, f32. */
int gsmpm_mpm_set_particles(gsmpm_mpm* h, const float* x, const float* cov6, const float* vol,
                            const float* v_or_null, void* stream);

/* Boundary conditions (mpm_solver/boundary_conditions.py, solver.py:110-167).
 * Each returns (>=0) a bc id; ids index the bit of the per-substep activity mask.
 *   fixed_cube  -> BasicBC.apply           (boundary_conditions.py:23-27)
 *   impulse     -> ImpulseBC.apply         (boundary_conditions.py:41-45)
 *   plane       -> MPM_Collider.collide    (collider.py:13-44), always active;
 *                  normal is normalised in f64 as solver.py:153-154 does. */
int gsmpm_mpm_add_fixed_cube(gsmpm_mpm* h, const double center[3], const double size[3]);
int gsmpm_mpm_add_impulse(gsmpm_mpm* h, const double center[3], const double size[3], const double force[3],
                          double substep_dt);
int gsmpm_mpm_add_plane_collider(gsmpm_mpm* h, const double point[3], const double normal[3], double friction);

/* Extended colliders: a shape, a surface, friction, damping and an activity
 * bit.  No reference counterpart beyond the arguments that
 * add_surface_collider declares and never uses (surface, start_time,
 * end_time: "For now, not used", solver.py:140-147); the semantics are this
 * library's (DESIGN.md "Extended colliders").  Unlike the legacy plane a
 * record honours its bit of bc_active (NULL: active), so the caller can
 * switch it on and off in time.  Only nodes with mass > 1e-15 are touched;
 * records apply in table order, mixed freely with fixed cubes and legacy
 * planes; all arithmetic is f32, unfused, left to right, on the node
 * p = (i dx, j dx, k dx).  Geometry is converted to f32 here.
 *   shape     a        b                  inside the collider    normal n (out of it)
 *   PLANE     point    normal (f64-       (p - a) . n < 0        n
 *                      normalised here)
 *   BALL      centre   radius in b[0]     |p - a| < radius       (p - a) / |p - a|   (sticky where |p - a| <= 1e-20)
 *   BOX       centre   half extents       |d_x| < b_x, all x     sign(d_x*) e_x*, x* the first axis of least b_x - |d_x|
 *   WALLS     centre   half extents       |d_x| > b_x, any x     -sign(d_x) e_x for each violated axis in turn
 * Response with nc = v . n:
 *   STICKY    v = 0 (friction must be 0; damping ignored)
 *   SEPARATE  v -= min(nc, 0) n      SLIP  v -= nc n
 *   then, for both, if nc < 0 and |v| > 1e-20: v = max(0, |v| + nc friction) v / |v|; then v *= damping
 *   (WALLS: damping once, after the axis loop, if any axis fired).
 * PLANE + SEPARATE + damping 0.99f is, operation for operation,
 * gsmpm_mpm_add_plane_collider's update.
 * Returns the bc id (shared with the other BCs, at most 32), or GSMPM_EINVAL:
 * unknown shape or surface, radius or a half extent <= 0, zero normal,
 * negative friction, STICKY with friction != 0, too many BCs.  GSMPM_ESTATE,
 * with a message and nothing changed: a slab handle (and gsmpm_mpm_slab_init
 * refuses a handle that holds such records), or a handle created with
 * GSMPM_FOLD=1.  A handle without extended records launches the grid kernels
 * it always did; the first record switches it to their EXT instantiations. */
#define GSMPM_SHAPE_PLANE 0
#define GSMPM_SHAPE_BALL 1
#define GSMPM_SHAPE_BOX 2
#define GSMPM_SHAPE_WALLS 3
#define GSMPM_SURF_STICKY 0
#define GSMPM_SURF_SLIP 1
#define GSMPM_SURF_SEPARATE 2
typedef struct {
  int32_t shape, surface;  /* GSMPM_SHAPE_*, GSMPM_SURF_* */
  double a[3], b[3];       /* geometry, by shape (table above) */
  double friction;         /* Coulomb coefficient, >= 0 */
  double damping;          /* factor on v of a node the collider acted on (1: none); stored as f32 */
} gsmpm_collider;
int gsmpm_mpm_add_collider(gsmpm_mpm* h, const gsmpm_collider* collider);

/* MPM_Simulator.p2g2p (solver.py:27-52) x n_substeps.  bc_active[s] holds
 * the activity bits of substep s, decided by the caller from the f64 host
 * clock exactly as BasicBC.isActive (boundary_conditions.py:30-31); NULL =
 * all active.  Asynchronous on `stream`.  Returns GSMPM_ESTATE (and launches
 * nothing) once an earlier call's substeps produced non-finite (NaN / Inf)
 * particle state: a position, or a scatter input of P2G -- mass, velocity
 * (after an impulse), C or the stress term -- while x may still be finite
 * (SURVEY 5's per-frame check; the kernels set a sticky host-mapped word,
 * read here without a sync: the error surfaces at the call after the frame
 * that produced it, or at gsmpm_mpm_check_finite). */
int gsmpm_mpm_step(gsmpm_mpm* h, float dt, int32_t n_substeps, const uint32_t* bc_active, void* stream);

/* Moving colliders: an extended collider record (above, unchanged) that
 * translates.  No reference counterpart; the semantics are this library's
 * (DESIGN.md "Moving colliders").  The motion is a velocity w and a motion
 * window [t_start, t_end) on the caller's clock, all four stored as f32 of the
 * doubles given; t_end may be +inf.  The library keeps no clock: the caller
 * hands gsmpm_mpm_step_timed, for each substep, the time at which it decided
 * that substep's bc_active word.  On a substep whose time reads t (f32 of the
 * double), in f32, unfused, left to right, with t0 = t_start, t1 = t_end:
 *   tc = fminf(fmaxf(t, t0), t1)     tau = tc - t0
 *   c  = a + w tau                   (point of a plane, centre of ball / box / walls)
 *   wc = (t >= t0 && t < t1) ? w : 0 (the collider's velocity now)
 * so the record stands at a before t0, translates inside the window and
 * stands where it arrived from t1 on.  The inside test and the normal are
 * gsmpm_mpm_add_collider's with c in place of a (a plane keeps its normal).
 * On a node the record hits, the response acts on the relative velocity:
 *   u = v - wc;  u = response(u) (sticky u = 0; WALLS once per violated axis;
 *   damping on u as above on v);  v = u + wc.
 * A node it does not hit keeps v bit for bit.  The record's bit of bc_active
 * means what it does for a static record: an inactive record is skipped, and
 * its clock still runs (a record switched on halfway through its motion
 * window appears halfway along).  An all-zero velocity is legal and still
 * makes a moving record.
 * Returns the bc id, or GSMPM_EINVAL: everything gsmpm_mpm_add_collider
 * refuses, a non-finite velocity, a non-finite t_start, t_end NaN, t_end <
 * t_start.  GSMPM_ESTATE as gsmpm_mpm_add_collider: a slab handle (and
 * gsmpm_mpm_slab_init refuses a handle that holds such a record), a handle
 * created with GSMPM_FOLD=1.  The first moving record switches the handle to
 * the MOV instantiations of the grid kernels; a static extended record in
 * such a table gives what the EXT ones give (==). */
typedef struct {
  double velocity[3];     /* w */
  double t_start, t_end;  /* motion window [t_start, t_end) on the caller's clock */
} gsmpm_collider_motion;
int gsmpm_mpm_add_moving_collider(gsmpm_mpm* h, const gsmpm_collider* collider, const gsmpm_collider_motion* motion);
/* gsmpm_mpm_step with the caller's clock: time[s] is the clock at substep s
 * (the value it had when bc_active[s] was decided).  The times go to a small
 * device table (one f32 per substep, written on `stream` before the substeps,
 * with no host synchronisation; calls may be queued back to back), and the
 * grid kernel of substep s reads entry s: the cached step graphs do not
 * depend on time.  GSMPM_EINVAL: NULL time, a non-finite entry.  On a handle
 * without moving records it is gsmpm_mpm_step: the times are ignored, the
 * same kernels and graphs run, the results are bit-equal.  gsmpm_mpm_step on
 * a handle that holds a moving record returns GSMPM_ESTATE and launches
 * nothing; gsmpm_mpm_time_kernels and gsmpm_mpm_profile_substeps run such a
 * handle at t = 0. */
int gsmpm_mpm_step_timed(gsmpm_mpm* h, float dt, int32_t n_substeps, const uint32_t* bc_active, const double* time,
                         void* stream);
/* The step graphs the handle caches now (diagnostics). */
int gsmpm_mpm_graph_count(gsmpm_mpm* h);

/* Rotating colliders: a moving record (above, unchanged) that also turns with
 * a constant angular velocity about a pivot which travels with the body.  No
 * reference counterpart; the semantics are this library's (DESIGN.md
 * "Rotating colliders").
 * Stored at add time: w32, om32 = f32(omega), t0, t1 and piv32, each the f32
 * of the double given; wm = |omega| and the unit axis k = omega / wm, computed
 * and kept in f64 for the pose.
 * Pose on a substep whose time reads t (f32 of the double); tc, tau and the
 * moving flag are the moving record's:
 *   tc = fminf(fmaxf(t, t0), t1)     tau = tc - t0     mov = t >= t0 && t < t1
 *   theta = wm * (double)tau                                   (f64)
 *   R = I + sin(theta) K + (1 - cos(theta)) K K                (f64; K the
 *       cross-product matrix of k, K K its matrix square), each of the nine
 *       entries then rounded to f32
 *   o = piv32 + w32 * tau            (f32, unfused, per component)
 *   c = o + R (a - piv32)            (f32, unfused, row sums left to right;
 *       a is the record's point or centre)
 * Action on a massive node at p, all f32, unfused, left to right, row and
 * column sums in index order 0, 1, 2:
 *   q = p - c          d = R^T q     (the node in the body frame)
 *   r = p - o          wc = mov ? w32 + om32 x r : 0
 *       ((om32 x r)[0] = om32[1] r[2] - om32[2] r[1], and cyclically)
 *   u = R^T (v - wc)                 (the relative velocity in the body frame)
 *   the extended record acts on u with the node offset d in place of p - a
 *   and its own b (plane normal, radius, half extents): inside test, normal
 *   choice, response, friction and damping are gsmpm_mpm_add_collider's,
 *   with the box tie rule, the per-violated-axis loop of WALLS, the sticky
 *   centre of a ball and the damping applied once;
 *   where the record hit the node v = R u + wc, otherwise v keeps its bits.
 * Outside the window the record stands (wc = 0) in the pose of t0 before it
 * and in the pose of t1 from its end on.  The activity bit means what it does
 * for a moving record: the clock runs while the record is switched off.
 * Returns the bc id, or GSMPM_EINVAL: everything gsmpm_mpm_add_moving_collider
 * refuses, a non-finite omega or pivot, and an all-zero omega (use
 * gsmpm_mpm_add_moving_collider: the two are not bit-equal, and a silent
 * fallback would hide that).  GSMPM_ESTATE as gsmpm_mpm_add_moving_collider:
 * a slab handle (and gsmpm_mpm_slab_init refuses a handle that holds such a
 * record), a handle created with GSMPM_FOLD=1; gsmpm_mpm_step refuses a handle
 * that holds one; gsmpm_mpm_time_kernels and gsmpm_mpm_profile_substeps run it
 * at t = 0.  The differentiable simulator (gsmpm_fit_*) has no colliders of
 * this kind.  The first rotating record switches the handle to the ROT
 * instantiations of the grid kernels, which read one 16-float pose
 * {R[9], c[3], o[3], 0} per substep and rotating record from a table that
 * gsmpm_mpm_step_timed fills on `stream` right after the times (sin and cos
 * are evaluated there, once per substep and record, never in the grid
 * kernel); a translating or static record in such a table gives what the MOV
 * / EXT instantiations give. */
typedef struct {
  double velocity[3];     /* w, as gsmpm_collider_motion (may be all zero) */
  double t_start, t_end;  /* motion window [t_start, t_end) on the caller's clock */
  double omega[3];        /* angular velocity vector, radians per unit of that clock */
  double pivot[3];        /* a point of the axis at t_start, grid space */
} gsmpm_collider_spin;
int gsmpm_mpm_add_rotating_collider(gsmpm_mpm* h, const gsmpm_collider* collider,
                                    const gsmpm_collider_spin* spin);
/* Particle drivers: a boundary-condition record attached to a fixed SELECTION
 * of particles -- ImpulseBC with the mask its "#TODO: Need to replace this
 * with a mask" (boundary_conditions.py:43) asks for, and two records that
 * enforce a velocity on the selection.  The selection is chosen once, when
 * the record is added, and is held per caller row: a re-bin, a re-sort, a
 * permuted input or gsmpm_mpm_set_particles never changes who is selected,
 * and a particle that leaves the box it was chosen with stays driven.
 * With x, v, m the particle's values in the front of P2G (registers only:
 * G2P replaces particle_v afterwards), all arithmetic f32, unfused:
 *   PARTICLE_IMPULSE    v += force / m * substep_dt        (ImpulseBC.apply's arithmetic)
 *   ENFORCE_TRANSLATION v  = velocity                      (the f32 of the doubles given)
 *   ENFORCE_ROTATION    v  = omega * cross(axis, x - point) + along * axis
 *                       (axis normalised in f64 here and rounded once; the
 *                       axis line is invariant under the motion, so no clock)
 * Order inside a substep: the box impulses (gsmpm_mpm_add_impulse) in their
 * order, then the drivers in the order they were added, then the stress --
 * particle_preprocess (solver.py:41-42) with the drivers after the impulses;
 * a later enforce overrides an earlier kick and a later kick adds to an
 * earlier enforce.  The driven v enters the non-finite check and the P2G
 * scatter as a kicked v does.  The record takes one bc id and honours its
 * bit of bc_active (NULL: active); the caller's clock decides its window.
 * Selection: with mask == NULL the rows whose current position passes the
 * region records' strict f32 test |x - center| < size on every axis (a
 * kernel on `stream`); else mask[n] bytes on the device, caller order, non-zero
 * = selected (center / size ignored).  An empty selection is legal.  The
 * first driver allocates one uint32 word per particle (4 * capacity bytes,
 * once; bit j = the j-th driver) and switches the handle to the driver entry
 * points of its P2G kernels (k_fused_drv, k_p2g_drv and their mixed forms);
 * a handle without one launches the kernels it always did.
 * Returns the bc id, or GSMPM_EINVAL: unknown kind, a non-finite parameter,
 * a zero axis, a box size <= 0 (or a non-finite box) without a mask, too
 * many BCs.  GSMPM_ESTATE, with a message and nothing changed: a slab handle
 * (migration moves rows between ranks; gsmpm_mpm_slab_init refuses a handle
 * that holds a driver), a handle created with GSMPM_FOLD=1, particles not
 * set.  The differentiable simulator (gsmpm_fit_*) has no drivers. */
#define GSMPM_DRIVER_PARTICLE_IMPULSE 0
#define GSMPM_DRIVER_ENFORCE_TRANSLATION 1
#define GSMPM_DRIVER_ENFORCE_ROTATION 2
typedef struct {
  int32_t kind;                /* GSMPM_DRIVER_* */
  double center[3], size[3];   /* selection box (mask == NULL) */
  double force[3];             /* PARTICLE_IMPULSE */
  double substep_dt;           /* PARTICLE_IMPULSE */
  double velocity[3];          /* ENFORCE_TRANSLATION */
  double point[3], axis[3];    /* ENFORCE_ROTATION: a point of the axis, its direction (any length > 0) */
  double omega, along;         /* ENFORCE_ROTATION: angular speed about the axis, speed along it */
} gsmpm_driver;
int gsmpm_mpm_add_driver(gsmpm_mpm* h, const gsmpm_driver* driver, const uint8_t* mask_or_null /* device [n] */,
                         void* stream);
/* The selection of the driver with bc id `id`, out[n] bytes (0 / 1) on the
 * device, caller order.  GSMPM_EINVAL: no driver has that id. */
int gsmpm_mpm_get_driver_selection(gsmpm_mpm* h, int32_t id, uint8_t* out /* device [n] */, void* stream);

/* Diagnostics: synchronizes `stream` and copies the poses of the last step
 * call, out[n_substeps][n_rot][16], rotating records in table order.
 * GSMPM_ESTATE on a handle without rotating records, GSMPM_EINVAL for more
 * substeps than that call had. */
int gsmpm_mpm_get_poses(gsmpm_mpm* h, int32_t n_substeps, float* out /* [n_substeps][n_rot][16] */, void* stream);
/* Synchronizes `stream`, then GSMPM_ESTATE if any substep so far produced a
 * non-finite particle state (position, mass, velocity, C or stress; clear
 * != 0 resets the word; set_particles does too), else GSMPM_OK.  No
 * reference counterpart. */
int gsmpm_mpm_check_finite(gsmpm_mpm* h, int32_t clear, void* stream);

/* ------------------------------------------------- multi-GPU slabs ---
 * SURVEY 8(e); no reference counterpart (the reference is one device,
 * main.py:28): the substep of mpm_solver/solver.py:27-52 sharded by spatial
 * slab along grid axis 0, one rank per GPU (csrc/slab.h, gsmpm/dist.py).
 *
 * A transport moves the boundary-node partial sums (every substep) and the
 * migrating particles (every `interval` substeps) between neighbouring ranks:
 *   GSMPM_XPORT_RCCL      comm is an ncclComm_t (gsmpm_rccl_comm_init):
 *                         grouped ncclSend/ncclRecv with ranks r-1 / r+1 on
 *                         a stream of the simulator's, overlapping the
 *                         interior grid update;
 *   GSMPM_XPORT_CALLBACK  fn(user, n, peers, send, send_bytes, recv,
 *                         recv_bytes) is called on the host after the stream
 *                         is synchronised, with pinned HOST copies of the
 *                         buffers (tests: gloo, several ranks on one GPU).
 * Both sides of every pair post the same sizes in the same order. */
#define GSMPM_XPORT_NONE 0
#define GSMPM_XPORT_RCCL 1
#define GSMPM_XPORT_CALLBACK 2
typedef int (*gsmpm_exchange_fn)(void* user, int32_t n, const int32_t* peers, void* const* send,
                                 const size_t* send_bytes, void* const* recv, const size_t* recv_bytes);
typedef struct {
  int32_t kind;          /* GSMPM_XPORT_* */
  int32_t rank, world;
  void* comm;            /* ncclComm_t (RCCL) */
  gsmpm_exchange_fn fn;  /* CALLBACK */
  void* user;
} gsmpm_transport;

/* RCCL communicator for the slab exchange (ncclGetUniqueId / ncclCommInitRank
 * of the RCCL already loaded in the process, dlopen'ed -- torch's when torch
 * is imported).  id is 128 bytes: rank 0 creates it, every rank receives it
 * (e.g. torch.distributed broadcast) and calls comm_init on its own GPU. */
int gsmpm_rccl_unique_id(uint8_t id[128]);
int gsmpm_rccl_comm_init(const uint8_t id[128], int32_t rank, int32_t world, void** comm);
int gsmpm_rccl_comm_destroy(void* comm);

/* Make `h` (created with n_particles = this rank's particle CAPACITY) rank
 * `rank` of a `world`-slab domain owning grid planes [lo, hi) of axis 0;
 * particles may drift `margin` planes between migrations, which happen every
 * `interval` substeps inside gsmpm_mpm_slab_step.  Call before
 * gsmpm_mpm_slab_set_particles.  Neighbouring slabs must be >= 2*margin+2
 * planes thick. */
int gsmpm_mpm_slab_init(gsmpm_mpm* h, int32_t rank, int32_t world, int32_t lo, int32_t hi, int32_t margin,
                        int32_t interval);
/* This rank's initial particles (n <= capacity) with their global ids
 * (device int32[n]); otherwise as gsmpm_mpm_set_particles. */
int gsmpm_mpm_slab_set_particles(gsmpm_mpm* h, int32_t n, const float* x, const float* cov6, const float* vol,
                                 const float* v_or_null, const int32_t* gid, void* stream);
/* n_substeps substeps of the slab (bc masks as gsmpm_mpm_step), window
 * exchange every substep and particle migration every `interval` substeps
 * through `xp`, all on the device (with RCCL one captured graph per call:
 * counts never visit the host inside the call).  Migration payloads have a
 * fixed capacity, grown between calls; leavers beyond it stay for a later
 * migration.  Returns GSMPM_ESTATE if a particle drifted past the margin or a
 * window node outside the exchanged rect got mass (contributions were not
 * exchanged: the state is invalid) or a slab would exceed its capacity: every
 * rank's record goes to every rank at the end of the call, so all ranks return
 * it from the same call, with the same message naming the rank at fault. */
int gsmpm_mpm_slab_step(gsmpm_mpm* h, float dt, int32_t n_substeps, const uint32_t* bc_active_mask,
                        const gsmpm_transport* xp, void* stream);
/* current particle count of this rank (changes with migration) */
int gsmpm_mpm_count(gsmpm_mpm* h);
/* global ids of this rank's particles, in the order gsmpm_mpm_get returns rows */
int gsmpm_mpm_get_gid(gsmpm_mpm* h, int32_t* out, void* stream);
/* {migrations, particles migrated (sent), lo, hi, margin, interval, window planes, capacity,
 *  leavers deferred (payload full), migration payload capacity, host syncs inside
 *  gsmpm_mpm_slab_step (one per call, plus one on the first call after set_particles),
 *  step calls} */
int gsmpm_mpm_slab_stats(gsmpm_mpm* h, int64_t out12[12]);
/* The yz rect of each window that the exchange moves, agreed by the two ranks of
 * the bound at every migration: {y0, ny, z0, nz} of the lower window, then of the
 * upper one (ny = nz = 0: nothing to exchange; before the first slab_step, the
 * whole cross-section). */
int gsmpm_mpm_slab_rects(gsmpm_mpm* h, int32_t out8[8]);
/* Re-cutting the slabs ("rebalance per frame"; on by default,
 * tolerance 0.05): at the end of a step call, when the most loaded slab holds
 * more than (1 + tolerance) x the mean particle count, every rank moves the
 * bounds to the count quantiles of all ranks' base-plane histograms (the same
 * records on every rank: the same bounds), each bound staying inside its old
 * neighbouring slabs; the next call opens with the migration to them. */
int gsmpm_mpm_slab_set_rebalance(gsmpm_mpm* h, int32_t on, float tolerance);
/* This rank's weight in the re-cut (default 1; > 0): the bounds move to the
 * quantiles that give rank r the share w_r / sum(w) of the particles, and a
 * rank holding more than (1 + tolerance) x its share triggers the re-cut.  A
 * rank with other work per frame takes a smaller share: the rank that renders
 * the gathered frame (bench.py, SlabDomain.set_render_share) sets
 * w = (W s - (W - 1) r) / (W s + r) from its simulation time s at an even
 * share and its render time r (W = world size), so its sim + render matches
 * the other ranks' sim when the sim time is linear in the particle count.
 * Carried in each rank's record (the next step call's), so every rank sees
 * every weight.  No reference counterpart. */
int gsmpm_mpm_slab_set_weight(gsmpm_mpm* h, float weight);
/* The current bounds of every slab, out[world + 1] (before the first step call
 * only this rank's own two, the rest -1), and the re-cuts made so far. */
int gsmpm_mpm_slab_bounds(gsmpm_mpm* h, int32_t* out, int32_t n, int64_t* rebalances);

/* Re-sort particle storage into Morton order of the current cells now (only
 * summation order changes; rows stay in caller order).  interval >= 0 also sets
 * how many substeps gsmpm_mpm_step lets pass between automatic re-sorts
 * (0 = never; default 100).  No counterpart in the reference. */
int gsmpm_mpm_resort(gsmpm_mpm* h, int32_t interval, void* stream);

/* Fused pipeline: substeps between re-binnings of the particles into tiles
 * (at most; default 20 for stress-free materials, 25 for stress-bearing ones; any
 * value is correct -- particles that moved more than one cell
 * since their binning take a slower global path).  Fixes the spacing: the
 * adaptive choice (gsmpm_mpm_rebin_state) is turned off.  No counterpart in
 * the reference (its p2g2p has no binning, solver.py:27-52). */
int gsmpm_mpm_set_rebin_interval(gsmpm_mpm* h, int32_t substeps);
/* Fused pipeline, one domain: with GSMPM_REBIN_AUTO=1 in the environment at
 * create (off by default: DESIGN.md §3.4), the re-binnings of each step call
 * adapt to the particles' speed (gsmpm_mpm_set_rebin_interval fixes the
 * spacing again): from the fastest
 * velocity component the previous call ended with (copied to pinned memory
 * without a sync) plus what gravity adds, enough re-binnings that no
 * particle moves more than 0.8 cell between two -- a particle that leaves
 * its chunk's window (an escape) appends its stencil's tiles to the touched
 * list and scatters through the global accumulator -- and at least one per
 * rebin_interval substeps.  out3 = {rebin_interval, auto
 * (0/1), re-binnings chosen for the last call (0: from rebin_interval)};
 * *vmax (may be null) = the last fastest velocity component seen.  No
 * reference counterpart (the reference does not bin, solver.py:27-52). */
int gsmpm_mpm_rebin_state(gsmpm_mpm* h, int32_t* out3, float* vmax);
/* GSMPM_PIPE_FUSED or GSMPM_PIPE_PHASED: the pipeline gsmpm_mpm_step runs now. */
int gsmpm_mpm_pipeline(gsmpm_mpm* h);
/* 1 when the fused pipeline folds each substep's grid update into the next
 * k_fused launch (one launch per substep; a k_grid_f launch only after a
 * re-binning): GSMPM_FOLD=1 in the environment at create, off by default
 * (measured slower); 0 otherwise (the default, the per-phase
 * pipeline, slabs).  The grid update it folds is utils.py:177-183 +
 * solver.py:41-46; without escapes the results are bit-identical either way.
 * The FOLD buffers exist only on a handle created with GSMPM_FOLD=1: one for
 * which this returns 1, or a slab made from one. */
int gsmpm_mpm_folded(gsmpm_mpm* h);
/* Device memory the handle holds now, in bytes: out4 = {total, per-phase
 * pipeline's buffers, fused pipeline's buffers, FOLD buffers} (the last three
 * are parts of the total; a handle has the buffers of the pipeline it runs
 * only).  The figures are the sizes requested from hipMalloc; the driver may
 * round each allocation up.  Pinned host memory is not counted.  Buffers
 * allocated on first use (per-particle material ids, the re-sort's and the
 * slab's) count once they exist.  Makes no HIP call.  No reference counterpart. */
int gsmpm_mpm_device_bytes(gsmpm_mpm* h, uint64_t* out4);
/* Fused pipeline diagnostics: the particle scatters since set_particles (or
 * the last clear) that left their chunk's window -- they took the global
 * float-atomic path, and the next grid update evaluates every node they may
 * reach -- (particles binned outside the grid count every substep).
 * Synchronizes `stream`.  0 on the per-phase pipeline.  No reference
 * counterpart (the reference scatters every particle with atomics,
 * utils.py:89-134). */
int gsmpm_mpm_escapes(gsmpm_mpm* h, int32_t clear, int64_t* out, void* stream);

/* MPM_Simulator.postprocess (solver.py:135-137): compute_cov_from_F and
 * compute_R_from_F (utils.py:376-433). */
int gsmpm_mpm_postprocess(gsmpm_mpm* h, void* stream);

/* Field readback / write in the reference layout (Taichi to_torch shapes):
 * rows follow the caller's original particle order. */
#define GSMPM_FIELD_X 0        /* particle_xyz      [N,3]   */
#define GSMPM_FIELD_V 1        /* particle_vel      [N,3]   */
#define GSMPM_FIELD_C 2        /* particle_C        [N,3,3] */
#define GSMPM_FIELD_F_TRIAL 3  /* particle_F_trial  [N,3,3] */
#define GSMPM_FIELD_COV 4      /* particle_cov      [6N]    */
#define GSMPM_FIELD_INIT_COV 5 /* particle_init_cov [6N]    */
#define GSMPM_FIELD_R 6        /* particle_R        [N,3,3] */
#define GSMPM_FIELD_MASS 7     /* particle_mass     [N]     */
#define GSMPM_FIELD_VOL 8      /* particle_vol      [N]     */
#define GSMPM_FIELD_MU 9       /* mpm_model.mu      [N]     */
#define GSMPM_FIELD_LAM 10     /* mpm_model.lam     [N]     */
#define GSMPM_FIELD_YIELD 11   /* mpm_model.yield_stress [N] */
#define GSMPM_FIELD_MATERIAL 12 /* mpm_model.material [N]  (per-particle materials, below) */
#define GSMPM_FIELD_COUNT 13
int gsmpm_mpm_field_width(int32_t field);
int gsmpm_mpm_get(gsmpm_mpm* h, int32_t field, float* out, void* stream);
int gsmpm_mpm_set(gsmpm_mpm* h, int32_t field, const float* in, void* stream);
/* The per-Gaussian SH view-direction rotations (gsmpm_raster_args.sh_rotations)
 * that belong to the last gsmpm_mpm_postprocess: out [N,9] row-major, in the
 * caller's original particle order as gsmpm_mpm_get.  A == NULL: particle_R
 * unchanged (bit-equal to gsmpm_mpm_get(GSMPM_FIELD_R)).  Otherwise
 * A particle_R A^T, A (host, row-major) the 3x3 with means_render = A
 * means_world, as apply_inverse_rotations applies the scene's rotation
 * matrices: the polar rotation of the A-conjugated F is the conjugated
 * rotation, so this is the Q of render-space means.  particle_R = R^T, see
 * gsmpm_raster_args.  No reference counterpart (the reference
 * computes particle_R and never reads it).  Asynchronous on `stream`.
 * GSMPM_ESTATE before the first postprocess since the particles were set, and
 * on a slab handle of a multi-GPU domain (not supported). */
int gsmpm_mpm_sh_rotations(gsmpm_mpm* h, const float A[9], float* out, void* stream);

/* Per-particle materials (the reference's f32 model.material, dispatched per
 * particle by compute_stress_from_F_trial, utils.py:13-54).  A handle is
 * uniform (one material, chosen at create) until it enters MIXED mode:
 *   - gsmpm_mpm_set(GSMPM_FIELD_MATERIAL) stores the floats as given (caller
 *     order) and enters mixed mode; no host sync, no check that they differ;
 *   - gsmpm_mpm_set_region_material enters it too.
 * In mixed mode the stress of each particle follows its own value as the
 * reference's comparisons read it: == 1 metal, == 2 sand, == 3 foam, and
 * == 5 fluid (GSMPM_MAT_FLUID; the reference has no such comparison -- this
 * is the one value whose meaning differs from its `else`); anything else (0,
 * 4, 7, other numbers, non-integers, NaN) is the `else` branch, F = F_trial
 * with the jelly rule of the handle (zero stress as written, SURVEY F3, or FCR
 * when created with GSMPM_FLAG_JELLY_FCR).  The re-binning interval takes the
 * stress-bearing default unless the caller set one.  gsmpm_mpm_get works on
 * any handle; a uniform one returns the create-time code in every row.
 * On a mixed handle metal rows run the reference's own SVD sequence
 * (correctly rounded square roots, a second SVD of the returned F for the
 * stress) where a uniform metal handle runs a refined-rsqrt SVD and reuses its
 * factors: a scene salted particle by particle needs it to stay within the
 * parity bounds.  So a metal particle's results differ in the last bits
 * between a mixed and a uniform handle, and the mixed kernel costs more
 * (k_fused, lego 100k, every id metal: 33.9 us against 22.8 us a launch).
 * Which bodies take that exact form is the build-time GSMPM_MIXED_EXACT, one
 * bit per kernel code (default 0x2: metal; bit 5 is the fluid's, clear, so a
 * fluid row runs the uniform fluid kernel's body bit for bit).
 * Mixed mode lasts until gsmpm_mpm_set_particles, which resets the ids to the
 * create-time material as it re-initialises mu / lam / yield.
 * Not supported (GSMPM_ESTATE, nothing launched, the message says why): a
 * slab handle, GSMPM_FOLD=1, and gsmpm_mpm_slab_init on a mixed handle.  The
 * differentiable simulator (gsmpm_fit_*) has one material. */
/* 0 uniform, 1 mixed */
int gsmpm_mpm_material_mode(gsmpm_mpm* h);
/* The region records of boundary_conditions.py:47-85 as their plain intent
 * (the reference raises before either takes effect).  Both run the
 * impulse's box test, fabsf(x - center) < size on all three axes, strict, in
 * f32, on the particles' current positions; asynchronous on `stream`; applied
 * in call order, so a later box overrides an earlier one.
 * set_region_material (modify_material): rows inside get `material`
 *   (GSMPM_MAT_*, else GSMPM_EINVAL); enters mixed mode.
 * set_region_params (additional_params): rows inside get mu and lam from E
 *   and nu by the path create takes (model.py:41-44, utils.py:349-362: the
 *   create-time E and nu reproduce the create-time mu / lam bit for bit),
 *   mass = f32(density) * vol, and then mu = mu_override unless that is
 *   exactly 1000, the reference's sentinel (boundary_conditions.py:69).  Does
 *   not by itself enter mixed mode.  Needs E > 0 and 0 < nu < 0.49 (the
 *   logit of nu the create path takes, else GSMPM_EINVAL) and particles set;
 *   refused on a slab handle (GSMPM_ESTATE: the positions and planes there
 *   are one rank's share, and the box would have to be applied on every rank
 *   before the first migration).
 * Both need gsmpm_mpm_set_particles first (GSMPM_ESTATE otherwise). */
int gsmpm_mpm_set_region_material(gsmpm_mpm* h, const double center[3], const double size[3], int32_t material,
                                  void* stream);
int gsmpm_mpm_set_region_params(gsmpm_mpm* h, const double center[3], const double size[3], double E, double nu,
                                double density, double mu_override, void* stream);

/* Grid readback [n^3] / [n^3,3] (grid_mass / grid_v_in / grid_v_out,
 * model.py:117-121).  mass and v_in need GSMPM_FLAG_KEEP_GRID. */
#define GSMPM_GRID_MASS 0
#define GSMPM_GRID_V_IN 1
#define GSMPM_GRID_V_OUT 2
int gsmpm_mpm_get_grid(gsmpm_mpm* h, int32_t which, float* out, void* stream);

/* Fused frame output (main.py:310-313 + render_frame 139-146), f32 as torch does it:
 * means_out[N,3] = (x - extent/2)/s + c            (grid2world, transform_utils.py:18-21)
 *                  and, if render_space != 0, then c + (means - 1)/1.0
 *                  (undoshift2center111 + undotransform2origin with scale 1.0);
 * cov_out[N,6]   = cov / (s*s).   Rows in original particle order. */
int gsmpm_mpm_world_outputs(gsmpm_mpm* h, float scale, const float center[3], int32_t render_space,
                            float* means_out, float* cov_out, void* stream);

/* Measurement: run n substeps eagerly on `stream`, each kernel launched with
 * hipExtLaunchKernel start/stop events (stamped by its own dispatch, the
 * interval rocprofv3 reports); kernel_ms[0..3] = summed time of k_p2g,
 * k_grid, k_g2p and the binning (k_finish_bins, or k_scan_tiles..k_scatter)
 * -- for the fused pipeline {k_fused, k_grid_f, binning + the re-binning
 * permute, the number of k_grid_f launches (one per substep; folded: one per
 * re-binning)}.
 * Synchronises `stream`. */
int gsmpm_mpm_profile_substeps(gsmpm_mpm* h, float dt, int32_t n_substeps, const uint32_t* bc_active,
                               float* kernel_ms, void* stream);
/* Measurement: average duration (ms) of one launch of k_p2g, k_grid, k_g2p
 * and the binning, each launched `reps` times back to back between two
 * hipEvents on `stream` (so event overhead is amortised); the launches use the
 * current substep's inputs (BC mask `bc_active`).  Fused pipeline: {k_fused
 * (G2P + P2G), k_grid_f, binning, 0}.  Particle state and bins are
 * restored afterwards.  Synchronises `stream`. */
int gsmpm_mpm_time_kernels(gsmpm_mpm* h, float dt, uint32_t bc_active, int32_t reps, float* ms4, void* stream);
/* Diagnostics of the tile buckets the next substep reads: {active tiles, max
 * particles in a tile, particles outside the grid, chunks, touched tiles (owned
 * by the next grid update), binned total, parity, substeps since the last
 * re-sort}.  Synchronises `stream`. */
int gsmpm_mpm_debug_stats(gsmpm_mpm* h, int32_t* out8, void* stream);
/* Workgroup timelines of the last k_p2g / k_g2p / k_finish_bins launches:
 * out[4][8192][8] phase stamps in s_memrealtime ticks (100 MHz).  Diagnostics. */
int gsmpm_debug_stamps(uint64_t* out, void* stream);
/* Node box (lo[3], hi[3]) of the tiles the next grid update owns; synchronises `stream`. */
int gsmpm_mpm_live_box(gsmpm_mpm* h, int32_t* box6, void* stream);

/* Device 3x3 SVD (the ti.svd restatement used by the constitutive kernels) on
 * n row-major matrices: A[n*9] -> U[n*9], sig[n*3], V[n*9].  Test entry point. */
int gsmpm_svd3(const float* A, int32_t n, float* U, float* sig, float* V, void* stream);

/* Constitutive step alone (compute_stress_from_F_trial, utils.py:13-54) on n
 * particles: F_trial[n*9], mu[n], lam[n], yield[n] (updated in place for
 * metal) -> F[n*9] (return-mapped), tau[n*9] (symmetrised Kirchhoff stress).
 * material: GSMPM_MAT_* (5 = GSMPM_MAT_FLUID, at plastic_viscosity 0.008), or
 * 4 = jelly with FCR (F3 fixed).  Test entry point. */
int gsmpm_constitutive(int32_t material, const float* F_trial, int32_t n, const float* mu, const float* lam,
                       float* yield, float dt, float* F_out, float* tau_out, void* stream);
/* The same with a material value per row (material[n], read as mixed mode
 * reads it, == 5 fluid included); jelly_fcr != 0: the `else` rows take FCR.
 * yield is written for metal rows only.  Test entry point of the mixed dispatch. */
int gsmpm_constitutive_mixed(const float* material, const float* F_trial, int32_t n, const float* mu,
                             const float* lam, float* yield, float dt, int32_t jelly_fcr, float* F_out,
                             float* tau_out, void* stream);

/* get_particle_volume (internel_filling/filling.py:27-42): vol[N] from
 * x[N,3] (grid space) with an n^3 i32 count grid in `scratch` (>= 4*n^3 B). */
int gsmpm_particle_volume(const float* x, int32_t n, int32_t n_grid, double grid_extent, int32_t* scratch,
                          float* vol_out, void* stream);

/* ------------------------------------------------- interior filling ---
 * The first half of PhysGaussian's internal-filling pass (fill_particles,
 * internel_filling/filling.py): new particles inside a hollow shell of
 * Gaussians.  No handle: the caller owns one workspace of
 * gsmpm_fill_workspace_size bytes (256-byte aligned) that carries the grids
 * from gsmpm_fill_interior to gsmpm_fill_emit / gsmpm_fill_get_grid, which
 * take the same params.  Semantics, the fixed-point quantum and the hash are
 * in DESIGN.md "Interior filling".  The fill grid is its own: n_grid here is
 * independent of the simulation's.  Linear cell = (i * n + j) * n + l for
 * cell (i, j, l) = floor(x / dx) per axis. */
typedef struct {
  int32_t n_grid;             /* 4..512 */
  double grid_extent;         /* > 0 */
  double density_threshold;   /* > 0; occupied = density > threshold */
  int32_t support;            /* 0..16: largest stamp half-width in cells */
  int32_t min_hits;           /* 1..6 of the six axis directions must meet an occupied cell */
  int32_t parity_dir;         /* -1 off; 0..5 = +x -x +y -y +z -z: the occupied runs met that way must be odd */
  int32_t per_cell;           /* 1..8 particles per interior cell */
  uint32_t seed;
  int32_t use_box;            /* != 0: only cells whose centre lies in [lo, hi] (grid space) */
  float lo[3], hi[3];
  int64_t capacity;           /* gsmpm_fill_emit writes at most this many particles */
} gsmpm_fill_params;

int gsmpm_fill_workspace_size(const gsmpm_fill_params* p, uint64_t* bytes);
/* Density, occupied and interior masks and the emission offsets from x [N,3]
 * (grid space), cov6 [N,6] (gsmpm_mpm_set_particles' layout), opacity [N].
 * *total: particles the interior cells emit (per_cell each), whatever the
 * capacity; *skipped: particles left out (non-finite value, opacity outside
 * [0, 1], cell outside the grid).  Synchronises the stream once. */
int gsmpm_fill_interior(const gsmpm_fill_params* p, const float* x, const float* cov6, const float* opacity, int64_t n,
                        void* ws, uint64_t ws_bytes, int64_t* total, int64_t* skipped, void* stream);
/* out_pos [min(total, capacity), 3]: the particles in linear-cell order, then
 * k; nothing beyond is written. */
int gsmpm_fill_emit(const gsmpm_fill_params* p, const void* ws, uint64_t ws_bytes, float* out_pos, void* stream);
/* index[q] = the source nearest to query q (exact, f32 d2 = (dx*dx + dy*dy) +
 * dz*dz, lowest index among equals). */
int gsmpm_fill_nearest(const float* query, int64_t n_query, const float* source, int64_t n_source, int32_t* index,
                       void* stream);
#define GSMPM_FILL_DENSITY 0        /* f32 [n^3] = fixed-point sum * 2^-24 */
#define GSMPM_FILL_OCCUPIED 1       /* u8  [n^3] */
#define GSMPM_FILL_INTERIOR 2       /* u8  [n^3] */
#define GSMPM_FILL_BITS 3           /* u16 [n^3]: bit d = direction d meets an occupied cell, bit 8+d = run parity */
#define GSMPM_FILL_DENSITY_FIXED 4  /* u64 [n^3]: the fixed-point sums themselves */
int gsmpm_fill_get_grid(const gsmpm_fill_params* p, const void* ws, uint64_t ws_bytes, int32_t which, void* out,
                        void* stream);

/* ------------------------------------------------ differentiable MPM ---
 * Replaces MPM_Simulator with args.fitting=True (solver.py:54-108,131-133,
 * 167-177) over MPM_model's logE/y/mu/lam (model.py:35-44) and
 * MPM_state_opt (model.py:135-223): L state levels of x, v, F, stress, C
 * (level s+1 = substep s of level s), adjoints of all of them, the dense grid
 * and its adjoints.  Same numerics and the same accumulation behaviour as
 * Taichi's reverse mode on those kernels.
 */
typedef struct gsmpm_fit gsmpm_fit;

typedef struct {
  int32_t n_particles;
  int32_t n_grid;               /* MPMParams.n_grid */
  double grid_extent;
  int32_t levels;               /* 31 in the reference (model.py:145-149) */
  double E, nu, density;        /* logE = log10 E, y = -log(0.49/nu - 1) (model.py:41-43) */
  double gravity[3];
} gsmpm_fit_params;

int gsmpm_fit_create(const gsmpm_fit_params* p, gsmpm_fit** out);
int gsmpm_fit_destroy(gsmpm_fit* h);
/* MPM_state_opt.__init__ + init2 (model.py:150-187): xyz [N,3], cov6 [N,6],
 * vol [N], init_v [N,3] (NULL = 0) as level 0; F[0] = I, C[0] = stress[0] = 0;
 * mass = density * vol; mu/lam from logE/y (model.py:44). */
int gsmpm_fit_set_particles(gsmpm_fit* h, const float* xyz, const float* cov6, const float* vol,
                            const float* init_v, void* stream);
/* grid_postprocess[0] as a fixed cube (set_bc_ground_only, solver.py:131-133,
 * StickyGroundBC boundary_conditions.py:88-95 = center (1,0.6,1), size (1,0.1,1)). */
int gsmpm_fit_set_fixed_cube(gsmpm_fit* h, const double center[3], const double size[3]);
/* p2g2p_forward(dt, s), solver.py:54-69: level s -> level s+1. */
int gsmpm_fit_forward(gsmpm_fit* h, float dt, int32_t s, void* stream);
/* p2g2p_backward(dt, s), solver.py:71-90. */
int gsmpm_fit_backward(gsmpm_fit* h, float dt, int32_t s, void* stream);
/* postprocess_forward / _backward, solver.py:167-171 (compute_cov_from_F_opt, utils.py:435-467) */
int gsmpm_fit_postprocess_forward(gsmpm_fit* h, void* stream);
int gsmpm_fit_postprocess_backward(gsmpm_fit* h, void* stream);
/* MPM_state_opt.set_grads (model.py:192-202): xyz_grad [N,3] -> x.grad[L-1], cov_grad [6N] -> cov.grad */
int gsmpm_fit_set_grads(gsmpm_fit* h, const float* xyz_grad, const float* cov_grad, void* stream);
int gsmpm_fit_learn(gsmpm_fit* h, void* stream);        /* solver.py:92-108 */
int gsmpm_fit_cycle_init(gsmpm_fit* h, void* stream);   /* model.py:216-223 */
int gsmpm_fit_clear_grads(gsmpm_fit* h, void* stream);  /* solver.py:173-175 */
int gsmpm_fit_mu_lam(gsmpm_fit* h, void* stream);       /* compute_mu_lam_from_E_nu, utils.py:349-362 */

/* Fields, external particle order; leveled ones take `level`, the rest ignore it. */
#define GSMPM_FIT_X 0          /* particle_xyz[level]    [N,3] */
#define GSMPM_FIT_V 1          /* particle_vel[level]    [N,3] */
#define GSMPM_FIT_F 2          /* particle_F[level]      [N,9] */
#define GSMPM_FIT_C 3          /* particle_C[level]      [N,9] */
#define GSMPM_FIT_STRESS 4     /* particle_stress[level] [N,9] */
#define GSMPM_FIT_GX 5         /* .grad of the above, same shapes */
#define GSMPM_FIT_GV 6
#define GSMPM_FIT_GF 7
#define GSMPM_FIT_GC 8
#define GSMPM_FIT_GSTRESS 9
#define GSMPM_FIT_LOGE 10      /* [N] */
#define GSMPM_FIT_Y 11
#define GSMPM_FIT_MU 12
#define GSMPM_FIT_LAM 13
#define GSMPM_FIT_GLOGE 14
#define GSMPM_FIT_GY 15
#define GSMPM_FIT_GMU 16
#define GSMPM_FIT_GLAM 17
#define GSMPM_FIT_COV 18       /* particle_cov [N,6] */
#define GSMPM_FIT_GCOV 19
#define GSMPM_FIT_INIT_COV 20
#define GSMPM_FIT_VOL 21
#define GSMPM_FIT_MASS 22
#define GSMPM_FIT_FIELD_COUNT 23
int gsmpm_fit_field_width(int32_t field);
int gsmpm_fit_get(gsmpm_fit* h, int32_t field, int32_t level, float* out, void* stream);
int gsmpm_fit_set(gsmpm_fit* h, int32_t field, int32_t level, const float* in, void* stream);
/* Dense grid of the last substep: GSMPM_GRID_MASS [n^3], _V_IN / _V_OUT [n^3,3],
 * and 3 / 4 for grid_v_in.grad / grid_v_out.grad [n^3,3]. */
int gsmpm_fit_get_grid(gsmpm_fit* h, int32_t which, float* out, void* stream);

/* -------------------------------------------------------- rasterizer ---
 * Replaces diff_gaussian_rasterization._C.rasterize_gaussians (forward;
 * called via GaussianRasterizer.forward at main.py:148-156).  Upstream
 * third-party, pre-2024 API; not vendored in the reference.
 */
typedef struct gsmpm_raster gsmpm_raster;

typedef struct {
  int32_t P;                 /* number of Gaussians */
  int32_t D;                 /* sh degree */
  int32_t M;                 /* SH coefficients per Gaussian (shs.size(1)), 0 if colors_precomp */
  int32_t W, H;
  const float* means3D;      /* [P,3] */
  const float* shs;          /* [P,M,3] or NULL */
  const float* colors_precomp; /* [P,3] or NULL */
  const float* opacities;    /* [P] */
  const float* scales;       /* [P,3] or NULL */
  const float* rotations;    /* [P,4] or NULL */
  const float* cov3D_precomp;/* [P,6] or NULL */
  float scale_modifier;
  const float* viewmatrix;   /* [4,4] (transposed world->view, as upstream) */
  const float* projmatrix;   /* [4,4] */
  const float* campos;       /* [3] */
  const float* bg;           /* [3] */
  float tanfovx, tanfovy;
  int32_t prefiltered;
  const float* sh_rotations; /* [P,9] row-major or NULL */
  float* aux_depth;          /* [H,W] or NULL (output) */
  float* aux_alpha;          /* [H,W] or NULL (output) */
} gsmpm_raster_args;
/* sh_rotations (no counterpart in the reference, which computes particle_R
 * and renders the harmonics unrotated; PhysGaussian shades a
 * Gaussian carried through a local rotation R with f_t(d) = f_0(R^T d)):
 * one 3x3 Q per Gaussian.  The forward forms d = (mean - campos) / |mean -
 * campos| as always, then evaluates the SH polynomial, the +0.5, the clamp
 * and the clamp bits at d' = Q d (d'_i = sum_j Q[i][j] d_j).  No
 * renormalisation and no orthogonality check: the caller owns Q.  The
 * physical choice is Q = particle_R: the project stores particle_R =
 * (U V^T)^T = R^T (utils.py:376-398), so Q d = R^T d; for render-space means
 * gsmpm_mpm_sh_rotations conjugates it.  NULL is the behaviour without the
 * option, on the kernels that ran before it existed.  With colors_precomp it
 * is GSMPM_EINVAL ("sh_rotations needs shs", before any launch); with
 * sh_degree 0 it is accepted and has no effect.  All three forward forms
 * honour it; the async form bakes the pointer into a captured graph like the
 * others. */
/* aux_depth, aux_alpha (not in the pre-2024 upstream API, which returns colour
 * and radii only): two optional per-pixel maps of the forward, caller-owned
 * device memory, [H,W] f32 each, independent of each other; NULL is off.  A
 * pixel's blend takes, skips and stops on Gaussians exactly as for the colour
 * (power > 0 and alpha < 1/255 skip, T < 1e-4 stop, front to back); over the
 * contributors i it takes,
 *   aux_depth = sum_i z_i alpha_i T_i   (z_i: the f32 view-space depth the
 *               preprocess stores and the Gaussians are ordered by; NOT
 *               normalised, and the background adds nothing),
 *   aux_alpha = 1 - T_final.
 * A pixel no Gaussian reaches has 0 in both (P = 0 and K = 0 included); the
 * normalised depth aux_depth / aux_alpha is the caller's to form.  Every pixel
 * of a requested map is written whenever out_color is (so not on GSMPM_ESPACE;
 * an async frame whose flags are set has maps as invalid as its colour).
 * Their gradients go in through gsmpm_raster_backward_aux (dL_ddepth,
 * dL_dalpha); every backward ignores the two fields themselves, and a context
 * that is not forward-only records the same final T and last contributor with
 * or without them, so its colour backward is unchanged.  The workspace and
 * async forms stay forward-only.  Both NULL is the
 * behaviour without the option, on the kernels that ran before it existed
 * (k_render<false>); otherwise k_render<true> runs, and out_color and
 * out_radii are bit-identical either way.  All three forward forms honour the
 * pointers; the async form bakes them into a captured graph like the others.
 * gsmpm_raster_workspace_size does not depend on them. */

int gsmpm_raster_create(gsmpm_raster** out);
int gsmpm_raster_destroy(gsmpm_raster* r);
/* out_color [3,H,W] f32, out_radii [P] i32 (device).  *num_rendered gets K.
 * The binning buffers grow inside the context (not graph-capturable: the
 * upstream forward also syncs on num_rendered). */
int gsmpm_raster_forward(gsmpm_raster* r, const gsmpm_raster_args* a, float* out_color, int32_t* out_radii,
                         int32_t* num_rendered, void* stream);
/* Replaces _C.rasterize_gaussians_backward (upstream's _RasterizeGaussians.backward,
 * used by extra.py's loss.backward(), extra.py:198-200,218).  Uses the state of
 * the last gsmpm_raster_forward on this context (same args; keep one context
 * per differentiable forward).  dL_dcolor [3,H,W]; outputs, all [P,...] and
 * fully written: dL_dmeans2D [P,3] (w.r.t. NDC, z = 0), dL_dcolors [P,3],
 * dL_dopacity [P], dL_dmeans3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3] (if
 * shs), dL_dscales [P,3] and dL_drotations [P,4] (if scales/rotations). */
int gsmpm_raster_backward(gsmpm_raster* r, const gsmpm_raster_args* a, const int32_t* radii, const float* dL_dcolor,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                          float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, void* stream);
/* The same with dL_dsh_rotations [P,9] (may be NULL; needs a->sh_rotations),
 * fully written: with g' = dL/dd' from the polynomial's derivative at d' = Q d,
 * dL/dQ[i][j] = g'_i d_j (zeros for culled Gaussians and clamped channels),
 * dL_dsh uses the basis at d', and dL/dd = Q^T g' enters dL_dmeans3D.
 * gsmpm_raster_backward forwards here with NULL. */
int gsmpm_raster_backward_rot(gsmpm_raster* r, const gsmpm_raster_args* a, const int32_t* radii,
                              const float* dL_dcolor, float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                              float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                              float* dL_drotations, float* dL_dsh_rotations, void* stream);
/* The same with the gradients of the two maps of the forward (aux_depth,
 * aux_alpha above): dL_ddepth = dL/dD and dL_dalpha = dL/dA, [H,W] f32 each,
 * either may be NULL (= zero).  Over a pixel's contributors i, with T_i the
 * transmittance in front of i and S^D_i the depth blended behind it,
 *   dL/dz_i     += alpha_i T_i dL/dD,
 *   dL/dalpha_i += T_i (z_i - S^D_i) dL/dD + T_final / (1 - alpha_i) dL/dA
 * (the alpha map enters as a background of -dL/dA), and z_i = vm[2] x + vm[6] y
 * + vm[10] z + vm[14] adds (vm[2], vm[6], vm[10]) sum dL/dz_i to dL_dmeans3D;
 * z_i is the f32 view depth the forward stored.  Upstream's conventions hold
 * (the 0.99 clamp is straight-through; no gradient to the camera matrices).
 * Uses the state of the context's last forward whether or not that forward
 * wrote the maps (a->aux_depth / aux_alpha are ignored here).  Outputs and
 * their rules as gsmpm_raster_backward_rot, which forwards here with both
 * NULL: then the kernels of the colour backward run (k_render_bwd<false>) and
 * the result is bit-identical to it; with a map gradient k_render_bwd<true>
 * and the matching k_preprocess_bwd run.  A forward-only context fails;
 * P = 0 returns GSMPM_OK and writes nothing; a frame that bins no pair writes
 * zeros. */
int gsmpm_raster_backward_aux(gsmpm_raster* r, const gsmpm_raster_args* a, const int32_t* radii,
                              const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                              float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                              float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                              float* dL_dsh_rotations, void* stream);
/* Forward-only context (on != 0): gsmpm_raster_forward skips the per-pixel
 * state (final T, last contributor: 8 B a pixel) that only a backward reads,
 * and gsmpm_raster_backward on it fails.  Used for main.py's frames
 * (main.py:148-157 never differentiates); autograd forwards use contexts
 * with it off (the default). */
int gsmpm_raster_set_forward_only(gsmpm_raster* r, int32_t on);
/* Caller-owned workspace form of the forward (upstream's
 * RasterizeGaussiansCUDA takes torch byte tensors for its geometry / binning /
 * image buffers, rasterize_points.cu).  gsmpm_raster_workspace_size: the
 * bytes a forward of P Gaussians into an H x W image needs when the frame
 * bins at most `pairs` (Gaussian, tile) pairs (pairs = 0: the part that does
 * not depend on the pair count).  gsmpm_raster_forward_ws: the forward with
 * every buffer carved from `workspace` (device memory, 256-byte aligned,
 * ws_bytes long, ZERO-FILLED ONCE when created: the hand-written depth order
 * keeps its bucket state at the workspace's start and leaves it zero after
 * every call); no allocation inside, forward-only (no backward state).
 * The pair count is known only after the binning scan (upstream resizes its
 * binning buffer at that point): when the frame needs more pairs than the
 * workspace holds, the call returns GSMPM_ESPACE with *pairs_needed set,
 * out_color and num_rendered unwritten, and out_radii possibly overwritten
 * (k_preprocess runs before the count is known); the depth-order kernels may
 * still be queued on `stream` at return (they leave the workspace's state
 * zero), so the old workspace must not be freed for reuse by another stream
 * before `stream` reaches that point.  The caller sizes a larger workspace
 * for that many pairs and calls again. */
int gsmpm_raster_workspace_size(int32_t P, int32_t H, int32_t W, int64_t pairs, uint64_t* bytes);
int gsmpm_raster_forward_ws(const gsmpm_raster_args* a, float* out_color, int32_t* out_radii,
                            int32_t* num_rendered, void* workspace, uint64_t ws_bytes, int64_t* pairs_needed,
                            void* stream);
/* The forward with the pair count left on the device (the round-4 verdict's
 * item 4: upstream and gsmpm_raster_forward_ws read it on the host to size
 * the binning, main.py:148-156).  The pair buffers are carved for pairs_cap
 * pairs (the workspace must hold gsmpm_raster_workspace_size(P, H, W,
 * pairs_cap), else GSMPM_ESPACE before any launch); every launch size is
 * fixed by P, H, W and pairs_cap, the kernels cut at the device's count, and
 * nothing waits on the host: the call only enqueues on `stream`, and the
 * sequence can be captured into a graph and replayed (the argument pointers
 * are baked in).  When the stream reaches the end, counts (device-accessible:
 * host-mapped pinned or device memory, 4 words) holds {K, num_rendered,
 * flags, internal}: flags bit 0 = a depth bucket above 8,192 Gaussians (the hand-
 * written order needs its LSD fallback, which this form does not take), bit 1
 * = K > pairs_cap (the emission stopped at pairs_cap).  Either bit means
 * out_color is not the frame: render it again with gsmpm_raster_forward_ws
 * (or with pairs_cap >= K).  The default depth-ordered path with the chunked
 * tile sort only (<= 4,096 tiles: the lego camera's 2,500); more tiles or an
 * A/B switch that selects another path: GSMPM_EINVAL. */
int gsmpm_raster_forward_async(const gsmpm_raster_args* a, float* out_color, int32_t* out_radii, void* workspace,
                               uint64_t ws_bytes, int64_t pairs_cap, uint32_t* counts, void* stream);

/* In-frame timing of the forwards (diagnostics; process-wide).  With timing
 * on, every forward not issued into a stream capture records three events on
 * its stream (entry, before and after k_render); gsmpm_raster_timing waits
 * for the forwards recorded since the last call and returns the sums of
 * their k_render and whole-forward times (ms) and their count.  Replaces
 * nothing in the reference (upstream has no timing); bench.py reports
 * k_render's in-frame average with it. */
int gsmpm_raster_set_timing(int32_t on);
int gsmpm_raster_timing(double* k_render_ms, double* forward_ms, int64_t* forwards);
/* Diagnostics of the context's last forward: *binned = the (Gaussian, tile)
 * pairs actually sorted and listed (each Gaussian binned into the tiles its
 * alpha >= 1/255 box reaches, a subset of the 3-sigma rect), *rendered = its
 * num_rendered (upstream's 3-sigma pair count).  Either pointer may be null. */
int gsmpm_raster_pair_counts(const gsmpm_raster* r, uint32_t* binned, uint32_t* rendered);
/* Diagnostics of the context's last hand-written depth order (csrc/dsort.h):
 * out8 = {buckets, occupied buckets sorted by a wave, by a workgroup, largest
 * bucket, overflow flag, visible Gaussians, fallbacks so far (a bucket above
 * 8,192 entries: the LSD form instead), shift}. */
int gsmpm_raster_dsort_stats(const gsmpm_raster* r, int64_t out8[8]);
/* GaussianRasterizer.markVisible -> _C.mark_visible: visible[P] (u8) = view z > 0.2 */
int gsmpm_raster_mark_visible(const float* means3D, int32_t P, const float* viewmatrix, const float* projmatrix,
                              uint8_t* visible, void* stream);

/* ---- export: a deformed state back to the 3DGS file format's parameters (csrc/export.hip) ----
 * The file format holds a Gaussian as three log-scales, a quaternion and SH
 * coefficients; the simulator ends a frame with a full covariance F Sigma F^T
 * (gsmpm_mpm_world_outputs) and a view-direction rotation Q
 * (gsmpm_mpm_sh_rotations).  These two device passes produce the former from
 * the latter.  Not in the reference (its --save_pcd writes the moved means
 * only).  Both only enqueue on `stream`.  Arguments are validated before any
 * HIP call: n < 0, D outside 0..3, M < (D+1)^2 or, with n > 0, a null
 * required pointer is GSMPM_EINVAL; n == 0 is GSMPM_OK with nothing launched
 * (the arrays of an empty set may be null).
 *
 * gsmpm_cov_to_scale_rot: cov6 [n,6] (xx, xy, xz, yy, yz, zz) -> log_scale
 * [n,3], quat [n,4] = (w, x, y, z), unit length, w >= 0 (the convention of
 * GaussianModel's build_rotation), with
 *     R(quat) diag(exp(2 log_scale)) R(quat)^T = cov
 * from a float64 cyclic Jacobi eigen-solve (fixed sweep count).  The scales
 * come out in descending order and R is a proper rotation (det +1), so the
 * result is a function of the row alone.  Eigenvalues are clamped from below
 * at max(1e-14 * lambda_max, 1e-36) before the log, so every log_scale is
 * finite for any finite row (rank-deficient, zero, slightly indefinite from
 * f32 rounding).  A row with a NaN or Inf entry gets the identity quaternion
 * and the floor scale 0.5 log(1e-36) and adds one to *n_bad (device memory,
 * may be NULL; the kernel adds, the caller zeroes).
 *
 * gsmpm_sh_rotate: shs [n,M,3], Q [n,3,3] row-major, degree D with
 * M >= (D+1)^2 -> out [n,M,3] with
 *     sh(D, out_p, d) = sh(D, shs_p, Q_p d)   for every unit d,
 * sh the rasterizer's SH polynomial (its signs and constants), Q d the
 * product gsmpm_raster_args.sh_rotations forms: evaluating out without
 * sh_rotations renders what shs renders with them.  Exact (to rounding) for
 * orthogonal Q; for a Q that is off orthogonal by delta the two sides differ
 * by O(delta |shs|), as Y_l(Q d) then leaves band l.  Band 0 and the
 * coefficients past (D+1)^2 are copied bit for bit.  out may be shs. */
int gsmpm_cov_to_scale_rot(const float* cov6, int64_t n, float* log_scale, float* quat,
                           int64_t* n_bad /* device, may be NULL */, void* stream);
int gsmpm_sh_rotate(const float* shs, const float* Q, int64_t n, int32_t D, int32_t M, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
