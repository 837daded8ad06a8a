// mpm_common.h -- particle/grid layout, BC tables and small device helpers
// shared by the MPM kernels (mpm.hip) and the constitutive models.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"

namespace gsmpm {

// ------------------------------------------------------------------ layout --
// Hot planes: what a substep reads and writes, in STORAGE order (re-sorted /
// permuted into bin order with the particles).
enum Plane : int {
  PX = 0,      // x y z
  PV = 3,      // v
  PC = 6,      // C (row-major 3x3)
  PF = 15,     // F_trial between substeps; return-mapped F inside p2g
  PMASS = 24,
  PVOL = 25,
  PMU = 26,
  PLAM = 27,
  PYLD = 28,
  NPLANES = 29
};
// Cold planes: only touched at init and by the per-frame postprocess /
// readback, kept in CALLER order (row = orig[storage row]) so re-sorting and
// re-binning never move them.
enum ColdPlane : int {
  PICOV = 0,   // init cov (upper 6)
  PCOV = 6,    // cov (upper 6)
  PR = 12,     // particle_R
  NCOLD = 21
};

constexpr int kMaxBC = 32;

// Tiles: the grid is cut into kTile^3-cell tiles; a particle belongs to the
// tile of its base cell, so its 3x3x3 stencil lies in the tile's
// (kTile+2)^3-node window.
constexpr int kTile = 8;  // k_grid decodes node offsets with 3-bit shifts
constexpr int kTW = kTile + 2;          // window edge
constexpr int kWin = kTW * kTW * kTW;   // window nodes (1000)

struct Impulse {
  float c[3], s[3], f[3], sdt;
  int bit;
};
struct GridOp {
  int kind;  // 0 fixed cube, 1 plane collider, 2 extended collider (its shape, surface and damping in BcTable::ext)
  int bit;
  float a[3], b[3], friction;
};
// Extended collider records (gsmpm_mpm_add_collider): GridOp o of kind 2
// holds the geometry -- a = point / centre, b = unit normal (plane), radius
// in b[0] (ball), half extents (box, walls) -- and the friction; ext[o] the
// rest.  Only the EXT instantiations of the grid kernels read them, and a
// table without such a record is updated by the plain ones.
enum ColliderShape : int { kShapePlane = 0, kShapeBall = 1, kShapeBox = 2, kShapeWalls = 3 };
enum ColliderSurface : int { kSurfSticky = 0, kSurfSlip = 1, kSurfSeparate = 2 };
struct GridOpExt {
  int shape, surface;
  float damping;
};
// The motion of a moving record (gsmpm_mpm_add_moving_collider): velocity w
// and motion window [t0, t1) on the caller's clock, f32 of the caller's
// doubles.  moving = 0: a static record (gsmpm_mpm_add_collider) in a table
// that holds a moving one; the MOV instantiations then run apply_ext as the
// EXT ones do.
struct GridOpMov {
  float w[3], t0, t1;
  int moving;
};
// The spin of a rotating record (gsmpm_mpm_add_rotating_collider): idx is the
// record's index among the table's rotating records -- its column of the pose
// table -- or -1 for any other op; om the angular velocity, f32 of the caller's
// doubles.  Its mov[] entry holds w, t0 and t1.  The rest of the spin (axis,
// |omega|, pivot) stays with k_set_poses (RotRec).
struct GridOpRot {
  int idx;
  float om[3];
};
// A particle driver (gsmpm_mpm_add_driver): a record on a fixed selection of
// particles, bit j of the selection words for drv[j].  kind 0 masked impulse:
// a = force, p0 = substep_dt; 1 enforced translation: a = velocity; 2
// enforced rotation: a = unit axis, b = point, p0 = omega, p1 = along.
enum DriverKind : int { kDrvImpulse = 0, kDrvTranslate = 1, kDrvRotate = 2 };
struct Driver {
  int kind, bit;
  float a[3], b[3], p0, p1;
};
struct BcTable {
  int n_imp, n_ops;
  Impulse imp[kMaxBC];
  GridOp op[kMaxBC];
  GridOpExt ext[kMaxBC];  // parallel to op[], after it: the offsets the plain instantiations read do not move
  GridOpMov mov[kMaxBC];  // parallel again, after ext[]: read by the MOV instantiations only
  GridOpRot rot[kMaxBC];  // parallel again, after mov[]: read by the ROT instantiations only
  // the particle drivers, last: read by the driver entry points of the P2G kernels only
  int n_drv;
  Driver drv[kMaxBC];
};

// The drivers' selection: the last argument of the driver entry points of the
// P2G kernels (k_fused_drv, k_p2g_drv and their mixed forms).  Empty for the
// plain entry points, which do not take it.  One word per particle in CALLER
// order (bit j: drv[j] drives the row), read through the storage -> caller
// map as MatIds reads the ids; bits: the OR of the drivers' activity bits.
template <bool DRV>
struct DrvSel {};
template <>
struct DrvSel<true> {
  const uint32_t* sel;  // [n] caller order
  const int* orig;      // [n] caller row of each storage row
  uint32_t bits;
};
// The drivers of storage row p, in table order, after the box impulses and
// before the stress.  Outside every driver's window the cost is the uniform
// test mask & bits; inside one, the indirect load of the row's word and a
// loop whose record loads are uniform (scalar).  (The empty overload only
// lets the shared bodies name the call under their `if constexpr (DRV)`.)
__device__ __forceinline__ void apply_drivers(const DrvSel<false>&, const BcTable*, uint32_t, int, const float (&)[3],
                                              float, float (&)[3]) {}
__device__ __forceinline__ void apply_drivers(const DrvSel<true>& ds, const BcTable* __restrict__ bct, uint32_t mask,
                                              int p, const float (&x)[3], float m, float (&v)[3]) {
  if (!(mask & ds.bits)) return;
  const uint32_t word = ds.sel[ds.orig[p]];
  const int nd = bct->n_drv;
  for (int j = 0; j < nd; ++j) {
    const Driver& dr = bct->drv[j];
    if (!((mask >> dr.bit) & 1u)) continue;  // uniform
    if (!((word >> j) & 1u)) continue;
    if (dr.kind == kDrvImpulse) {  // ImpulseBC.apply's arithmetic (boundary_conditions.py:45)
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = v[d] + dr.a[d] / m * dr.p0;
    } else if (dr.kind == kDrvTranslate) {
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = dr.a[d];
    } else {
      const float r0 = x[0] - dr.b[0], r1 = x[1] - dr.b[1], r2 = x[2] - dr.b[2];
      v[0] = dr.p0 * (dr.a[1] * r2 - dr.a[2] * r1) + dr.p1 * dr.a[0];
      v[1] = dr.p0 * (dr.a[2] * r0 - dr.a[0] * r2) + dr.p1 * dr.a[1];
      v[2] = dr.p0 * (dr.a[0] * r1 - dr.a[1] * r0) + dr.p1 * dr.a[2];
    }
  }
}
// One rotating record as k_set_poses reads it: unit axis k and |omega| in f64
// (the angle is wm * tau in f64), the rest f32 of the caller's doubles.
struct RotRec {
  double k[3], wm;
  float w[3], piv[3], a[3], t0, t1;
  int pad;
};
// One pose of the pose table: {R[9] row-major, c[3], o[3], pad}
constexpr int kPoseFloats = 16;

#ifndef GSMPM_PSTORE
#define GSMPM_PSTORE 2
#endif
struct Particles {
  float* P;
  int n, np;
  float* cold;          // [NCOLD][np], caller order
  const int* nlive;     // slab: the live count on the device (migration changes it inside a captured frame), else null
  // particles live now: kernels of a slab's step read it from the device and
  // run on a capacity-sized grid (the host learns n at the end of the step)
  __device__ __forceinline__ int count() const { return nlive ? *nlive : n; }
  // Plane access through a buffer resource: SGPR descriptor + SGPR plane
  // offset + ONE 32-bit VGPR lane offset for all hot planes (a flat access
  // holds a 64-bit VGPR address per plane, which costs the transfer kernels
  // ~48 VGPRs).  Requires NPLANES * np * 4 < 2^31, checked on the host.
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc() const {
    return __builtin_amdgcn_make_buffer_rsrc(P, (short)0, NPLANES * np * 4, 0x00020000);
  }
  __device__ __forceinline__ float ld(int plane, int i) const {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc(), i * 4, plane * np * 4, 0));
  }
  // GSMPM_PSTORE: the hot-plane stores' cache policy (buffer aux bits: 2 nt,
  // 16 sc1 write-through, 18 both)
  __device__ __forceinline__ void st(int plane, int i, float v) const {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc(), i * 4, plane * np * 4, GSMPM_PSTORE);
  }
  // cold planes, by caller row
  __device__ __forceinline__ float ldc(int plane, int row) const { return cold[(size_t)plane * np + row]; }
  __device__ __forceinline__ void stc(int plane, int row, float v) const { cold[(size_t)plane * np + row] = v; }
};

// Per-particle material ids (mixed mode, constitutive.h): the last argument
// of the mixed P2G kernels (k_fused_mixed, k_p2g_mixed).  Empty for every
// uniform instantiation, whose kernels do not take it; the mixed one
// (MAT == 6) carries the id array in CALLER order, read through the storage
// -> caller map, so a re-bin or re-sort never moves it (NPLANES stays what
// it is).
template <int MAT>
struct MatIds {};
template <>
struct MatIds<6> {
  const float* mat;  // [n] the reference's model.material, caller order
  const int* orig;   // [n] caller row of each storage row
  int jelly;         // kernel code of the `else` rows: 0 as written, 4 FCR
  __device__ __forceinline__ float id(int p) const { return mat[orig[p]]; }
};

struct GridDims {
  int ng;
  float dx, inv_dx;
};

struct MatConsts {
  float alpha, hardening, xi, pvisc;
};

// live node box [lo, hi] of the last G2P (int x3 lo, x3 hi), used by k_grid
struct Box {
  int lo[3], hi[3];
};

// -------------------------------------------------------- device helpers --
__device__ __forceinline__ void bspline(const float x[3], float inv_dx, int base[3], float fx[3], float w[3][3],
                                        float dw[3][3]) {
  // utils.py:92-109: base = (x*inv_dx - 0.5).cast(int) (truncation), quadratic B-spline
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float gp = x[d] * inv_dx;
    base[d] = (int)(gp - 0.5f);
    fx[d] = gp - (float)base[d];
    const float wa = 1.5f - fx[d], wb = fx[d] - 1.0f, wc = fx[d] - 0.5f;
    w[d][0] = wa * wa * 0.5f;
    w[d][1] = 0.75f - wb * wb;
    w[d][2] = wc * wc * 0.5f;
    dw[d][0] = fx[d] - 1.5f;
    dw[d][1] = -2.0f * (fx[d] - 1.0f);
    dw[d][2] = fx[d] - 0.5f;
  }
}

__device__ __forceinline__ float det3(const float (&A)[3][3]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
         A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// U diag(d) V^T
__device__ __forceinline__ void usv(const float (&U)[3][3], const float (&d)[3], const float (&V)[3][3],
                                    float (&O)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O[i][j] = (U[i][0] * d[0]) * V[j][0] + (U[i][1] * d[1]) * V[j][1] + (U[i][2] * d[2]) * V[j][2];
}

// A B^T
__device__ __forceinline__ void mmT(const float (&A)[3][3], const float (&B)[3][3], float (&O)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O[i][j] = A[i][0] * B[j][0] + A[i][1] * B[j][1] + A[i][2] * B[j][2];
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// Whole-wave reductions through DPP (no LDS crossbar: a __shfl_xor compiles to
// ds_bpermute_b32): within each 16-lane row by quad swaps and the two row
// mirrors, then the four rows' results read out as uniform values.  Every lane
// of the wave must be active.
template <typename Op>
__device__ __forceinline__ int dpp_row_reduce(int v, Op op) {
  v = op(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false));  // row_mirror
  return v;
}
__device__ __forceinline__ int wave_or_dpp(int v) {
  v = dpp_row_reduce(v, [](int a, int b) { return a | b; });
  return __builtin_amdgcn_readlane(v, 0) | __builtin_amdgcn_readlane(v, 16) | __builtin_amdgcn_readlane(v, 32) |
         __builtin_amdgcn_readlane(v, 48);
}
// max of non-negative floats (their bit patterns order as integers)
__device__ __forceinline__ float wave_max_nonneg_dpp(float x) {
  int v = dpp_row_reduce(__float_as_int(x), [](int a, int b) { return max(a, b); });
  v = max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
          max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
  return __int_as_float(v);
}

}  // namespace gsmpm
