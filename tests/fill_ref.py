"""numpy reference of the interior filling (csrc/fill.hip, DESIGN.md "Interior filling").

* density: float64 sums of o * exp(-q/2) over each particle's stamp, the
  number of contributions per cell, the skipped count.  The stamp (cell and
  half-width) is integer logic and is taken exactly as the kernel defines it,
  in float32.  `dtype=np.float32` evaluates the same formula in float32 (the
  oracle-side measure of the f32 rounding).
* occupied / direction bits / interior: exact integer logic, by walking every
  line from its far end (nothing like the kernel's bit-packed popcounts).
* emission: the counter hash in uint32 and the positions in float32.
* nearest: float32, d2 = (dx*dx + dy*dy) + dz*dz, first minimum.
* shell(): the fixture, a hollow sphere of Gaussians.
"""
from __future__ import annotations

import numpy as np

Q = 2.0 ** -24  # the density quantum
DIRS = ((0, +1), (0, -1), (1, +1), (1, -1), (2, +1), (2, -1))  # +x -x +y -y +z -z


# ------------------------------------------------------------------ density --
def stamps(x, cov6, opa, n, extent, support):
    """valid[N], cell[N,3] (int), r[N] (int), in the kernel's float32 integer logic."""
    x = np.asarray(x, np.float32)
    cov6 = np.asarray(cov6, np.float32)
    opa = np.asarray(opa, np.float32)
    inv_dx = np.float32(n / extent)
    dx = np.float32(extent / n)
    with np.errstate(invalid="ignore", over="ignore"):
        cf = np.floor(x * inv_dx)
        valid = (np.isfinite(x).all(1) & np.isfinite(cov6).all(1) & (opa >= 0) & (opa <= 1) &
                 (cf >= 0).all(1) & (cf < np.float32(n)).all(1))
    cell = np.where(valid[:, None], cf, 0).astype(np.int64)
    m9 = np.float32(9.0) * np.maximum(np.maximum(cov6[:, 0], cov6[:, 3]), cov6[:, 5])
    dx2 = dx * dx
    r = np.zeros(len(x), np.int64)
    for k in range(support):  # r = first integer with (r dx)^2 >= 9 max diag, at most support
        with np.errstate(invalid="ignore"):
            r += (r == k) & (np.float32(k * k) * dx2 < m9)
    return valid, cell, r


def density(x, cov6, opa, n, extent, support, dtype=np.float64):
    """-> density [n,n,n] (dtype), n_c [n,n,n] (contributions per cell), skipped."""
    valid, cell, r = stamps(x, cov6, opa, n, extent, support)
    T = dtype
    dens = np.zeros((n, n, n), T)
    n_c = np.zeros((n, n, n), np.int64)
    dx = T(np.float32(extent / n)) if T == np.float32 else T(extent) / T(n)
    h2 = (T(0.5) * dx) ** 2
    for p in np.flatnonzero(valid):
        c = np.asarray(cov6[p], np.float32).astype(T)
        A = np.array([[c[0] + h2, c[1], c[2]], [c[1], c[3] + h2, c[4]], [c[2], c[4], c[5] + h2]], T)
        inv = np.linalg.inv(A.astype(np.float64)).astype(T) if T == np.float64 else _inv3_f32(A)
        lo = np.maximum(cell[p] - r[p], 0)
        hi = np.minimum(cell[p] + r[p], n - 1)
        ax = [(np.arange(lo[a], hi[a] + 1).astype(T) + T(0.5)) * dx - T(np.float32(x[p][a])) for a in range(3)]
        d = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
        with np.errstate(invalid="ignore", over="ignore"):
            qf = np.einsum("...a,ab,...b->...", d, inv, d).astype(T)
            v = np.where(qf >= 0, T(np.float32(opa[p])) * np.exp(T(-0.5) * qf),
                         np.where(qf < 0, T(np.float32(opa[p])), T(0)))
        sl = tuple(slice(lo[a], hi[a] + 1) for a in range(3))
        dens[sl] += v.astype(T)
        n_c[sl] += 1
    return dens, n_c, int((~valid).sum())


def _inv3_f32(A):
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    k00, k01, k02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    k11, k12, k22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * k00 + a01 * k01) + a02 * k02
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.array([[k00, k01, k02], [k01, k11, k12], [k02, k12, k22]], np.float32) / det).astype(np.float32)


def f32_term(dens_ref, dens_f32):
    """The relative f32 term of the bound: 4e-6, or twice the largest relative error that the
    float32 evaluation of the formula (density(..., dtype=np.float32)) shows against float64 on
    the same particles, if that is more.  Cells below one quantum are left to the n_c q/2 term.
    -> (term, measured)."""
    m = dens_ref >= Q
    measured = float((np.abs(dens_f32.astype(np.float64) - dens_ref)[m] / dens_ref[m]).max()) if m.any() else 0.0
    return max(4e-6, 2.0 * measured), measured


def density_bound(dens_ref, n_c, rel=4e-6):
    """Per-cell bound on |gpu - ref|: half a quantum per contribution plus the f32 term."""
    return n_c * (Q / 2) + rel * dens_ref


# ------------------------------------------------------------ integer logic --
def direction_bits(occ):
    """u16 [n,n,n]: bit d = direction d meets an occupied cell before the edge,
    bit 8+d = the number of maximal occupied runs met that way is odd."""
    occ = np.asarray(occ, bool)
    n = occ.shape[0]
    bits = np.zeros(occ.shape, np.uint16)
    for d, (axis, sign) in enumerate(DIRS):
        o = np.moveaxis(occ, axis, 0)
        if sign < 0:
            o = o[::-1]
        hit = np.zeros(o.shape, bool)
        runs = np.zeros(o.shape, np.int64)
        for t in range(n - 2, -1, -1):  # from the far end: what lies beyond t is what lay beyond t+1, plus t+1
            nxt2 = o[t + 2] if t + 2 < n else np.zeros(o.shape[1:], bool)
            hit[t] = hit[t + 1] | o[t + 1]
            runs[t] = runs[t + 1] + (o[t + 1] & ~nxt2)
        if sign < 0:
            hit, runs = hit[::-1], runs[::-1]
        hit, runs = np.moveaxis(hit, 0, axis), np.moveaxis(runs, 0, axis)
        bits |= (hit.astype(np.uint16) << d) | ((runs & 1).astype(np.uint16) << (8 + d))
    return bits


def count_runs(occ, cell, d):
    """Maximal occupied runs met from `cell` (exclusive) to the grid's edge in direction d, by walking."""
    axis, sign = DIRS[d]
    c = list(cell)
    runs, prev = 0, False
    while True:
        c[axis] += sign
        if not 0 <= c[axis] < occ.shape[axis]:
            return runs
        cur = bool(occ[tuple(c)])
        runs += cur and not prev
        prev = cur


def box_cells(n, extent, box):
    """Inclusive cell ranges of the cells whose centre lies in [lo, hi] (float32 box, float64 arithmetic)."""
    if box is None:
        return np.zeros(3, np.int64), np.full(3, n - 1, np.int64)
    dx = extent / n
    lo = np.asarray(box[0], np.float32).astype(np.float64)
    hi = np.asarray(box[1], np.float32).astype(np.float64)
    ilo = np.clip(np.ceil(lo / dx - 0.5), 0, n).astype(np.int64)
    ihi = np.clip(np.floor(hi / dx - 0.5), -1, n - 1).astype(np.int64)
    return ilo, ihi


def interior(occ, bits, min_hits=6, parity_dir=-1, box=None, extent=2.0):
    occ = np.asarray(occ, bool)
    n = occ.shape[0]
    hits = np.zeros(occ.shape, np.int64)
    for d in range(6):
        hits += (bits >> d) & 1
    inside = ~occ & (hits >= min_hits)
    if parity_dir >= 0:
        inside &= ((bits >> (8 + parity_dir)) & 1).astype(bool)
    ilo, ihi = box_cells(n, extent, box)
    idx = np.arange(n)
    for a in range(3):
        keep = (idx >= ilo[a]) & (idx <= ihi[a])
        inside &= keep.reshape([-1 if b == a else 1 for b in range(3)])
    return inside


# ----------------------------------------------------------------- emission --
def mix32(v):
    """lowbias32 on uint32 arrays."""
    v = np.asarray(v, np.uint32).copy()
    v ^= v >> np.uint32(16)
    v *= np.uint32(0x7feb352d)
    v ^= v >> np.uint32(15)
    v *= np.uint32(0x846ca68b)
    v ^= v >> np.uint32(16)
    return v


def fill_hash(seed, cell, k, axis):
    with np.errstate(over="ignore"):
        a = mix32(np.uint32(seed & 0xFFFFFFFF)) + np.asarray(cell, np.uint32)
        return mix32(mix32(a) + (np.uint32(4) * np.asarray(k, np.uint32) + np.asarray(axis, np.uint32)))


def emit(inside, per_cell, seed, extent, capacity=None):
    """-> (positions float32 [min(total, capacity), 3], total): linear cell order, then k."""
    inside = np.asarray(inside, bool)
    n = inside.shape[0]
    cells = np.flatnonzero(inside.ravel()).astype(np.uint32)
    total = len(cells) * per_cell
    ijl = np.stack(np.unravel_index(cells.astype(np.int64), inside.shape), -1)  # [C,3]
    dx = np.float32(extent / n)
    k = np.arange(per_cell, dtype=np.uint32)
    pos = np.empty((len(cells), per_cell, 3), np.float32)
    for a in range(3):
        h = fill_hash(seed, cells[:, None], k[None, :], a)
        u = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        pos[:, :, a] = (ijl[:, a, None].astype(np.float32) + u) * dx
    pos = pos.reshape(-1, 3)
    return (pos if capacity is None else pos[:capacity]), total


# ------------------------------------------------------------------ nearest --
def nearest(query, source, chunk=256):
    query = np.asarray(query, np.float32)
    source = np.asarray(source, np.float32)
    out = np.empty(len(query), np.int32)
    for s in range(0, len(query), chunk):
        d = query[s:s + chunk, None, :] - source[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[s:s + chunk] = np.argmin(d2, axis=1)  # the first minimum
    return out


# ------------------------------------------------------------------ fixture --
def shell(n_points, n, extent=2.0, radius_cells=10.0, centre_cells=None, thickness_cells=0.5, seed=0,
          hole_deg=None, anisotropic=True):
    """A hollow sphere of Gaussians in grid space: centres on a sphere of
    `radius_cells` cells about `centre_cells`, jittered radially by
    +-thickness/2; covariances of about one cell (sigma 0.6..1.0 cells per
    axis, randomly rotated when `anisotropic`), opacity 0.5..1.  hole_deg: no
    Gaussian within that angle of +x.  -> x [N,3], cov6 [N,6], opacity [N], float32."""
    rng = np.random.default_rng(seed)
    dx = extent / n
    c = (np.full(3, n / 2.0) if centre_cells is None else np.asarray(centre_cells, float)) * dx
    # quasi-uniform directions (a Fibonacci lattice) so that the shell has no accidental gaps
    i = np.arange(n_points) + 0.5
    z = 1 - 2 * i / n_points
    phi = np.pi * (1 + 5 ** 0.5) * i
    s = np.sqrt(1 - z * z)
    u = np.stack([z, s * np.cos(phi), s * np.sin(phi)], -1)  # the lattice axis along x
    rad = (radius_cells + thickness_cells * (rng.random(n_points) - 0.5)) * dx
    x = c + u * rad[:, None]
    sig = rng.uniform(0.6, 1.0, (n_points, 3 if anisotropic else 1)) * dx
    sig = np.broadcast_to(sig, (n_points, 3))
    if anisotropic:
        qr = np.linalg.qr(rng.normal(size=(n_points, 3, 3)))[0]
    else:
        qr = np.broadcast_to(np.eye(3), (n_points, 3, 3))
    S = np.einsum("nab,nb,ncb->nac", qr, sig * sig, qr)
    cov6 = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
    opa = rng.uniform(0.5, 1.0, n_points)
    if hole_deg is not None:
        keep = u[:, 0] < np.cos(np.radians(hole_deg))
        x, cov6, opa = x[keep], cov6[keep], opa[keep]
    return x.astype(np.float32), cov6.astype(np.float32), opa.astype(np.float32)
