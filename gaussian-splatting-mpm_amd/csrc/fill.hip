// fill.hip -- interior particle filling for hollow Gaussian shells (the first
// half of PhysGaussian's internal-filling pass; get_particle_volume, the
// second half, is k_fill_count / k_fill_vol in mpm.hip).  A one-off
// initialisation: density grid from the Gaussians, occupied mask, interior
// mask from six directional line tests, seeded particle emission, and the
// nearest source Gaussian of every emitted particle.  DESIGN.md "Interior
// filling" has the semantics; the short form:
//
//  density   u64 fixed point, quantum q = 2^-24.  A contribution is
//            o * exp(-q/2) in [0, 1] (opacities outside [0, 1] are skipped), so
//            one add is <= 2^24 and a cell that every one of N < 2^31
//            particles hits stays below 2^55: the sum cannot wrap, and integer
//            adds commute, so the grid is bit-identical for any particle order.
//  occupied  integer sum > floor(threshold * 2^24)  (== sum * q > threshold).
//  lines     the occupied mask is bit-packed three times, once per axis, so
//            that every line of the grid is ceil(n/64) words whichever axis it
//            runs along.  "Is there an occupied cell beyond me" and "how many
//            maximal occupied runs lie beyond me" are then a mask and a
//            popcount of rising edges per word, for all six directions, with
//            coalesced loads for the lines across the fastest axis as well.
//  emission  inclusive scan (scan.h) of per_cell * interior in linear cell
//            order; particle k of cell c at ((float)i + u) * dx per axis,
//            u = (h >> 8) * 2^-24, h = fill_hash(seed, c, k, axis).
//  nearest   exact brute force over LDS tiles, d2 = (dx*dx + dy*dy) + dz*dz in
//            f32 (the library is built with -ffp-contract=off), lowest index
//            wins ties.
#include "common.h"

#include <cmath>

namespace gsmpm {

#include "scan.h"

namespace {

constexpr float kFillQ = 16777216.0f;  // 1 / quantum
constexpr int kFillMaxSupport = 16;
constexpr int kFillMaxGrid = 512;  // n^3 * 8 particles stays below 2^32 (u32 scan)

struct FillWs {
  unsigned long long* dens;   // [n^3] fixed-point density
  unsigned long long* cnt;    // [n^3] per_cell * interior (the scan's input)
  uint32_t* inc;              // [n^3] inclusive scan of cnt
  uint32_t* btot;             // [ceil(n^3 / 1024)]
  uint16_t* bits;             // [n^3] hit bits 0..5, run-parity bits 8..13
  uint8_t* occ;               // [n^3]
  uint8_t* interior;          // [n^3]
  unsigned long long* zmask;  // [(i*n + j)*W + w]   bits over l
  unsigned long long* ymask;  // [(i*W + w)*n + l]   bits over j
  unsigned long long* xmask;  // [(j*W + w)*n + l]   bits over i
  uint32_t* skipped;          // [1]
};

inline uint64_t align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }

// carves the workspace; returns the bytes it needs
uint64_t fill_layout(int n, void* base, FillWs* w) {
  const uint64_t n3 = (uint64_t)n * n * n, W = (uint64_t)(n + 63) / 64, nm = (uint64_t)n * n * W;
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    char* p = base ? (char*)base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  FillWs t;
  t.dens = (unsigned long long*)take(8 * n3);
  t.cnt = (unsigned long long*)take(8 * n3);
  t.inc = (uint32_t*)take(4 * n3);
  t.btot = (uint32_t*)take(4 * ((n3 + kScanBlk - 1) / kScanBlk));
  t.bits = (uint16_t*)take(2 * n3);
  t.occ = (uint8_t*)take(n3);
  t.interior = (uint8_t*)take(n3);
  t.zmask = (unsigned long long*)take(8 * nm);
  t.ymask = (unsigned long long*)take(8 * nm);
  t.xmask = (unsigned long long*)take(8 * nm);
  t.skipped = (uint32_t*)take(4);
  if (w) *w = t;
  return off;
}

// ---------------------------------------------------------------- density --
// One wave per particle; the lanes walk the particle's stamp in linear order
// (l fastest), so a wave's atomics land on runs of consecutive cells.
__global__ __launch_bounds__(256) void k_fill_density(const float* __restrict__ x, const float* __restrict__ cov6,
                                                      const float* __restrict__ opa, long n_part, int n, double dxd,
                                                      float inv_dx, int support,
                                                      unsigned long long* __restrict__ dens,
                                                      uint32_t* __restrict__ skipped) {
  const int lane = threadIdx.x & 63;
  const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const float dx = (float)dxd, h = 0.5f * dx, h2 = h * h, dx2 = dx * dx;
  for (long p = wave0; p < n_part; p += nwaves) {
    const float px = x[3 * p], py = x[3 * p + 1], pz = x[3 * p + 2], o = opa[p];
    const float cxx = cov6[6 * p], cxy = cov6[6 * p + 1], cxz = cov6[6 * p + 2], cyy = cov6[6 * p + 3],
                cyz = cov6[6 * p + 4], czz = cov6[6 * p + 5];
    // every lane evaluates the same (wave-uniform) tests
    bool ok = isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(cxx) && isfinite(cxy) && isfinite(cxz) &&
              isfinite(cyy) && isfinite(cyz) && isfinite(czz) && o >= 0.0f && o <= 1.0f;
    const float fi = floorf(px * inv_dx), fj = floorf(py * inv_dx), fl = floorf(pz * inv_dx);
    const float fn = (float)n;
    ok = ok && fi >= 0.0f && fi < fn && fj >= 0.0f && fj < fn && fl >= 0.0f && fl < fn;
    if (!ok) {
      if (lane == 0) atomicAdd(skipped, 1u);
      continue;
    }
    const int ci = (int)fi, cj = (int)fj, cl = (int)fl;
    // A = cov + (dx/2)^2 I, inverse by cofactors
    const float a00 = cxx + h2, a11 = cyy + h2, a22 = czz + h2, a01 = cxy, a02 = cxz, a12 = cyz;
    const float k00 = a11 * a22 - a12 * a12, k01 = a02 * a12 - a01 * a22, k02 = a01 * a12 - a02 * a11;
    const float k11 = a00 * a22 - a02 * a02, k12 = a01 * a02 - a00 * a12, k22 = a00 * a11 - a01 * a01;
    const float det = (a00 * k00 + a01 * k01) + a02 * k02;
    const float i00 = k00 / det, i01 = k01 / det, i02 = k02 / det, i11 = k11 / det, i12 = k12 / det, i22 = k22 / det;
    // r = the first integer with (r dx)^2 >= 9 max diag, at most `support`
    const float m9 = 9.0f * fmaxf(cxx, fmaxf(cyy, czz));
    int r = 0;
    while (r < support && (float)(r * r) * dx2 < m9) ++r;
    const int lo0 = max(ci - r, 0), lo1 = max(cj - r, 0), lo2 = max(cl - r, 0);
    const int e0 = min(ci + r, n - 1) - lo0 + 1, e1 = min(cj + r, n - 1) - lo1 + 1, e2 = min(cl + r, n - 1) - lo2 + 1;
    const int total = e0 * e1 * e2;
    for (int s = lane; s < total; s += 64) {
      const int c = s % e2, ab = s / e2, b = ab % e1, a = ab / e1;
      const int i = lo0 + a, j = lo1 + b, l = lo2 + c;  // inside [0, n) by the clamps above
      // the offsets are small differences of numbers near the grid's extent: taken in f64 and rounded
      // once (three f64 operations a cell), everything after them is f32
      const float d0 = (float)(((double)i + 0.5) * dxd - (double)px), d1 = (float)(((double)j + 0.5) * dxd - (double)py),
                  d2 = (float)(((double)l + 0.5) * dxd - (double)pz);
      const float qf = d0 * ((i00 * d0 + i01 * d1) + i02 * d2) + d1 * ((i01 * d0 + i11 * d1) + i12 * d2) +
                       d2 * ((i02 * d0 + i12 * d1) + i22 * d2);
      // a quadratic form that is negative (indefinite input) counts as 0; a NaN one adds nothing
      float v = qf >= 0.0f ? o * expf(-0.5f * qf) : (qf < 0.0f ? o : 0.0f);
      const unsigned long long iv = (unsigned long long)rintf(v * kFillQ);  // v in [0, 1]: <= 2^24
      if (iv) atomicAdd(&dens[((size_t)i * n + j) * n + l], iv);
    }
  }
}

// ------------------------------------------------------- occupied + masks --
// one wave per (z line, word): threshold 64 consecutive cells, ballot them
__global__ __launch_bounds__(256) void k_fill_occupied(const unsigned long long* __restrict__ dens, int n, int W,
                                                       unsigned long long thr, uint8_t* __restrict__ occ,
                                                       unsigned long long* __restrict__ zmask) {
  const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nlines = (long)n * n;
  if (g >= nlines * W) return;  // wave-uniform
  const long line = g / W;
  const int w = (int)(g % W), l = w * 64 + (threadIdx.x & 63);
  bool o = false;
  if (l < n) {
    o = dens[line * n + l] > thr;
    occ[line * n + l] = o ? 1 : 0;
  }
  const unsigned long long m = __ballot(o);
  if ((threadIdx.x & 63) == 0) zmask[g] = m;
}

// lines across the fastest axis: one thread per (outer, l); it walks the line
// while its wave reads 64 consecutive l of every step (coalesced bytes).
// axis 1: outer = i, the line runs over j; axis 0: outer = j, the line runs over i.
__global__ __launch_bounds__(256) void k_fill_linemask(const uint8_t* __restrict__ occ, int n, int W, int axis,
                                                       unsigned long long* __restrict__ mask) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n * n) return;
  const int outer = (int)(t / n), l = (int)(t % n);
  const size_t step = axis == 1 ? (size_t)n : (size_t)n * n;
  const size_t base = axis == 1 ? (size_t)outer * n * n + l : (size_t)outer * n + l;
  for (int w = 0; w < W; ++w) {
    unsigned long long word = 0;
    const int cnt = min(64, n - w * 64);
    for (int b = 0; b < cnt; ++b) word |= (unsigned long long)occ[base + (size_t)(w * 64 + b) * step] << b;
    mask[((size_t)outer * W + w) * n + l] = word;
  }
}

// hit and run parity on both sides of position t of one bit-packed line.
// Runs of a bit set = its rising edges, counted with the carry across words.
struct LineBits {
  unsigned up_runs = 0, dn_runs = 0;
  bool up_hit = false, dn_hit = false;
  unsigned long long up_c = 0, dn_c = 0;
  __device__ __forceinline__ void word(unsigned long long m, int w, int t) {
    const int base = w * 64;
    const int s = t + 1 - base;  // bits >= s of this word lie beyond t
    const unsigned long long up = s <= 0 ? m : (s >= 64 ? 0ull : m & (~0ull << s));
    const int e = t - base;      // bits < e of this word lie before t
    const unsigned long long dn = e >= 64 ? m : (e <= 0 ? 0ull : m & ((1ull << e) - 1ull));
    up_hit |= up != 0;
    dn_hit |= dn != 0;
    up_runs += __popcll(up & ~((up << 1) | up_c));
    dn_runs += __popcll(dn & ~((dn << 1) | dn_c));
    up_c = up >> 63;
    dn_c = dn >> 63;
  }
};

// directions: 0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z  (x = i slowest, z = l fastest)
__global__ __launch_bounds__(256) void k_fill_interior(const uint8_t* __restrict__ occ,
                                                       const unsigned long long* __restrict__ zmask,
                                                       const unsigned long long* __restrict__ ymask,
                                                       const unsigned long long* __restrict__ xmask, int n, int W,
                                                       int min_hits, int parity_dir, int per_cell, int blo0, int blo1,
                                                       int blo2, int bhi0, int bhi1, int bhi2,
                                                       uint16_t* __restrict__ bits, uint8_t* __restrict__ interior,
                                                       unsigned long long* __restrict__ cnt) {
  const size_t n3 = (size_t)n * n * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n3; c += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(c % n), j = (int)((c / n) % n), i = (int)(c / ((size_t)n * n));
    LineBits X, Y, Z;
    for (int w = 0; w < W; ++w) {
      X.word(xmask[((size_t)j * W + w) * n + l], w, i);
      Y.word(ymask[((size_t)i * W + w) * n + l], w, j);
      Z.word(zmask[((size_t)i * n + j) * W + w], w, l);
    }
    const unsigned hit = (unsigned)X.up_hit | (unsigned)X.dn_hit << 1 | (unsigned)Y.up_hit << 2 |
                         (unsigned)Y.dn_hit << 3 | (unsigned)Z.up_hit << 4 | (unsigned)Z.dn_hit << 5;
    const unsigned par = (X.up_runs & 1u) | (X.dn_runs & 1u) << 1 | (Y.up_runs & 1u) << 2 | (Y.dn_runs & 1u) << 3 |
                         (Z.up_runs & 1u) << 4 | (Z.dn_runs & 1u) << 5;
    bool in = !occ[c] && i >= blo0 && i <= bhi0 && j >= blo1 && j <= bhi1 && l >= blo2 && l <= bhi2 &&
              __popc(hit) >= min_hits;
    if (parity_dir >= 0) in = in && ((par >> parity_dir) & 1u);
    bits[c] = (uint16_t)(hit | par << 8);
    interior[c] = in ? 1 : 0;
    cnt[c] = in ? (unsigned long long)per_cell : 0ull;
  }
}

// ---------------------------------------------------------------- emission --
// lowbias32 (C. Wellons' 32-bit integer mixer)
__device__ __forceinline__ uint32_t fill_mix(uint32_t v) {
  v ^= v >> 16;
  v *= 0x7feb352du;
  v ^= v >> 15;
  v *= 0x846ca68bu;
  v ^= v >> 16;
  return v;
}
// counter hash of (seed, linear cell, k, axis)
__device__ __forceinline__ uint32_t fill_hash(uint32_t seed, uint32_t cell, uint32_t k, uint32_t axis) {
  return fill_mix(fill_mix(fill_mix(seed) + cell) + (4u * k + axis));
}

__global__ __launch_bounds__(256) void k_fill_emit(const uint8_t* __restrict__ interior,
                                                   const uint32_t* __restrict__ inc, int n, float dx, int per_cell,
                                                   uint32_t seed, unsigned long long capacity,
                                                   float* __restrict__ out) {
  const size_t n3 = (size_t)n * n * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n3; c += (size_t)gridDim.x * blockDim.x) {
    if (!interior[c]) continue;
    const int cell[3] = {(int)(c / ((size_t)n * n)), (int)((c / n) % n), (int)(c % n)};
    const unsigned long long first = (unsigned long long)inc[c] - (unsigned)per_cell;
    for (int k = 0; k < per_cell; ++k) {
      const unsigned long long idx = first + k;
      if (idx >= capacity) break;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float u = (float)(fill_hash(seed, (uint32_t)c, (uint32_t)k, (uint32_t)a) >> 8) * (1.0f / 16777216.0f);
        out[3 * idx + a] = ((float)cell[a] + u) * dx;
      }
    }
  }
}

// ----------------------------------------------------------------- nearest --
constexpr int kNearTile = 1024;  // sources per LDS tile (16 KiB as float4)
constexpr int kNearQpt = 4;      // queries per thread

__global__ __launch_bounds__(256) void k_fill_nearest(const float* __restrict__ q, long nq,
                                                      const float* __restrict__ src, long ns,
                                                      int32_t* __restrict__ idx) {
  __shared__ float4 s_src[kNearTile];
  float qx[kNearQpt], qy[kNearQpt], qz[kNearQpt], best[kNearQpt];
  int32_t bi[kNearQpt];
  const long q0 = (long)blockIdx.x * (256 * kNearQpt) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kNearQpt; ++k) {
    const long qi = q0 + 256L * k;
    const bool live = qi < nq;
    qx[k] = live ? q[3 * qi] : 0.0f;
    qy[k] = live ? q[3 * qi + 1] : 0.0f;
    qz[k] = live ? q[3 * qi + 2] : 0.0f;
    best[k] = INFINITY;
    bi[k] = 0;
  }
  for (long t0 = 0; t0 < ns; t0 += kNearTile) {
    const int cnt = (int)min((long)kNearTile, ns - t0);
    __syncthreads();  // the previous tile is read out
    for (int e = threadIdx.x; e < 3 * cnt; e += 256) ((float*)s_src)[(e / 3) * 4 + e % 3] = src[3 * t0 + e];
    __syncthreads();
    for (int s = 0; s < cnt; ++s) {
      const float4 p = s_src[s];  // one address for the whole wave: a broadcast read
#pragma unroll
      for (int k = 0; k < kNearQpt; ++k) {
        const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best[k]) {  // strict: the lowest index keeps a tie
          best[k] = d2;
          bi[k] = (int32_t)(t0 + s);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kNearQpt; ++k) {
    const long qi = q0 + 256L * k;
    if (qi < nq) idx[qi] = bi[k];
  }
}

__global__ __launch_bounds__(256) void k_fill_density_f32(const unsigned long long* __restrict__ dens, size_t n3,
                                                          float* __restrict__ out) {
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n3; c += (size_t)gridDim.x * blockDim.x)
    out[c] = (float)dens[c] * (1.0f / 16777216.0f);
}

// the optional box as inclusive cell ranges: the cells whose centre lies in [lo, hi]
void box_cells(const gsmpm_fill_params* p, int lo[3], int hi[3]) {
  const double dx = p->grid_extent / p->n_grid;
  for (int a = 0; a < 3; ++a) {
    lo[a] = 0;
    hi[a] = p->n_grid - 1;
    if (!p->use_box) continue;
    const double l = std::ceil((double)p->lo[a] / dx - 0.5), h = std::floor((double)p->hi[a] / dx - 0.5);
    lo[a] = (int)std::fmin(std::fmax(l, 0.0), (double)p->n_grid);       // an empty range if past the grid
    hi[a] = (int)std::fmin(std::fmax(h, -1.0), (double)p->n_grid - 1);
  }
}

int check_params(const gsmpm_fill_params* p, const char* who) {
  const std::string w(who);
  GSMPM_REQUIRE(p, w + ": null params");
  GSMPM_REQUIRE(p->n_grid >= 4 && p->n_grid <= kFillMaxGrid, w + ": n_grid outside 4..512");
  GSMPM_REQUIRE(p->grid_extent > 0.0 && std::isfinite(p->grid_extent), w + ": grid_extent must be positive");
  GSMPM_REQUIRE(p->density_threshold > 0.0 && p->density_threshold <= 1073741824.0,
                w + ": density_threshold must be positive (and at most 2^30)");
  GSMPM_REQUIRE(p->support >= 0 && p->support <= kFillMaxSupport, w + ": support outside 0..16");
  GSMPM_REQUIRE(p->min_hits >= 1 && p->min_hits <= 6, w + ": min_hits outside 1..6");
  GSMPM_REQUIRE(p->parity_dir >= -1 && p->parity_dir <= 5, w + ": parity_dir outside -1..5");
  GSMPM_REQUIRE(p->per_cell >= 1 && p->per_cell <= 8, w + ": per_cell outside 1..8");
  GSMPM_REQUIRE(p->capacity >= 0, w + ": negative capacity");
  if (p->use_box)
    for (int a = 0; a < 3; ++a)
      GSMPM_REQUIRE(std::isfinite(p->lo[a]) && std::isfinite(p->hi[a]), w + ": non-finite box");
  return GSMPM_OK;
}

int check_ws(const gsmpm_fill_params* p, const void* ws, uint64_t ws_bytes, FillWs* w, const char* who) {
  const std::string s(who);
  GSMPM_REQUIRE(ws, s + ": null workspace");
  GSMPM_REQUIRE(((uintptr_t)ws & 255) == 0, s + ": the workspace must be 256-byte aligned");
  if (ws_bytes < fill_layout(p->n_grid, nullptr, nullptr)) {
    set_error(s + ": workspace smaller than gsmpm_fill_workspace_size");
    return GSMPM_ESPACE;
  }
  fill_layout(p->n_grid, const_cast<void*>(ws), w);
  return GSMPM_OK;
}

inline int grid_for(size_t work, int block) { return (int)std::min<size_t>((work + block - 1) / block, 16384); }

}  // namespace
}  // namespace gsmpm

using namespace gsmpm;

extern "C" {

int gsmpm_fill_workspace_size(const gsmpm_fill_params* p, uint64_t* bytes) {
  if (int rc = check_params(p, "gsmpm_fill_workspace_size")) return rc;
  GSMPM_REQUIRE(bytes, "gsmpm_fill_workspace_size: null argument");
  *bytes = fill_layout(p->n_grid, nullptr, nullptr);
  return GSMPM_OK;
}

int gsmpm_fill_interior(const gsmpm_fill_params* p, const float* x, const float* cov6, const float* opacity, int64_t n,
                        void* ws, uint64_t ws_bytes, int64_t* total, int64_t* skipped, void* stream) {
  if (int rc = check_params(p, "gsmpm_fill_interior")) return rc;
  GSMPM_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "gsmpm_fill_interior: particle count outside 0..2^31-1");
  GSMPM_REQUIRE(n == 0 || (x && cov6 && opacity), "gsmpm_fill_interior: null particle array");
  GSMPM_REQUIRE(total && skipped, "gsmpm_fill_interior: null argument");
  FillWs w;
  if (int rc = check_ws(p, ws, ws_bytes, &w, "gsmpm_fill_interior")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int ng = p->n_grid, W = (ng + 63) / 64;
  const size_t n3 = (size_t)ng * ng * ng;
  const double dx = p->grid_extent / ng;
  const unsigned long long thr = (unsigned long long)std::floor(p->density_threshold * 16777216.0);
  int blo[3], bhi[3];
  box_cells(p, blo, bhi);
  GSMPM_HIP(hipMemsetAsync(w.dens, 0, 8 * n3, st));
  GSMPM_HIP(hipMemsetAsync(w.skipped, 0, 4, st));
  if (n > 0) {
    k_fill_density<<<grid_for((size_t)n, 4), 256, 0, st>>>(x, cov6, opacity, (long)n, ng, dx,
                                                           (float)(ng / p->grid_extent), p->support, w.dens,
                                                           w.skipped);
    GSMPM_LAUNCH_CHECK();
  }
  k_fill_occupied<<<div_up((long)ng * ng * W, 4), 256, 0, st>>>(w.dens, ng, W, thr, w.occ, w.zmask);
  GSMPM_LAUNCH_CHECK();
  k_fill_linemask<<<div_up((long)ng * ng, 256), 256, 0, st>>>(w.occ, ng, W, 1, w.ymask);
  GSMPM_LAUNCH_CHECK();
  k_fill_linemask<<<div_up((long)ng * ng, 256), 256, 0, st>>>(w.occ, ng, W, 0, w.xmask);
  GSMPM_LAUNCH_CHECK();
  k_fill_interior<<<grid_for(n3, 256), 256, 0, st>>>(w.occ, w.zmask, w.ymask, w.xmask, ng, W, p->min_hits,
                                                     p->parity_dir, p->per_cell, blo[0], blo[1], blo[2], bhi[0],
                                                     bhi[1], bhi[2], w.bits, w.interior, w.cnt);
  GSMPM_LAUNCH_CHECK();
  const int nb = div_up((long)n3, kScanBlk);
  k_scan_blocks<uint32_t><<<nb, 256, 0, st>>>(w.cnt, (int)n3, w.btot);
  GSMPM_LAUNCH_CHECK();
  k_scan_apply<uint32_t><<<nb, 256, 0, st>>>(w.cnt, (int)n3, w.btot, w.inc);
  GSMPM_LAUNCH_CHECK();
  uint32_t host[2] = {0, 0};
  GSMPM_HIP(hipMemcpyAsync(&host[0], w.inc + (n3 - 1), 4, hipMemcpyDeviceToHost, st));
  GSMPM_HIP(hipMemcpyAsync(&host[1], w.skipped, 4, hipMemcpyDeviceToHost, st));
  GSMPM_HIP(hipStreamSynchronize(st));
  *total = host[0];
  *skipped = host[1];
  return GSMPM_OK;
}

int gsmpm_fill_emit(const gsmpm_fill_params* p, const void* ws, uint64_t ws_bytes, float* out_pos, void* stream) {
  if (int rc = check_params(p, "gsmpm_fill_emit")) return rc;
  FillWs w;
  if (int rc = check_ws(p, ws, ws_bytes, &w, "gsmpm_fill_emit")) return rc;
  if (p->capacity == 0) return GSMPM_OK;
  GSMPM_REQUIRE(out_pos, "gsmpm_fill_emit: null output");
  const int ng = p->n_grid;
  const size_t n3 = (size_t)ng * ng * ng;
  k_fill_emit<<<grid_for(n3, 256), 256, 0, (hipStream_t)stream>>>(w.interior, w.inc, ng,
                                                                  (float)(p->grid_extent / ng), p->per_cell, p->seed,
                                                                  (unsigned long long)p->capacity, out_pos);
  GSMPM_LAUNCH_CHECK();
  return GSMPM_OK;
}

int gsmpm_fill_nearest(const float* query, int64_t n_query, const float* source, int64_t n_source, int32_t* index,
                       void* stream) {
  GSMPM_REQUIRE(n_query >= 0 && n_query < (int64_t(1) << 31), "gsmpm_fill_nearest: query count outside 0..2^31-1");
  GSMPM_REQUIRE(n_source >= 1 && n_source < (int64_t(1) << 31), "gsmpm_fill_nearest: source count outside 1..2^31-1");
  GSMPM_REQUIRE(source, "gsmpm_fill_nearest: null source array");
  if (n_query == 0) return GSMPM_OK;
  GSMPM_REQUIRE(query && index, "gsmpm_fill_nearest: null argument");
  k_fill_nearest<<<div_up((long)n_query, 256 * kNearQpt), 256, 0, (hipStream_t)stream>>>(query, (long)n_query, source,
                                                                                        (long)n_source, index);
  GSMPM_LAUNCH_CHECK();
  return GSMPM_OK;
}

int gsmpm_fill_get_grid(const gsmpm_fill_params* p, const void* ws, uint64_t ws_bytes, int32_t which, void* out,
                        void* stream) {
  if (int rc = check_params(p, "gsmpm_fill_get_grid")) return rc;
  FillWs w;
  if (int rc = check_ws(p, ws, ws_bytes, &w, "gsmpm_fill_get_grid")) return rc;
  GSMPM_REQUIRE(out, "gsmpm_fill_get_grid: null output");
  GSMPM_REQUIRE(which >= GSMPM_FILL_DENSITY && which <= GSMPM_FILL_DENSITY_FIXED, "gsmpm_fill_get_grid: unknown grid");
  hipStream_t st = (hipStream_t)stream;
  const size_t n3 = (size_t)p->n_grid * p->n_grid * p->n_grid;
  switch (which) {
    case GSMPM_FILL_DENSITY:
      k_fill_density_f32<<<grid_for(n3, 256), 256, 0, st>>>(w.dens, n3, (float*)out);
      GSMPM_LAUNCH_CHECK();
      break;
    case GSMPM_FILL_OCCUPIED:
      GSMPM_HIP(hipMemcpyAsync(out, w.occ, n3, hipMemcpyDeviceToDevice, st));
      break;
    case GSMPM_FILL_INTERIOR:
      GSMPM_HIP(hipMemcpyAsync(out, w.interior, n3, hipMemcpyDeviceToDevice, st));
      break;
    case GSMPM_FILL_BITS:
      GSMPM_HIP(hipMemcpyAsync(out, w.bits, 2 * n3, hipMemcpyDeviceToDevice, st));
      break;
    default:
      GSMPM_HIP(hipMemcpyAsync(out, w.dens, 8 * n3, hipMemcpyDeviceToDevice, st));
      break;
  }
  return GSMPM_OK;
}

}  // extern "C"
