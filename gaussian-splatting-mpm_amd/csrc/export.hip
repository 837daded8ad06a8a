// export.hip -- deformed Gaussians back to the 3DGS file format's parameters:
// a per-Gaussian symmetric 3x3 eigendecomposition (covariance -> log-scales
// and a proper-rotation quaternion) and the rotation of the SH coefficient
// bands 1..3 by the per-Gaussian Q of gsmpm_raster_args.sh_rotations.  A
// once-per-saved-frame pass, not the substep: the arithmetic is float64
// (export_math.h), the kernels are shaped by their memory access alone.
// DESIGN.md 3.12 has the method, the floors and the measured numbers.
//
//  access    one Gaussian is 24 B of covariance, 28 B of output, 36 B of Q and
//            up to 192 B of SH: a thread that walked its own row would touch a
//            new cache line with every load.  Both kernels therefore move a
//            tile of 256 Gaussians between global memory and LDS with
//            consecutive lanes on consecutive words, and a thread reads and
//            writes its Gaussian's row in LDS.  The LDS row strides are odd
//            (7, 5, 3, 9 and 3K | 1 words), so the 32 lanes of a ds access
//            group fall on 32 different banks.
//  sh tile   only the coefficients that change, bands 1..D, are staged; band 0
//            and every coefficient past (D+1)^2 go from the load straight to
//            the output (bit-identical by construction), which also bounds
//            the LDS use for any M.  A block has read its whole tile before it
//            writes any of it, so out may alias shs.
//  grid      grid-stride over tiles; no atomics but one add per block into the
//            optional bad-row counter.
#include "common.h"

#include "export_math.h"

namespace gsmpm {

namespace {

constexpr int kExpBlk = 256;
constexpr int kExpMaxGrid = 2048;
constexpr int kShMaxStride = 49;  // 3 * 16 | 1

__global__ __launch_bounds__(kExpBlk) void k_cov_to_scale_rot(const float* __restrict__ cov6, long n,
                                                              float* __restrict__ log_scale,
                                                              float* __restrict__ quat,
                                                              unsigned long long* __restrict__ n_bad) {
  __shared__ float s_cov[kExpBlk * 7];
  __shared__ float s_ls[kExpBlk * 3];
  __shared__ float s_q[kExpBlk * 5];
  const int tid = threadIdx.x;
  const long tiles = (n + kExpBlk - 1) / kExpBlk;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long p0 = tile * kExpBlk;
    const int np = (int)((n - p0 < kExpBlk) ? (n - p0) : kExpBlk);
    for (int i = tid; i < np * 6; i += kExpBlk) s_cov[(i / 6) * 7 + i % 6] = cov6[p0 * 6 + i];
    __syncthreads();
    bool bad = false;
    if (tid < np) {
      float c[6], ls[3], q[4];
#pragma unroll
      for (int i = 0; i < 6; ++i) c[i] = s_cov[tid * 7 + i];
      bad = exportm::cov_to_scale_rot(c, ls, q);
#pragma unroll
      for (int i = 0; i < 3; ++i) s_ls[tid * 3 + i] = ls[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) s_q[tid * 5 + i] = q[i];
    }
    const int nb = __syncthreads_count(bad);  // also the barrier between the LDS writes and the stores
    if (tid == 0 && nb > 0 && n_bad) atomicAdd(n_bad, (unsigned long long)nb);
    for (int i = tid; i < np * 3; i += kExpBlk) log_scale[p0 * 3 + i] = s_ls[i];
    for (int i = tid; i < np * 4; i += kExpBlk) quat[p0 * 4 + i] = s_q[(i >> 2) * 5 + (i & 3)];
    __syncthreads();  // the next tile overwrites the LDS rows
  }
}

__global__ __launch_bounds__(kExpBlk) void k_sh_rotate(const float* shs, const float* __restrict__ Q, long n, int D,
                                                       int M, float* out) {
  __shared__ float s_c[kExpBlk * kShMaxStride];
  __shared__ float s_Q[kExpBlk * 9];
  const int tid = threadIdx.x;
  const int K3 = 3 * (D + 1) * (D + 1);  // staged words of a row are [3, K3)
  const int stride = K3 | 1;
  const long row = 3L * M;
  const long tiles = (n + kExpBlk - 1) / kExpBlk;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long p0 = tile * kExpBlk;
    const int np = (int)((n - p0 < kExpBlk) ? (n - p0) : kExpBlk);
    const float* src = shs + p0 * row;
    float* dst = out + p0 * row;
    const long total = np * row;
    for (long i = tid; i < total; i += kExpBlk) {
      const int p = (int)(i / row);
      const long j = i - p * row;
      const float v = src[i];
      if (j >= 3 && j < K3)
        s_c[p * stride + (int)j] = v;
      else
        dst[i] = v;
    }
    for (int i = tid; i < np * 9; i += kExpBlk) s_Q[i] = Q[p0 * 9 + i];
    __syncthreads();
    if (tid < np) {
      double q[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) q[i] = (double)s_Q[tid * 9 + i];
      exportm::sh_rotate_row(q, D, &s_c[tid * stride]);
    }
    __syncthreads();
    for (long i = tid; i < total; i += kExpBlk) {
      const int p = (int)(i / row);
      const long j = i - p * row;
      if (j >= 3 && j < K3) dst[i] = s_c[p * stride + (int)j];
    }
    __syncthreads();  // the next tile overwrites the LDS rows
  }
}

int grid_for_tiles(int64_t n) {
  const int64_t tiles = (n + kExpBlk - 1) / kExpBlk;
  return (int)(tiles < kExpMaxGrid ? tiles : kExpMaxGrid);
}

}  // namespace

}  // namespace gsmpm

using namespace gsmpm;

extern "C" {

int gsmpm_cov_to_scale_rot(const float* cov6, int64_t n, float* log_scale, float* quat, int64_t* n_bad, void* stream) {
  GSMPM_REQUIRE(n >= 0, "gsmpm_cov_to_scale_rot: negative count");
  if (n == 0) return GSMPM_OK;  // nothing to read or write: empty arrays may be null
  GSMPM_REQUIRE(cov6 && log_scale && quat, "gsmpm_cov_to_scale_rot: null argument");
  k_cov_to_scale_rot<<<grid_for_tiles(n), kExpBlk, 0, (hipStream_t)stream>>>(cov6, (long)n, log_scale, quat,
                                                                            (unsigned long long*)n_bad);
  GSMPM_LAUNCH_CHECK();
  return GSMPM_OK;
}

int gsmpm_sh_rotate(const float* shs, const float* Q, int64_t n, int32_t D, int32_t M, float* out, void* stream) {
  GSMPM_REQUIRE(n >= 0, "gsmpm_sh_rotate: negative count");
  GSMPM_REQUIRE(D >= 0 && D <= 3, "gsmpm_sh_rotate: degree outside 0..3");
  GSMPM_REQUIRE(M >= (D + 1) * (D + 1), "gsmpm_sh_rotate: fewer than (D+1)^2 coefficients");
  if (n == 0) return GSMPM_OK;  // nothing to read or write: empty arrays may be null
  GSMPM_REQUIRE(shs && Q && out, "gsmpm_sh_rotate: null argument");
  k_sh_rotate<<<grid_for_tiles(n), kExpBlk, 0, (hipStream_t)stream>>>(shs, Q, (long)n, D, M, out);
  GSMPM_LAUNCH_CHECK();
  return GSMPM_OK;
}

}  // extern "C"
