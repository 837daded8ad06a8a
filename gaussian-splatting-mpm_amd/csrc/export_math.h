// export_math.h -- per-Gaussian float64 math of the 3DGS export pass
// (export.hip): symmetric 3x3 eigendecomposition -> log-scales + quaternion,
// and the rotation of one SH band by a 3x3 Q.  Plain C++ behind GSMPM_HD so
// that a host program can run the same lines; DESIGN.md 3.12 has the method.
#pragma once
#include <cmath>

#ifndef GSMPM_HD
#ifdef __HIPCC__
#define GSMPM_HD __host__ __device__ __forceinline__
#else
#define GSMPM_HD inline
#endif
#endif
#ifndef GSMPM_TABLE
#ifdef __HIPCC__
#define GSMPM_TABLE __constant__ const
#else
#define GSMPM_TABLE static const
#endif
#endif

namespace gsmpm {
namespace exportm {

// Eigenvalue floors (on lambda = scale^2).  Relative: f64 Jacobi leaves an
// absolute error of a few 1e-16 lambda_max in every eigenvalue, so anything
// below 1e-14 lambda_max is noise of the solve (and already far below the
// 6e-8 lambda_max the f32 input resolves).  Absolute: keeps log() finite for
// the zero matrix and exp(log_scale)^2 a normal f32.
constexpr double kEigRelFloor = 1e-14;
constexpr double kEigAbsFloor = 1e-36;
constexpr int kJacobiSweeps = 8;  // 3x3 f64 converges in 4-5; fixed, no convergence test

// One Jacobi rotation that zeroes a_pq; r is the third index.  vp / vq are
// columns p and q of the eigenvector matrix.  Branch-free: a zero (or, against
// the diagonal gap, vanishing) a_pq gives t = 0, the identity.
GSMPM_HD void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double vp[3],
                            double vq[3]) {
  const double theta = (aqq - app) / (2.0 * apq);      // inf / nan when apq == 0: t is selected to 0 below
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));  // theta^2 = inf -> t = 0
  t = (apq == 0.0 || t != t) ? 0.0 : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  for (int i = 0; i < 3; ++i) {
    const double a = vp[i], b = vq[i];
    vp[i] = c * a - s * b;
    vq[i] = s * a + c * b;
  }
}

GSMPM_HD void order_desc(double& la, double& lb, double va[3], double vb[3]) {
  const bool sw = lb > la;
  const double l0 = sw ? lb : la, l1 = sw ? la : lb;
  la = l0;
  lb = l1;
  for (int i = 0; i < 3; ++i) {
    const double a = va[i], b = vb[i];
    va[i] = sw ? b : a;
    vb[i] = sw ? a : b;
  }
}

// cov6 (xx, xy, xz, yy, yz, zz) -> log_scale[3] (descending), quat[4] (w, x, y, z; unit, w >= 0) with
// R(quat) diag(exp(2 log_scale)) R(quat)^T = cov up to the floors.  Returns true for a row with a
// non-finite entry (identity quaternion, floor scale).
GSMPM_HD bool cov_to_scale_rot(const float cov[6], float log_scale[3], float quat[4]) {
  bool bad = false;
  for (int i = 0; i < 6; ++i) bad = bad || !(fabsf(cov[i]) <= 3.4028234663852886e38f);
  double a00 = cov[0], a01 = cov[1], a02 = cov[2], a11 = cov[3], a12 = cov[4], a22 = cov[5];
  if (bad) a00 = a01 = a02 = a11 = a12 = a22 = 0.0;
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);  // (p, q) = (0, 1), r = 2
    jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);  // (0, 2), r = 1
    jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);  // (1, 2), r = 0
  }
  order_desc(a00, a11, v0, v1);
  order_desc(a00, a22, v0, v2);
  order_desc(a11, a22, v1, v2);
  // proper rotation: det [v0 v1 v2] = v0 . (v1 x v2)
  const double det = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v0[1] * (v1[0] * v2[2] - v1[2] * v2[0]) +
                     v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
  if (det < 0.0)
    for (int i = 0; i < 3; ++i) v2[i] = -v2[i];
  const double floor = fmax(kEigRelFloor * a00, kEigAbsFloor);
  log_scale[0] = (float)(0.5 * log(fmax(a00, floor)));
  log_scale[1] = (float)(0.5 * log(fmax(a11, floor)));
  log_scale[2] = (float)(0.5 * log(fmax(a22, floor)));
  // Shepperd: divide by the largest of (trace, r00, r11, r22) so that w = 0 (180 degrees) is exact.
  // R[i][j] = v_j[i].
  const double r00 = v0[0], r10 = v0[1], r20 = v0[2], r01 = v1[0], r11 = v1[1], r21 = v1[2], r02 = v2[0],
               r12 = v2[1], r22 = v2[2];
  const double tr = r00 + r11 + r22;
  double w, x, y, z;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const double s = 2.0 * sqrt(fmax(1.0 + tr, 0.0));
    w = 0.25 * s, x = (r21 - r12) / s, y = (r02 - r20) / s, z = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const double s = 2.0 * sqrt(fmax(1.0 + r00 - r11 - r22, 0.0));
    w = (r21 - r12) / s, x = 0.25 * s, y = (r01 + r10) / s, z = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const double s = 2.0 * sqrt(fmax(1.0 + r11 - r00 - r22, 0.0));
    w = (r02 - r20) / s, x = (r01 + r10) / s, y = 0.25 * s, z = (r12 + r21) / s;
  } else {
    const double s = 2.0 * sqrt(fmax(1.0 + r22 - r00 - r11, 0.0));
    w = (r10 - r01) / s, x = (r02 + r20) / s, y = (r12 + r21) / s, z = 0.25 * s;
  }
  const double inv = (w < 0.0 ? -1.0 : 1.0) / sqrt(w * w + x * x + y * y + z * z);
  quat[0] = (float)(w * inv + 0.0);  // + 0.0: no negative zero in w
  quat[1] = (float)(x * inv);
  quat[2] = (float)(y * inv);
  quat[3] = (float)(z * inv);
  return bad;
}

#include "sh_rot_tables.inc"

constexpr double kC1 = 0.4886025119029199;
constexpr double kC2a = 1.0925484305920792, kC2b = 0.31539156525252005, kC2c = 0.5462742152960396;
constexpr double kC3a = 0.5900435899266435, kC3b = 2.890611442640554, kC3c = 0.4570457994644658,
                 kC3d = 0.3731763325901154, kC3e = 1.445305721320277;

// Y_lm(d) of band L in the rasterizer's basis (signs and constants of kSH_C1..3, raster.hip).
template <int L>
GSMPM_HD void sh_band(double x, double y, double z, double Y[2 * L + 1]) {
  if (L == 1) {
    Y[0] = -kC1 * y, Y[1] = kC1 * z, Y[2] = -kC1 * x;
  } else {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    if (L == 2) {
      Y[0] = kC2a * xy, Y[1] = -kC2a * yz, Y[2] = kC2b * (2.0 * zz - xx - yy), Y[3] = -kC2a * xz;
      Y[4] = kC2c * (xx - yy);
    } else {
      Y[0] = -kC3a * y * (3.0 * xx - yy), Y[1] = kC3b * xy * z, Y[2] = -kC3c * y * (4.0 * zz - xx - yy);
      Y[3] = kC3d * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), Y[4] = -kC3c * x * (4.0 * zz - xx - yy);
      Y[5] = kC3e * z * (xx - yy), Y[6] = -kC3a * x * (xx - 3.0 * yy);
    }
  }
}

// Rotates the 2L+1 coefficients of band L, c[m*3 + ch] (three channels interleaved, as in shs[P,M,3]),
// in place: c' = A^+ B c with A[k][m] = Y_lm(d_k) over NS fixed sample directions (constant; its
// pseudo-inverse is the table) and B[k][m] = Y_lm(Q d_k), i.e. the least-squares c' with
// sum_m c'_m Y_lm(d_k) = sum_m c_m Y_lm(Q d_k).  For orthogonal Q both sides lie in the band's
// 2L+1-dimensional space and the fit is exact for every d; NS = 2 (2L+1) for L >= 2 keeps it close to
// the best in-band answer when Q is off orthogonal by rounding (tools/sh_rot_tables.py).
template <int L, int NS>
GSMPM_HD void sh_rotate_band(const double Q[9], float* c, const double* dir, const double* pinv) {
  constexpr int N = 2 * L + 1;
  double cin[N][3], acc[N][3];
#pragma unroll
  for (int m = 0; m < N; ++m)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) cin[m][ch] = (double)c[m * 3 + ch], acc[m][ch] = 0.0;
  // rolled over the samples: one direction and one column of the table per trip (scalar loads),
  // not the whole table held in registers; cin / acc keep compile-time indices
#pragma unroll 1
  for (int k = 0; k < NS; ++k) {
    const double dx = dir[k * 3], dy = dir[k * 3 + 1], dz = dir[k * 3 + 2];
    const double ex = fma(Q[0], dx, fma(Q[1], dy, Q[2] * dz));
    const double ey = fma(Q[3], dx, fma(Q[4], dy, Q[5] * dz));
    const double ez = fma(Q[6], dx, fma(Q[7], dy, Q[8] * dz));
    double Y[N], t[3];
    sh_band<L>(ex, ey, ez, Y);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < N; ++m) s = fma(Y[m], cin[m][ch], s);
      t[ch] = s;
    }
#pragma unroll
    for (int m = 0; m < N; ++m) {
      const double w = pinv[m * NS + k];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[m][ch] = fma(w, t[ch], acc[m][ch]);
    }
  }
#pragma unroll
  for (int m = 0; m < N; ++m)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[m * 3 + ch] = (float)acc[m][ch];
}

// bands 1..D of one Gaussian's coefficient row (row[m*3 + ch], m < (D+1)^2), in place
GSMPM_HD void sh_rotate_row(const double Q[9], int D, float* row) {
  if (D >= 1) sh_rotate_band<1, 3>(Q, row + 1 * 3, kShDir1, kShPinv1);
  if (D >= 2) sh_rotate_band<2, 10>(Q, row + 4 * 3, kShDir2, kShPinv2);
  if (D >= 3) sh_rotate_band<3, 14>(Q, row + 9 * 3, kShDir3, kShPinv3);
}

}  // namespace exportm
}  // namespace gsmpm
