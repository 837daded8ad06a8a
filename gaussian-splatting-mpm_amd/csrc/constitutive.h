// constitutive.h -- return mapping + Kirchhoff stress per material
// (mpm_solver/constitutive_models.py, dispatched as utils.py:13-54).
#pragma once
#include "mpm_common.h"
#include "svd3.h"

namespace gsmpm {

// ---------------------------------------------------- constitutive models --
// Material codes as template: 0 = jelly as written (zero stress),
// 1 metal, 2 sand, 3 foam, 4 = jelly with FCR (F3 fixed), 5 = the cohesive
// fluid of fluid_return_mapping (constitutive_models.py:142-213), which the
// reference defines but never dispatches (utils.py:13-54 has no branch for
// it); here it is paired with the StVK Kirchhoff stress its viscoplastic
// sibling (material 3) uses.
//
// The stress needs the SVD of the returned F (utils.py:32-52 takes a second
// ti.svd).  Where the return map left F unchanged that is the SVD it already
// took (the same input, so the same factors, bit for bit); where it set
// F = U diag(se) V^T the factors are U, se, V, and the stresses below are
// isotropic functions of F (any SVD of it gives the same U f(s) V^T), so the
// second SVD is skipped on both branches.  The difference from a fresh SVD of
// the rounded product is rounding-level.  Foam (material 3) forms its new F
// element-wise, which is no SVD of anything, so its plastic lanes
// take the second SVD.  GSMPM_SVD_REUSE=0 at build time: always two SVDs.
#ifndef GSMPM_SVD_REUSE
#define GSMPM_SVD_REUSE 1
#endif
// GSMPM_LOG_REUSE=0 (A/B): metal's stress takes its three logs again even
// where the return map kept F
#ifndef GSMPM_LOG_REUSE
#define GSMPM_LOG_REUSE 1
#endif
// EXACT (the mixed dispatch below): the reference's own arithmetic -- the
// correctly rounded SVD for every material and a second SVD of the returned F
// for the stress, no reuse.  Where materials are salted particle by particle
// a stress-free row integrates the velocity gradient its foam and metal
// neighbours' stresses leave on the grid, and the two shortcuts together put
// such a scene 14x further from the oracle (30 substeps, non-foam F_trial
// 3.2e-4 against 2.3e-5 with every body exact); either one
// alone changes nothing.
// GSMPM_MIXED_EXACT (build time): the materials whose mixed body is the EXACT
// form, one bit per kernel code.  Default metal alone: its log-strain return
// map with hardening is what the shortcuts disturb (salt layout, non-foam
// F_trial, fused / phased: none 3.2e-4 / 4.6e-4, sand 3.1e-4 / 3.6e-4, foam
// 3.2e-4 / 4.6e-4, metal 5.5e-5 / 8.9e-5, metal + foam the same, all four
// 2.3e-5 / 4.0e-5), and the exact form costs a metal wave ~10 us a launch.
// Bit 5 is the fluid's: clear, so a fluid row of a mixed handle runs the body
// of the uniform fluid kernel bit for bit.
#ifndef GSMPM_MIXED_EXACT
#define GSMPM_MIXED_EXACT 0x2
#endif
template <int MAT, bool EXACT = false>
__device__ __forceinline__ void return_map_and_stress(float (&F)[3][3], float mu, float lam, float& yld, float dt,
                                                      const MatConsts& mc, float (&tau)[3][3]) {
  float U[3][3], V[3][3], s[3];
  bool fresh = false;  // F changed in a way U, s, V do not describe: take its SVD
  // metal whose F the return map left unchanged: the stress's log(max(s, 0.01))
  // and its StVK diagonal are the return map's eps and t3 (the same f32
  // operations on the same s, utils.py:23-38 vs constitutive_models.py:62-75)
  bool kept = false;
  float t3_k[3] = {0.f, 0.f, 0.f};
  constexpr bool kFast = MAT != 3 && !EXACT;  // foam's plastic F depends on the SVD basis (svd3.h)
  constexpr bool kReuse = GSMPM_SVD_REUSE != 0 && !EXACT;
  if constexpr (MAT == 1) {
    // von_mises_return_mapping, constitutive_models.py:62-103
    svd3<kFast>(F, U, s, V);
    float eps[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) eps[d] = logf(fmaxf(s[d], 0.01f));
    const float tr = eps[0] + eps[1] + eps[2];
    const float temp = tr / 3.0f;
    float t3[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) t3[d] = 2.0f * mu * eps[d] + lam * tr * 1.0f;
    const float st = t3[0] + t3[1] + t3[2];
    float cond[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) cond[d] = t3[d] - st / 3.0f;
    const float cn = sqrtf(cond[0] * cond[0] + cond[1] * cond[1] + cond[2] * cond[2]);
    kept = !(cn > yld);
#pragma unroll
    for (int d = 0; d < 3; ++d) t3_k[d] = t3[d];
    if (cn > yld) {
      float eh[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) eh[d] = eps[d] - temp;
      const float ehn = sqrtf(eh[0] * eh[0] + eh[1] * eh[1] + eh[2] * eh[2]) + 1e-6f;
      const float dg = ehn - yld / (2.0f * mu);
      float se[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) se[d] = expf(eps[d] - (dg / ehn) * eh[d]);
      usv(U, se, V, F);
#pragma unroll
      for (int d = 0; d < 3; ++d) s[d] = se[d];
      if (mc.hardening == 1.0f) yld += 2.0f * mu * mc.xi * dg;
    }
  } else if constexpr (MAT == 2) {
    // sand_return_mapping, constitutive_models.py:105-140
    svd3<kFast>(F, U, s, V);
    float eps[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) eps[d] = logf(fmaxf(fabsf(s[d]), 1e-14f));
    const float tr = eps[0] + eps[1] + eps[2];
    float eh[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) eh[d] = eps[d] - tr / 3.0f;
    const float ehn = sqrtf(eh[0] * eh[0] + eh[1] * eh[1] + eh[2] * eh[2]);
    const float dg = ehn + (3.0f * lam + 2.0f * mu) / (2.0f * mu) * tr * mc.alpha;
    if (dg > 0.0f) {
      if (tr > 0.0f) {
        mmT(U, V, F);
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] = 1.0f;
      } else {
        float sn[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) sn[d] = expf(eps[d] - eh[d] * (dg / ehn));
        usv(U, sn, V, F);
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] = sn[d];
      }
    }
  } else if constexpr (MAT == 3) {
    // viscoplasticity_return_mapping_with_StVK, constitutive_models.py:216-259
    svd3<kFast>(F, U, s, V);
    float sg[3], eps[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      sg[d] = fmaxf(s[d], 0.01f);
      eps[d] = logf(sg[d]);
    }
    const float tr = eps[0] + eps[1] + eps[2];
    float stv[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) stv[d] = 2.0f * mu * (eps[d] - tr / 3.0f);
    const float stn = sqrtf(stv[0] * stv[0] + stv[1] * stv[1] + stv[2] * stv[2]);
    const float y = stn - 0.8f * sqrtf(2.0f / 3.0f) * yld;
    if (y > 0.0f) {
      const float mu_hat = mu * (sg[0] * sg[0] + sg[1] * sg[1] + sg[2] * sg[2]) / 3.0f;
      const float snn = stn - y / (1.0f + mc.pvisc * 2.0f / (2.0f * mu_hat * dt));
      // element-wise U * diag * V^T (constitutive_models.py:256)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float en = 1.0f / (2.0f * mu) * ((snn / stn) * stv[i]) + tr / 3.0f;
          const float se = (i == j) ? expf(en) : 0.0f;
          F[i][j] = U[i][j] * se * V[j][i];
        }
      fresh = true;
    }
  }
  else if constexpr (MAT == 5) {
    // fluid_return_mapping, constitutive_models.py:142-213
    svd3<kFast>(F, U, s, V);
    float eps[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) eps[d] = logf(fmaxf(fabsf(s[d]), 0.01f));
    const float tr = eps[0] + eps[1] + eps[2];
    float stv[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) stv[d] = 2.0f * mu * (eps[d] - tr / 3.0f);
    const float stn = sqrtf(stv[0] * stv[0] + stv[1] * stv[1] + stv[2] * stv[2]);
    const float y = stn - sqrtf(2.0f / 3.0f) * yld;
    if (y > 0.0f) {
      const float mu_hat = mu * (s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) / 3.0f;
      const float pf = 1.0f + mc.pvisc / (2.0f * mu_hat * dt);
      const float snn = stn - y / pf;
      float se[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) se[d] = expf(1.0f / (2.0f * mu) * ((snn / stn) * stv[d]) + tr / 3.0f);
      usv(U, se, V, F);  // a true matrix product here (U @ sig_elastic @ V^T, :205)
#pragma unroll
      for (int d = 0; d < 3; ++d) s[d] = se[d];
    }
  }
  // Kirchhoff stress of the (returned) F, utils.py:32-52
  float T[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[i][j] = 0.0f;
  if constexpr (MAT != 0) {
    if (MAT == 4 || !kReuse || fresh) svd3<kFast>(F, U, s, V);
    if constexpr (MAT == 1 || MAT == 3 || MAT == 5) {
      // kirchoff_stress_StVK, constitutive_models.py:23-38
      float tv[3];
      if (MAT == 1 && kReuse && GSMPM_LOG_REUSE && kept) {
#pragma unroll
        for (int d = 0; d < 3; ++d) tv[d] = t3_k[d];
      } else {
        float ls[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) ls[d] = logf(fmaxf(s[d], 0.01f));
        const float lss = ls[0] + ls[1] + ls[2];
#pragma unroll
        for (int d = 0; d < 3; ++d) tv[d] = 2.0f * mu * ls[d] + lam * lss * 1.0f;
      }
      float W[3][3];
      usv(U, tv, V, W);
      mmT(W, F, T);
    } else if constexpr (MAT == 2) {
      // kirchoff_stress_Drucker_Prager, constitutive_models.py:41-58
      const float lss = logf(s[0]) + logf(s[1]) + logf(s[2]);
      float cv[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) cv[d] = 2.0f * mu * logf(s[d]) / s[d] + lam * lss / s[d];
      float W[3][3];
      usv(U, cv, V, W);
      mmT(W, F, T);
    } else if constexpr (MAT == 4) {
      // kirchoff_stress_FCR, constitutive_models.py:10-20
      const float J = det3(F);
      float R[3][3], D[3][3];
      mmT(U, V, R);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) D[i][j] = 2.0f * mu * (F[i][j] - R[i][j]);
      mmT(D, F, T);
      const float l = lam * J * (J - 1.0f);
      T[0][0] += l;
      T[1][1] += l;
      T[2][2] += l;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tau[i][j] = (T[i][j] + T[j][i]) / 2.0f;
}

// ------------------------------------------------------ mixed materials --
// Template code 6: the material is a per-particle f32 (the reference's
// model.material), dispatched per particle as utils.py:13-54 does.
constexpr int kMatMixed = 6;

// Kernel code of a stored material value, by the reference's own comparisons:
// m == 1 metal, m == 2 sand, m == 3 foam; anything else (0, other numbers,
// non-integers, NaN) is its `else` branch, F = F_trial with the jelly stress
// rule of the handle (`jelly`: 0 = zero stress as written, 4 = FCR).  m == 5
// is the fluid (GSMPM_MAT_FLUID), a comparison the reference does not have:
// the one stored value read differently from its `else`.
__device__ __forceinline__ int material_code(float m, int jelly) {
  return m == 1.0f ? 1 : (m == 2.0f ? 2 : (m == 3.0f ? 3 : (m == 5.0f ? 5 : jelly)));
}

// The per-particle dispatch around the bodies above.  Every lane that
// holds a particle calls it (the caller's `if (k < cnt)`).  Each trip takes
// the code of the first pending lane (readfirstlane), ballots the lanes that
// share it and makes one scalar branch into that material's body with the
// other lanes masked off.  Particles are stored in bin order, so the waves of
// a region-painted scene almost always hold one code: they make one trip --
// one ballot and one scalar branch on top of the uniform kernel -- and a
// wave with k distinct codes makes k <= 5 trips (jelly, metal, sand, foam,
// fluid: a handle has one jelly rule).  Both kinds of wave run the
// same single copy of each body, so a particle's result does not depend on
// which other particles share its wave.  Metal's body is the EXACT form.
__device__ __forceinline__ void return_map_and_stress_mixed(int code, float (&F)[3][3], float mu, float lam, float& yld,
                                                            float dt, const MatConsts& mc, float (&tau)[3][3]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) tau[i / 3][i % 3] = 0.0f;
  unsigned long long pending = __ballot(1);  // the lanes that called
  while (pending) {  // wave-uniform: one trip per distinct code of the wave
    // the first pending lane's code (the first trip's is the first active lane: a readfirstlane)
    const int c = __builtin_amdgcn_readlane(code, __ffsll(pending) - 1);
    const bool mine = code == c;  // a finished lane's code differs from every later trip's
    if (mine) {
      switch (c) {  // c is uniform: a scalar branch
        case 1: return_map_and_stress<1, ((GSMPM_MIXED_EXACT >> 1) & 1) != 0>(F, mu, lam, yld, dt, mc, tau); break;
        case 2: return_map_and_stress<2, ((GSMPM_MIXED_EXACT >> 2) & 1) != 0>(F, mu, lam, yld, dt, mc, tau); break;
        case 3: return_map_and_stress<3, ((GSMPM_MIXED_EXACT >> 3) & 1) != 0>(F, mu, lam, yld, dt, mc, tau); break;
        case 4: return_map_and_stress<4, ((GSMPM_MIXED_EXACT >> 4) & 1) != 0>(F, mu, lam, yld, dt, mc, tau); break;
        case 5: return_map_and_stress<5, ((GSMPM_MIXED_EXACT >> 5) & 1) != 0>(F, mu, lam, yld, dt, mc, tau); break;
        default: break;  // jelly as written: F kept, zero stress
      }
    }
    pending &= ~__ballot(mine);
  }
}

}  // namespace gsmpm
