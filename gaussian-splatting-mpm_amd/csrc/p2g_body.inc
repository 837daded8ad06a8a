// p2g_body.inc -- the body of k_p2g<MAT> and k_p2g_mixed (mpm.hip), included
// inside both kernels and their driver entry points (k_p2g_drv,
// k_p2g_mixed_drv): it reads their arguments, MAT, the material ids `mi`, DRV
// and the drivers' selection `ds` by name.
#ifndef GSMPM_P2G_BODY_INCLUDER
#error "p2g_body.inc is the body of k_p2g / k_p2g_mixed: it is included inside those two kernels in mpm.hip only"
#endif
  // channel-planar window: a wave's 8-byte atomics to random nodes of one
  // channel spread over all 64 banks (the node-interleaved float4 layout put
  // every channel on 16 of them: 75 % of LDS cycles were bank conflicts)
  __shared__ unsigned long long s_acc[4 * kWin];
  __shared__ float s_max[4];
  stamp(0, 0);
  const int nch = ck.nchunk[0];
  for (int w = blockIdx.x; w < nch; w += gridDim.x) {
    const int4 cr = ck.chunk[w];
    const int t = cr.x, first = cr.y, cnt = cr.z;
    const int k = threadIdx.x;
    if (t == tl.ntiles) {
      // particles outside the grid: bounds-checked global f32 atomics (reference UB region)
      if (k < cnt) {
        const int p = ck.list[first + k];
        float x[3], v[3], C[3][3], m, nvt[3][3];
        particle_front<MAT, DRV>(ps, p, bct, mask, dt, mc, mi, x, v, C, m, nvt, ds);
        p2g_global<MAT>(x, v, C, m, nvt, g, dt, gacc);
      }
      continue;  // workgroup-uniform
    }
    const int tx = t / (tl.td * tl.td), ty = (t / tl.td) % tl.td, tz = t % tl.td;
    for (int q = k; q < kWin * 4; q += kChunk) s_acc[q] = 0ull;
    float x[3], v[3], C[3][3], m = 0.f, nvt[3][3];
    int base[3] = {0, 0, 0};
    float fx[3] = {1.f, 1.f, 1.f}, ww[3][3], dw[3][3];
    float bound = 0.f;
    if (k < cnt) {
      const int p = ck.list[first + k];
      particle_front<MAT, DRV>(ps, p, bct, mask, dt, mc, mi, x, v, C, m, nvt, ds);
      bspline(x, g.inv_dx, base, fx, ww, dw);
      {  // non-finite scatter inputs (the fixed-point conversion would hide them; fused.h)
        float chk = m + v[0] + v[1] + v[2];
#pragma unroll
        for (int i = 0; i < 9; ++i) chk += nvt[i / 3][i % 3] + C[i / 3][i % 3];
        if (!__builtin_isfinite(chk)) *nonfin = 1;
      }
      float vm = 0.f, cm = 0.f, sm = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        vm = fmaxf(vm, fabsf(v[r]));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          cm = fmaxf(cm, fabsf(C[r][c]));
          sm = fmaxf(sm, fabsf(nvt[r][c]));
        }
      }
      // |m v + m C dpos| <= m (|v| + 3 * 1.5 dx |C|), |dt nvt dweight| <= dt * 3 * 1.5 inv_dx |nvt|
      bound = fmaxf(m, m * (vm + 4.5f * g.dx * cm) + dt * 4.5f * g.inv_dx * sm) * 1.01f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bound = fmaxf(bound, __shfl_xor(bound, o));
    if ((k & 63) == 0) s_max[k >> 6] = bound;
    __syncthreads();  // also orders the window zeroing before the adds
    if (w == (int)blockIdx.x) {
      stamp(0, 2);
      stamp_val(0, 5, cnt);
      stamp_val(0, 6, GSMPM_HWREG(4));  // HW_ID
    }
    const float bmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    int ebits;
    frexpf(bmax, &ebits);                     // bmax < 2^ebits
    // every contribution below 2^50 (to_fixed needs < 2^51); a node sums <= 256 of them
    const int S = bmax > 0.f ? 50 - ebits : 0;
    if (k < cnt) {
      const int l0 = base[0] - tx * kTile, l1 = base[1] - ty * kTile, l2 = base[2] - tz * kTile;
      p2g_scatter<MAT>(s_acc + ((l0 * kTW + l1) * kTW + l2), fx, ww, dw, v, C, m, nvt, g, dt, ldexp(1.0, S));
    }
    __syncthreads();
    if (w == (int)blockIdx.x) stamp(0, 3);
    float* dst = reinterpret_cast<float*>(slots + (size_t)w * kWin);
    for (int q = k; q < kWin * 4; q += kChunk)
      dst[q] = (float)ldexp((double)(long long)s_acc[(q & 3) * kWin + (q >> 2)], -S);
    __syncthreads();  // LDS reuse by the next chunk
    if (w == (int)blockIdx.x) stamp(0, 4);
  }
  stamp(0, 1);
