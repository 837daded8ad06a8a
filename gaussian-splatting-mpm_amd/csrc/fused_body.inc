// fused_body.inc -- the body of k_fused<MAT, MODE> and k_fused_mixed<MODE>
// (fused.h), included inside both kernels and their driver entry points: it
// reads their arguments, MAT, MODE, the material ids `mi`, DRV and the
// drivers' selection `ds` by name.
#ifndef GSMPM_FUSED_BODY_INCLUDER
#error "fused_body.inc is the body of k_fused / k_fused_mixed: it is included inside those two kernels in fused.h only"
#endif
  constexpr bool G2P = (MODE & 1) != 0, P2G = (MODE & 2) != 0;
  constexpr bool FOLD = G2P && (MODE & 4) != 0;  // the previous substep's grid update staged from its chunk windows
  __shared__ int s_fc0[27], s_fnc[27], s_fbx[27];  // FOLD: the 27 neighbour tiles' tables
  // FOLD: particles outside their chunk's window (escapes; rare): their stencil
  // nodes are evaluated by the whole workgroup into the upper half of s_acc
  // (free while G2P runs: the v window uses the lower half), kEscMax at a time
  constexpr int kEscMax = kFWin / 27;
  __shared__ int s_nesc;
  __shared__ int s_eb[3][kEscMax];
  // FOLD: the previous substep's grid step, and whether its P2G had escapes (uniform)
  GridStep fgs{};
  bool fesc = false;
  if constexpr (FOLD) {
    fgs.dt = dt;
    fgs.dgx = dt * rare->grav[0];
    fgs.dgy = dt * rare->grav[1];
    fgs.dgz = dt * rare->grav[2];
    fgs.mask = mask_prev;
    fgs.keep = 0;
    fesc = __builtin_amdgcn_readfirstlane(*rare->esc_prev) != 0;
  }
  // channel-planar u64 accumulators; the G2P v window aliases them (it is
  // consumed before the accumulators are zeroed)
  __shared__ unsigned long long s_acc[4 * kFWin];
  __shared__ float s_max[4];
  __shared__ int s_mxy[4], s_mz[4];
  __shared__ int s_cnt[27], s_base[27];
  __shared__ int s_rcnt[16];
  float4* s_win = reinterpret_cast<float4*>(s_acc);
  const int ng = g.ng;
  constexpr int SK = (MODE & 3) == 3 ? 0 : 1;  // diagnostics slot (k_p2g's / k_g2p's in the per-phase pipeline)
  sim_prio();
  stamp(SK, 0);
  // the first chunk's record, box and lane order are requested with the chunk
  // count (clamped: a workgroup past the last chunk discards them), which
  // takes dependent round trips off every workgroup's chain (the same for
  // every further chunk: its record, box and lane order are requested while
  // the chunk before it is processed).  The empty asm takes the pointers
  // into SGPRs in the first argument batch and the loads go through the
  // global address space as vector loads, so all four leave together: as
  // plain scalar loads the compiler serialised them -- box, then count, then
  // record, three memory round trips behind each other at the kernel start
  // (one shared lgkmcnt, argument reloads between them)
  // (all four unconditional, straight-line: an unused lane order reads
  // cbox[0] instead, selected away below)
  // use_box bit 0: the last launch did the P2G of these bins (cbox, perm are
  // this chunk's); bit 1: multi-chunk tiles store and publish boxes (below)
  const bool boxed = (use_box & 1) != 0, dense_box = (use_box & 2) != 0;
  const int w0 = min((int)blockIdx.x, tl.max_chunks - 1);
  const bool perm0 = boxed && tc.perm;
  const int* nch_p = ck.nchunk;
  const int4* chk_p = ck.chunk;
  const int* cbx_p = tc.cbox;
  const unsigned char* prm_p = perm0 ? tc.perm : reinterpret_cast<const unsigned char*>(tc.cbox);
  asm volatile("" : "+s"(nch_p), "+s"(chk_p), "+s"(cbx_p), "+s"(prm_p));
  typedef const int __attribute__((address_space(1)))* gint_p;
  typedef const unsigned char __attribute__((address_space(1)))* guc_p;
  const gint_p c4 = (gint_p)chk_p + 4 * (size_t)w0;
  const int r0 = c4[0], r1 = c4[1], r2 = c4[2], r3 = c4[3];
  const int bx0 = ((gint_p)cbx_p)[w0];
  const int qv0 = ((guc_p)prm_p)[perm0 ? (size_t)w0 * 256 + threadIdx.x : 0];
  const int nch = *(gint_p)nch_p;
  int4 cr_n = make_int4(r0, r1, r2, r3);
  int box_n = boxed ? bx0 : kFullBox;
  int q_n = perm0 ? qv0 : (int)threadIdx.x;
  for (int w = blockIdx.x; w < nch; w += gridDim.x) {
    const int4 cr = cr_n;
    const int cbox = box_n, q_lane = q_n;
    if (w + (int)gridDim.x < nch) {  // workgroup-uniform; chunk w + grid is only ever touched by this workgroup
      const int wn = w + gridDim.x;
      cr_n = ck.chunk[wn];
      box_n = boxed ? tc.cbox[wn] : kFullBox;
      q_n = (boxed && tc.perm) ? (int)tc.perm[(size_t)wn * 256 + threadIdx.x] : (int)threadIdx.x;
    }
    const int t = cr.x, first = cr.y, cnt = cr.z;
    const int k = threadIdx.x;
    const bool outside = t == tl.ntiles;  // workgroup-uniform
    int tx = 0, ty = 0, tz = 0;
    if (!outside) ftile_decode(tl, t, tx, ty, tz);
    const int o0 = tx * kFT0 - 1, o1 = ty * kFT1 - 1, o2 = tz * kFT2 - 1;  // first window node
    // lane e < 27: the touched position of tile T = t - (a, b, c), whose cover
    // record takes this chunk's stencil box as its neighbour e (published after
    // the P2G below); requested now, used at the end
    int tpos_e = -1;
    const int* __restrict__ tposp = rare->tpos;
    if (tposp && !outside && k < 27) {
      const int x0 = tx - (k / 9 - 1), y0 = ty - ((k / 3) % 3 - 1), z0 = tz - (k % 3 - 1);
      if ((unsigned)x0 < (unsigned)tl.td0 && (unsigned)y0 < (unsigned)tl.td1 && (unsigned)z0 < (unsigned)tl.td2)
        tpos_e = tposp[(x0 * tl.td1 + y0) * tl.td2 + z0];
    }
    int p = -1;
    float x[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f}, C[3][3], F[3][3], m = 0.f;
    // this lane's particle: the lane balance of the last P2G on these bins (use_box), else in order
    const int q = k >= cnt ? k : q_lane;
    // particle loads first: their round trips overlap the window staging
    if (k < cnt) {
      p = first + q;
#pragma unroll
      for (int d = 0; d < 3; ++d) x[d] = ps.ld(PX + d, p);
      if (G2P || MAT != 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i / 3][i % 3] = ps.ld(PF + i, p);
      }
      if (P2G) m = ps.ld(PMASS, p);
      if (!G2P) {
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = ps.ld(PV + d, p);
#pragma unroll
        for (int i = 0; i < 9; ++i) C[i / 3][i % 3] = ps.ld(PC + i, p);
      }
    }
    int eslot = -1;  // FOLD: this lane's escape slot (its stencil nodes at s_win[kFWin + 27 eslot ...])
    if constexpr (G2P) {
      if (FOLD && !outside) {
        // the 27 neighbour tiles' first chunk, chunk count and stencil box of the previous P2G (lanes 0..26)
        if (k < 27) {
          const int x0 = tx + k / 9 - 1, y0 = ty + (k / 3) % 3 - 1, z0 = tz + k % 3 - 1;
          int c0 = 0, nc = 0, bx = 0;
          if ((unsigned)x0 < (unsigned)tl.td0 && (unsigned)y0 < (unsigned)tl.td1 && (unsigned)z0 < (unsigned)tl.td2) {
            const int u = (x0 * tl.td1 + y0) * tl.td2 + z0;
            c0 = ck.cbase[u];
            nc = (ck.count[u] + kChunk - 1) / kChunk;
            bx = rare->tbox_prev[u];
          }
          s_fc0[k] = c0;
          s_fnc[k] = nc;
          s_fbx[k] = bx;
        }
        if (k == 0) s_nesc = 0;
        __syncthreads();
        // a lane whose particle left the window takes an escape slot (its base in s_eb)
        if (k < cnt) {
          int bq[3];
          base_of(x, g.inv_dx, bq);
          if (!(in_grid(x, g) && in_window(bq, o0, o1, o2))) {
            eslot = atomicAdd(&s_nesc, 1);
            if (eslot < kEscMax) {
              s_eb[0][eslot] = bq[0];
              s_eb[1][eslot] = bq[1];
              s_eb[2][eslot] = bq[2];
            }
          }
        }
        int lo[3], hi[3];
        box_unpack(cbox, lo, hi);
        const int n1 = hi[1] - lo[1] + 1, n2 = hi[2] - lo[2] + 1, n12 = n1 * n2;
        const int nvol = (hi[0] - lo[0] + 1) * n12;
        const float r12 = 1.0f / (float)n12, r2 = 1.0f / (float)n2;
        const float4* __restrict__ sp = rare->slots_prev;
        const BcTable* __restrict__ fbct = static_cast<const BcTable*>(rare->bct);
        auto tab = [&](int ci, int& c0, int& nc, int& q) {
          c0 = s_fc0[ci];
          nc = s_fnc[ci];
          q = s_fbx[ci];
        };
        // kFoldB nodes a lane at a time: all their cover loads in flight together
        for (int q0 = k; q0 < nvol; q0 += 256 * kFoldB) {
          FoldNode fn[kFoldB];
          int w3[kFoldB][3];
          bool gin[kFoldB], live[kFoldB];
#pragma unroll
          for (int u = 0; u < kFoldB; ++u) {
            const int qn = min(q0 + u * 256, nvol - 1);
            live[u] = q0 + u * 256 < nvol;
            const int a = (int)(((float)qn + 0.5f) * r12), rem = qn - a * n12;
            const int b = (int)(((float)rem + 0.5f) * r2), c = rem - b * n2;
            w3[u][0] = lo[0] + a;
            w3[u][1] = lo[1] + b;
            w3[u][2] = lo[2] + c;
            const int ix = o0 + w3[u][0], iy = o1 + w3[u][1], iz = o2 + w3[u][2];
            gin[u] = live[u] && (unsigned)ix < (unsigned)ng && (unsigned)iy < (unsigned)ng && (unsigned)iz < (unsigned)ng;
            fold_prep(w3[u], tab, fn[u]);
            if (!gin[u]) fn[u].on = 0;
          }
          float4 vv[kFoldB][8];
#pragma unroll
          for (int u = 0; u < kFoldB; ++u) fold_load(sp, fn[u], vv[u]);
#pragma unroll
          for (int u = 0; u < kFoldB; ++u) {
            const int ix = o0 + w3[u][0], iy = o1 + w3[u][1], iz = o2 + w3[u][2];
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gin[u]) {
              float4 sum = fold_acc(sp, w3[u], tab, fn[u], vv[u]);
              if (fesc) add4f(sum, rare->gacc_prev[((size_t)ix * ng + iy) * ng + iz]);
              val = node_update(sum, ix, iy, iz, g, fgs, fbct);
            }
            if (live[u]) s_win[(w3[u][0] * kFW1 + w3[u][1]) * kFW2 + w3[u][2]] = val;
          }
        }
        // the escaped particles' stencil nodes, one node a lane (workgroup-uniform skip when none)
        __syncthreads();
        const int ne = min(s_nesc, kEscMax);
        for (int t = k; t < ne * 27; t += 256) {
          const int sl = t / 27, qn = t - sl * 27;
          s_win[kFWin + t] = fold_node(s_eb[0][sl] + qn / 9, s_eb[1][sl] + (qn / 3) % 3, s_eb[2][sl] + qn % 3, g, tl,
                                       ck, rare, fgs, fbct, fesc);
        }
      } else if (!outside) {
        // the chunk's stencil box from its last P2G (particles unmoved since), else the whole window
        int lo[3], hi[3];
        box_unpack(cbox, lo, hi);
        const int n1 = hi[1] - lo[1] + 1, n2 = hi[2] - lo[2] + 1, n12 = n1 * n2;
        const int nvol = (hi[0] - lo[0] + 1) * n12;
        const float r12 = 1.0f / (float)n12, r2 = 1.0f / (float)n2;  // exact floor for q < 2^11
        constexpr int kStageU = (kFWin + 255) / 256;  // window nodes per lane, at most
        // all loads first, the out-of-grid zeroing as a select afterwards: a
        // zeroing branch right after each load made the compiler wait for
        // that load before issuing the next (the zeros and the in-flight load
        // share the registers), 7 round trips in a row instead of one
        float4 gv[kStageU];
        int dst[kStageU];
        bool gin[kStageU];
#pragma unroll
        for (int u = 0; u < kStageU; ++u) {
          const int qn = min(k + u * 256, nvol - 1);
          const int a = (int)(((float)qn + 0.5f) * r12), rem = qn - a * n12;
          const int b = (int)(((float)rem + 0.5f) * r2), c = rem - b * n2;
          const int wa = lo[0] + a, wb = lo[1] + b, wc = lo[2] + c;
          dst[u] = (wa * kFW1 + wb) * kFW2 + wc;
          const int ix = o0 + wa, iy = o1 + wb, iz = o2 + wc;
          gin[u] = (unsigned)ix < (unsigned)ng && (unsigned)iy < (unsigned)ng && (unsigned)iz < (unsigned)ng;
          gv[u] = gvel[gin[u] ? ((size_t)ix * ng + iy) * ng + iz : 0];
        }
#pragma unroll
        for (int u = 0; u < kStageU; ++u) {
          const float4 z = gv[u];
          const bool in = gin[u];
          const float4 val = make_float4(in ? z.x : 0.f, in ? z.y : 0.f, in ? z.z : 0.f, in ? z.w : 0.f);
          if (k + u * 256 < nvol) s_win[dst[u]] = val;
        }
      }
      if (k < 27) s_cnt[k] = 0;
      __syncthreads();
      if (w == (int)blockIdx.x) {
        stamp(SK, 2);
        stamp_val(SK, 5, cnt);
        stamp_val(SK, 6, GSMPM_HWREG(4));   // HW_ID
        stamp_val(SK, 7, GSMPM_HWREG(20));  // XCC_ID
      }
      int code = -1, lslot = 0, nt = -1;
      if (k < cnt) {
        int b[3];
        base_of(x, g.inv_dx, b);
        float gvd[3][3];
        const bool inwin = !outside && in_grid(x, g) && in_window(b, o0, o1, o2);
        const bool eslds = eslot >= 0 && eslot < kEscMax;  // nodes evaluated by the workgroup (LDS)
        if (FOLD && !inwin && !eslds) {
          // the outside chunk, or more escapes than LDS slots (rarer still): this
          // lane's 27 stencil nodes one at a time through the owner tiles' tables,
          // into its rows of esc_nodes (a rolled loop: no call, no stack)
          float4* en = rare->esc_nodes + (size_t)p * 27;
#pragma unroll 1
          for (int qn = 0; qn < 27; ++qn)
            en[qn] = fold_node(b[0] + qn / 9, b[1] + (qn / 3) % 3, b[2] + qn % 3, g, tl, ck, rare, fgs,
                               static_cast<const BcTable*>(rare->bct), fesc);
        }
        if (inwin) {
          g2p_gather<kG2pB128>(x, g,
                     [&](const int (&base)[3], int i, int j, int kk) {
                       const int q = ((base[0] - o0 + i) * kFW1 + (base[1] - o1 + j)) * kFW2 + (base[2] - o2 + kk);
                       return s_win[q];
                     },
                     v, C, gvd);
        } else {
          g2p_gather(x, g,
                     [&](const int (&base)[3], int i, int j, int kk) {
                       const int ix = base[0] + i, iy = base[1] + j, iz = base[2] + kk;
                       float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                       if constexpr (FOLD) {
                         const int qn = i * 9 + j * 3 + kk;
                         r = eslds ? s_win[kFWin + eslot * 27 + qn] : rare->esc_nodes[(size_t)p * 27 + qn];
                       } else {
                         if ((unsigned)ix < (unsigned)ng && (unsigned)iy < (unsigned)ng && (unsigned)iz < (unsigned)ng)
                           r = gvel[((size_t)ix * ng + iy) * ng + iz];
                       }
                       return r;
                     },
                     v, C, gvd);
        }
        float Fn[3][3];
        f_trial(gvd, F, dt, Fn);
        // v and C: stored by the last launch of a step only.  The P2G half
        // takes them from registers, and the next launch's G2P recomputes
        // both from the grid, so a G2P + P2G launch's copies are never read.
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (!P2G || GSMPM_STORE_VC) ps.st(PV + d, p, v[d]);
          x[d] = x[d] + dt * v[d];
          ps.st(PX + d, p, x[d]);
        }
        if (!finite3(x)) *rare->nonfin = 1;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          if (!P2G || GSMPM_STORE_VC) ps.st(PC + i, p, C[i / 3][i % 3]);
          F[i / 3][i % 3] = Fn[i / 3][i % 3];
        }
        // F_trial is stored here unless the return map below replaces it
        if (!P2G || MAT == 0 || MAT == 4) {
#pragma unroll
          for (int i = 0; i < 9; ++i) ps.st(PF + i, p, F[i / 3][i % 3]);
        }
        if (bin == 1) {
          int tc[3];
          nt = ftile_of(x, g, tl, tc);
          if (!outside && nt < tl.ntiles) {
            const int d0 = tc[0] - tx, d1 = tc[1] - ty, d2 = tc[2] - tz;
            if (abs(d0) <= 1 && abs(d1) <= 1 && abs(d2) <= 1) code = (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1);
          }
        }
      }
      if (bin == 1) {
        // the slot of the particle in its new tile's bin, reserved once per
        // (wave, neighbour tile): nearly every lane of a wave stays in the
        // chunk's own tile, and one LDS counter hit by 64 lanes serializes
        // them (2 cycles a lane, ~half of round 4's k_fused LDS bank-conflict
        // cycles); GSMPM_BIN_AGG=0: a lane-level atomic (A/B)
        if constexpr (kBinAgg) {
          unsigned long long pending = __ballot(code >= 0);
          while (pending) {  // wave-uniform: one trip per distinct neighbour tile of the wave
            const int lead = __ffsll(pending) - 1;
            const int lc = __builtin_amdgcn_readlane(code, lead);
            const unsigned long long mk = __ballot(code == lc);
            int base = 0;
            if ((k & 63) == lead) base = atomicAdd(&s_cnt[lc], __popcll(mk));
            base = __builtin_amdgcn_readlane(base, lead);
            if (code == lc)
              lslot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
            pending &= ~mk;
          }
        } else if (code >= 0) {
          lslot = atomicAdd(&s_cnt[code], 1);
        }
        __syncthreads();
        if (k < 27) {
          const int c = s_cnt[k];
          if (c > 0) {
            const int ntile = ((tx + k / 9 - 1) * tl.td1 + (ty + (k / 3) % 3 - 1)) * tl.td2 + (tz + k % 3 - 1);
            s_base[k] = reserve_f(rare->bo, ntile, c);
          }
        }
        __syncthreads();
        if (p >= 0) {
          const BinOutF bo = rare->bo;
          bo.ptile[p] = nt;
          bo.pslot[p] = code >= 0 ? s_base[code] + lslot : reserve_f(bo, nt, 1);
        }
      }
      if constexpr (!P2G) {  // the call's last launch: the particles' fastest velocity component
        float vm = 0.f;
        if (k < cnt) vm = fmaxf(fabsf(v[0]), fmaxf(fabsf(v[1]), fabsf(v[2])));
        if (!(vm <= 3.0e38f)) vm = 3.0e38f;  // NaN / Inf (flagged elsewhere): keep the bits ordered
        vm = wave_max_nonneg_dpp(vm);
        if ((k & 63) == 0 && vm > 0.f && rare->vmax) atomicMax(rare->vmax, __float_as_uint(vm));
      }
      __syncthreads();  // the window is consumed (and s_cnt / s_base read) before LDS is reused
      if (w == (int)blockIdx.x) stamp(SK, 3);
    }
    if constexpr (P2G) {
      if (!outside) {  // 16-byte stores: half the LDS write instructions of u64 ones
        uint4* z = reinterpret_cast<uint4*>(s_acc);
        for (int e = k; e < kFWin * 2; e += 256) z[e] = make_uint4(0u, 0u, 0u, 0u);
      }
      if (k < 16) s_rcnt[k] = 0;
      float nvt[3][3];
#pragma unroll
      for (int i = 0; i < 9; ++i) nvt[i / 3][i % 3] = 0.f;
      float bound = 0.f;
      if (k < cnt) {
        // ImpulseBC.apply (boundary_conditions.py:41-45); the kicked v lives in registers only
        if (mask) {
          const BcTable* __restrict__ bct = static_cast<const BcTable*>(rare->bct);
          const int ni = bct->n_imp;
          for (int b = 0; b < ni; ++b) {
            const Impulse& im = bct->imp[b];
            if (!((mask >> im.bit) & 1u)) continue;
            const bool in = fabsf(x[0] - im.c[0]) < im.s[0] && fabsf(x[1] - im.c[1]) < im.s[1] &&
                            fabsf(x[2] - im.c[2]) < im.s[2];
            if (in) {
#pragma unroll
              for (int d = 0; d < 3; ++d) v[d] = v[d] + im.f[d] / m * im.sdt;
            }
          }
        }
        // the particle drivers (gsmpm_mpm_add_driver), after the impulses
        if constexpr (DRV) apply_drivers(ds, static_cast<const BcTable*>(rare->bct), mask, p, x, m, v);
        // compute_stress_from_F_trial (utils.py:13-54)
        if constexpr (MAT == kMatMixed) {
          // the per-particle dispatch (constitutive.h).  The returned F is
          // stored for metal / sand / foam / fluid rows (a G2P + P2G launch left
          // F_trial to this store, so there every row: a jelly row's F is its
          // F_trial); the yield for metal rows only
          float tau[3][3];
          const int code = material_code(mi.id(p), mi.jelly);
          float yld = ps.ld(PYLD, p);
          const float mu = ps.ld(PMU, p), lam = ps.ld(PLAM, p);
          return_map_and_stress_mixed(code, F, mu, lam, yld, dt, mc, tau);
          if (G2P || (code >= 1 && code <= 3) || code == 5) {
#pragma unroll
            for (int i = 0; i < 9; ++i) ps.st(PF + i, p, F[i / 3][i % 3]);
          }
          if (code == 1) ps.st(PYLD, p, yld);
          const float nvol = -ps.ld(PVOL, p);
          if (code != 0) {  // jelly as written: nvt stays 0
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
              for (int j = 0; j < 3; ++j) nvt[i][j] = nvol * tau[i][j];
          }
        } else if constexpr (MAT != 0) {
          float tau[3][3];
          float yld = ps.ld(PYLD, p);
          const float mu = ps.ld(PMU, p), lam = ps.ld(PLAM, p);
          return_map_and_stress<MAT>(F, mu, lam, yld, dt, mc, tau);
          if constexpr (MAT == 1 || MAT == 2 || MAT == 3 || MAT == 5) {
#pragma unroll
            for (int i = 0; i < 9; ++i) ps.st(PF + i, p, F[i / 3][i % 3]);
          }
          if constexpr (MAT == 1) ps.st(PYLD, p, yld);
          const float nvol = -ps.ld(PVOL, p);
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) nvt[i][j] = nvol * tau[i][j];
        }
        // non-finite inputs of the scatter (a NaN / Inf would turn into finite
        // garbage through the fixed-point conversion, not propagate as the
        // reference's float atomics do): mass, velocity (impulse), stress, and
        // in a P2G-only launch the x and C it starts from
        {
          float chk = m + v[0] + v[1] + v[2];
          if constexpr (MAT != 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) chk += nvt[i / 3][i % 3];
          }
          if constexpr (!G2P) {
            chk += x[0] + x[1] + x[2];
#pragma unroll
            for (int i = 0; i < 9; ++i) chk += C[i / 3][i % 3];
          }
          if (!__builtin_isfinite(chk)) *rare->nonfin = 1;
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
        bound = fmaxf(m, m * (vm + 4.5f * g.dx * cm) + dt * 4.5f * g.inv_dx * sm) * 1.01f;
      }
      if (outside) {
        // chunk of particles binned outside the grid: bounds-checked global path
        if (k < cnt) {
          p2g_global<MAT>(x, v, C, m, nvt, g, dt, rare->gacc);
          int bq[3];
          base_of(x, g.inv_dx, bq);
          mark_escape_tiles(rare->tflag, rare->touched, rare->nchunk + 1, rare->rcov, tl, ng, bq[0], bq[1], bq[2]);
        }
        if (k == 0 && cnt > 0) {
          *rare->esc = 1;
          atomicAdd(rare->esc_count, (unsigned)cnt);
        }
        // the next launch on these bins reads this chunk's lane order too: the
        // identity (round 4 left it unwritten, so a lane of the next G2P took a
        // stale row -- another chunk's particle, or one past the live rows)
        if (tc.perm && k < cnt) tc.perm[(size_t)w * 256 + k] = (unsigned char)q;
        __syncthreads();
        continue;  // workgroup-uniform
      }
      int b[3];
      base_of(x, g.inv_dx, b);
      const bool win = k < cnt && in_grid(x, g) && in_window(b, o0, o1, o2);
      // slab: a particle past the margin scatters where no window exchange reaches (slab.h)
      if (k < cnt && (b[0] < xlo || b[0] >= xhi)) *rare->drift = 1;
      // window coordinates covered by this particle's stencil, as per-axis bit masks
      int mxy = win ? (7 << (b[0] - o0)) | (7 << (16 + b[1] - o1)) : 0;
      int mz = win ? 7 << (b[2] - o2) : 0;
      // wave reductions by DPP (the bound is >= 0; a NaN bound -- non-finite
      // inputs, flagged above -- orders above every finite one as integer bits);
      // GSMPM_DPP_REDUCE=0 (A/B): shuffles (ds_bpermute_b32)
      if constexpr (GSMPM_DPP_REDUCE != 0) {
        bound = wave_max_nonneg_dpp(bound);
        mxy = wave_or_dpp(mxy);
        mz = wave_or_dpp(mz);
      } else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          bound = fmaxf(bound, __shfl_xor(bound, o));
          mxy |= __shfl_xor(mxy, o);
          mz |= __shfl_xor(mz, o);
        }
      }
      if ((k & 63) == 0) {
        s_max[k >> 6] = bound;
        s_mxy[k >> 6] = mxy;
        s_mz[k >> 6] = mz;
      }
      __syncthreads();  // also orders the zeroing before the adds
      // lane balance for the next launch: this particle's rank among those of its base-node residue
      const int res = win ? (((b[0] - o0) * kFW1 + (b[1] - o1)) * kFW2 + (b[2] - o2)) & 15 : (q & 15);
      const int rrank = (tc.perm && k < cnt) ? atomicAdd(&s_rcnt[res], 1) : 0;
      const float bmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
      const int Mxy = s_mxy[0] | s_mxy[1] | s_mxy[2] | s_mxy[3], Mz = s_mz[0] | s_mz[1] | s_mz[2] | s_mz[3];
      const int Mx = Mxy & 0xffff, My = (unsigned)Mxy >> 16;
      // axes on which some stencil reaches below the tile (window coordinate 0)
      const int lo_all = (Mx & 1) | ((My & 1) << 1) | ((Mz & 1) << 2);
      if (lo_all & ~cr.w) {  // workgroup-uniform; rare (a new axis since the binning)
        Touch tr = tc;
        tr.tflag = rare->tflag;
        tr.touched = rare->touched;
        tr.nchunk = rare->nchunk;
        tr.rcov = rare->rcov;
        add_lower_tiles(tr, tl, tx, ty, tz, (lo_all | cr.w) & 7);
        if (k == 0) rare->chunk[w].w = lo_all | cr.w;
      }
      // stencil box of the chunk (empty chunk window: a 1-node box)
      int box = kFullBox;
      if (Mx && My && Mz)
        box = (__builtin_ctz(Mx)) | (__builtin_ctz(My) << 4) | (__builtin_ctz(Mz) << 8) | ((31 - __builtin_clz(Mx)) << 12) |
              ((31 - __builtin_clz(My)) << 16) | ((31 - __builtin_clz(Mz)) << 20);
      else
        box = 0;
      const bool multi = (cr.w & 8) != 0;  // the tile has several chunks
      if (k == 0) {
        tc.cbox[w] = box;
        rare->tbox[t] = multi ? kFullBox : box;  // tile tables: whole windows (outside its box a slot holds +0)
      }
      // The box as per-axis hull masks into the 27 cover records that see the
      // tile.  A single-chunk tile's chunk stores its own, exact every substep.
      // The chunks of a multi-chunk tile cannot agree on one box inside a
      // launch: each ORs its own in, so the record holds a superset of every
      // chunk's box since the re-binning zeroed it (write_cover_record) --
      // a stale bit costs k_grid_f a load of +0, never a result.
      if (tpos_e >= 0) {
        int* rb = rare->rbox + (size_t)tpos_e * kBoxStride + k;
        const int2 bm = box_masks(multi && !dense_box ? kFullBox : box);
        if (multi && dense_box) {
          atomicOr(rb, bm.x);
          atomicOr(rb + 32, bm.y);
        } else {
          rb[0] = bm.x;
          rb[32] = bm.y;
        }
      }
      // A multi-chunk tile's chunk stores the hull of its last box and this
      // one (the part outside the new box as +0 from the zeroed accumulators),
      // so outside the box it stored last its slot always holds +0; the whole
      // window on new bins (cbox is kFullBox: the slot was another chunk's)
      if (multi) box = dense_box ? box_hull(cbox, box) : kFullBox;
      int ebits;
      frexpf(bmax, &ebits);
      const int S = bmax > 0.f ? 50 - ebits : 0;  // see k_p2g
      if (k < cnt) {
        if (win) {
          int bb[3];
          float fx[3], ww[3][3], dw[3][3];
          bspline(x, g.inv_dx, bb, fx, ww, dw);
          p2g_scatter<MAT, kFW1, kFW2, kFWin>(s_acc + ((b[0] - o0) * kFW1 + (b[1] - o1)) * kFW2 + (b[2] - o2), fx, ww,
                                              dw, v, C, m, nvt, g, dt, ldexp(1.0, S));
        } else {
          p2g_global<MAT>(x, v, C, m, nvt, g, dt, rare->gacc);
          *rare->esc = 1;
        }
      }
      {  // escape statistics (gsmpm_mpm_escapes): one atomic a wave with escapes; their tiles
        const unsigned long long eb = __ballot(k < cnt && !win);
        if (eb) {  // wave-uniform; rare.  (The tiles are marked here, after the scatter, not in its branch:
                   // there the code cost k_fused<metal> 1 % with no escape, profiles/r06/ab_esc_r06o.txt)
          if ((k & 63) == 0) atomicAdd(rare->esc_count, (unsigned)__popcll(eb));
          if (k < cnt && !win)
            mark_escape_tiles(rare->tflag, rare->touched, rare->nchunk + 1, rare->rcov, tl, ng, b[0], b[1], b[2]);
        }
      }
      __syncthreads();
      if (w == (int)blockIdx.x) stamp(SK, 4);
      if (tc.perm && k < cnt) tc.perm[(size_t)w * 256 + balanced_lane(s_rcnt, cnt, res, rrank)] = (unsigned char)q;
      int lo[3], hi[3];
      box_unpack(box, lo, hi);
      const int n1 = hi[1] - lo[1] + 1, n2 = hi[2] - lo[2] + 1, n12 = n1 * n2;
      const int nvol = (hi[0] - lo[0] + 1) * n12;
      const float r12 = 1.0f / (float)n12, r2 = 1.0f / (float)n2;
      // the window's slot: the chunk's tile-order id (an ordered record carries it, k_chunk_order)
      const int cid = (cr.w & 16) ? (int)((unsigned)cr.w >> 5) : w;
      float4* dst = slots + (size_t)cid * kFWin;
      for (int qn = k; qn < nvol; qn += 256) {
        const int a = (int)(((float)qn + 0.5f) * r12), rem = qn - a * n12;
        const int bq = (int)(((float)rem + 0.5f) * r2), c = rem - bq * n2;
        const int node = ((lo[0] + a) * kFW1 + lo[1] + bq) * kFW2 + lo[2] + c;
        float4 r;
        r.x = from_fixed32(s_acc[0 * kFWin + node], S);
        r.y = from_fixed32(s_acc[1 * kFWin + node], S);
        r.z = from_fixed32(s_acc[2 * kFWin + node], S);
        r.w = from_fixed32(s_acc[3 * kFWin + node], S);
        // write-through: a slot is read by other XCDs' grid updates, and a dirty
        // line left in this XCD's L2 would be written back by the end-of-kernel
        // release (k_fused 21.9 -> 18.2 us on the lego frame)
        wt_store4(dst + node, r);
      }
      __syncthreads();  // LDS reuse by the next chunk
    }
  }
  // end-of-launch housekeeping (no load of this launch depends on it)
  if (bin == 2) {  // the next launch re-bins into rare->bo: its counts and flags start at zero
    const BinOutF bo = rare->bo;
    for (int t = blockIdx.x * 256 + threadIdx.x; t <= tl.ntiles; t += gridDim.x * 256) {
      bo.count[t] = 0;
      if (t < tl.ntiles) bo.tflag[t] = 0;
    }
  }
  if (rare->esc_clr) {  // FOLD rotation (null outside it): escapes of launch r - 2, flag r - 3
    if (__builtin_amdgcn_readfirstlane(*rare->esc_old) != 0) {
      const size_t nn = (size_t)ng * ng * ng;
      for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nn; q += (size_t)gridDim.x * 256)
        rare->gacc_old[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *rare->esc_clr = 0;
  }
  stamp(SK, 1);
