// fused.h -- the default substep pipeline of libgsmpm (included by mpm.hip
// inside namespace gsmpm, after the per-phase kernels it shares helpers with).
//
// The reference runs every substep as stress -> p2g -> grid -> g2p
// (mpm_solver/solver.py:27-52).  Here G2P of substep s and P2G of substep
// s + 1 run in ONE kernel, `k_fused`, so a substep is two launches
// (k_fused, k_grid_f) instead of four:
//
//   k_fused   one workgroup per <= 256-particle chunk of a tile: stage the
//             tile's v_out window in LDS, gather (g2p, utils.py:218-282),
//             then -- with x, v, C, F_trial still in registers -- impulse,
//             return map + stress (utils.py:13-54) and the APIC scatter
//             (p2g, utils.py:89-134) into the chunk's 64-bit fixed-point LDS
//             window, stored to the chunk's slot
//   k_grid_f  one workgroup per touched tile: sum the covering chunk windows
//             (fixed order), normalise + gravity + BC list -> v_out
//
// Particles keep the chunk (tile) they were binned into for `rebin_interval`
// substeps, so a chunk's window must hold the stencils of particles that
// moved since the binning: the window is the tile plus a ONE-cell margin on
// every side (base cell in [o - 1, o + T], nodes [o - 1, o + T + 3)).  With
// tiles of 8 x 8 x 7 cells that is 12 x 12 x 11 = 1584 nodes, 50.7 KB of u64
// accumulators -- three workgroups per CU.  A particle that moved further
// gathers from the dense v_out and scatters with global float atomics into
// the dense accumulator, raises the escape flag and appends the tiles that own
// its stencil nodes to the touched list, so the next grid update adds the
// accumulator to those nodes (correct for any motion, fast for CFL-bounded
// motion; the lego scene moves < 0.06 cells per substep).
//
// Binning is done by the G2P half of k_fused every `rebin_interval` substeps
// (counts + touched flags), `k_finish_bins` turns the counts into chunk
// records, exactly as in the per-phase pipeline.

#ifndef GSMPM_FT2
#define GSMPM_FT2 7
#endif
constexpr int kFT0 = 8, kFT1 = 8, kFT2 = GSMPM_FT2;          // tile cells per axis
constexpr int kFW0 = kFT0 + 4, kFW1 = kFT1 + 4, kFW2 = kFT2 + 4;  // window nodes per axis
constexpr int kFWin = kFW0 * kFW1 * kFW2;                      // 1584
constexpr int kFTN = kFT0 * kFT1 * kFT2;                       // owned nodes per tile (448)

// where window node (w0, w1, w2) lives in its chunk's slot: window order ([kFW0][kFW1][kFW2])
__device__ __forceinline__ int slot_loc(int w0, int w1, int w2) { return (w0 * kFW1 + w1) * kFW2 + w2; }

// ---- multi-GPU slab hooks (slab.h has the exchange and migration kernels) ----
struct SlabWin {
  int W;            // window planes (0: not a slab)
  int a[2];         // first plane of the lower (0) / upper (1) window; window w is [a[w], a[w] + W)
  int on[2];        // window w present (a neighbour on that side)
  float4* part[2];  // [W][ny][nz] this rank's partial sums of the window's nodes in its rect (k_grid_f writes,
                    // k_win_update zeroes)
  int y0[2], ny[2];  // window w's rect of nodes [y0, y0 + ny) x [z0, z0 + nz): what the two ranks of the bound can
  int z0[2], nz[2];  // touch before the next migration (agreed at every migration); only it is exchanged
  int* oob;          // set when a window node outside the rect has mass (the exchange would miss it)
  int pass;          // k_grid_f: 0 every touched tile, 1 tiles meeting a window, 2 the others
};

__device__ __forceinline__ int slab_window_of(const SlabWin& sw, int i) {
  if (sw.on[0] && i >= sw.a[0] && i < sw.a[0] + sw.W) return 0;
  if (sw.on[1] && i >= sw.a[1] && i < sw.a[1] + sw.W) return 1;
  return -1;
}
// does tile-x ti (planes [ti * kFT0, ti * kFT0 + kFT0)) meet a window?
__device__ __forceinline__ bool slab_tile_in_window(const SlabWin& sw, int ti) {
  const int p0 = ti * kFT0, p1 = p0 + kFT0;
  bool r = false;
#pragma unroll
  for (int w = 0; w < 2; ++w) r = r || (sw.on[w] && p0 < sw.a[w] + sw.W && sw.a[w] < p1);
  return r;
}

// per-particle checks of k_fused: the slab drift check (base plane allowed in
// [xlo, xhi), else *FusedRare::drift) and the non-finite check (a
// NaN / Inf position sets *FusedRare::nonfin, which the step call reports as
// GSMPM_ESTATE; without it a non-finite particle is silently binned
// "outside" and scatters nowhere)
__device__ __forceinline__ bool finite3(const float (&x)[3]) {
  return __builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]);
}

struct FTiles {
  int td0, td1, td2;  // tiles per axis
  int ntiles;         // td0 * td1 * td2 (the pseudo-tile "outside" is index ntiles)
  int max_chunks;
};

struct BinOutF {
  int* count;  // [ntiles + 1] (zeroed before a binning launch)
  int* ptile;  // [n]
  int* pslot;  // [n]
  int* tflag;  // [ntiles] (zeroed with count)
  FTiles tl;
};

// Arguments of k_fused that only rare paths use -- the re-binning launches'
// outputs, the escape path, impulses, tiles appended during the launch, the
// error flags, the once-a-chunk box publishing -- read through one pointer
// where they are used.  As kernel arguments they made ~150 dwords against
// 102 SGPRs, and the compiler kept 89 SGPRs spilled to VGPR lanes (348
// v_readlane restores in the code); now 38 (69).  k_fused's time did not
// move (5 interleaved rounds: 16.07 against 16.11 us steady), the same
// change to k_grid_f did (its slab-free form below).  One per (bins parity,
// escape flag) in device memory (mpm.hip sync_rare).
struct FusedRare {
  BinOutF bo;          // re-binning outputs (bins parity c ^ 1)
  float4* gacc;        // escape accumulator
  int* esc;            // escape flag this launch raises
  int* drift;          // slab: a particle past the margin (unused outside slabs)
  int* nonfin;         // non-finite state word
  const void* bct;     // const BcTable* (impulses)
  int* tflag;          // Touch members of add_lower_tiles (bins parity c)
  int* touched;
  int* nchunk;
  int4* chunk;
  int2* rcov;
  int* tbox;           // Touch's per-chunk box publishing (once a chunk: a scalar load, not a live SGPR)
  const int* tpos;
  int* rbox;
  // ---- the folded grid update (FOLD launches, below; null / unused otherwise) ----
  // Launch r of a step call (phase r mod 12) writes its chunk windows to the
  // slot buffer r mod 2, its tile boxes to tbox buffer r mod 2, its escapes to
  // gacc buffer r mod 3 and raises escape flag r mod 12.  The previous
  // launch's outputs are what a FOLD launch's staging reads:
  const float4* slots_prev;  // chunk windows of launch r - 1
  const int* tbox_prev;      // tile boxes of launch r - 1
  const float4* gacc_prev;   // escapes of launch r - 1 (read when *esc_prev)
  const int* esc_prev;       // escape flag of launch r - 1
  // launch r's housekeeping at its end: the escapes of launch r - 2 (read by
  // launch r - 1, written next by launch r + 1) are zeroed when *esc_old, and
  // flag r - 3 (read by launches r - 2 and r - 1) is cleared
  const int* esc_old;
  float4* gacc_old;
  int* esc_clr;
  float grav[3];  // gravity (f32): a FOLD launch forms dt * gravity as the host's grid_step does
  unsigned* esc_count;  // particle scatters that escaped their chunk window, summed (gsmpm_mpm_escapes)
  float4* esc_nodes;    // FOLD: [np][27] the stencil node values of a particle outside its chunk's window
  unsigned* vmax;       // G2P-only launches (a step call's last): max |v| component over the particles, as
                        // f32 bits (atomicMax), for the next call's re-binning count (mpm.hip choose_rebins)
};

// ---------------------------------------------------------------- the fold --
// FOLD launches (MODE bit 4) take the grid update of the previous substep
// into their own G2P staging instead of reading the dense v_out that a
// k_grid_f launch would have written: every node of the chunk's stencil box
// is summed from the chunk windows that cover it (the previous P2G's slots,
// in k_grid_f's fixed order: the node's owner tile's window first, then the
// covering neighbours by k_grid_f's e order, the second and further chunks
// after, the escape accumulator last), then normalised, gravity and the BC
// list applied (node_update, utils.py:177-183 + solver.py:41-46).  The staged
// value is bit-identical to k_grid_f's, so a step runs one launch per substep
// (k_grid_f only after a re-binning, whose next launch reads chunk windows of
// the old bins).  A node lies in up to 8 chunk windows (3.5 on average), so
// the slot bytes a launch reads grow by that factor over k_grid_f's; they come
// from L2 / MALL, written by the launch before.
constexpr int kFT[3] = {kFT0, kFT1, kFT2};
#ifndef GSMPM_FOLD_BATCH
#define GSMPM_FOLD_BATCH 1
#endif
constexpr int kFoldB = GSMPM_FOLD_BATCH;  // nodes a lane stages at once (their loads in flight together)
// per axis: window coordinate w (node o + w of tile t's window, o = t T - 1) ->
// the node's owner tile offset d in {-1, 0, 1} and k_grid_f's section sec of
// its owner-local coordinate l = w - 1 - d T (sec -1: l < 3, +1: l = T - 1)
__device__ __forceinline__ void fold_axis(int w, int T, int& d, int& sec) {
  d = w == 0 ? -1 : (w <= T ? 0 : 1);
  const int l = w - 1 - d * T;
  sec = l < 3 ? -1 : (l == T - 1 ? 1 : 0);
}
// (global address space: the loads may move across the staging's LDS stores)
__device__ __forceinline__ float4 ld_slot4(const float4* __restrict__ slots, int off) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef const f4v __attribute__((address_space(1)))* gf4_p;
  const f4v r = *(gf4_p)((const char*)slots + (unsigned)off * 16u);
  return make_float4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ void add4f(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
// The summed window value of one node from per-neighbour tables: covering
// tile e of the node is t + a_e (a_e per axis = d + (bit e ? sec : 0)), its
// {first chunk, chunks, box} read through `tab(ci, c0, nc, bx)` for the
// 27-neighbour index ci of a_e, and the node's coordinate in that window is
// w - a_e T.  Loads of covers outside the window's box (nothing was scattered
// there) are not issued.  Order of the sum: k_grid_f's (node_reads,
// node_extra).  fold_prep computes the 8 covers' slot offsets, fold_load
// issues their loads, fold_acc sums them (+ further chunks): split so a
// caller can have several nodes' loads in flight at once.
struct FoldNode {
  int off[8];  // first chunk's slot offset of each cover (valid where on)
  int on;      // bit e: cover e exists and its box holds the node
  int extra;   // bit e: ... and that cover's tile has further chunks
};
// cover e of window node w: its 27-neighbour index and the node's offset in its window
__device__ __forceinline__ void fold_cover(const int (&w)[3], int e, int& ci, int (&wn)[3], bool& valid) {
  int d[3], sec[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) fold_axis(w[ax], kFT[ax], d[ax], sec[ax]);
  const int b0 = e >> 2, b1 = (e >> 1) & 1, b2 = e & 1;
  const int a0 = d[0] + (b0 ? sec[0] : 0), a1 = d[1] + (b1 ? sec[1] : 0), a2 = d[2] + (b2 ? sec[2] : 0);
  ci = (a0 + 1) * 9 + (a1 + 1) * 3 + (a2 + 1);
  wn[0] = w[0] - a0 * kFT0;
  wn[1] = w[1] - a1 * kFT1;
  wn[2] = w[2] - a2 * kFT2;
  valid = ((!b0) | (sec[0] != 0)) & ((!b1) | (sec[1] != 0)) & ((!b2) | (sec[2] != 0));
}
__device__ __forceinline__ bool in_box(const int (&wn)[3], int q) {
  return (wn[0] >= (q & 15)) & (wn[1] >= ((q >> 4) & 15)) & (wn[2] >= ((q >> 8) & 15)) & (wn[0] <= ((q >> 12) & 15)) &
         (wn[1] <= ((q >> 16) & 15)) & (wn[2] <= ((q >> 20) & 15));
}
template <typename Tab>
__device__ __forceinline__ void fold_prep(const int (&w)[3], Tab tab, FoldNode& f) {
  f.on = 0;
  f.extra = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int ci, wn[3];
    bool valid;
    fold_cover(w, e, ci, wn, valid);
    int c0, nc, q;
    tab(ci, c0, nc, q);
    const bool on = valid & (nc > 0) & in_box(wn, q);
    f.on |= on ? (1 << e) : 0;
    f.extra |= (on & (nc > 1)) ? (1 << e) : 0;
    f.off[e] = c0 * kFWin + slot_loc(wn[0], wn[1], wn[2]);
  }
}
__device__ __forceinline__ void fold_load(const float4* __restrict__ slots, const FoldNode& f, float4 (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = ((f.on >> e) & 1) ? ld_slot4(slots, f.off[e]) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// the sum: the first chunks in e order, then (rare: tiles of > 256 particles)
// the second chunks in e order and the third and later ones, their offsets
// recomputed from the tables (not kept live across the loads)
template <typename Tab>
__device__ __forceinline__ float4 fold_acc(const float4* __restrict__ slots, const int (&w)[3], Tab tab,
                                           const FoldNode& f, const float4 (&v)[8]) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int e = 0; e < 8; ++e) add4f(a, v[e]);
  if (f.extra) {
    int c0s[8], ncs[8], locs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int ci, wn[3];
      bool valid;
      fold_cover(w, e, ci, wn, valid);
      int q;
      tab(ci, c0s[e], ncs[e], q);
      locs[e] = slot_loc(wn[0], wn[1], wn[2]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float4 u = ((f.extra >> e) & 1) ? ld_slot4(slots, (c0s[e] + 1) * kFWin + locs[e])
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
      add4f(a, u);
    }
    // (an unrolled scan, not a ctz loop: a dynamic index would put the arrays in scratch)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((f.extra >> e) & 1)
        for (int c = c0s[e] + 2; c < c0s[e] + ncs[e]; ++c) add4f(a, ld_slot4(slots, c * kFWin + locs[e]));
  }
  return a;
}
template <typename Tab>
__device__ __forceinline__ float4 fold_sum(const float4* __restrict__ slots, const int (&w)[3], Tab tab) {
  FoldNode f;
  fold_prep(w, tab, f);
  float4 v[8];
  fold_load(slots, f, v);
  return fold_acc(slots, w, tab, f, v);
}

// The slow path: the updated velocity of any grid node (i, j, k) from the
// previous P2G's windows, through the tile tables of the node's owner tile
// (a particle of a FOLD launch that left its chunk's window, or one binned
// outside the grid).  0 outside the grid.
__device__ __forceinline__ float4 fold_node(int i, int j, int k, const GridDims& g, const FTiles& tl, const ChunkIn& ck,
                                            const FusedRare* __restrict__ rare, const GridStep& gs,
                                            const BcTable* __restrict__ bct, bool esc) {
  const int ng = g.ng;
  if ((unsigned)i >= (unsigned)ng || (unsigned)j >= (unsigned)ng || (unsigned)k >= (unsigned)ng)
    return make_float4(0.f, 0.f, 0.f, 0.f);
  const int ti = i / kFT0, tj = j / kFT1, tk = k / kFT2;
  // window coordinates of the node in its owner tile's window (owner offset d = 0)
  const int w[3] = {i - ti * kFT0 + 1, j - tj * kFT1 + 1, k - tk * kFT2 + 1};
  float4 a = fold_sum(rare->slots_prev, w, [&](int ci, int& c0, int& nc, int& q) {
    const int x = ti + ci / 9 - 1, y = tj + (ci / 3) % 3 - 1, z = tk + ci % 3 - 1;
    c0 = 0;
    nc = 0;
    q = 0;
    if ((unsigned)x < (unsigned)tl.td0 && (unsigned)y < (unsigned)tl.td1 && (unsigned)z < (unsigned)tl.td2) {
      const int u = (x * tl.td1 + y) * tl.td2 + z;
      c0 = ck.cbase[u];
      nc = (ck.count[u] + kChunk - 1) / kChunk;
      q = rare->tbox_prev[u];
    }
  });
  if (esc) add4f(a, rare->gacc_prev[((size_t)i * ng + j) * ng + k]);
  return node_update(a, i, j, k, g, gs, bct);
}

__device__ __forceinline__ void ftile_decode(const FTiles& tl, int t, int& tx, int& ty, int& tz) {
  tz = t % tl.td2;
  ty = (t / tl.td2) % tl.td1;
  tx = t / (tl.td1 * tl.td2);
}

// tile of a particle's base cell (utils.py:95 truncation), `ntiles` outside the grid
__device__ __forceinline__ int ftile_of(const float (&x)[3], const GridDims& g, const FTiles& tl, int (&tc)[3]) {
  bool ok = true;
  int b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float gp = x[d] * g.inv_dx - 0.5f;
    ok = ok && (gp >= 0.0f) && (gp < (float)g.ng);  // false for NaN
    b[d] = ok ? (int)gp : 0;
  }
  tc[0] = b[0] / kFT0;
  tc[1] = b[1] / kFT1;
  tc[2] = b[2] / kFT2;
  return ok ? (tc[0] * tl.td1 + tc[1]) * tl.td2 + tc[2] : tl.ntiles;
}

// Touched tiles.  At binning time a tile's particles have their base cell in
// the tile, so their stencils reach the tiles t + {0, 1}^3: the first
// reservation in t flags those (idempotent plain stores).  A particle that
// later moves below its tile (base = tile origin - 1 on some axis) also
// reaches the lower neighbours; k_fused adds those to the touched list when
// it first sees such a particle in a chunk (add_lower_tiles).
__device__ __noinline__ void mark8(int* __restrict__ tflag, int t, int td0, int td1, int td2) {
  const int tz = t % td2, ty = (t / td2) % td1, tx = t / (td1 * td2);
  for (int a = 0; a <= 1; ++a)
    for (int b = 0; b <= 1; ++b)
      for (int c = 0; c <= 1; ++c)
        if (tx + a < td0 && ty + b < td1 && tz + c < td2) tflag[((tx + a) * td1 + ty + b) * td2 + tz + c] = 1;
}
__device__ __forceinline__ int reserve_f(const BinOutF& bo, int t, int c) {
  const int old = atomicAdd(&bo.count[t], c);
  if (old == 0 && t < bo.tl.ntiles) mark8(bo.tflag, t, bo.tl.td0, bo.tl.td1, bo.tl.td2);
  return old;
}

// The touched list of the bins a k_fused launch reads (the grid update that
// follows walks it) and the chunk records, whose .w holds the lower-neighbour
// axes already added for the chunk.
struct Touch {
  int* tflag;
  int* touched;
  int* nchunk;  // [1] = touched count
  int4* chunk;
  int* cbox;    // [max_chunks] stencil box of the chunk's last P2G (packed, window coordinates)
  int* tbox;    // [ntiles] the same per tile (the full window when the tile has several chunks)
  unsigned char* perm;  // [max_chunks][256] lane -> particle of the chunk (lane balance, below); null: off
  int2* rcov;           // cover records per touched position (ChunkIn): an appended tile's gets the "none" flag
  const int* tpos;      // [ntiles] touched position of each tile (-1: none); null: no box publishing
  int* rbox;            // [ntiles][kBoxStride] the neighbours' stencil boxes (box_masks), per touched position
};

// Lane balance.  A wave's LDS accesses to the chunk window (G2P's ds_read_b128
// of float4 nodes, P2G's 64-bit atomics into channel planes) are serviced in
// lane groups of 16 whose banks follow the node index mod 16 -- and with the
// same stencil offset added by every lane, a group is conflict-free exactly
// when its 16 particles' base nodes are distinct mod 16.  Every P2G records,
// per chunk, the lane assignment that puts a particle whose base node has
// residue r on a lane L with L mod 16 = r wherever the residue counts allow
// (the leftovers fill the remaining lanes in order); the next launch on the
// same bins (the particles moved < 1 cell) runs its lanes through it.  Both
// b128 and b64 lane groups hold 16 lanes of distinct L mod 16.
__device__ __forceinline__ int balanced_lane(const int* __restrict__ rcnt, int cnt, int r, int rank) {
  const int Lr = (cnt - r + 15) >> 4;  // lanes of residue r in [0, cnt)
  if (rank < Lr) return rank * 16 + r;
  int o = rank - Lr;
  for (int q = 0; q < r; ++q) o += max(0, rcnt[q] - ((cnt - q + 15) >> 4));
  int acc = 0;
  for (int q = 0; q < 16; ++q) {
    const int Lq = (cnt - q + 15) >> 4, d = max(0, Lq - rcnt[q]);
    if (o < acc + d) return (rcnt[q] + (o - acc)) * 16 + q;
    acc += d;
  }
  return rank * 16 + r;  // unreachable: overflow == deficit
}

// Stencil boxes: lo/hi window coordinates (0..11) per axis in 4-bit fields,
// lo0 | lo1 << 4 | lo2 << 8 | hi0 << 12 | hi1 << 16 | hi2 << 20.  The P2G of
// a chunk writes only the nodes inside its box, the next G2P of the chunk
// stages only those (the particles have not moved in between), and the grid
// update reads a tile's windows only inside its box.
constexpr int kFullBox = 0 | (0 << 4) | (0 << 8) | ((kFW0 - 1) << 12) | ((kFW1 - 1) << 16) | ((kFW2 - 1) << 20);
__device__ __forceinline__ void box_unpack(int b, int (&lo)[3], int (&hi)[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = (b >> (4 * d)) & 15;
    hi[d] = (b >> (12 + 4 * d)) & 15;
  }
}
// the hull of two boxes: per axis the lower lo and the higher hi
__device__ __forceinline__ int box_hull(int a, int b) {
  int r = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r |= min((a >> (4 * d)) & 15, (b >> (4 * d)) & 15) << (4 * d);
    r |= max((a >> (12 + 4 * d)) & 15, (b >> (12 + 4 * d)) & 15) << (12 + 4 * d);
  }
  return r;
}
// A box as a cover record holds it (k_grid_f): per-axis bit masks with bits
// lo..hi set, {x | y << 16, z}.  Masks of several boxes OR into a superset of
// each, which is how the chunks of a multi-chunk tile publish theirs.
__device__ __forceinline__ int2 box_masks(int b) {
  int lo[3], hi[3];
  box_unpack(b, lo, hi);
  const int mx = (2 << hi[0]) - (1 << lo[0]), my = (2 << hi[1]) - (1 << lo[1]), mz = (2 << hi[2]) - (1 << lo[2]);
  return make_int2(mx | (my << 16), mz);
}

// Lanes 0..26: add the tiles t + a, a_d in {-1 if d in lo, 0, 1}, with some
// a_d = -1, that are not yet flagged (one append per tile: the flag CAS).
__device__ __forceinline__ void add_lower_tiles(const Touch& tc, const FTiles& tl, int tx, int ty, int tz, int lo) {
  const int e = threadIdx.x;
  if (e < 27) {
    const int a = e / 9 - 1, b = (e / 3) % 3 - 1, c = e % 3 - 1;
    const bool need = (a < 0 || b < 0 || c < 0) && (a >= 0 || (lo & 1)) && (b >= 0 || (lo & 2)) && (c >= 0 || (lo & 4));
    const int x = tx + a, y = ty + b, z = tz + c;
    if (need && (unsigned)x < (unsigned)tl.td0 && (unsigned)y < (unsigned)tl.td1 && (unsigned)z < (unsigned)tl.td2) {
      const int t = (x * tl.td1 + y) * tl.td2 + z;
      if (atomicCAS(&tc.tflag[t], 0, 1) == 0) {
        const int pos = atomicAdd(&tc.nchunk[1], 1);
        tc.touched[pos] = t;
        // no cover record (its neighbours publish no boxes for it): k_grid_f reads the tile tables
        if (tc.rcov) tc.rcov[(size_t)pos * kRecStride + 27] = make_int2(1, 0);
      }
    }
  }
}

// base cell of a particle as bspline() computes it
__device__ __forceinline__ void base_of(const float (&x)[3], float inv_dx, int (&b)[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = (int)(x[d] * inv_dx - 0.5f);
}

// Escapes and the grid update.  A particle that scatters through the dense
// accumulator (p2g_global: it left its chunk's window, or its chunk lies
// outside the grid) adds the tiles owning its in-grid stencil nodes to the
// touched list, as add_lower_tiles does for a new lower neighbour, so the
// next k_grid_f -- which adds the accumulator to the nodes it owns and zeroes
// it -- finds every node an escape wrote among the touched tiles (round 5
// swept every tile of the grid after any escape: 4,864 tiles at 128^3 against
// ~900 touched).
__device__ __forceinline__ void mark_escape_tiles(int* __restrict__ tflag, int* __restrict__ touched,
                                               int* __restrict__ ntouch, int2* __restrict__ rcov, const FTiles& tl,
                                               int ng, int b0, int b1, int b2) {
  const int lo0 = max(b0, 0), lo1 = max(b1, 0), lo2 = max(b2, 0);
  const int hi0 = min(b0 + 2, ng - 1), hi1 = min(b1 + 2, ng - 1), hi2 = min(b2 + 2, ng - 1);
  if (lo0 > hi0 || lo1 > hi1 || lo2 > hi2) return;  // no stencil node in the grid
  for (int a = lo0 / kFT0; a <= hi0 / kFT0; ++a)
    for (int c = lo1 / kFT1; c <= hi1 / kFT1; ++c)
      for (int e = lo2 / kFT2; e <= hi2 / kFT2; ++e) {
        const int t = (a * tl.td1 + c) * tl.td2 + e;
        if (__hip_atomic_load(&tflag[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
            atomicCAS(&tflag[t], 0, 1) == 0) {
          const int pos = atomicAdd(ntouch, 1);
          touched[pos] = t;
          if (rcov) rcov[(size_t)pos * kRecStride + 27] = make_int2(1, 0);  // no cover record: the tile tables
        }
      }
}
// stencil inside the chunk window whose first node is o
__device__ __forceinline__ bool in_window(const int (&b)[3], int o0, int o1, int o2) {
  return (unsigned)(b[0] - o0) <= (unsigned)(kFW0 - 3) && (unsigned)(b[1] - o1) <= (unsigned)(kFW1 - 3) &&
         (unsigned)(b[2] - o2) <= (unsigned)(kFW2 - 3);
}
// the per-phase pipeline's in-grid test (tile_of): base cell inside [0, ng)^3
__device__ __forceinline__ bool in_grid(const float (&x)[3], const GridDims& g) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float gp = x[d] * g.inv_dx - 0.5f;
    ok = ok && (gp >= 0.0f) && (gp < (float)g.ng);
  }
  return ok;
}

// MODE bit 1: G2P of the previous grid update; bit 2: P2G of this substep.
// `bin` (uniform): re-bin the particles by their new x into `bo`.
// Particle storage is in bin order (permuted at every binning), so chunk w's
// particles are storage rows [first, first + cnt).
#ifndef GSMPM_STORE_VC
#define GSMPM_STORE_VC 0  // 1: every G2P stores v and C (A/B)
#endif
// GSMPM_SIM_PRIO=n (A/B): the simulator's waves raise their issue priority
// (s_setprio n, 0..3) so that a SIMD's arbiter serves them before the waves of
// the render of the previous frame, which runs on a second stream beside them
// (the frame costs sim + ~0.25 ms of that render's interference, §6)
#ifndef GSMPM_SIM_PRIO
#define GSMPM_SIM_PRIO 0
#endif
constexpr int kSimPrio = GSMPM_SIM_PRIO;
__device__ __forceinline__ void sim_prio() {
  if constexpr (kSimPrio > 0) __builtin_amdgcn_s_setprio(kSimPrio);
}
#ifndef GSMPM_DPP_REDUCE
#define GSMPM_DPP_REDUCE 1
#endif
// GSMPM_G2P_B128 (A/B, default 1): G2P's 27 LDS gathers as ds_read_b128
#ifndef GSMPM_G2P_B128
#define GSMPM_G2P_B128 1
#endif
constexpr bool kG2pB128 = GSMPM_G2P_B128 != 0;
#ifndef GSMPM_BIN_AGG
#define GSMPM_BIN_AGG 1
#endif
constexpr bool kBinAgg = GSMPM_BIN_AGG != 0;
// The kernel's body is fused_body.inc, included by its two entry points:
// k_fused<MAT, MODE> (one material: the symbols, arguments and code of the
// uniform scenes, unchanged) and k_fused_mixed<MODE> (MAT = 6, the
// per-particle ids as one more argument), and by their driver entry points
// below.  It reads the arguments, MAT, MODE, `mi`, DRV and `ds` by name.
// bin: 1 = re-bin the particles by their new x into rare->bo; 2 = zero
// rare->bo's counts and flags for the next launch's re-binning (at the end)
template <int MAT, int MODE>
__global__ __launch_bounds__(256, 3) void k_fused(Particles ps, GridDims g, FTiles tl, ChunkIn ck, Touch tc, int bin,
                                               int use_box, const float4* __restrict__ gvel, uint32_t mask, float dt,
                                               MatConsts mc, float4* __restrict__ slots, int xlo, int xhi,
                                               const FusedRare* __restrict__ rare, uint32_t mask_prev) {
  static_assert(MAT != kMatMixed, "the mixed dispatch is k_fused_mixed");
  const MatIds<MAT> mi{};
  constexpr bool DRV = false;
  const DrvSel<DRV> ds{};
#define GSMPM_FUSED_BODY_INCLUDER
#include "fused_body.inc"
#undef GSMPM_FUSED_BODY_INCLUDER
}

// k_fused<6, MODE>: each particle's material from its id (constitutive.h)
template <int MODE>
__global__ __launch_bounds__(256, 3) void k_fused_mixed(Particles ps, GridDims g, FTiles tl, ChunkIn ck, Touch tc,
                                                     int bin, int use_box, const float4* __restrict__ gvel,
                                                     uint32_t mask, float dt, MatConsts mc,
                                                     float4* __restrict__ slots, int xlo, int xhi,
                                                     const FusedRare* __restrict__ rare, uint32_t mask_prev,
                                                     MatIds<kMatMixed> mi) {
  constexpr int MAT = kMatMixed;
  constexpr bool DRV = false;
  const DrvSel<DRV> ds{};
#define GSMPM_FUSED_BODY_INCLUDER
#include "fused_body.inc"
#undef GSMPM_FUSED_BODY_INCLUDER
}

// The driver entry points (gsmpm_mpm_add_driver; P2G modes 2 and 3, never
// FOLD): the same body with the particle drivers after the impulse kick, the
// selection as one more argument.  Launched only by a handle that holds a
// driver; every other handle launches the symbols above.
template <int MAT, int MODE>
__global__ __launch_bounds__(256, 3) void k_fused_drv(Particles ps, GridDims g, FTiles tl, ChunkIn ck, Touch tc,
                                                      int bin, int use_box, const float4* __restrict__ gvel,
                                                      uint32_t mask, float dt, MatConsts mc,
                                                      float4* __restrict__ slots, int xlo, int xhi,
                                                      const FusedRare* __restrict__ rare, uint32_t mask_prev,
                                                      DrvSel<true> ds) {
  static_assert(MAT != kMatMixed, "the mixed dispatch is k_fused_mixed_drv");
  static_assert((MODE & 2) != 0 && (MODE & 4) == 0, "drivers act in the P2G half of the unfolded pipeline");
  const MatIds<MAT> mi{};
  constexpr bool DRV = true;
#define GSMPM_FUSED_BODY_INCLUDER
#include "fused_body.inc"
#undef GSMPM_FUSED_BODY_INCLUDER
}
template <int MODE>
__global__ __launch_bounds__(256, 3) void k_fused_mixed_drv(Particles ps, GridDims g, FTiles tl, ChunkIn ck, Touch tc,
                                                            int bin, int use_box, const float4* __restrict__ gvel,
                                                            uint32_t mask, float dt, MatConsts mc,
                                                            float4* __restrict__ slots, int xlo, int xhi,
                                                            const FusedRare* __restrict__ rare, uint32_t mask_prev,
                                                            MatIds<kMatMixed> mi, DrvSel<true> ds) {
  static_assert((MODE & 2) != 0 && (MODE & 4) == 0, "drivers act in the P2G half of the unfolded pipeline");
  constexpr int MAT = kMatMixed;
  constexpr bool DRV = true;
#define GSMPM_FUSED_BODY_INCLUDER
#include "fused_body.inc"
#undef GSMPM_FUSED_BODY_INCLUDER
}

// The end of a FOLD step call: the escape accumulators that the call's last
// launches left dirty are zeroed and every rotation flag cleared, so the next
// call starts from clean buffers.  One workgroup (no flag is cleared while
// another workgroup could still test it); nothing to do in a call without
// escapes.
__global__ __launch_bounds__(1024) void k_fold_tail(int* __restrict__ flags, float4* __restrict__ g0,
                                                    float4* __restrict__ g1, float4* __restrict__ g2, int ng) {
  __shared__ int s_f[12];
  if (threadIdx.x < 12) s_f[threadIdx.x] = flags[threadIdx.x];
  __syncthreads();
  const size_t nn = (size_t)ng * ng * ng;
  bool dirty[3] = {false, false, false};
  for (int r = 0; r < 12; ++r) dirty[r % 3] = dirty[r % 3] || s_f[r] != 0;
  float4* gb[3] = {g0, g1, g2};
  for (int b = 0; b < 3; ++b)
    if (dirty[b])
      for (size_t q = threadIdx.x; q < nn; q += 1024) gb[b][q] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  if (threadIdx.x < 12 && s_f[threadIdx.x]) flags[threadIdx.x] = 0;
}

// Chunk ranges and stencil boxes of the 27 tiles whose windows reach tile
// (ti, tj, tk) -> LDS (lanes 0..26; caller syncs), in a cover record's layout:
// s_cov[2 e] = first chunk, s_cov[2 e + 1] = chunk count, s_bx[e] and
// s_bx[32 + e] = the box's masks (box_masks of the packed tile box).
__device__ __forceinline__ void load_cover27(const ChunkIn& ck, const int* __restrict__ tbox, const FTiles& tl, int ti,
                                             int tj, int tk, int* s_cov, int* s_bx) {
  const int e = threadIdx.x;
  if (e < 27) {
    const int x = ti + e / 9 - 1, y = tj + (e / 3) % 3 - 1, z = tk + e % 3 - 1;
    int c0 = 0, nc = 0, bx = 0;
    if ((unsigned)x < (unsigned)tl.td0 && (unsigned)y < (unsigned)tl.td1 && (unsigned)z < (unsigned)tl.td2) {
      const int t = (x * tl.td1 + y) * tl.td2 + z;
      const int cnt = ck.count[t];
      c0 = ck.cbase[t];
      bx = tbox[t];
      nc = (cnt + kChunk - 1) / kChunk;
    }
    s_cov[2 * e] = c0;
    s_cov[2 * e + 1] = nc;
    const int2 bm = box_masks(bx);
    s_bx[e] = bm.x;
    s_bx[32 + e] = bm.y;
  }
}

// The <= 8 window reads of owned node (l0, l1, l2) of a tile.  Per axis a node
// lies in its own tile's window and, when l < 3, in the lower neighbour's
// (l + T + 1 < T + 4), when l = T - 1 in the upper one's.  A read outside the
// covering tile's stencil box (nothing was scattered there this substep) is
// redirected to the all-zero slot, so the 8 loads stay unconditional.
struct NodeReads {
  int off[8];  // slot offsets (float4 units) of the first chunk of each covering tile
  int extra;   // bit e: covering tile e has further chunks
  int live;    // bit e: the node lies inside covering tile e's stencil box (some stencil may reach it)
};
// covering tile e of node (l0, l1, l2): its index in the 27-neighbourhood and the node's window offset there
__device__ __forceinline__ void node_cover(int l0, int l1, int l2, int e, int& ci, int& loc) {
  const int sec0 = l0 < 3 ? -1 : (l0 == kFT0 - 1 ? 1 : 0);
  const int sec1 = l1 < 3 ? -1 : (l1 == kFT1 - 1 ? 1 : 0);
  const int sec2 = l2 < 3 ? -1 : (l2 == kFT2 - 1 ? 1 : 0);
  const int a = (e >> 2) ? sec0 : 0, b = ((e >> 1) & 1) ? sec1 : 0, c = (e & 1) ? sec2 : 0;
  ci = (a + 1) * 9 + (b + 1) * 3 + (c + 1);
  loc = slot_loc(l0 - a * kFT0 + 1, l1 - b * kFT1 + 1, l2 - c * kFT2 + 1);
}
__device__ __forceinline__ void node_reads(int max_chunks, const int* s_cov, const int* s_bx, int l0,
                                           int l1, int l2, NodeReads& r) {
  const int sec0 = l0 < 3 ? -1 : (l0 == kFT0 - 1 ? 1 : 0);
  const int sec1 = l1 < 3 ? -1 : (l1 == kFT1 - 1 ? 1 : 0);
  const int sec2 = l2 < 3 ? -1 : (l2 == kFT2 - 1 ? 1 : 0);
  r.extra = 0;
  r.live = 0;
  // every LDS read first, unconditionally (ci is a valid neighbour index for
  // all e), then the tests as plain bit operations: with the reads behind
  // short-circuit tests the compiler branched around each one and waited on
  // each, 8 dependent LDS round trips in front of the slot loads
  int nc[8], bxy[8], bz[8], c0[8], ci[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int a = (e >> 2) ? sec0 : 0, b = ((e >> 1) & 1) ? sec1 : 0, c = (e & 1) ? sec2 : 0;
    ci[e] = (a + 1) * 9 + (b + 1) * 3 + (c + 1);
    nc[e] = s_cov[2 * ci[e] + 1];
    bxy[e] = s_bx[ci[e]];
    bz[e] = s_bx[32 + ci[e]];
    c0[e] = s_cov[2 * ci[e]];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ax = e >> 2, ay = (e >> 1) & 1, az = e & 1;
    const int a = ax ? sec0 : 0, b = ay ? sec1 : 0, c = az ? sec2 : 0;
    const int w0 = l0 - a * kFT0 + 1, w1 = l1 - b * kFT1 + 1, w2 = l2 - c * kFT2 + 1;
    // inside the cover's box: the node's bit of each axis mask (box_masks)
    const int inb = ((unsigned)bxy[e] >> w0) & ((unsigned)bxy[e] >> (16 + w1)) & ((unsigned)bz[e] >> w2) & 1;
    const bool on = ((!ax) | (sec0 != 0)) & ((!ay) | (sec1 != 0)) & ((!az) | (sec2 != 0)) & (nc[e] > 0) & (inb != 0);
    const int loc = slot_loc(w0, w1, w2);
    r.off[e] = on ? c0[e] * kFWin + loc : max_chunks * kFWin;
    r.extra |= (on & (nc[e] > 1)) ? (1 << e) : 0;
    r.live |= on ? (1 << e) : 0;
  }
}
__device__ __forceinline__ void add4(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
// one dword a lane, global -> LDS (LDS-DMA): lane l's word lands at
// lds_base + 4 l (lds_base wave-uniform), tracked by vmcnt like a load
__device__ __forceinline__ void glds4(const int* src, int* lds_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_base, 4, 0, 0);
}
// a window slot by its float4 offset, addressed as the slots' SGPR base plus a
// 32-bit byte offset (global_load saddr form: one VGPR per address, not a
// 64-bit pair; the slot array is < 4 GiB, checked where it is sized)
__device__ __forceinline__ float4 ld_slot(const float4* __restrict__ slots, int off) {
  return *(const float4*)((const char*)slots + (unsigned)off * 16u);
}
// The further chunks of covering tiles with several (tiles of > 256 particles:
// a lego scene at rest holds three quarters of its particles in tiles of 4-6
// chunks, profiles/chunk_hist/).  A node's remaining window loads form one
// ordered stream: the second chunks of its multi-chunk covers, e ascending,
// then for e ascending chunks 2 .. nc - 1 of cover e -- the order of the sum
// since round 5, minus the terms that were reads of the zero slot (an exact
// + 0 on a sum that is never -0, so every node's sum keeps its bits).  The
// stream is issued in batches of 8, a batch's loads in flight together (what
// the first chunks' batch already holds in VGPRs; 16 in flight spilled), and
// summed in stream order.  Until this form the second chunks went out as two
// batches of 4, most of them to the zero slot, and every later chunk was a
// load and its wait: a corner node of four 5-chunk tiles waited for 1 + 2 + 12
// dependent trips to slots that k_fused wrote through from other XCDs, where
// it now waits for 1 + 2.
// Per lane the stream is a list of runs (bit e of `runs`: cover e's second
// chunk; bit 8 + e: its chunks 2 .. nc - 1, when nc > 2) walked with two slot
// offsets {cur, end}: the next load is at cur, a chunk further each time, and
// a run that reaches end takes the next set bit (the cover's offsets again
// from the LDS cover table, as before: nothing of node_reads stays live).  The loop is
// wave-uniform -- it runs while any lane has a load left, the wave's maximum
// of ceil(remaining / 8) trips, at most 8 x the largest chunk count -- and a
// lane that is done reads the zero slot.  A wave without a multi-chunk cover
// never enters (the caller's wave-uniform guard).
#ifndef GSMPM_STREAM_BATCH
#define GSMPM_STREAM_BATCH 8
#endif
constexpr int kStreamBatch = GSMPM_STREAM_BATCH;  // loads of the stream in flight together (A/B)
__device__ __forceinline__ void node_extra(const float4* __restrict__ slots, const int* s_cov, int l0,
                                           int l1, int l2, int extra2, int zero, float4& acc) {
  int runs = extra2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int ci, loc;
    node_cover(l0, l1, l2, e, ci, loc);
    runs |= (((extra2 >> e) & 1) & (s_cov[2 * ci + 1] > 2)) << (8 + e);
  }
  // (one VGPR across the batches instead of l0, l1, l2: the node's offset in
  // its own tile's window and its three sections, two bits each)
  const int sec0 = l0 < 3 ? -1 : (l0 == kFT0 - 1 ? 1 : 0);
  const int sec1 = l1 < 3 ? -1 : (l1 == kFT1 - 1 ? 1 : 0);
  const int sec2 = l2 < 3 ? -1 : (l2 == kFT2 - 1 ? 1 : 0);
  const int key = slot_loc(l0 + 1, l1 + 1, l2 + 1) | ((sec0 & 3) << 12) | ((sec1 & 3) << 14) | ((sec2 & 3) << 16);
  static_assert(kFWin <= (1 << 12), "node_extra: the window offset takes 12 bits of the key");
  int cur = 0, end = 0;  // slot offsets of the run's next load and of its end
  auto next_run = [&]() {  // (runs != 0)
    const int r = __builtin_ctz(runs);
    runs &= runs - 1;
    const int a = (r & 4) ? (int)((unsigned)key << 18) >> 30 : 0, b = (r & 2) ? (int)((unsigned)key << 16) >> 30 : 0,
              c = (r & 1) ? (int)((unsigned)key << 14) >> 30 : 0;
    const int ci = (a + 1) * 9 + (b + 1) * 3 + (c + 1);
    const int loc = (key & 0xfff) - slot_loc(a * kFT0, b * kFT1, c * kFT2);
    const int c0 = s_cov[2 * ci], nc = s_cov[2 * ci + 1];
    cur = (c0 + (r < 8 ? 1 : 2)) * kFWin + loc;
    end = (c0 + (r < 8 ? 2 : nc)) * kFWin + loc;
  };
  if (runs) next_run();
  while (__builtin_amdgcn_ballot_w64(cur < end)) {
    float4 u[kStreamBatch];
#pragma unroll
    for (int j = 0; j < kStreamBatch; ++j) {
      u[j] = ld_slot(slots, cur < end ? cur : zero);
      cur += kFWin;
      if (cur >= end && runs) next_run();
    }
#pragma unroll
    for (int j = 0; j < kStreamBatch; ++j) add4(acc, u[j]);
  }
}

// Grid update of the fused pipeline: kGridParts one-wave workgroups per
// touched tile (64 consecutive owned nodes each), one owned node per lane (all
// 8 window reads in flight); a scene's ~900 touched tiles run in one round.
// Measured (lego frame): one 448-lane workgroup per tile 17.4 us, two 224-lane
// 12.45, four 112-lane 12.1, seven 64-lane 12.2 with k_fused unaffected
// (sim 3.27-3.28 against 3.29-3.32 ms/frame for two).
// esc_in: some particle scattered through gacc in the P2G this update consumes
// -> gacc is added to the owned nodes (and re-zeroed).  esc_clear: the flag the next P2G
// raises.  zc / zf (optional): the counts / touched flags the next binning
// launch accumulates into.
#ifndef GSMPM_GRID_PARTS
#define GSMPM_GRID_PARTS 7
#endif
constexpr int kGridParts = GSMPM_GRID_PARTS;  // workgroups per touched tile
constexpr int kGridT = kFTN / kGridParts;     // lanes per grid workgroup
// Nodes that no particle stencil can reach keep whatever v_out they held: a
// node outside every covering chunk's stencil box (the union of its
// particles' stencils at this P2G, which the next G2P gathers from unmoved)
// is read by no G2P before the next grid update rewrites it.  Every node
// inside a box is stored, massless or not, so a stencil node of a particle
// too light to register in the fixed-point sums (below 2^-51 of its chunk's
// heaviest: its mass rounds to zero) reads 0 as from the reference's reset
// grid (utils.py:177-183), not a stale value (round 4 skipped every massless
// node; test_gpu_mpm.py::test_heterogeneous_masses).  GSMPM_GRID_SKIP0=0
// stores every node of the touched tiles, =2 only nodes with mass (round 4's
// form, A/B).
#ifndef GSMPM_GRID_SKIP0
#define GSMPM_GRID_SKIP0 1
#endif
constexpr bool kGridSkip0 = GSMPM_GRID_SKIP0 != 0;
// GSMPM_GVEL_STORE (A/B): the v_out store of k_grid_f plain (0), streaming nt
// (1) or write-through sc1 (2; round 2: the gap after k_grid_f 2.6 -> 1.5 us,
// k_grid_f +0.8 us)
#ifndef GSMPM_GVEL_STORE
#define GSMPM_GVEL_STORE 0
#endif
constexpr int kGvelStore = GSMPM_GVEL_STORE;
// SLAB: a slab rank's grid pass (SlabWin hooks); the single-domain form is
// compiled without them -- their ~20 argument dwords pushed the kernel past
// the SGPR budget: 21 spilled SGPRs (21 v_writelane at the start, 26
// v_readlane restores, ~13 % of the ~350 VALU instructions a wave issues)
// against 4 now; k_grid_f 12.06 -> 11.67 us in the lego frame (5
// interleaved rounds, profiles/r05/ab/ab_rare_args_pk_r05k.txt)
// XCD-grouped work order (round 6).  Workgroup b runs on XCD b % 8, and each
// XCD has its own L2.  A window slot is read by the grid update of its own
// tile and of the upper neighbours whose low nodes it covers, and a tile's
// seven parts read one cover record; in the plain order (work item b: tile
// b / 7, part b % 7) the seven parts of a tile land on seven XCDs and
// neighbouring tiles on others, so each line is fetched once per XCD that
// reads it.  Here a tile's parts run on one XCD, and kGridGroup consecutive
// touched tiles (the touched list is in tile order: z-neighbours, whose
// windows share lines, are adjacent) go to one XCD before the next XCD's
// group.  tools/grid_f_bytes.py models the lego launch at 20.5 MB fetched in
// the plain order (FETCH_SIZE: 21.3 MB) and 10.9 MB grouped by 16.  The grid
// is a multiple of 8 workgroups (launch_grid_f).  GSMPM_GRID_GROUP=0: the
// plain order (A/B).
#ifndef GSMPM_GRID_GROUP
#define GSMPM_GRID_GROUP 16
#endif
constexpr int kGridGroup = GSMPM_GRID_GROUP;
// work item it of workgroup b (grid stride S): touched position P, part
// (P never decreases with it, so a workgroup stops at the first P past the count)
__device__ __forceinline__ void grid_work(int b, int it, int S, int& P, int& part) {
  if constexpr (kGridGroup == 0) {
    const int wt = b + it * S;
    P = wt / kGridParts;
    part = wt - P * kGridParts;
  } else {
    const int x = b & 7, m = (b >> 3) + it * (S >> 3);
    const int u = m / kGridParts, k = u / kGridGroup;
    part = m - u * kGridParts;
    P = (k * 8 + x) * kGridGroup + (u - k * kGridGroup);
  }
}
// EXT: node_update's, for a table that holds extended collider records
// (launch_grid_f; never with SLAB, whose handles refuse such records);
// GS = GridStepT: its MOV form, for a table that holds moving records
template <bool SLAB, bool EXT = false, class GS = GridStep>
__global__ __launch_bounds__(kGridT) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_grid_f(GridDims g, FTiles tl, ChunkIn ck, const int* __restrict__ tbox,
                                                    const float4* __restrict__ slots, float4* __restrict__ gacc,
                                                    float4* __restrict__ gvel, const BcTable* __restrict__ bct,
                                                    GS gs, const int* __restrict__ esc_in,
                                                    int* __restrict__ esc_clear, int* __restrict__ zc,
                                                    int* __restrict__ zf, SlabWin sw) {
  sim_prio();
  stamp(3, 0);
  // a slab's grid update runs as two passes (window tiles first, so their
  // partials can travel while the rest updates): the flag and the zeroing go
  // with the second
  const int pass = SLAB ? sw.pass : 0;
  // Every first load of the workgroup is issued here, together, before any
  // store: the escape flag, the touched count, the first touched tile (its
  // index clamped) and that tile's cover record -- its 27 neighbours' chunk
  // ranges (from the binning) and stencil boxes (published by this
  // substep's k_fused), so the slot addresses need no hop through the tile
  // tables.  Round 5 first had the flag and count after the zeroing stores
  // below, which the compiler may not hoist loads over (the pointers could
  // alias): three dependent scalar round trips before the first record load.
  int P0, part0;
  grid_work(blockIdx.x, 0, gridDim.x, P0, part0);
  const int i0 = min(P0, tl.ntiles - 1);
  // (the empty asm takes the three pointers into SGPRs at once, so their
  // kernel-argument loads come in the first batch and the three scalar loads
  // below leave together: one round trip, not two behind each other)
  const int* esc_p = esc_in;
  const int* cnt_p = ck.nchunk;
  const int* tch_p = ck.touched;
  asm volatile("" : "+s"(esc_p), "+s"(cnt_p), "+s"(tch_p));
  const bool pre = ck.rcov != nullptr;  // workgroup-uniform: records in LDS, the next one prefetched
  const int le = threadIdx.x;  // lane: record entry
  // Cover records reach LDS by LDS-DMA (global_load_lds: no VGPR holds
  // them): buffer b of s_rec / s_box holds the tile being updated, and at the
  // top of each iteration the NEXT tile's record and id are requested into
  // the other buffer, so a workgroup owning several tiles (config D: ~27 a
  // launch) pays one round trip a tile (its slot loads) instead of two.  A
  // record is 64 dwords (27 {first chunk, count} pairs + the "none" flag at
  // dword 54) and its boxes 64 (the masks' x | y << 16 words at 0..26, their
  // z words at 32..58); lane le moves dword le of each.
  __shared__ int s_rec[2][64];
  __shared__ int s_box[2][64];
  __shared__ int s_tn[2];
  // (wave 0's lanes only: the DMA writes lds_base + 4 x lane-in-wave)
  if (pre && threadIdx.x < 64) {
    glds4(reinterpret_cast<const int*>(ck.rcov) + (size_t)i0 * 2 * kRecStride + le, &s_rec[0][0]);
    glds4(ck.rbox + (size_t)i0 * kBoxStride + le, &s_box[0][0]);
  }
  typedef const int __attribute__((address_space(1)))* gint_p;  // global, not flat (flat loads count in lgkmcnt too)
  // (uniform words: readfirstlane keeps them in SGPRs, not three VGPRs live across the tile loop)
  const int esc0 = __builtin_amdgcn_readfirstlane(*(gint_p)esc_p);
  const int cnt0 = __builtin_amdgcn_readfirstlane(((gint_p)cnt_p)[1]);
  const int T0 = __builtin_amdgcn_readfirstlane(((gint_p)tch_p)[i0]);
  const int ng = g.ng;
  const bool esc = esc0 != 0;            // the escape accumulator holds sums: add it to the owned nodes
  const int ntouch = cnt0;               // tiles to update
  int b = 0;
  for (int it = 0;; ++it, b ^= 1) {
    int P, part;
    grid_work(blockIdx.x, it, gridDim.x, P, part);
    if (P >= ntouch) break;  // workgroup-uniform
    // this tile's DMA (issued a tile ago, or in the prologue) has landed;
    // readers of the other buffer are done.  The wait is explicit: the
    // compiler's own waits for LDS-DMA did not cover every read of these
    // arrays (the slab test caught stale records), and a one-wave
    // workgroup's barrier compiles to nothing.  What else it waits for is
    // the previous tile's v_out stores (L2 write acks, not an HBM trip).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int pn, partn;
    grid_work(blockIdx.x, it + 1, gridDim.x, pn, partn);
    if (pre && pn < ntouch && threadIdx.x < 64) {  // workgroup-uniform (kGridT = 64: one wave)
      glds4(reinterpret_cast<const int*>(ck.rcov) + (size_t)pn * 2 * kRecStride + le, &s_rec[b ^ 1][0]);
      glds4(ck.rbox + (size_t)pn * kBoxStride + le, &s_box[b ^ 1][0]);
      if (le == 0) glds4(ck.touched + pn, &s_tn[b ^ 1]);
    }
    int* s_cov = s_rec[b];
    int* s_bx = s_box[b];
    const int q = threadIdx.x + part * kGridT;
    const int l0 = q / (kFT1 * kFT2), l1 = (q / kFT2) % kFT1, l2 = q % kFT2;
    const int T = it == 0 ? T0 : pre ? s_tn[b] : ck.touched[P];
    if ((unsigned)T >= (unsigned)tl.ntiles) continue;  // workgroup-uniform; never taken (P < count)
    int ti, tj, tk;
    ftile_decode(tl, T, ti, tj, tk);
    if (SLAB && pass != 0 && slab_tile_in_window(sw, ti) != (pass == 1)) continue;  // workgroup-uniform
    if (it == 0) stamp(3, 2);
    // a tile k_fused appended (add_lower_tiles) has no record: "none" flag
    const bool tables = !pre || s_cov[54] != 0;  // workgroup-uniform
    if (tables) {
      load_cover27(ck, tbox, tl, ti, tj, tk, s_cov, s_bx);
      __syncthreads();
    }
    if (it == 0) stamp(3, 3);
#ifdef GSMPM_STAMPS
    if (it == 0 && threadIdx.x == 0) {  // the tile, its part, its own and its covers' largest chunk count
      int ncmax = 0;
      for (int e = 0; e < 27; ++e) ncmax = max(ncmax, s_cov[2 * e + 1]);
      stamp_val(3, 5, (unsigned long long)T);
      stamp_val(3, 6, (unsigned long long)(s_cov[2 * 13 + 1] | (ncmax << 16)));
      stamp_val(3, 7, (unsigned long long)part);
    }
#endif
    const int i = ti * kFT0 + l0, j = tj * kFT1 + l1, k = tk * kFT2 + l2;
    if ((unsigned)i < (unsigned)ng && (unsigned)j < (unsigned)ng && (unsigned)k < (unsigned)ng) {
      const size_t idx = ((size_t)i * ng + j) * ng + k;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      NodeReads r;
      node_reads(tl.max_chunks, s_cov, s_bx, l0, l1, l2, r);
      const bool reach = r.live != 0;  // some stencil box covers the node
      float4 v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ld_slot(slots, r.off[e]);
#pragma unroll
      for (int e = 0; e < 8; ++e) add4(a, v[e]);
      if (__builtin_amdgcn_ballot_w64(r.extra != 0))  // wave-uniform: a wave of single-chunk covers skips it whole
        node_extra(slots, s_cov, l0, l1, l2, r.extra, tl.max_chunks * kFWin, a);
      if (esc) {  // the nodes an escape wrote lie in touched tiles (mark_escape_tiles); zero what was written
        const float4 e = gacc[idx];
        add4(a, e);
        if (e.x != 0.f || e.y != 0.f || e.z != 0.f || e.w != 0.f) gacc[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      bool inrect = false;
      if constexpr (SLAB) {
        const int sww = sw.W ? slab_window_of(sw, i) : -1;
        inrect = sww >= 0 && (unsigned)(j - sw.y0[sww]) < (unsigned)sw.ny[sww] &&
                 (unsigned)(k - sw.z0[sww]) < (unsigned)sw.nz[sww];
        if (sww >= 0 && !inrect && a.w != 0.f) *sw.oob = 1;
        if (inrect)  // a window node: this rank's partial, totalled after the exchange (k_win_update)
          sw.part[sww][((size_t)(i - sw.a[sww]) * sw.ny[sww] + (j - sw.y0[sww])) * sw.nz[sww] + (k - sw.z0[sww])] = a;
      }
      if (inrect) {
      } else if (!kGridSkip0 || a.w != 0.f || (reach && GSMPM_GRID_SKIP0 == 1)) {
        if constexpr (kGvelStore == 1)
          nt_store4(gvel + idx, node_update<EXT>(a, i, j, k, g, gs, bct));
        else if constexpr (kGvelStore == 2)
          wt_store4(gvel + idx, node_update<EXT>(a, i, j, k, g, gs, bct));
        else
          gvel[idx] = node_update<EXT>(a, i, j, k, g, gs, bct);
      }
    }
    if (it == 0) stamp(3, 4);
  }
  // the zeroing for the next launches, after the tiles: its stores are not
  // in front of any wait above
  if (blockIdx.x == 0 && threadIdx.x == 0 && pass != 1) *esc_clear = 0;
  if (zc && pass != 1) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t <= tl.ntiles; t += gridDim.x * blockDim.x) {
      zc[t] = 0;
      if (t < tl.ntiles) zf[t] = 0;
    }
  }
  stamp(3, 1);
}

// bin every particle by its current x (set_particles / resort / set x)
__global__ __launch_bounds__(256) void k_bin_all_f(Particles ps, GridDims g, BinOutF bo) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < ps.count()) {
    float x[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = ps.ld(PX + d, p);
    int tc[3];
    const int t = ftile_of(x, g, bo.tl, tc);
    bo.ptile[p] = t;
    bo.pslot[p] = reserve_f(bo, t, 1);
  }
}
