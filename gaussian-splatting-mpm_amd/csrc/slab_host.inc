// slab_host.inc -- host side of the multi-GPU slabs (slab.h): transports
// (RCCL, host callback), the per-substep window exchange, particle migration
// and the C-ABI entry points.  Included by mpm.hip after the simulator
// helpers; see slab.h for the decomposition.

namespace gsmpm {

// ------------------------------------------------------------------ RCCL --
// The RCCL already loaded in the process (torch's librccl.so.1 when torch is
// imported; else the ROCm one), bound by dlsym: libgsmpm.so itself has no
// link-time RCCL dependency, so it loads on hosts without it.
struct RcclId {
  char internal[128];
};
struct RcclApi {
  bool ok = false;
  std::string why;
  int (*get_unique_id)(RcclId*) = nullptr;
  int (*comm_init_rank)(void**, int, RcclId, int) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  int (*send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*error_string)(int) = nullptr;
};
constexpr int kRcclInt8 = 0;  // ncclInt8: byte counts (send/recv do no arithmetic)

static RcclApi load_rccl() {
  RcclApi a;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW);
  if (!lib) {
    a.why = "cannot load librccl.so.1";
    return a;
  }
  auto sym = [&](const char* n) { return dlsym(lib, n); };
  a.get_unique_id = reinterpret_cast<int (*)(RcclId*)>(sym("ncclGetUniqueId"));
  a.comm_init_rank = reinterpret_cast<int (*)(void**, int, RcclId, int)>(sym("ncclCommInitRank"));
  a.comm_destroy = reinterpret_cast<int (*)(void*)>(sym("ncclCommDestroy"));
  a.group_start = reinterpret_cast<int (*)()>(sym("ncclGroupStart"));
  a.group_end = reinterpret_cast<int (*)()>(sym("ncclGroupEnd"));
  a.send = reinterpret_cast<int (*)(const void*, size_t, int, int, void*, hipStream_t)>(sym("ncclSend"));
  a.recv = reinterpret_cast<int (*)(void*, size_t, int, int, void*, hipStream_t)>(sym("ncclRecv"));
  a.error_string = reinterpret_cast<const char* (*)(int)>(sym("ncclGetErrorString"));
  a.ok = a.get_unique_id && a.comm_init_rank && a.comm_destroy && a.group_start && a.group_end && a.send && a.recv &&
         a.error_string;
  if (!a.ok) a.why = "librccl.so.1 lacks an ncclSend/ncclRecv/ncclCommInitRank symbol";
  return a;
}
static RcclApi& rccl() {
  static RcclApi api = load_rccl();
  return api;
}

#define GSMPM_RCCL(call)                                                                   \
  do {                                                                                     \
    const int r_ = (call);                                                                 \
    if (r_ != 0) {                                                                         \
      ::gsmpm::set_error(std::string(#call) + ": " + ::gsmpm::rccl().error_string(r_));   \
      return GSMPM_EHIP;                                                                   \
    }                                                                                      \
  } while (0)

// ------------------------------------------------------------- exchange --
// One symmetric exchange round with n peers: send[i] (send_bytes[i])
// to peers[i], recv[i] (recv_bytes[i]) from peers[i], device buffers.  RCCL:
// enqueued on the comm stream behind everything `st` has queued; with
// join, `st` waits for it (else the caller joins later, xport_join).
// CALLBACK: synchronous on the host, through pinned host copies.
static int xport_exchange(gsmpm_mpm* h, const gsmpm_transport* xp, hipStream_t st, int n, const int* peers,
                          void* const* send, const size_t* sb, void* const* recv, const size_t* rb, bool join) {
  if (n == 0) return GSMPM_OK;
  GSMPM_REQUIRE(xp && xp->kind != GSMPM_XPORT_NONE, "slab exchange: this slab has neighbours but no transport");
  if (xp->kind == GSMPM_XPORT_RCCL) {
    RcclApi& R = rccl();
    GSMPM_REQUIRE(R.ok, ("slab exchange: " + R.why).c_str());
    GSMPM_REQUIRE(xp->comm, "slab exchange: null RCCL communicator");
    // Eager, the group runs on the comm stream (forked from and joined back
    // to `st` by events), overlapping the interior grid update.  Inside a
    // capture it runs on `st` itself: RCCL's capture of a group on a stream
    // that joined the capture through an event wait crashed
    // hipStreamEndCapture (tools/probe/rccl_shared_probe.py, 2 ranks, RCCL
    // 2.26.6).  GSMPM_RCCL_INSTREAM=1 does the same eagerly.
    static const bool env_in = std::getenv("GSMPM_RCCL_INSTREAM") && std::getenv("GSMPM_RCCL_INSTREAM")[0] == '1';
    const bool instream = env_in || h->capturing;
    hipStream_t cs = instream ? st : h->s_comm;
    const hipEvent_t ev_pack = h->s_ev_pack, ev_x = h->s_ev_x;
    if (!instream) {
      GSMPM_HIP(hipEventRecord(ev_pack, st));
      GSMPM_HIP(hipStreamWaitEvent(cs, ev_pack, 0));
    }
    gtrace("rccl group");
    GSMPM_RCCL(R.group_start());
    for (int i = 0; i < n; ++i) {
      if (sb[i]) GSMPM_RCCL(R.send(send[i], sb[i], kRcclInt8, peers[i], xp->comm, cs));
      if (rb[i]) GSMPM_RCCL(R.recv(recv[i], rb[i], kRcclInt8, peers[i], xp->comm, cs));
    }
    GSMPM_RCCL(R.group_end());
    gtrace("rccl group end");
    if (!instream) {
      GSMPM_HIP(hipEventRecord(ev_x, cs));
      h->s_ev_join = ev_x;
      if (join) GSMPM_HIP(hipStreamWaitEvent(st, ev_x, 0));
    } else {
      h->s_ev_join = nullptr;
    }
    return GSMPM_OK;
  }
  GSMPM_REQUIRE(xp->kind == GSMPM_XPORT_CALLBACK && xp->fn, "slab exchange: unknown transport");
  // host-staged: the callback sees pinned host copies of the buffers
  size_t tot = 0;
  for (int i = 0; i < n; ++i) tot += ((sb[i] + 255) & ~size_t(255)) + ((rb[i] + 255) & ~size_t(255));
  if (tot > h->x_host_cap) {
    release(h, &h->x_host);
    h->x_host_cap = 0;
    GSMPM_HIP(alloc_host(h, &h->x_host, tot + tot / 2 + 4096));
    h->x_host_cap = tot + tot / 2 + 4096;
  }
  std::vector<void*> hs(n), hr(n);
  char* q = h->x_host;
  for (int i = 0; i < n; ++i) {
    hs[i] = q;
    q += (sb[i] + 255) & ~size_t(255);
    hr[i] = q;
    q += (rb[i] + 255) & ~size_t(255);
    if (sb[i]) GSMPM_HIP(hipMemcpyAsync(hs[i], send[i], sb[i], hipMemcpyDeviceToHost, st));
  }
  GSMPM_HIP(hipStreamSynchronize(st));
  const int rc = xp->fn(xp->user, n, peers, hs.data(), sb, hr.data(), rb);
  GSMPM_REQUIRE(rc == 0, "slab exchange: the transport callback failed");
  for (int i = 0; i < n; ++i)
    if (rb[i]) GSMPM_HIP(hipMemcpyAsync(recv[i], hr[i], rb[i], hipMemcpyHostToDevice, st));
  return GSMPM_OK;
}
static int xport_join(gsmpm_mpm* h, const gsmpm_transport* xp, hipStream_t st) {
  if (xp && xp->kind == GSMPM_XPORT_RCCL && (h->s_has[0] || h->s_has[1]) && h->s_ev_join)
    GSMPM_HIP(hipStreamWaitEvent(st, h->s_ev_join, 0));
  return GSMPM_OK;
}

// Grid update of one slab substep: window tiles first (their nodes' partials
// into the send buffers), the partials' exchange on the comm stream while the
// interior tiles update, then the window totals' update.
static int slab_grid_phase(gsmpm_mpm* h, int wp, float dt, uint32_t mask, int ep, int* zc, int* zf, hipStream_t st,
                           const gsmpm_transport* xp) {
  SlabWin sw = h->sw;
  const bool any = sw.on[0] || sw.on[1];
  sw.pass = any ? 1 : 0;
  int rc = GSMPM_OK;
  if (any) rc = launch_grid_f(h, wp, dt, mask, ep, nullptr, nullptr, st, nullptr, &sw);
  if (rc) return rc;
  if (any) {
    int peers[2];
    void* snd[2];
    void* rcv[2];
    size_t sb[2], rb[2];
    int n = 0;
    for (int w = 0; w < 2; ++w)
      if (sw.on[w]) {
        peers[n] = h->s_rank + (w == 0 ? -1 : 1);
        snd[n] = sw.part[w];
        rcv[n] = h->s_recv[w];
        sb[n] = rb[n] = sizeof(float4) * (size_t)sw.W * sw.ny[w] * sw.nz[w];  // the rect (same on both ranks)
        ++n;
      }
    if (h->capturing && xp && xp->kind == GSMPM_XPORT_RCCL) {
      // inside a capture the RCCL group stays on `st` (xport_exchange) and the
      // interior pass is the branch forked to the comm stream, so the graph
      // still overlaps the exchange with the interior update
      GSMPM_HIP(hipEventRecord(h->s_ev_pack, st));
      GSMPM_HIP(hipStreamWaitEvent(h->s_comm, h->s_ev_pack, 0));
      SlabWin sw2 = sw;
      sw2.pass = 2;
      rc = launch_grid_f(h, wp, dt, mask, ep, zc, zf, h->s_comm, nullptr, &sw2);
      if (rc) return rc;
      GSMPM_HIP(hipEventRecord(h->s_ev_x, h->s_comm));
      rc = xport_exchange(h, xp, st, n, peers, snd, sb, rcv, rb, /*join=*/true);
      if (rc) return rc;
      GSMPM_HIP(hipStreamWaitEvent(st, h->s_ev_x, 0));
      sw.pass = 0;  // the interior pass is done
    } else {
      rc = xport_exchange(h, xp, st, n, peers, snd, sb, rcv, rb, /*join=*/false);
      if (rc) return rc;
    }
  }
  if (!any || sw.pass != 0) {
    sw.pass = any ? 2 : 0;
    rc = launch_grid_f(h, wp, dt, mask, ep, zc, zf, st, nullptr, &sw);
    if (rc || !any) return rc;
    rc = xport_join(h, xp, st);
    if (rc) return rc;
  }
  size_t nodes = 0;
  for (int w = 0; w < 2; ++w)
    if (sw.on[w]) nodes += (size_t)sw.W * sw.ny[w] * sw.nz[w];
  if (nodes == 0) return GSMPM_OK;
  hipLaunchKernelGGL(k_win_update, dim3((unsigned)std::min<size_t>((nodes + 255) / 256, 2048)), dim3(256), 0, st, h->g,
                     h->sw, (const float4*)h->s_recv[0], (const float4*)h->s_recv[1], h->gvel,
                     (const BcTable*)h->dev_bc, grid_step(h, dt, mask));
  GSMPM_LAUNCH_CHECK();
  return GSMPM_OK;
}

// the migration payloads of `cap` leavers a way, zeroed (they only grow; the
// caller drops the graphs, which bake their size and addresses)
static int grow_mig(gsmpm_mpm* h, int cap) {
  for (int w = 0; w < 2; ++w) {
    if (!h->s_has[w]) continue;
    release(h, &h->mig_send[w]);
    release(h, &h->mig_recv[w]);
    GSMPM_HIP(alloc(h, &h->mig_send[w], mig_payload_floats(cap), kMemCommon, kFillZero));
    GSMPM_HIP(alloc(h, &h->mig_recv[w], mig_payload_floats(cap), kMemCommon, kFillZero));
  }
  h->mig_cap = cap;
  return GSMPM_OK;
}

static MigGeom mig_geom(const gsmpm_mpm* h) { return MigGeom{h->g.inv_dx, h->s_lo, h->s_hi, h->s_has[0], h->s_has[1]}; }

// Every rank's record (slab.h SlabRec) to every rank, at the start of the
// first step call after the particles were set and at the end of every call:
// the host then knows the live count, every rank's errors (so an invalid
// state stops ALL ranks at the same call, with the same message -- one rank
// stopping alone would leave the others blocked in their next exchange with
// it), the boxes the next call's window rects are agreed from, and the
// migration payload capacity all ranks use.  One exchange round of 64 bytes a
// peer and one host sync per call.  The exchange and the copy to the host
// are the last work of a step call's body, so with RCCL they are part of the
// captured graph (eager RCCL sends between replays of captured ones lost
// their ordering on RCCL's socket transport: a 64-byte record receive met a
// window-exchange chunk); slab_check reads them after the sync.
static int slab_records(gsmpm_mpm* h, const gsmpm_transport* xp, hipStream_t st) {
  const int world = h->s_world, me = h->s_rank;
  const int nrec = rec_ints_of(h->g.ng);
  int* mine = h->s_rec + (size_t)nrec * me;
  hipLaunchKernelGGL(k_rec_init, dim3(1), dim3(256), 0, st, (const int*)h->s_drift, (const int*)h->d_n,
                     h->prm.n_particles, h->s_lo, h->s_hi, nrec, mine, (const float*)h->s_wdev);
  hipLaunchKernelGGL(k_slab_record, dim3(std::max(1, std::min(div_up(h->np, 256), 1024))), dim3(256), 0, st,
                     particles_of(h), mig_geom(h), h->s_margin, h->g.ng, mine);
  GSMPM_LAUNCH_CHECK();
  if (world > 1) {
    std::vector<int> peers;
    std::vector<void*> snd, rcv;
    std::vector<size_t> sz;
    for (int r = 0; r < world; ++r)
      if (r != me) {
        peers.push_back(r);
        snd.push_back(mine);
        rcv.push_back(h->s_rec + (size_t)nrec * r);
        sz.push_back(sizeof(int) * nrec);
      }
    int rc = xport_exchange(h, xp, st, (int)peers.size(), peers.data(), snd.data(), sz.data(), rcv.data(), sz.data(),
                            /*join=*/true);
    if (rc) return rc;
  }
  GSMPM_HIP(hipMemcpyAsync(h->s_rec_host, h->s_rec, sizeof(int) * nrec * (size_t)world, hipMemcpyDeviceToHost,
                           st));
  return GSMPM_OK;
}

// Re-cut the slabs (SURVEY 8(e): "balance slab thickness by particle count,
// rebalance per frame").  Every rank holds every rank's record -- its bounds
// and its particles' base-plane histogram -- so all ranks compute the same new
// bounds here, at the end of a step call.  When the most loaded slab holds more
// than (1 + tol) x the mean, the bounds move to the count quantiles of the
// summed histogram, clamped so that (a) each new bound stays inside the old
// slabs next to it -- every particle's new owner is its old owner or a
// neighbour, which the ordinary migration reaches -- and (b) every slab keeps
// 2 margin + 2 planes.  The next call then opens with a migration to the new
// bounds (inside its captured graph), with the payload capacity raised to the
// most particles any bound moves; the windows move with the bounds and their
// rects cover every rank's particles for that call.
static int slab_rebalance(gsmpm_mpm* h) {
  const int world = h->s_world, ng = h->g.ng, nrec = rec_ints_of(ng), W = 2 * h->s_margin + 2;
  if (!h->s_rebal_on || world < 2 || h->s_rebal_pending) return GSMPM_OK;
  const int* R = h->s_rec_host;
  std::vector<long> hist(ng, 0);
  // each rank's share of the particles is its weight over the sum (all 1: equal
  // counts); a rank with other work per frame -- the one that renders the
  // gathered frame -- takes a smaller share (gsmpm_mpm_slab_set_weight)
  std::vector<double> wt(world, 1.0);
  long n = 0;
  double wsum = 0.0;
  for (int r = 0; r < world; ++r) {
    const int* q = R + (size_t)nrec * r;
    for (int p = 0; p < ng; ++p) hist[p] += q[kRecHdr + p];
    n += q[RF_N];
    float wf;
    std::memcpy(&wf, q + RF_WEIGHT, sizeof(float));
    wt[r] = (std::isfinite(wf) && wf > 0.f) ? (double)wf : 1.0;
    wsum += wt[r];
  }
  bool off = false;  // some rank holds more than (1 + tol) times its share
  for (int r = 0; r < world; ++r)
    off = off || (double)R[(size_t)nrec * r + RF_N] > (1.0 + h->s_rebal_tol) * (double)n * wt[r] / wsum;
  if (n == 0 || !off) return GSMPM_OK;
  const std::vector<int>& b = h->s_bounds;
  std::vector<int> nb(world + 1);
  nb[0] = 0;
  nb[world] = ng;
  long cum = 0;
  int p = 0;
  double wcum = 0.0;
  for (int r = 1; r < world; ++r) {  // the plane where the cumulative count crosses the shares of ranks < r
    wcum += wt[r - 1];
    const double target = (double)n * wcum / wsum;
    while (p < ng && (double)(cum + hist[p]) <= target) cum += hist[p++];
    const bool next = p < ng && (double)(cum + hist[p]) - target < target - (double)cum;  // the nearer edge
    nb[r] = next ? p + 1 : p;
  }
  for (int r = 1; r < world; ++r) nb[r] = std::min(std::max(nb[r], b[r - 1]), b[r + 1]);  // (a)
  for (int r = 1; r < world; ++r) nb[r] = std::max(nb[r], nb[r - 1] + W);                // (b)
  for (int r = world - 1; r >= 1; --r) nb[r] = std::min(nb[r], nb[r + 1] - W);
  for (int r = 1; r < world; ++r)
    if (nb[r] < b[r - 1] || nb[r] > b[r + 1] || nb[r] - nb[r - 1] < W) return GSMPM_OK;  // no feasible cut
  if (nb == b) return GSMPM_OK;
  // the particles each bound moves, and each new slab's count (within every capacity)
  long moved = 0;
  for (int r = 1; r < world; ++r) {
    long m = 0;
    for (int q = std::min(b[r], nb[r]); q < std::max(b[r], nb[r]); ++q) m += hist[q];
    moved = std::max(moved, m);
  }
  for (int r = 0; r < world; ++r) {
    long c = 0;
    for (int q = nb[r]; q < nb[r + 1]; ++q) c += hist[q];
    if (c > R[(size_t)nrec * r + RF_CAP]) return GSMPM_OK;
  }
  int cap = std::max(256, h->mig_cap);
  while (cap < 2 * moved && cap < h->np) cap *= 2;
  if (cap > h->mig_cap) {
    const int rc = grow_mig(h, cap);
    if (rc) return rc;
  }
  h->s_bounds = nb;
  h->s_lo = nb[h->s_rank];
  h->s_hi = nb[h->s_rank + 1];
  h->sw.a[0] = h->s_lo - h->s_margin;
  h->sw.a[1] = h->s_hi - h->s_margin;
  h->s_rebal_pending = true;
  drop_graphs(h);  // the drift bounds, windows and payload size are baked into them
  return GSMPM_OK;
}

static int slab_check(gsmpm_mpm* h, hipStream_t st) {
  const int world = h->s_world, me = h->s_rank;
  GSMPM_HIP(hipStreamSynchronize(st));
  h->s_host_syncs += 1;
  const int* R = h->s_rec_host;
  const int nrec = rec_ints_of(h->g.ng);
  h->n = R[(size_t)nrec * me + RF_N];
  h->s_migrated = R[(size_t)nrec * me + RF_MIGRATED];
  h->s_deferred = R[(size_t)nrec * me + RF_DEFERRED];
  h->s_bounds.assign(world + 1, 0);
  for (int r = 0; r < world; ++r) h->s_bounds[r + 1] = R[(size_t)nrec * r + RF_SHI];
  h->s_synced = true;
  // payload capacity for the next call (the same on every rank: the same
  // records): a power of two >= twice the most leavers one migration sent and
  // >= half the particles within the margin of a bound (round 3 took a
  // quarter: a call's payload size is fixed, and a leaver deferred at one
  // migration keeps drifting and can trip the drift check by the next, so
  // the band term now covers a surge of half the band at once; the payload
  // is 204 B a particle, sent whole at every migration); it only grows
  long need = 0;
  for (int r = 0; r < world; ++r) {
    const int* q = R + (size_t)nrec * r;
    need = std::max(need, 2L * q[RF_SENDMAX]);
    need = std::max(need, (long)std::max(q[RF_BAND_LO], q[RF_BAND_HI]) / 2);
  }
  int cap = 256;
  while (cap < need && cap < h->np) cap *= 2;
  // GSMPM_SLAB_MIG_CAP: the first capacity (tests: force deferrals); it grows as usual after
  if (const char* mc = std::getenv("GSMPM_SLAB_MIG_CAP"))
    if (h->mig_cap == 0) cap = std::max(1, std::atoi(mc));
  if (world > 1 && cap > h->mig_cap) {
    const int rc = grow_mig(h, cap);
    if (rc) return rc;
    drop_graphs(h);  // the payload size and buffers are baked into them
  }
  for (int r = 0; r < world; ++r) {
    const int* q = R + (size_t)nrec * r;
    const std::string who = "gsmpm_mpm_slab_step: rank " + std::to_string(r) + ": ";
    if (q[RF_FLAGS] & 16) {
      set_error(who + "particle state (position, mass, velocity, C or stress) became non-finite (NaN / Inf); the "
                "state is invalid");
      return GSMPM_ESTATE;
    }
    if (q[RF_FLAGS] & 2) {
      set_error(who + "a window node outside the exchanged rect received mass (a particle moved further across the "
                "slab plane than the rect's margin allows since the rects were agreed); the window exchange missed "
                "it and the state is invalid");
      return GSMPM_ESTATE;
    }
    if (q[RF_FLAGS] & 1) {
      set_error(who + "a particle drifted more than `margin` planes past its slab between migrations; the window "
                "exchange missed its contributions and the state is invalid (use a smaller interval or a larger "
                "margin)");
      return GSMPM_ESTATE;
    }
    if (q[RF_FLAGS] & 8) {
      set_error(who + std::to_string(q[RF_NWANT]) + " particles after a migration, in a slab of capacity " +
                std::to_string(q[RF_CAP]) + " (create the slab with more capacity)");
      return GSMPM_ESTATE;
    }
  }
  return slab_rebalance(h);
}

// The rect of each window: the yz nodes the two ranks of its bound can touch
// during this step call.  Both ranks hold the same two records (slab_check), so
// they form the same union of their particles' base-node boxes, widened by
// the stencil (+3) and by how far a particle can move in the call, T = nsub
// dt: twice (v_max + dv_imp) T + |g| T^2 / 2 per axis, with v_max the larger
// rank's max |v| on that axis and dv_imp the most velocity the call's active
// impulses can add to the lightest particle of either rank (sum over the
// substeps of |f| sdt / m_min, boundary_conditions.py:41-45), at least
// interval + 1 nodes; aligned to 8 nodes and never shrinking after the first
// agreement.  Velocity gained from stress (elastic rebound) is not bounded
// here: the factor 2 is its allowance, and a window node outside the rect
// that receives mass raises a flag (k_grid_f) and the state is reported
// invalid.  A changed rect re-lays the partial buffers (zeroed) and drops
// the captured graphs (their exchange sizes change).
static int slab_rect_update(gsmpm_mpm* h, float dt, int nsub, const uint32_t* bc, hipStream_t st) {
  if (h->s_world == 1) return GSMPM_OK;
  const int ng = h->g.ng, me = h->s_rank;
  const int* R = h->s_rec_host;
  const double T = (double)nsub * dt;
  const double g = std::sqrt(h->prm.gravity[0] * h->prm.gravity[0] + h->prm.gravity[1] * h->prm.gravity[1] +
                             h->prm.gravity[2] * h->prm.gravity[2]);
  auto fbits = [](int b) {
    float f;
    std::memcpy(&f, &b, 4);
    return (double)f;
  };
  // impulse budget per unit mass (y, z): sum over the call's substeps of the active impulses' |f| sdt
  double imp[2] = {0.0, 0.0};
  for (int s = 0; s < nsub; ++s)
    for (int b = 0; b < h->host_bc.n_imp; ++b) {
      const Impulse& im = h->host_bc.imp[b];
      if (bc && !((bc[s] >> im.bit) & 1u)) continue;
      imp[0] += std::fabs((double)im.f[1]) * im.sdt;
      imp[1] += std::fabs((double)im.f[2]) * im.sdt;
    }
  auto widen = [&](double v) {
    const double cells = 2.0 * (v * T + 0.5 * g * T * T) * h->g.inv_dx;
    if (!std::isfinite(cells) || cells > ng) return ng;
    return std::max(h->s_interval + 1, (int)std::ceil(cells) + 1);
  };
  SlabWin& sw = h->sw;
  bool changed = false;
  for (int w = 0; w < 2; ++w) {
    if (!sw.on[w]) continue;
    const int nrec = rec_ints_of(ng);
    const int* a = R + (size_t)nrec * me;
    const int* b = R + (size_t)nrec * (me + (w == 0 ? -1 : 1));
    int ylo = std::min(a[RF_YLO], b[RF_YLO]), yhi = std::max(a[RF_YHI], b[RF_YHI]);
    int zlo = std::min(a[RF_ZLO], b[RF_ZLO]), zhi = std::max(a[RF_ZHI], b[RF_ZHI]);
    if (h->s_rebal_pending)  // particles change owner this call: every rank's box
      for (int r = 0; r < h->s_world; ++r) {
        const int* q = R + (size_t)nrec * r;
        ylo = std::min(ylo, q[RF_YLO]);
        yhi = std::max(yhi, q[RF_YHI]);
        zlo = std::min(zlo, q[RF_ZLO]);
        zhi = std::max(zhi, q[RF_ZHI]);
      }
    const double mmin = std::min(fbits(a[RF_MMIN]), fbits(b[RF_MMIN]));  // NaN when neither has particles
    const double dvy = imp[0] > 0.0 ? imp[0] / mmin : 0.0, dvz = imp[1] > 0.0 ? imp[1] / mmin : 0.0;
    const int Ey = widen(std::max(fbits(a[RF_VY]), fbits(b[RF_VY])) + dvy);
    const int Ez = widen(std::max(fbits(a[RF_VZ]), fbits(b[RF_VZ])) + dvz);
    int y0 = 0, y1 = 0, z0 = 0, z1 = 0;  // empty when neither side has particles
    if (ylo <= yhi) {
      auto lo8 = [](int v) { return v <= 0 ? 0 : (v / 8) * 8; };
      auto hi8 = [ng](int v) { return std::min(ng, ((std::max(v, 0) + 7) / 8) * 8); };
      y0 = lo8(ylo - Ey);
      y1 = hi8(yhi + 3 + Ey);
      z0 = lo8(zlo - Ez);
      z1 = hi8(zhi + 3 + Ez);
    }
    if (h->s_rect_set && sw.ny[w] > 0 && sw.nz[w] > 0) {
      if (y1 <= y0 || z1 <= z0) {
        y0 = sw.y0[w], y1 = sw.y0[w] + sw.ny[w], z0 = sw.z0[w], z1 = sw.z0[w] + sw.nz[w];
      } else {
        y0 = std::min(y0, sw.y0[w]);
        y1 = std::max(y1, sw.y0[w] + sw.ny[w]);
        z0 = std::min(z0, sw.z0[w]);
        z1 = std::max(z1, sw.z0[w] + sw.nz[w]);
      }
    }
    const int ny = std::max(0, y1 - y0), nz = std::max(0, z1 - z0);
    if (!h->s_rect_set || y0 != sw.y0[w] || ny != sw.ny[w] || z0 != sw.z0[w] || nz != sw.nz[w]) {
      sw.y0[w] = y0;
      sw.ny[w] = ny;
      sw.z0[w] = z0;
      sw.nz[w] = nz;
      GSMPM_HIP(hipMemsetAsync(sw.part[w], 0, sizeof(float4) * (size_t)sw.W * ng * ng, st));
      changed = true;
    }
  }
  h->s_rect_set = true;
  if (changed) drop_graphs(h);
  return GSMPM_OK;
}

// Particle migration, on the device (capturable): leavers to the neighbours'
// fixed-size payloads (beyond the capacity they stay for a later
// migration), stayers compacted, arrivals appended; the live count d_n and
// caller order := the new storage order; then a full re-binning.
static int slab_migrate(gsmpm_mpm* h, const gsmpm_transport* xp, hipStream_t st) {
  const int nblk = std::max(1, div_up(h->np, 256));
  const MigGeom mg = mig_geom(h);
  const MigSend ms{{h->s_has[0] ? h->mig_send[0] : nullptr, h->s_has[1] ? h->mig_send[1] : nullptr}, h->mig_cap,
                   h->s_drift};
  hipLaunchKernelGGL(k_mig_count, dim3(nblk), dim3(256), 0, st, particles_of(h), mg, h->mig_bcnt);
  hipLaunchKernelGGL(k_mig_scan, dim3(1), dim3(1024), 0, st, nblk, (const int*)h->mig_bcnt, h->mig_boff, h->mig_tot,
                     ms);
  const MigOut mo{h->fu.planes_alt, h->cold_alt, h->gid_alt};
  hipLaunchKernelGGL(k_mig_scatter, dim3(nblk), dim3(256), 0, st, particles_of(h), (const int*)h->orig,
                     (const int*)h->gid, mg, (const int*)h->mig_boff, (const int*)h->mig_tot, mo, ms);
  GSMPM_LAUNCH_CHECK();
  {
    int peers[2], n_x = 0;
    void* snd[2];
    void* rcv[2];
    size_t sb[2];
    for (int w = 0; w < 2; ++w)
      if (h->s_has[w]) {
        peers[n_x] = h->s_rank + (w == 0 ? -1 : 1);
        snd[n_x] = h->mig_send[w];
        rcv[n_x] = h->mig_recv[w];
        sb[n_x] = mig_payload_floats(h->mig_cap) * sizeof(float);
        ++n_x;
      }
    const int rc = xport_exchange(h, xp, st, n_x, peers, snd, sb, rcv, sb, /*join=*/true);
    if (rc) return rc;
  }
  const MigRecv mr{{h->s_has[0] ? h->mig_recv[0] : nullptr, h->s_has[1] ? h->mig_recv[1] : nullptr}, h->mig_cap};
  hipLaunchKernelGGL(k_mig_unpack, dim3(std::max(1, div_up(h->mig_cap, 256)), 2), dim3(256), 0, st, mr,
                     (const int*)h->mig_tot, h->fu.planes_alt, h->cold_alt, h->gid_alt, h->np, h->prm.n_particles);
  hipLaunchKernelGGL(k_mig_finish, dim3(nblk), dim3(256), 0, st, mr, (const int*)h->mig_tot, h->prm.n_particles,
                     h->d_n, h->orig, h->s_drift);
  GSMPM_LAUNCH_CHECK();
  std::swap(h->planes, h->fu.planes_alt);
  std::swap(h->cold, h->cold_alt);
  std::swap(h->gid, h->gid_alt);
  h->s_migrations += 1;
  return rebin_f(h, st);
}

// One step call's substeps: chunks up to the next migration, each followed by
// the migration (every rank runs the same chunks: same interval, same call
// sequence, so the exchanges pair up).  Host-free: captured whole with RCCL.
static int slab_body(gsmpm_mpm* h, float dt, int nsub, const uint32_t* bc, hipStream_t st,
                     const gsmpm_transport* xp) {
  if (h->s_rebal_pending && h->s_world > 1) {  // to the bounds slab_rebalance set (every rank alike)
    const int rc = slab_migrate(h, xp, st);
    if (rc) return rc;
  }
  int done = 0;
  while (done < nsub) {
    const int k = std::min(nsub - done, h->s_interval - (int)(h->s_since % h->s_interval));
    int rc = launch_substeps_f(h, dt, k, bc ? bc + done : nullptr, st, h->fbpar, h->fep, nullptr, nullptr, xp);
    if (rc) return rc;
    done += k;
    h->s_since += k;
    if (h->s_since % h->s_interval == 0 && h->s_world > 1) {
      rc = slab_migrate(h, xp, st);
      if (rc) return rc;
    }
  }
  return slab_records(h, xp, st);
}

}  // namespace gsmpm

extern "C" {

int gsmpm_rccl_unique_id(uint8_t id[128]) {
  GSMPM_REQUIRE(id, "gsmpm_rccl_unique_id: null argument");
  RcclApi& R = rccl();
  GSMPM_REQUIRE(R.ok, ("gsmpm_rccl_unique_id: " + R.why).c_str());
  RcclId u;
  GSMPM_RCCL(R.get_unique_id(&u));
  std::memcpy(id, u.internal, 128);
  return GSMPM_OK;
}

int gsmpm_rccl_comm_init(const uint8_t id[128], int32_t rank, int32_t world, void** comm) {
  GSMPM_REQUIRE(id && comm && world >= 1 && rank >= 0 && rank < world, "gsmpm_rccl_comm_init: bad argument");
  RcclApi& R = rccl();
  GSMPM_REQUIRE(R.ok, ("gsmpm_rccl_comm_init: " + R.why).c_str());
  RcclId u;
  std::memcpy(u.internal, id, 128);
  void* c = nullptr;
  GSMPM_RCCL(R.comm_init_rank(&c, world, u, rank));
  *comm = c;
  return GSMPM_OK;
}

int gsmpm_rccl_comm_destroy(void* comm) {
  if (!comm) return GSMPM_OK;
  RcclApi& R = rccl();
  GSMPM_REQUIRE(R.ok, ("gsmpm_rccl_comm_destroy: " + R.why).c_str());
  GSMPM_RCCL(R.comm_destroy(comm));
  return GSMPM_OK;
}

int gsmpm_mpm_slab_init(gsmpm_mpm* h, int32_t rank, int32_t world, int32_t lo, int32_t hi, int32_t margin,
                        int32_t interval) {
  GSMPM_REQUIRE(h, "gsmpm_mpm_slab_init: null handle");
  if (h->mixed) {
    set_error("gsmpm_mpm_slab_init: the handle holds per-particle materials, which slabs do not support "
              "(the migration payload does not carry the ids)");
    return GSMPM_ESTATE;
  }
  if (h->host_bc.n_drv > 0) {
    set_error("gsmpm_mpm_slab_init: the handle holds particle drivers (gsmpm_mpm_add_driver), which slabs do not "
              "support (migration moves rows between ranks and the selection does not follow)");
    return GSMPM_ESTATE;
  }
  if (h->n_ext > 0) {
    set_error("gsmpm_mpm_slab_init: the handle holds extended colliders (gsmpm_mpm_add_collider), which slabs do "
              "not support (their grid passes apply fixed cubes and plane colliders only)");
    return GSMPM_ESTATE;
  }
  GSMPM_REQUIRE(h->fused, "gsmpm_mpm_slab_init: slabs run the fused pipeline (no GSMPM_FLAG_PHASED / KEEP_GRID)");
  GSMPM_REQUIRE(!h->has_particles, "gsmpm_mpm_slab_init: call before setting particles");
  GSMPM_REQUIRE(!h->slab, "gsmpm_mpm_slab_init: already a slab");
  GSMPM_REQUIRE(world >= 1 && rank >= 0 && rank < world, "gsmpm_mpm_slab_init: bad rank / world");
  GSMPM_REQUIRE(margin >= 0 && interval >= 1, "gsmpm_mpm_slab_init: margin >= 0, interval >= 1");
  const int ng = h->g.ng, W = 2 * margin + 2;
  GSMPM_REQUIRE(0 <= lo && lo < hi && hi <= ng, "gsmpm_mpm_slab_init: need 0 <= lo < hi <= n_grid");
  GSMPM_REQUIRE(rank > 0 || lo == 0, "gsmpm_mpm_slab_init: rank 0 owns plane 0");
  GSMPM_REQUIRE(rank < world - 1 || hi == ng, "gsmpm_mpm_slab_init: the last rank owns the last plane");
  // the two windows of a rank must not overlap (no third rank reaches a window)
  GSMPM_REQUIRE(world == 1 || hi - lo >= W, "gsmpm_mpm_slab_init: slab thinner than 2 * margin + 2 planes");
  h->slab = true;
  h->s_rank = rank;
  h->s_world = world;
  h->s_lo = lo;
  h->s_hi = hi;
  h->s_margin = margin;
  h->s_interval = interval;
  h->rebin_interval = interval;  // bins are rebuilt at every migration anyway
  if (const char* sg = std::getenv("GSMPM_SLAB_GRAPH")) h->s_graph = sg[0] != '0';
  h->s_has[0] = rank > 0;
  h->s_has[1] = rank < world - 1;
  SlabWin sw{};
  sw.W = W;
  sw.a[0] = lo - margin;
  sw.a[1] = hi - margin;
  sw.on[0] = h->s_has[0];
  sw.on[1] = h->s_has[1];
  for (int w = 0; w < 2; ++w) {  // the whole cross-section until the first agreement
    sw.y0[w] = sw.z0[w] = 0;
    sw.ny[w] = sw.nz[w] = ng;
  }
  const size_t wcount = (size_t)W * ng * ng;
  for (int w = 0; w < 2; ++w) {
    if (!sw.on[w]) continue;
    GSMPM_HIP(alloc(h, &sw.part[w], wcount, kMemCommon, kFillZero));
    GSMPM_HIP(alloc(h, &h->s_recv[w], wcount, kMemCommon, kFillZero));
  }
  h->sw = sw;
  const size_t np = (size_t)h->np, nblk = (size_t)std::max(1, div_up(h->np, 256));
  GSMPM_HIP(alloc(h, &h->d_n, 1, kMemCommon, kFillZero));
  GSMPM_HIP(alloc(h, &h->s_drift, kSlabFlags, kMemCommon, kFillZero));
  if (!h->s_wdev) {
    GSMPM_HIP(alloc(h, &h->s_wdev, 1, kMemCommon));
    GSMPM_HIP(hipMemcpy(h->s_wdev, &h->s_weight, sizeof(float), hipMemcpyHostToDevice));
  }
  h->sw.oob = h->s_drift + SF_OOB;
  h->s_rect_set = false;
  h->s_synced = false;
  GSMPM_HIP(alloc(h, &h->gid, np, kMemCommon));
  GSMPM_HIP(alloc(h, &h->gid_alt, np, kMemCommon));
  GSMPM_HIP(alloc(h, &h->cold_alt, (size_t)NCOLD * np, kMemCommon, kFillZero));
  GSMPM_HIP(alloc(h, &h->mig_bcnt, 3 * nblk, kMemCommon));
  GSMPM_HIP(alloc(h, &h->mig_boff, 3 * nblk, kMemCommon));
  GSMPM_HIP(alloc(h, &h->mig_tot, 8, kMemCommon));
  GSMPM_REQUIRE(ng <= kRecMaxNg, "gsmpm_mpm_slab_init: n_grid above 4096");
  GSMPM_HIP(alloc(h, &h->s_rec, rec_ints_of(ng) * (size_t)world, kMemCommon));
  GSMPM_HIP(alloc_host(h, &h->s_rec_host, rec_ints_of(ng) * (size_t)world));
  GSMPM_HIP(hipStreamCreateWithFlags(&h->s_comm, hipStreamNonBlocking));
  GSMPM_HIP(hipEventCreateWithFlags(&h->s_ev_pack, hipEventDisableTiming));
  GSMPM_HIP(hipEventCreateWithFlags(&h->s_ev_x, hipEventDisableTiming));
  drop_graphs(h);
  return GSMPM_OK;
}

int gsmpm_mpm_slab_set_particles(gsmpm_mpm* h, int32_t n, const float* x, const float* cov6, const float* vol,
                                 const float* v, const int32_t* gid, void* stream) {
  GSMPM_REQUIRE(h && (gid || n == 0), "gsmpm_mpm_slab_set_particles: null argument");
  GSMPM_REQUIRE(h->slab, "gsmpm_mpm_slab_set_particles: call gsmpm_mpm_slab_init first");
  GSMPM_REQUIRE(n >= 0 && n <= h->prm.n_particles, "gsmpm_mpm_slab_set_particles: n exceeds the slab's capacity");
  hipStream_t st = (hipStream_t)stream;
  h->n = n;
  h->s_rect_set = false;  // new particles: records and window rects are agreed again before the next substep
  h->s_synced = false;
  GSMPM_HIP(hipMemsetAsync(h->s_drift, 0, kSlabFlags * sizeof(int), st));  // and the flags clear
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(64), 0, st, h->d_n, n);
  GSMPM_LAUNCH_CHECK();
  if (n == 0) {
    h->has_particles = true;
    return GSMPM_OK;
  }
  int rc = gsmpm_mpm_set_particles(h, x, cov6, vol, v, stream);
  if (rc) return rc;
  GSMPM_HIP(hipMemcpyAsync(h->gid, gid, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
  GSMPM_HIP(hipStreamSynchronize(st));
  return GSMPM_OK;
}

int gsmpm_mpm_slab_step(gsmpm_mpm* h, float dt, int32_t nsub, const uint32_t* bc, const gsmpm_transport* xp,
                        void* stream) {
  GSMPM_REQUIRE(h, "gsmpm_mpm_slab_step: null handle");
  GSMPM_REQUIRE(h->slab, "gsmpm_mpm_slab_step: not a slab (gsmpm_mpm_slab_init)");
  GSMPM_REQUIRE(nsub >= 0, "gsmpm_mpm_slab_step: n_substeps < 0");
  if (!h->has_particles) {
    set_error("gsmpm_mpm_slab_step: particles not set");
    return GSMPM_ESTATE;
  }
  if (xp) GSMPM_REQUIRE(xp->world == h->s_world && xp->rank == h->s_rank,
                        "gsmpm_mpm_slab_step: transport rank / world differ from the slab's");
  if (h->s_world > 1)
    GSMPM_REQUIRE(xp && xp->kind != GSMPM_XPORT_NONE, "slab exchange: this slab has neighbours but no transport");
  if (nsub == 0) return GSMPM_OK;
  hipStream_t st = (hipStream_t)stream;
  h->s_calls += 1;
  int rc = GSMPM_OK;
  if (!h->s_synced) {
    rc = slab_records(h, xp, st);
    if (!rc) rc = slab_check(h, st);
  }
  if (!rc) rc = slab_rect_update(h, dt, nsub, bc, st);
  if (rc) return rc;
  // RCCL: the whole call (window exchanges and migrations included) replays as
  // one captured graph
  const bool graph = xp && xp->kind == GSMPM_XPORT_RCCL && nsub >= 2 && h->s_graph &&
                     !(h->prm.flags & GSMPM_FLAG_NO_GRAPH);
  rc = graph ? graph_substeps(h, dt, nsub, bc, st, xp) : slab_body(h, dt, nsub, bc, st, xp);
  if (rc) return rc;
  if (h->s_rebal_pending) {
    h->s_rebal_pending = false;
    h->s_rebalances += 1;
  }
  return slab_check(h, st);
}

int gsmpm_mpm_slab_set_weight(gsmpm_mpm* h, float weight) {
  GSMPM_REQUIRE(h && std::isfinite(weight) && weight > 0.f, "gsmpm_mpm_slab_set_weight: weight must be > 0");
  GSMPM_REQUIRE(h->slab && h->s_wdev, "gsmpm_mpm_slab_set_weight: not a slab (gsmpm_mpm_slab_init)");
  GSMPM_HIP(hipMemcpy(h->s_wdev, &weight, sizeof(float), hipMemcpyHostToDevice));  // read by the next record
  h->s_weight = weight;
  return GSMPM_OK;
}

int gsmpm_mpm_slab_set_rebalance(gsmpm_mpm* h, int32_t on, float tolerance) {
  GSMPM_REQUIRE(h && tolerance >= 0.f, "gsmpm_mpm_slab_set_rebalance: bad argument");
  h->s_rebal_on = on != 0;
  h->s_rebal_tol = tolerance;
  return GSMPM_OK;
}

int gsmpm_mpm_slab_bounds(gsmpm_mpm* h, int32_t* out, int32_t n, int64_t* rebalances) {
  GSMPM_REQUIRE(h && out, "gsmpm_mpm_slab_bounds: null argument");
  GSMPM_REQUIRE(h->slab, "gsmpm_mpm_slab_bounds: not a slab");
  GSMPM_REQUIRE(n == h->s_world + 1, "gsmpm_mpm_slab_bounds: n must be world + 1");
  if ((int)h->s_bounds.size() != h->s_world + 1) {  // before the first record exchange: this rank's own
    for (int i = 0; i < n; ++i) out[i] = -1;
    out[h->s_rank] = h->s_lo;
    out[h->s_rank + 1] = h->s_hi;
  } else {
    for (int i = 0; i < n; ++i) out[i] = h->s_bounds[i];
  }
  if (rebalances) *rebalances = h->s_rebalances;
  return GSMPM_OK;
}

int gsmpm_mpm_count(gsmpm_mpm* h) {
  GSMPM_REQUIRE(h, "gsmpm_mpm_count: null handle");
  return h->n;
}

int gsmpm_mpm_get_gid(gsmpm_mpm* h, int32_t* out, void* stream) {
  GSMPM_REQUIRE(h && out, "gsmpm_mpm_get_gid: null argument");
  GSMPM_REQUIRE(h->slab, "gsmpm_mpm_get_gid: not a slab");
  if (h->n > 0)
    GSMPM_HIP(hipMemcpyAsync(out, h->gid, sizeof(int) * (size_t)h->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GSMPM_OK;
}

int gsmpm_mpm_slab_rects(gsmpm_mpm* h, int32_t out8[8]) {
  GSMPM_REQUIRE(h && out8, "gsmpm_mpm_slab_rects: null argument");
  GSMPM_REQUIRE(h->slab, "gsmpm_mpm_slab_rects: not a slab");
  for (int w = 0; w < 2; ++w) {
    out8[4 * w + 0] = h->sw.y0[w];
    out8[4 * w + 1] = h->sw.on[w] ? h->sw.ny[w] : 0;
    out8[4 * w + 2] = h->sw.z0[w];
    out8[4 * w + 3] = h->sw.on[w] ? h->sw.nz[w] : 0;
  }
  return GSMPM_OK;
}

int gsmpm_mpm_slab_stats(gsmpm_mpm* h, int64_t out8[12]) {
  GSMPM_REQUIRE(h && out8, "gsmpm_mpm_slab_stats: null argument");
  out8[8] = h->s_deferred;
  out8[9] = h->mig_cap;
  out8[10] = h->s_host_syncs;
  out8[11] = h->s_calls;
  out8[0] = h->s_migrations;
  out8[1] = h->s_migrated;
  out8[2] = h->s_lo;
  out8[3] = h->s_hi;
  out8[4] = h->s_margin;
  out8[5] = h->s_interval;
  out8[6] = h->sw.W;
  out8[7] = h->prm.n_particles;
  return GSMPM_OK;
}

}  // extern "C"
