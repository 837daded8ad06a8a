#!/usr/bin/env python3
"""bench.py -- PhysGaussian simulate+render loop (lego.json, 128^3) on MI355X.

One bench *step* = one lego frame exactly as main.py runs it (main.py:303-326):
steps_per_frame (= 100) MPM substeps, postprocess (cov/R), fused
grid2world + render-space transform, and the rasterizer forward of the frame
(800x800, SH degree 3).  PNG encoding is host I/O and not timed.

Workload (BASELINE.json configs[1]): lego.json, 100k synthetic lego-like
Gaussians (the lego PLY in the reference is a git-LFS pointer),
n_grid 128 (--n_grid override), jelly as written.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, runs W untimed warm-up steps, times K steps, and prints
the headline line (value, ms_per_step, the configuration).  --dump-outputs DIR
then also writes the last timed step's outputs (render-space means and
covariances, image, radii) as DIR/<name>.npy; the scene is seeded, so two
builds run with the same arguments can be compared array for array.  --full
adds every measurement that takes GPU (or CPU) runs of its own: the sim /
render breakdown, the per-kernel and roofline figures, configs B' / C / D / E
(other_configs), the CPU baseline, and for N > 1 the side measurements
(multi_gpu); --no-cpu-baseline, --no-extra-configs, --no-multi-configs and
--multi-configs trim what --full runs.

Multi-GPU (torch.distributed.run, one rank per GPU), two modes for the
headline line:
* default (--multi dp) -- every rank simulates and renders its own lego scene
  (synthetic seed = rank): independent objects, no collective in the data
  path; value = all ranks' particle-substeps / the slowest rank's time
  ("scaling": "weak").  One lego scene is latency-bound on one GPU (SURVEY
  8(e): "report honestly"): sharding it cannot beat one GPU per substep, so
  the job's throughput at N GPUs is N scenes.
* --multi slab -- strong scaling of ONE lego scene sharded by spatial slab
  (gsmpm.dist.SlabDomain, csrc/slab.h): every substep each pair of
  neighbouring ranks swaps the partial sums of the grid planes around their
  shared bound over RCCL (the pairwise all-reduce of boundary grid nodes),
  particles migrate between slabs every 10 substeps; the frame's means/covs
  are gathered to rank 0, which renders it.  value = scene particles x
  substeps / time.
Either way an N > 1 line under --full also carries `multi_gpu`: north_star's slab
sharding measured on lego and on config D (bicycle 1M, 256^3) with the
render-aware re-cut (rank 0 renders the gathered frame and takes the
particle share sim / (sim + render)), per-rank sim ms, rank-0 render and
gather ms, and lego's sim / render split (rank 1 simulates, rank 0 renders
frame f - 1 from a snapshot sent over RCCL).  Timing is barrier + max over
ranks.

Prints ONE JSON line (rank 0).  value = particle-substeps/s over all ranks.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "gaussian-splatting-mpm_amd")
sys.path.insert(0, PKG)

METRIC = "MPM substeps/sec (and particles·steps/sec) + rendered fps, lego 128³ grid"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--n_grid", type=int, default=128)
    ap.add_argument("--config", default="lego.json")
    ap.add_argument("--material", default=None, help="override (e.g. metal) -- not the headline config")
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every side measurement (the sim / render breakdown, the "
                         "per-kernel and roofline figures, configs B' / C / D / E, the CPU baseline; N > 1: "
                         "multi_gpu) and add their fields to the JSON line; off: set up, warm up, time the steps, "
                         "print the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed (the frame's render-space "
                         "means and covariances, its image and radii) as DIR/<name>.npy (float32, at most 64 MB in "
                         "all: a fixed seeded sample of a larger array)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="--full: skip the driver-timed config C (metal) / D (bicycle 1M, 256^3) side runs")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--multi", choices=("dp", "slab"), default="slab",
                    help="N > 1 headline: slab = one lego scene sharded by spatial slab over RCCL (default, "
                         "north_star's design, strong scaling); dp = independent lego scenes per rank (weak scaling)")
    ap.add_argument("--dp", action="store_const", const="dp", dest="multi", help="= --multi dp")
    ap.add_argument("--slab", action="store_const", const="slab", dest="multi", help="= --multi slab")
    ap.add_argument("--no-multi-configs", action="store_true",
                    help="N > 1: skip the side measurements (multi_gpu)")
    ap.add_argument("--multi-configs", default=None,
                    help="N > 1: which side measurements multi_gpu holds: bicycle (config D through the slabs), "
                         "dp (one lego scene per rank), lego (the lego slab form, when the headline is dp), split "
                         "(lego's sim / render split); default: bicycle,dp under the slab headline, "
                         "bicycle,lego under --dp")
    ap.add_argument("--rebin", type=int, default=0, help="fused pipeline: substeps between re-binnings (0: library default)")
    ap.add_argument("--render-overlap", type=int, default=int(os.environ.get("GSMPM_BENCH_RENDER_OVERLAP", "1")),
                    help="1: frame f-1 renders on a second stream while frame f simulates; 0: each frame renders "
                         "right after its simulation on the simulator's stream (main.py's order)")
    ap.add_argument("--render-delay-us", type=float, default=float(os.environ.get("GSMPM_BENCH_RENDER_DELAY_US", "0")),
                    help="overlapped render: the render stream idles this long (a one-wave spin kernel) after the "
                         "previous frame's snapshot before rendering it, so the render meets the next frame's "
                         "substeps instead of its first launches")
    ap.add_argument("--render-first", type=int, default=int(os.environ.get("GSMPM_BENCH_RENDER_FIRST", "0")),
                    help="overlapped render: 1 = frame f - 1 is rendered (its launches submitted) BEFORE frame f's "
                         "graph is launched, so the render's work is already queued when the graph starts; 0 = "
                         "after frame f's graph, postprocess and snapshot")
    ap.add_argument("--render-thread", type=int, default=int(os.environ.get("GSMPM_BENCH_RENDER_THREAD", "1")),
                    help="overlapped render: 1 = a host thread of its own issues the renders (its pair-count wait "
                         "no longer holds back the launch of the next frame's graph); 0 = the frame loop's thread")
    ap.add_argument("--render-async", type=int, default=int(os.environ.get("GSMPM_BENCH_RENDER_ASYNC", "0")),
                    help="1: frames render through gsmpm_raster_forward_async (the pair count stays on the device: "
                         "no host wait, no render thread; a frame whose counts flag an overflow is rendered again "
                         "by the synchronous form inside the timed region); 0 (default: measured faster with the render "
                         "thread, DESIGN.md §6): the synchronous form")
    ap.add_argument("--render-cu-layout", default=os.environ.get("GSMPM_BENCH_RENDER_CU_LAYOUT", "spread"),
                    choices=["spread", "low", "xmajor"],
                    help="which CU-mask bits --render-cus gives the render: spread = evenly spaced bits (round 4); "
                         "low = bits 0 .. N-1; xmajor = the first N/8 bits of each 32-bit word (one word per XCD "
                         "if the mask is XCD-major).  k_fused fills one round only if every XCD keeps enough CUs, "
                         "so the render's CUs must be spread over the XCDs, whichever way the bits map")
    ap.add_argument("--render-cus", type=int, default=int(os.environ.get("GSMPM_BENCH_RENDER_CUS", "0")),
                    help="N > 0: the overlapped render gets N of the device's CUs (every (CUs / N)-th CU-mask bit) "
                         "and the simulator the rest, on CU-masked streams (hipExtStreamCreateWithCUMask), so the "
                         "render never takes the CU slots of the simulator's one-round launches; 0: both streams "
                         "on every CU")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch check only: start the ranks, form the process group, print the JSON line's "
                         "rank bookkeeping (n_gpus, parallelism) with value null; no GPU work")
    return ap.parse_args()


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every array of `arrays` (name -> device tensor) as
    path/<name>.npy in float32.  The arrays share DUMP_BUDGET_BYTES equally;
    one above its share is written as a fixed sample of its flattened elements
    (indices drawn once from a generator seeded with 0, sorted), so two runs
    with the same arguments write the same elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BUDGET_BYTES // 4 // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().cpu().numpy().astype(np.float32)
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).integers(0, a.size, size=cap))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), a)


def launch_ranks(n):
    """--gpus N > 1 without a launcher around us: start N rank processes with
    torch.distributed.run (one per GPU, rendezvous on 127.0.0.1) and return
    their exit code.  Runs before anything touches the GPU in this process,
    and starts the ranks as a child (never exec)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def cu_split_streams(dev, n_render, layout="spread"):
    """Two streams on disjoint CU masks (hipExtStreamCreateWithCUMask through the
    HIP runtime torch already loaded): the simulator's (every CU but the
    render's) and the render's: exactly n_render evenly spaced CUs.  Returns
    (sim stream, render stream, render CU count)."""
    import ctypes
    import torch
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_render = max(1, min(int(n_render), ncu - 1))
    if layout == "low":
        rbits = set(range(n_render))
    elif layout == "xmajor":
        per = max(1, n_render // 8)
        rbits = {32 * w + j for w in range((ncu + 31) // 32) for j in range(per) if 32 * w + j < ncu}
        rbits = set(sorted(rbits)[:n_render])
    else:
        rbits = {min(ncu - 1, round((i + 0.5) * ncu / n_render)) for i in range(n_render)}
    sbits = set(range(ncu)) - rbits
    assert len(rbits) == n_render and sbits, (ncu, n_render)
    words = (ncu + 31) // 32
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipExtStreamCreateWithCUMask.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                                 ctypes.POINTER(ctypes.c_uint32)]

    def make(bits):
        arr = (ctypes.c_uint32 * words)()
        for i in bits:
            arr[i // 32] |= 1 << (i % 32)
        h = ctypes.c_void_p()
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(h), words, arr)
        if rc != 0:
            raise RuntimeError(f"hipExtStreamCreateWithCUMask failed ({rc})")
        return torch.cuda.ExternalStream(h.value, device=dev)

    return make(sbits), make(rbits), len(rbits)


def resolve_world(args):
    """(rank, world, local_rank) of this process, checked against --gpus: the
    rank count comes from the flag, and a launcher that started a different
    number of ranks is an error -- never a silent one-rank run."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} ranks were started")
    return int(os.environ.get("RANK", "0")), world, int(os.environ.get("LOCAL_RANK", "0"))


# models/bicycle/cameras.json record 0 of the reference (intrinsics only: main.py's
# orbit camera replaces the pose, main.py:84-106) -- data, so the bench needs no
# reference files on the GPU box
BICYCLE_CAM0 = {"width": 4946, "height": 3286, "fx": 4649.505977743847, "fy": 4627.300372546341,
                "position": [0.0, 0.0, 0.0], "rotation": [[1, 0, 0], [0, 1, 0], [0, 0, 1]]}


def build_scene(args, dev, rank=0):
    import torch
    from arguments import MPMParams, ModelParams, RenderParams
    from argparse import ArgumentParser
    from gaussian_splatting.scene import GaussianModel
    from internel_filling.filling import get_particle_volume
    from utils.transform_utils import get_center_view_worldspace_and_observant_coordinate, world2grid
    import main as drv

    with open(os.path.join(PKG, "configs", args.config)) as f:
        cfg = json.load(f)
    parser = ArgumentParser()
    mp, sp, rp = ModelParams(parser, cfg["model"]), MPMParams(parser, cfg["mpm"]), RenderParams(parser, cfg["render"])
    cli = ["--n_grid", str(args.n_grid)] + (["--material", args.material] if args.material else [])
    a = parser.parse_args(cli)
    margs, sargs, rargs = mp.extract(a), sp.extract(a), rp.extract(a)
    # lego-like box for lego*; config D (bicycle) fills its sim_area [0,1]^3 as U([0.05, 0.95]^3)
    box = ((0.05,) * 3, (0.95,) * 3) if args.config.startswith("bicycle") else \
        ((-0.65, -0.65, -0.55), (0.65, 0.65, 0.55))
    g = GaussianModel(3, device=dev).init_synthetic(args.particles, seed=rank, box=box)
    bound = torch.tensor(sargs.sim_area, device=dev)
    xyz = g.get_xyz
    mask = torch.logical_and((xyz <= bound[1]).all(1), (xyz >= bound[0]).all(1))
    means = xyz[mask]
    covs = g.get_covariance()[mask]
    xg, c, s = world2grid(means, sargs)
    vols = get_particle_volume(xg, sargs)
    center_w, obs = get_center_view_worldspace_and_observant_coordinate(
        torch.tensor([[0.5, 0.5, 0.5]], device=dev), torch.tensor([[0, 0, 1]], device=dev), [], s, c)
    if args.config.startswith("bicycle"):
        cam0 = drv.camera_from_info(BICYCLE_CAM0)
    else:
        margs.model_path = "/nonexistent"  # -> lego camera 0 record (800x800, fx 1111.11)
        cam0 = drv.load_cameras(margs)[0]
    cam = drv.modify_cam(cam0, center_w, obs, device=dev)
    cam.toCuda(dev)
    return dict(g=g, mask=mask, xg=xg, covs=covs * (s * s), vols=vols, c=c, s=s, cam=cam, sargs=sargs, rargs=rargs)


def make_sim(scene, dev, use_graph=True, slab=None):
    """The scene's simulator and its BC specs.  slab = (rank, world, transport):
    this rank's gsmpm.dist.SlabDomain of the whole scene instead."""
    from gsmpm.bc import BCSpec
    from gsmpm.sim import Simulator
    sa = scene["sargs"]
    n = scene["xg"].shape[0]
    kw = dict(n_grid=sa.n_grid, grid_extent=sa.grid_extent, material=sa.material, E=sa.E, nu=sa.nu,
              density=sa.density, gravity=sa.gravity, jelly_fcr=sa.jelly_fcr, device=dev)
    if slab is not None:
        from gsmpm.dist import SlabDomain
        rank, world, xp = slab
        sim = SlabDomain(scene["xg"], scene["covs"], scene["vols"], rank=rank, world=world, transport=xp,
                         margin=2, interval=10, **kw)
    else:
        sim = Simulator(n, use_graph=use_graph, **kw)
        sim.set_particles(scene["xg"], scene["covs"], scene["vols"])
    specs = []
    for d in sa.boundary_conditions:
        end = d["start_time"] + sa.substep_dt * d["num_dt"]
        if d["type"] == "fixed_cube":
            specs.append(BCSpec("fixed_cube", sim.add_fixed_cube(d["center"], d["size"]), d["start_time"], end))
        elif d["type"] == "impulse":
            specs.append(BCSpec("impulse", sim.add_impulse(d["center"], d["size"], d["force"], sa.substep_dt),
                                d["start_time"], end))
    specs.append(BCSpec("collider", sim.add_plane_collider((0.0, 0.0, 0.4), (0.0, 0.0, 1.0), 0.0)))
    return sim, specs


def algorithmic_bytes_live(n, live_nodes, material, fold=False):
    """The same split with the grid counted as the nodes the kernels own: the
    touched tiles' nodes (live_nodes = touched tiles x 448 of the fused
    pipeline's 8x8x7 tiles) instead of the dense n^3 the reference sweeps --
    the bytes a sparse implementation must move at least, so the fraction it
    gives is a bandwidth fraction (<= 1).  fold: k_fused also does the grid
    update of the substep before (fused.h FOLD), so its launch carries the
    whole substep's 208 N + 56 B per live node."""
    plastic = 8 * n if material in ("metal",) else 0
    return {"k_fused": 208 * n + (56 if fold else 28) * live_nodes + plastic, "k_grid_f": 28 * live_nodes}


# translation units whose kernels are not the simulator's (the rasterizer, the
# differentiable MPM): their edits do not change k_fused / k_grid_f
NON_SIM_SOURCES = ("raster.hip", "fit.hip", "dsort.h", "scan.h", "lsd.h")  # rasterizer / fit units, the one-time sorts


def source_sha():
    """Hash of the simulator's kernel sources (csrc/*.hip, *.h, *.inc but
    NON_SIM_SOURCES): a committed PMC traffic figure of k_fused / k_grid_f is
    only reported while the kernels it was measured on are the ones built."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")) +
                    glob.glob(os.path.join(PKG, "csrc", "*.inc"))):
        if os.path.basename(f) in NON_SIM_SOURCES:
            continue
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def algorithmic_bytes(n, n_grid, material):
    """Per-launch algorithmic bytes: SURVEY.md §8(d)'s per-substep figure
    B_sub = 208 N + 56 n^3 (+ 8 N for plastic materials), split over the kernel
    that does each part of the work (Roofline):
      k_p2g  reads x v C F m vol mu lam (112 B/particle) and writes m + mv
             of every node (16 B/node, dense n^3 as the reference sweeps it);
      k_grid reads m + mv (16) and writes v (12) per node;
      k_g2p  reads v per node (12) and writes x v C F (96 B/particle).
    The three sum to B_sub exactly."""
    nodes = n_grid ** 3
    plastic = 8 * n if material in ("metal",) else 0
    return {"k_p2g": 112 * n + 16 * nodes + plastic, "k_grid": 28 * nodes, "k_g2p": 96 * n + 12 * nodes,
            # fused pipeline: one launch does G2P of substep s and P2G of s + 1
            "k_fused": 208 * n + 28 * nodes + plastic, "k_grid_f": 28 * nodes}


def measured_traffic(kernel, workload):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC
    summaries (profiles/traffic*.json, written by tools/traffic.py from
    separate FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE doubled per the gfx950
    note in MI355X_MICROARCH.md) measured on this same workload AND on the
    kernel sources built now (source_sha), else None."""
    import glob
    sha = source_sha()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic*.json"))):
        try:
            with open(path) as f:
                t = json.load(f)
            if t.get("workload") == workload and t.get("source_sha") == sha:
                return t["kernels"][kernel]["bytes_per_launch"]
        except (OSError, KeyError, ValueError):
            continue
    return None


def kernel_roofline(n, n_grid, material, live_nodes, us_per_launch, workload, launches=None, spf=100, fold=False):
    """Per-kernel roofline figures of the fused pipeline, on the live-byte
    basis: `bytes` = the bytes the kernel must move at least (208 N particle
    planes (+ 8 N plastic) + 28 B per live node for k_fused -- 56 when it
    folds the grid update in --, 28 B per live node for k_grid_f; live nodes =
    touched tiles x 448), `frac` = bytes / launch time / HBM peak (<= 1 by
    construction), and beside it the PMC-measured HBM traffic (when it
    matches the workload and sources) with its fraction.  The SURVEY 8(d)
    dense n^3 figure is what the reference sweeps, not what these kernels
    move, so it is given as bytes only (`dense_contract_bytes`), never as a
    rate or fraction.  `substep` = one substep's live bytes (208 N + 56 B per
    live node) over the time both kernels spend per substep (launches x
    per-launch time / substeps): the whole-substep fraction."""
    dense = algorithmic_bytes(n, n_grid, material)
    live = algorithmic_bytes_live(n, live_nodes, material, fold)
    launches = launches or {"k_fused": spf + 1, "k_grid_f": spf}
    out = {}
    for k, us in us_per_launch.items():
        if k not in live or not us:
            continue
        t = us * 1e-6
        tr = measured_traffic(k, workload)
        out[k] = {"us_per_launch": round(us, 2), "launches_per_frame": launches.get(k), "bytes": live[k],
                  "achieved_GBps": round(live[k] / t / 1e9, 1),
                  "frac": round(live[k] / t / 1e9 / HBM_PEAK_GBS, 4),
                  "traffic": tr, "traffic_frac": None if tr is None else round(tr / t / 1e9 / HBM_PEAK_GBS, 4),
                  "dense_contract_bytes": dense[k]}
    if all(k in out for k in ("k_fused", "k_grid_f")):
        b = algorithmic_bytes_live(n, live_nodes, material, True)["k_fused"]
        t = sum(us_per_launch[k] * launches[k] for k in ("k_fused", "k_grid_f")) / spf * 1e-6
        out["substep"] = {"kernels": ["k_fused", "k_grid_f"], "bytes": b,
                          "us": round(t * 1e6, 2), "achieved_GBps": round(b / t / 1e9, 1),
                          "frac": round(b / t / 1e9 / HBM_PEAK_GBS, 4)}
    return out


def cpu_baseline(scene, args, budget_s):
    """The CPU restatement (oracle/mpm_oracle.c built with OpenMP at -O3
    -ffast-math for AVX2/FMA: liboracle_fast.so, as Taichi's arch=cpu compiles
    the reference's kernels) on a bounded sample of the same workload -- as
    many lego substeps at N particles / n^3 as fit in ~budget_s -- timed on
    this host's cores (OMP_NUM_THREADS, else all cores in the affinity mask)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle as O  # cpu_baseline leg only
    sa = scene["sargs"]
    x = scene["xg"].cpu().numpy()
    os.environ.setdefault("OMP_NUM_THREADS", str(len(os.sched_getaffinity(0))))
    sim = O.OracleMPM(x, scene["covs"].cpu().numpy(), scene["vols"].cpu().numpy(), n_grid=sa.n_grid,
                      grid_extent=sa.grid_extent, material=sa.material, E=sa.E, nu=sa.nu, density=sa.density,
                      gravity=sa.gravity, jelly_quirk=not sa.jelly_fcr, threaded="fast")
    threads = int(O.lib("fast").om_threads())
    ops = []
    for d in sa.boundary_conditions:
        if d["type"] == "fixed_cube":
            sim.add_fixed_box(d["center"], d["size"])
            ops.append((d["start_time"], d["start_time"] + sa.substep_dt * d["num_dt"]))
    sim.add_collider([0.0, 0.0, 0.4], [0.0, 0.0, 1.0])
    ops.append(None)
    t, n_done = 0.0, 0
    t0 = time.perf_counter()
    while True:
        oa = [1 if o is None else int(o[0] <= t < o[1]) for o in ops]
        sim.substep(sa.substep_dt, None, oa)
        t += sa.substep_dt
        n_done += 1
        el = time.perf_counter() - t0
        if el > budget_s or n_done >= 2000:
            break
    sub_s = n_done / el
    # the frame's render on the CPU restatement of the rasterizer (oracle/raster_oracle.c, the same OpenMP
    # -O3 -ffast-math build and threads as the simulation: tiles sorted and blended in parallel), so the
    # baseline times the same work as the GPU value: steps_per_frame substeps + one 800x800 SH3 render
    render_s = None
    if not args.no_render:
        g, mask, cam = scene["g"], scene["mask"], scene["cam"]
        c = scene["c"].reshape(-1).cpu().numpy().astype(np.float32)
        means = (c + (g.get_xyz[mask].cpu().numpy() - np.float32(1.0))).astype(np.float32)  # main.py:139-146 (F7)
        covs = g.get_covariance()[mask].cpu().numpy()
        opa = g.get_opacity[mask].reshape(-1).cpu().numpy()
        shs = g.get_features[mask].cpu().numpy()
        t0 = time.perf_counter()
        O.raster_forward(means, opa, cam.view_mat.cpu().numpy(), cam.full_proj_mat.cpu().numpy(),
                         np.asarray(cam.cam_center.cpu().numpy(), np.float32), np.zeros(3, np.float32),
                         cam.width, cam.height, math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5), shs=shs,
                         sh_degree=3, cov3D_precomp=covs, threaded="fast")
        render_s = time.perf_counter() - t0
    spf = sa.steps_per_frame
    frame_s = spf / sub_s + (render_s or 0.0)
    return {"value": x.shape[0] * spf / frame_s, "unit": "particle-substeps/s", "cores": threads, "kind": "port",
            "sample": f"first {n_done} lego substeps of the same workload ({x.shape[0]} particles, {sa.n_grid}^3, "
                      f"same BCs), C restatement oracle/mpm_oracle.c, OpenMP ({threads} threads) -O3 -ffast-math "
                      f"-march=x86-64-v3, {el:.1f}s"
                      + ("" if render_s is None else
                         f"; plus one {cam.width}x{cam.height} SH3 render of the scene on oracle/raster_oracle.c "
                         f"(OpenMP, {threads} threads), {render_s:.2f}s")
                      + f"; value = particles x {spf} / (the frame's {spf} substeps at the measured rate + the "
                        "render): the same work per frame as the GPU value",
            "substeps_per_s": sub_s, "sim_only_particle_substeps_per_s": x.shape[0] * sub_s,
            "render_s_per_frame": render_s}


def other_configs(args, dev, frames=3, rank=0, world=1, xp=None, sync=None):
    """BASELINE configs[2] (lego-fracture --material metal, 100k, 128^3: the
    stress-bearing return-map path) and configs[3] (bicycle 1M, 256^3,
    rendered at the bicycle camera's 4946x3286): timed in the same run as the
    headline, sim and render separately.  With a transport (N > 1) both are
    sharded by slab over the N GPUs, timed barrier-to-barrier (max over ranks),
    and rank 0 renders the gathered frame."""
    import copy
    import torch
    from gsmpm import raster
    from gsmpm.bc import substep_masks
    slab = xp is not None
    sync = sync or torch.cuda.synchronize
    res = {}
    # B': the real lego's Gaussian count (models/lego/point_cloud/iteration_7000, 240,549: SURVEY F6)
    for key, cfg, mat, n, ng in (("B_prime_lego_240549", "lego.json", None, 240_549, 128),
                                 ("C_lego_fracture_metal", "lego-fracture.json", "metal", 100_000, 128),
                                 ("D_bicycle", "bicycle.json", None, 1_000_000, 256)):
        a = copy.copy(args)
        a.config, a.material, a.particles, a.n_grid = cfg, mat, n, ng
        sc = build_scene(a, dev)
        sim, specs = make_sim(sc, dev, slab=(rank, world, xp) if slab else None)
        sa = sc["sargs"]
        dt, spf, t = sa.substep_dt, sa.steps_per_frame, 0.0
        masks, t = substep_masks(specs, t, dt, spf)
        sim.step(dt, masks)  # warm-up frame (graph capture)
        sync()
        t0 = time.perf_counter()
        for _ in range(frames):
            masks, t = substep_masks(specs, t, dt, spf)
            sim.step(dt, masks)
        sync()
        sim_ms = (time.perf_counter() - t0) / frames * 1e3
        if slab:
            import torch.distributed as dist
            tt = torch.tensor([sim_ms], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            sim_ms = float(tt.item())
        nsim = sc["xg"].shape[0]
        r = {"config": cfg, "material": sa.material, "particles": nsim, "n_grid": sa.n_grid,
             "parallelism": f"slab{world}" if slab else "single",
             "sim_ms_per_frame": round(sim_ms, 4), "sim_substeps_per_s": round(spf / (sim_ms * 1e-3), 1),
             "sim_particle_substeps_per_s": nsim * spf / (sim_ms * 1e-3)}
        if not slab:
            masks, t = substep_masks(specs, t, dt, spf)
            prof = sim.profile(dt, masks)
            r["k_fused_us_per_launch"] = round(prof[0] / (spf + 1) * 1e3, 2)
            ngrid = int(prof[3]) if prof[3] > 0 else spf  # k_grid_f launches (folded: one per re-binning)
            r["k_grid_f_launches_per_frame"] = ngrid
            r["k_grid_f_us_per_launch"] = round(prof[1] / ngrid * 1e3, 2)
            live = sim.debug_stats()["touched_tiles"] * 448
            r["live_nodes"] = live
            r["folded"] = sim.folded
            r["roofline"] = kernel_roofline(
                nsim, sa.n_grid, sa.material, live,
                {"k_fused": r["k_fused_us_per_launch"], "k_grid_f": r["k_grid_f_us_per_launch"]},
                {"config": cfg, "particles": n, "n_grid": ng, "material": sa.material},
                launches={"k_fused": spf + 1, "k_grid_f": ngrid}, spf=spf, fold=sim.folded)
        else:
            st = sim.stats()
            r["rank0_slab_planes"] = [st["lo"], st["hi"]]
            r["rank0_window_rects"] = sim.engine.slab_rects()  # exchanged (y0, ny, z0, nz) per window
        sim.postprocess()
        cam, g, mask = sc["cam"], sc["g"], sc["mask"]
        w_args = (float(sc["s"]), [float(v) for v in sc["c"].reshape(-1).tolist()])
        means_r, covs_r = sim.gather_world(*w_args, render_space=True) if slab else \
            sim.world_outputs(*w_args, render_space=True)
        if means_r is not None:
            feats, opac = g.get_features[mask].contiguous(), g.get_opacity[mask].reshape(-1).contiguous()
            tx, ty = math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5)
            bg = torch.zeros(3, device=dev)
            rf = lambda: raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                        cam.height, cam.width, tx, ty, sh_degree=3, shs=feats, cov3D_precomp=covs_r)
            K, _, _ = rf()
            torch.cuda.synchronize()
            r0 = time.perf_counter()
            for _ in range(frames):
                rf()
            torch.cuda.synchronize()
            r["render"] = f"{cam.width}x{cam.height} SH3"
            r["render_ms"] = round((time.perf_counter() - r0) / frames * 1e3, 3)
            r["num_rendered"] = K
            del feats, opac
        res[key] = r
        del sim, sc, means_r, covs_r
        torch.cuda.empty_cache()
    if not slab:
        res["E_extra_fit"] = config_e(dev)
    return res


def slab_exchange_bytes(sim):
    """Bytes this rank sends per substep in the grid-window exchange (the same
    count arrives): float4 (m v, m) partials over the window planes x the
    exchanged yz rect of each window that has a neighbour (slab_host.inc,
    slab_grid_phase)."""
    st = sim.stats()
    w = int(st["window_planes"])
    return sum(16 * w * ny * nz for (_, ny, _, nz) in sim.engine.slab_rects() if ny > 0 and nz > 0)


def slab_frames(args, dev, rank, world, xp, barrier, red_dev, cfg, n, ng, frames=3, warmup=6, weighted=True,
                last=None):
    """One scene sharded by slab over the N ranks, frame by frame as main.py
    runs it (step, postprocess, gather to rank 0, rank 0 renders), with the
    render-aware re-cut: rank 0 measures its simulation and render times and
    takes the particle share given by SlabDomain.set_render_share
    (gsmpm_mpm_slab_set_weight); `warmup` untimed frames (the graph capture,
    the share measurement, and frames that let the library's re-cut move the
    bounds), then `frames` frames timed barrier to barrier (max over ranks).
    Per-rank fields: each rank's simulation device time per frame (hipEvents
    around its step call), its particle count, the bytes it sends per substep
    in the window exchange, its migrations, and rank 0's render and gather
    host times (the gather includes the wait for the slowest rank's
    simulation).  last: a dict that receives rank 0's last frame (the gathered
    means and covariances, the image and the radii)."""
    import copy
    import torch
    import torch.distributed as dist
    from gsmpm import raster
    from gsmpm.bc import substep_masks
    a = copy.copy(args)
    a.config, a.material, a.particles, a.n_grid = cfg, None, n, ng
    sc = build_scene(a, dev)
    sim, specs = make_sim(sc, dev, slab=(rank, world, xp))
    sa = sc["sargs"]
    dt, spf = sa.substep_dt, sa.steps_per_frame
    st = {"t": 0.0}
    cam, g, mask = sc["cam"], sc["g"], sc["mask"]
    w_args = (float(sc["s"]), [float(v) for v in sc["c"].reshape(-1).tolist()])
    feats = g.get_features[mask].contiguous() if rank == 0 else None
    opac = g.get_opacity[mask].reshape(-1).contiguous() if rank == 0 else None
    tx, ty = math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5)
    bg = torch.zeros(3, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = {"sim": 0.0, "render": 0.0, "gather": 0.0, "K": 0}

    def frame(timed):
        masks, st["t"] = substep_masks(specs, st["t"], dt, spf)
        e0, e1 = ev(), ev()
        e0.record()
        sim.step(dt, masks)
        e1.record()
        sim.postprocess()
        g0 = time.perf_counter()
        m, c = sim.gather_world(*w_args, render_space=True)
        g1 = time.perf_counter()
        if rank == 0:
            acc["K"], image, radii = raster.forward(m, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                                    cam.height, cam.width, tx, ty, sh_degree=3, shs=feats,
                                                    cov3D_precomp=c)
            torch.cuda.current_stream().synchronize()
            if last is not None:
                last.update(means=m, covs=c, image=image, radii=radii)
        g2 = time.perf_counter()
        e1.synchronize()
        if timed:
            acc["sim"] += e0.elapsed_time(e1)
            acc["gather"] += (g1 - g0) * 1e3
            acc["render"] += (g2 - g1) * 1e3

    frame(False)  # graph capture
    barrier()
    frame(True)  # this rank's sim and rank 0's render, for the share
    sim_ms, render_ms = acc["sim"], acc["render"]
    weight = 1.0
    if weighted and rank == 0:
        weight = sim.set_render_share(sim_ms, render_ms, world)
    for _ in range(max(0, warmup - 2)):
        frame(False)
    barrier()
    acc.update(sim=0.0, render=0.0, gather=0.0)
    st0 = sim.stats()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame(True)
    barrier()
    el = time.perf_counter() - t0
    st1 = sim.stats()
    tt = torch.tensor([el], dtype=torch.float64, device=red_dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    el = float(tt.item())
    mine = torch.tensor([acc["sim"] / frames, float(sim.n), float(slab_exchange_bytes(sim)),
                         float(st1["migrations"] - st0["migrations"]), float(st1["migrated"] - st0["migrated"])],
                        dtype=torch.float64, device=red_dev)
    allr = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    nsim = sc["xg"].shape[0]
    r = {"config": cfg, "particles": nsim, "n_grid": sa.n_grid, "parallelism": f"slab{world}", "scaling": "strong",
         "frames": frames, "substeps_per_frame": spf, "frame_ms": round(el / frames * 1e3, 4),
         "particle_substeps_per_s": nsim * spf * frames / el,
         "per_rank_sim_ms": [round(float(x[0]), 4) for x in allr],
         "per_rank_particles": [int(x[1]) for x in allr],
         "per_rank_exchange_bytes_per_substep": [int(x[2]) for x in allr],
         "per_rank_migrations_per_frame": [round(float(x[3]) / frames, 2) for x in allr],
         "per_rank_migrated_per_frame": [round(float(x[4]) / frames, 1) for x in allr],
         "rank0_render_ms": round(acc["render"] / frames, 4), "rank0_gather_ms": round(acc["gather"] / frames, 4),
         "rank0_weight": round(weight, 4), "rank0_first_frame": {"sim_ms": round(sim_ms, 4),
                                                                 "render_ms": round(render_ms, 4)},
         "render": f"{cam.width}x{cam.height} SH3", "num_rendered": acc["K"] if rank == 0 else None,
         "slab_bounds": sim.bounds, "slab_recuts": sim.rebalances, "cut_axis": sim.cut_axis}
    sim.engine.close()
    barrier()
    del sim, sc
    torch.cuda.empty_cache()
    return r


def dp_frames(args, dev, rank, world, barrier, red_dev, frames=5, warmup=2):
    """N independent lego scenes, one per rank (synthetic seed = rank), each
    simulated and rendered in main.py's order on its own GPU with no
    collective in the data path: the replicas form of the N > 1 job, kept
    beside north_star's slab sharding (weak scaling: value = all ranks'
    particle-substeps / the slowest rank's time)."""
    import torch
    import torch.distributed as dist
    from gsmpm import raster
    from gsmpm.bc import substep_masks
    sc = build_scene(args, dev, rank=rank)
    sim, specs = make_sim(sc, dev)
    sa = sc["sargs"]
    dt, spf = sa.substep_dt, sa.steps_per_frame
    cam, g, mask = sc["cam"], sc["g"], sc["mask"]
    feats, opac = g.get_features[mask].contiguous(), g.get_opacity[mask].reshape(-1).contiguous()
    tx, ty = math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5)
    bg = torch.zeros(3, device=dev)
    w_args = (float(sc["s"]), [float(v) for v in sc["c"].reshape(-1).tolist()])
    st = {"t": 0.0}

    def frame():
        masks, st["t"] = substep_masks(specs, st["t"], dt, spf)
        sim.step(dt, masks)
        sim.postprocess()
        m, c = sim.world_outputs(*w_args, render_space=True)
        raster.forward(m, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg, cam.height, cam.width, tx, ty,
                       sh_degree=3, shs=feats, cov3D_precomp=c)

    for _ in range(warmup):
        frame()
    barrier()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame()
    barrier()
    el = time.perf_counter() - t0
    tt = torch.tensor([el, float(sim.n)], dtype=torch.float64, device=red_dev)
    nt = tt.clone()
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dist.all_reduce(nt)
    el, n_total = float(tt[0].item()), int(nt[1].item())
    del sim, sc
    torch.cuda.empty_cache()
    return {"config": args.config, "parallelism": f"dp{world} independent scenes", "scaling": "weak",
            "particles_total": n_total, "frames": frames, "frame_ms": round(el / frames * 1e3, 4),
            "particle_substeps_per_s": n_total * spf * frames / el}


def sim_render_split(args, dev, rank, world, barrier, red_dev, frames=5):
    """Lego with the simulation and the render on different GPUs (the round-4
    verdict's item 2, N >= 2): rank 1 simulates the whole scene on one GPU
    (no slab exchange), sends each frame's render-space snapshot (means,
    cov6: 36 B a particle) to rank 0 over RCCL, and goes on with the next
    frame; rank 0 renders frame f while rank 1 simulates frame f + 1.  Ranks
    >= 2 idle.  frame_ms against the one-GPU line's ms_per_step is the gain of
    taking the render off the simulating GPU."""
    import torch
    import torch.distributed as dist
    from gsmpm import raster
    from gsmpm.bc import substep_masks
    sc = build_scene(args, dev)
    n = sc["xg"].shape[0]
    sa = sc["sargs"]
    dt, spf = sa.substep_dt, sa.steps_per_frame
    bm = torch.empty((n, 3), dtype=torch.float32, device=dev)  # the snapshot: render-space means, cov6
    bc = torch.empty((n, 6), dtype=torch.float32, device=dev)
    acc = {"render": 0.0, "sim": 0.0, "K": 0}
    if rank == 1:
        sim, specs = make_sim(sc, dev)
        w_args = (float(sc["s"]), [float(v) for v in sc["c"].reshape(-1).tolist()])
        st = {"t": 0.0}
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def frame(timed):
            masks, st["t"] = substep_masks(specs, st["t"], dt, spf)
            e0, e1 = ev(), ev()
            e0.record()
            sim.step(dt, masks)
            e1.record()
            sim.postprocess()
            sim.world_outputs(*w_args, render_space=True, means_out=bm, cov_out=bc)
            dist.send(bm, dst=0)
            dist.send(bc, dst=0)
            if timed:
                e1.synchronize()
                acc["sim"] += e0.elapsed_time(e1)
    elif rank == 0:
        cam, g, mask = sc["cam"], sc["g"], sc["mask"]
        feats, opac = g.get_features[mask].contiguous(), g.get_opacity[mask].reshape(-1).contiguous()
        tx, ty = math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5)
        bg = torch.zeros(3, device=dev)

        def frame(timed):
            dist.recv(bm, src=1)
            dist.recv(bc, src=1)
            r0 = time.perf_counter()
            acc["K"], _, _ = raster.forward(bm, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                            cam.height, cam.width, tx, ty, sh_degree=3, shs=feats, cov3D_precomp=bc)
            torch.cuda.current_stream().synchronize()
            if timed:
                acc["render"] += (time.perf_counter() - r0) * 1e3
    else:
        frame = None
    for _ in range(2):  # capture + warm-up
        if frame:
            frame(False)
    barrier()
    t0 = time.perf_counter()
    for _ in range(frames):
        if frame:
            frame(True)
    barrier()
    el = time.perf_counter() - t0
    tt = torch.tensor([el], dtype=torch.float64, device=red_dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    el = float(tt.item())
    mine = torch.tensor([acc["sim"] / frames, acc["render"] / frames], dtype=torch.float64, device=red_dev)
    allr = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    return {"config": args.config, "particles": n, "parallelism": "sim on rank 1, render on rank 0",
            "frame_ms": round(el / frames * 1e3, 4), "particle_substeps_per_s": n * spf * frames / el,
            "rank1_sim_ms": round(float(allr[1][0]), 4), "rank0_render_ms": round(float(allr[0][1]), 4),
            "snapshot_bytes": int((bm.numel() + bc.numel()) * 4), "num_rendered": acc["K"] if rank == 0 else None}


def multi_gpu_configs(args, dev, rank, world, xp, barrier, red_dev):
    """N > 1 side measurements beside the slab headline: config D (bicycle 1M,
    256^3) through the slab path with the render-aware re-cut, the replicas
    form (one lego scene per rank), and lego's sim / render split."""
    import torch
    res = {}
    which = set((args.multi_configs or ("bicycle,dp" if args.multi == "slab" else "bicycle,lego")).split(","))
    torch.cuda.empty_cache()
    if "bicycle" in which:
        res["D_bicycle_slab"] = slab_frames(args, dev, rank, world, xp, barrier, red_dev, "bicycle.json", 1_000_000,
                                            256, frames=3, warmup=5)
    if "lego" in which:  # the headline's own form at the bench's default size (when the headline was changed)
        res["B_lego_slab"] = slab_frames(args, dev, rank, world, xp, barrier, red_dev, "lego.json", 100_000, 128)
    if "dp" in which:
        res["B_lego_dp"] = dp_frames(args, dev, rank, world, barrier, red_dev)
    if "split" in which:
        res["B_lego_sim_render_split"] = sim_render_split(args, dev, rank, world, barrier, red_dev)
    return res


def config_e(dev, iters=5):
    """BASELINE configs[4] (extra.py system identification): extra.py training
    iterations of the differentiable MPM (30 forward substeps + postprocess,
    its backward, 30 backward substeps, learn, cycle_init; extra.py:205-241
    without the renderer) on tools/bench_fit.py's synthetic 20k-particle torus,
    n_grid 50.  One iteration is the unit; value counts the forward and the
    backward substeps of every particle."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_fit as bf
    from gsmpm.fit import FitSimulator
    n = 20_000
    x, cov, v = bf.torus(n)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    g = FitSimulator(n, n_grid=bf.NG, grid_extent=bf.EXT, gravity=bf.GRAV, **bf.MAT)
    g.set_particles(t(x), t(cov), t(bf.volumes(x)), t(v))
    g.set_bc_ground_only()
    gx = t(np.random.default_rng(1).normal(0, 1, (n, 3)).astype(np.float32))
    gc = t(np.full(n * 6, 10.0, np.float32))

    def iteration():
        for s in range(bf.NSUB):
            g.forward(bf.DT, s)
        g.postprocess_forward()
        g.clear_grads()
        g.set_grads(gx, gc)
        g.postprocess_backward()
        for s in reversed(range(bf.NSUB)):
            g.backward(bf.DT, s)
        g.learn()
        g.cycle_init()

    iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        iteration()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    del g
    torch.cuda.empty_cache()
    return {"config": "extra.py (synthetic torus)", "particles": n, "n_grid": bf.NG, "substeps": bf.NSUB,
            "ms_per_iteration": round(ms, 4), "iterations_per_s": round(1e3 / ms, 1),
            "particle_substeps_per_s_fwd_bwd": 2 * bf.NSUB * n / (ms * 1e-3)}


def slab_main(args, dev, rank, world, red_dev):
    """The N > 1 headline (north_star): ONE lego scene sharded by spatial slab
    over the N ranks (gsmpm.dist.SlabDomain, csrc/slab.h: every substep each
    pair of neighbouring ranks swaps the partial (m v, m) sums of the window
    planes around their shared bound over RCCL, the pairwise all-reduce of
    boundary grid nodes; particles migrate every 10 substeps), rank 0 renders
    the gathered frame and takes the render-aware particle share.  W untimed
    warm-up frames, K frames timed barrier + synchronize to barrier +
    synchronize, max over ranks; value = the scene's particles x substeps /
    that time (strong scaling).  Side fields: config D (bicycle 1M, 256^3)
    through the same slabs, and the replicas form (one scene per rank)."""
    import torch
    import torch.distributed as dist
    from gsmpm.dist import make_transport
    xp = make_transport(rank, world, device=dev)

    def barrier():
        dist.barrier()
        torch.cuda.synchronize()

    last = {} if args.dump_outputs and rank == 0 else None
    r = slab_frames(args, dev, rank, world, xp, barrier, red_dev, args.config, args.particles, args.n_grid,
                    frames=args.steps, warmup=max(2, args.warmup), last=last)
    if last:
        dump_outputs(args.dump_outputs, last)
    spf = r["substeps_per_frame"]
    out = {"metric": METRIC, "value": r["particle_substeps_per_s"], "unit": "particle-substeps/s",
           "n_gpus": world, "steps": args.steps, "warmup": max(2, args.warmup), "ms_per_step": r["frame_ms"],
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
           "data": "synthetic (lego-like Gaussians, seed 0; lego PLY is an LFS pointer in the reference)",
           "config": {"workload": f"{args.config} frame: {spf} substeps + postprocess + gather to rank 0 + render "
                                  f"{r['render']}", "particles_total": r["particles"], "n_grid": r["n_grid"],
                      "material": "jelly", "parallelism": f"slab{world}"},
           "substeps_per_s": spf * 1e3 / r["frame_ms"], "frames_per_s": 1e3 / r["frame_ms"],
           "num_rendered": r["num_rendered"], "slab": r}
    if args.full and not args.no_multi_configs and not args.no_extra_configs:
        out["multi_gpu"] = multi_gpu_configs(args, dev, rank, world, xp, barrier, red_dev)
    if rank == 0:
        print(json.dumps(out), flush=True)
    barrier()
    xp.close()
    dist.destroy_process_group()


def dry_run(args, rank, world):
    """--dry-run: the launch bookkeeping of the real run on the CPU (gloo), so
    tests can check that --gpus N starts N ranks that agree on N."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        ranks = int(t.item())
    else:
        ranks = 1
    slab = world > 1 and args.multi == "slab"
    out = {"metric": METRIC, "value": None, "unit": "particle-substeps/s", "n_gpus": ranks, "dry_run": True,
           "scaling": "strong" if slab else "weak",
           "config": {"parallelism": (f"slab{world}" if slab else f"dp{world} independent scenes") if world > 1
                      else "single"}}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    rank, world, local = resolve_world(args)
    if args.dry_run:
        return dry_run(args, rank, world)
    import torch
    import torch.distributed as dist
    # GSMPM_SHARE_GPU=1 (every rank on cuda:0; RCCL, or GSMPM_DIST_BACKEND=gloo)
    # rehearses the multi-rank path on a one-GPU box; the driver uses RCCL.
    backend = os.environ.get("GSMPM_DIST_BACKEND", "nccl")
    if os.environ.get("GSMPM_SHARE_GPU") == "1":
        local = 0
        if backend == "nccl":  # RCCL accepts ranks on one device as separate "hosts" (socket transport)
            os.environ.update(NCCL_HOSTID=f"gsmpm-bench-rank{rank}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    red_dev = dev if backend == "nccl" else torch.device("cpu")
    if world > 1 and args.multi == "slab":
        return slab_main(args, dev, rank, world, red_dev)
    # --render-cus: the simulator's stream (made current: everything below runs on it) and the
    # render's stream on disjoint CU masks
    masked_render_stream = None
    if args.render_cus > 0 and args.render_overlap and not args.no_render:
        sim_stream, masked_render_stream, render_cus_actual = cu_split_streams(dev, args.render_cus, args.render_cu_layout)
        torch.cuda.set_stream(sim_stream)

    from gsmpm import raster
    from gsmpm.bc import substep_masks

    # N > 1: independent scenes, one per rank (default), or --multi slab: one
    # scene sharded by spatial slab over RCCL; the RCCL transport serves the
    # slab side measurements (multi_gpu) in either mode
    slab = world > 1 and args.multi == "slab"
    xp = None
    if slab or (world > 1 and args.full and not args.no_multi_configs and not args.no_extra_configs):
        from gsmpm.dist import make_transport
        xp = make_transport(rank, world, device=dev)
    scene = build_scene(args, dev, rank=0 if slab else rank)
    sa = scene["sargs"]
    dt, spf = sa.substep_dt, sa.steps_per_frame
    g, mask, cam = scene["g"], scene["mask"], scene["cam"]
    feats = g.get_features[mask].contiguous()
    opac = g.get_opacity[mask].reshape(-1).contiguous()
    sim, specs = make_sim(scene, dev, slab=(rank, world, xp) if slab else None)
    if not slab and args.rebin > 0 and sim.pipeline == "fused":
        sim.set_rebin_interval(args.rebin)
    n_local = sim.n
    n_scene = scene["xg"].shape[0]
    bg = torch.zeros(3, device=dev)
    tanx, tany = math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5)
    # world2grid constants as host floats, once (a per-frame .tolist() / float() of the
    # device tensors would stall the host on the whole frame)
    w_scale, w_center = float(scene["s"]), [float(v) for v in scene["c"].reshape(-1).tolist()]
    state = {"t": 0.0, "K": 0}
    keep_last = bool(args.dump_outputs) and rank == 0  # state["last"]: the newest frame's outputs, for --dump-outputs

    host_t = [] if os.environ.get("GSMPM_BENCH_HOST_TIMING") else None  # per-call host time (diagnostic)

    # Frames are pipelined as main.py's loop allows: frame f's render-space
    # snapshot (world_outputs) is taken on the simulator's stream, then the
    # render of frame f - 1 runs on a second stream while frame f simulates
    # (the rasterizer's pair-count read-back waits on the host for frame f - 1
    # only).  Every timed step still simulates AND renders one frame: the
    # timed region ends with the last frame's render.
    render_stream = masked_render_stream if masked_render_stream is not None else torch.cuda.Stream(dev)
    pending = []

    delay_cycles = 0
    if args.render_delay_us > 0 and args.render_overlap and not args.no_render:
        # torch.cuda._sleep spins a one-wave kernel for N clock cycles: calibrate cycles per us
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(4_000_000)
        e1.record()
        e1.synchronize()
        delay_cycles = int(args.render_delay_us * 4_000_000 / (e0.elapsed_time(e1) * 1e3))

    def render(item):
        means_r, covs_r, ev = item
        if means_r is None or args.no_render:
            return
        with torch.cuda.stream(render_stream):
            render_stream.wait_event(ev)
            if delay_cycles:
                torch.cuda._sleep(delay_cycles)
            K, image, radii = raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                             cam.height, cam.width, tanx, tany, sh_degree=3, shs=feats,
                                             cov3D_precomp=covs_r)
        means_r.record_stream(render_stream)  # allocated on the simulator's stream
        covs_r.record_stream(render_stream)
        state["K"] = K
        if keep_last:
            state["last"] = {"means": means_r, "covs": covs_r, "image": image, "radii": radii}

    # --render-async: the forward with the pair count left on the device
    # (gsmpm_raster_forward_async), enqueued right behind the frame's
    # snapshot -- on the render stream (overlap) or the simulator's -- with no
    # host wait; pairs_cap from one synchronous render of the first snapshot.
    # Every frame keeps its snapshot until flush() has read its counts: a
    # flagged frame (more pairs than the capacity, or a depth bucket overflow)
    # is rendered again by the synchronous form before the timed region ends.
    ren_async = bool(args.render_async) and not slab and not args.no_render
    aq = []  # (AsyncRender, means, covs) of frames not yet checked
    acap = {"cap": 0, "reissued": 0}
    rq = worker = None
    if args.render_thread and args.render_overlap and not args.no_render and not ren_async:
        import queue
        import threading
        rq = queue.Queue(maxsize=2)
        werr = []

        def render_worker():
            torch.cuda.set_device(dev)
            while True:
                item = rq.get()
                try:
                    if item is None:
                        return
                    if not werr:
                        render(item)
                except Exception as e:  # surfaced by flush()
                    werr.append(e)
                finally:
                    rq.task_done()

        worker = threading.Thread(target=render_worker, daemon=True)
        worker.start()

    def flush():
        if ren_async:
            for ar, m, c in aq:
                nr, flags = ar.result()
                image, radii = ar.color, ar.radii
                if flags:  # the synchronous form renders it (counted in the frame's time)
                    state["K"], image, radii = raster.forward(m, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center,
                                                              bg, cam.height, cam.width, tanx, tany, sh_degree=3,
                                                              shs=feats, cov3D_precomp=c)
                    acap["reissued"] += 1
                    acap["cap"] = max(acap["cap"], int(ar.counts[0]) + int(ar.counts[0]) // 4 + 4096)
                else:
                    state["K"] = nr
                if keep_last:
                    state["last"] = {"means": m, "covs": c, "image": image, "radii": radii}
            aq.clear()
            return
        if rq is not None:
            while pending:
                rq.put(pending.pop(0))
            rq.join()
            if werr:
                raise werr[0]
            return
        while pending:
            render(pending.pop(0))

    def frame(render_frame=True):
        t = [time.perf_counter()]
        masks, state["t"] = substep_masks(specs, state["t"], dt, spf)
        if args.render_first and args.render_overlap and rq is None:
            flush()  # frame f - 1 renders while this one simulates, its launches queued first
        sim.step(dt, masks)
        t.append(time.perf_counter())
        sim.postprocess()
        t.append(time.perf_counter())
        if render_frame and not args.no_render:
            # slabs: every particle's render-space mean/cov gathered to rank 0, which
            # renders the frame (compositing order is view-dependent);
            # --dp / one GPU: every rank renders its own scene
            if slab:
                means_r, covs_r = sim.gather_world(w_scale, w_center, render_space=True)
            else:
                means_r, covs_r = sim.world_outputs(w_scale, w_center, render_space=True)
            if ren_async:
                if not acap["cap"]:  # the capacity: the binned pairs of one render of the first snapshot, + 15 %
                    nr, _, _ = raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                              cam.height, cam.width, tanx, tany, sh_degree=3, shs=feats,
                                              cov3D_precomp=covs_r)
                    probe = raster.forward_async(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                                 cam.height, cam.width, tanx, tany, sh_degree=3, shs=feats,
                                                 cov3D_precomp=covs_r, pairs_cap=nr + 4096)  # 3 sigma >= binned
                    probe.result()
                    kb = int(probe.counts[0])
                    acap["cap"] = kb + kb // 8 + 4096
                t.append(time.perf_counter())
                rs = render_stream if args.render_overlap else torch.cuda.current_stream()
                ev = torch.cuda.Event()
                ev.record()
                with torch.cuda.stream(rs):
                    rs.wait_event(ev)
                    ar = raster.forward_async(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                              cam.height, cam.width, tanx, tany, sh_degree=3, shs=feats,
                                              cov3D_precomp=covs_r, pairs_cap=acap["cap"])
                means_r.record_stream(rs)
                covs_r.record_stream(rs)
                aq.append((ar, means_r, covs_r))
                if len(aq) > 8:  # bounded: check the oldest (long done) frames
                    done = aq[:4]
                    del aq[:4]
                    keep = list(aq)
                    aq[:] = done
                    flush()
                    aq[:] = keep
                t.append(time.perf_counter())
            elif not args.render_overlap and means_r is not None:  # main.py's order, one stream
                t.append(time.perf_counter())
                K, image, radii = raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg,
                                                 cam.height, cam.width, tanx, tany, sh_degree=3, shs=feats,
                                                 cov3D_precomp=covs_r)
                state["K"] = K
                if keep_last:
                    state["last"] = {"means": means_r, "covs": covs_r, "image": image, "radii": radii}
                t.append(time.perf_counter())
            else:
                ev = torch.cuda.Event()
                ev.record()
                t.append(time.perf_counter())
                if rq is not None:
                    rq.put((means_r, covs_r, ev))  # the worker renders it while the next frames simulate
                else:
                    if not args.render_first:
                        flush()  # the previous frame renders while this one simulates
                    pending.append((means_r, covs_r, ev))
                t.append(time.perf_counter())
        if host_t is not None:
            host_t.append([1e6 * (b - a) for a, b in zip(t, t[1:])])

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        frame()
    flush()
    barrier()
    # k_render's and the whole forward's in-frame times: three events per
    # forward on its own stream (gsmpm_raster_set_timing), read after the
    # timed region; no host wait is added inside it
    time_render = args.full and not args.no_render and rank == 0
    if time_render:
        raster.timing()
        raster.set_timing(True)
    esc0 = sim.escapes() if args.full and hasattr(sim, "escapes") else None  # (a sync, outside the timed region)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        frame()
    flush()
    barrier()
    elapsed = time.perf_counter() - t0
    render_in_frame = None
    if time_render:
        raster.set_timing(False)
        kr_ms, fw_ms, n_fw = raster.timing()
        if n_fw:
            render_in_frame = {"forwards": n_fw, "k_render_ms": round(kr_ms / n_fw, 4),
                               "forward_ms": round(fw_ms / n_fw, 4)}
    # particle scatters that left their chunk window so far (fused pipeline; a diagnostic of the
    # re-binning interval: gsmpm_mpm_escapes)
    escapes = sim.escapes() if (args.full and world == 1 and hasattr(sim, "escapes")) else None
    escapes_timed = None if escapes is None or esc0 is None else escapes - esc0
    if rq is not None:  # the render worker's last frame is done (flush): stop it
        rq.put(None)
        worker.join()
    if host_t:
        print("host us per call (step, postprocess, world_outputs, render of the previous frame):",
              [round(sum(c) / len(host_t[-args.steps:]), 1) for c in zip(*host_t[-args.steps:])], file=sys.stderr)
    if world > 1:
        tt = torch.tensor([elapsed], device=red_dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        if slab:
            n_total = n_scene  # one scene, every particle simulated once per substep
        else:
            nt = torch.tensor([n_local], device=red_dev, dtype=torch.float64)
            dist.all_reduce(nt)
            n_total = int(nt.item())
    else:
        n_total = n_local

    if keep_last:
        last = state.get("last")
        if last is None:  # --no-render: the frame's outputs are the simulator's
            means_r, covs_r = sim.world_outputs(w_scale, w_center, render_space=True)
            last = {"means": means_r, "covs": covs_r}
        torch.cuda.synchronize()
        dump_outputs(args.dump_outputs, last)

    out = {
        "metric": METRIC,
        "value": n_total * spf * args.steps / elapsed,
        "unit": "particle-substeps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong" if slab else "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (lego-like Gaussians, seed 0; lego PLY is an LFS pointer in the reference)",
        "config": {"workload": f"{args.config} frame: {spf} substeps + postprocess + render "
                               f"{cam.width}x{cam.height} SH3", "particles_per_gpu": n_local,
                   "particles_total": n_total, "n_grid": sa.n_grid, "material": sa.material,
                   "substep_dt": dt, "render_overlap": bool(args.render_overlap),
                   "render_cus": render_cus_actual if masked_render_stream is not None else None,
                   "render_cu_layout": args.render_cu_layout if masked_render_stream is not None else None,
                   "render_delay_us": args.render_delay_us if args.render_overlap else None,
                   "render_first": bool(args.render_first) if args.render_overlap else None,
                   "render_thread": bool(rq is not None),
                   "render_async": ren_async,
                   "render_async_pairs_cap": acap["cap"] if ren_async else None,
                   "render_async_reissued": acap["reissued"] if ren_async else None,
                   "parallelism": (f"slab{world}" if slab else f"dp{world} independent scenes") if world > 1
                   else "single"},
        "substeps_per_s": spf * args.steps / elapsed,
        "frames_per_s": args.steps / elapsed,
        "num_rendered": state["K"],
        "rebin": sim.rebin_state() if hasattr(sim, "rebin_state") else None,
    }

    def finish():
        if rank == 0:
            print(json.dumps(out), flush=True)
        if slab:  # the simulator's captured graphs hold RCCL work: destroy them before the communicator
            sim.engine.close()
        if xp is not None:
            barrier()
            xp.close()
        if world > 1:
            dist.destroy_process_group()

    if not args.full:  # the plain run ends here: every measurement below takes GPU runs of its own
        return finish()

    # ---- breakdown (untimed by the contract; measured on the same stream) ----
    ev = lambda: torch.cuda.Event(enable_timing=True)
    e0, e1 = ev(), ev()
    masks, t_after = substep_masks(specs, state["t"], dt, spf)
    e0.record()
    sim.step(dt, masks)
    e1.record()
    barrier()
    sim_ms = e0.elapsed_time(e1)
    state["t"] = t_after
    render_ms = render_host_ms = render_cold_ms = None
    if not args.no_render and rank == 0 and world == 1:
        # on the stream the timed frames rendered on, after one warm-up render
        # there; device time between hipEvents recorded on that stream around 5
        # renders (each holds its host read-back of the pair count), and beside
        # it the host wall time of the same 5 calls
        means_r, covs_r = sim.world_outputs(w_scale, w_center, render_space=True)
        torch.cuda.synchronize()
        # round 3's form beside it: one render on the current (default) stream,
        # no warm-up there, host wall time (that breakdown read 0.685 ms on the
        # driver's box against 0.263 in the builder's runs)
        c0 = time.perf_counter()
        raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg, cam.height, cam.width,
                       tanx, tany, sh_degree=3, shs=feats, cov3D_precomp=covs_r)
        torch.cuda.synchronize()
        render_cold_ms = (time.perf_counter() - c0) * 1e3
        with torch.cuda.stream(render_stream):
            raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg, cam.height, cam.width,
                           tanx, tany, sh_degree=3, shs=feats, cov3D_precomp=covs_r)
            torch.cuda.synchronize()
            r_ev0, r_ev1 = ev(), ev()
            r0 = time.perf_counter()
            r_ev0.record(render_stream)
            for _ in range(5):
                raster.forward(means_r, opac, cam.view_mat, cam.full_proj_mat, cam.cam_center, bg, cam.height,
                               cam.width, tanx, tany, sh_degree=3, shs=feats, cov3D_precomp=covs_r)
            r_ev1.record(render_stream)
            torch.cuda.synchronize()
            render_host_ms = (time.perf_counter() - r0) / 5 * 1e3
        render_ms = r_ev0.elapsed_time(r_ev1) / 5
    kern = frame_prof = None
    if world == 1:
        fused = sim.pipeline == "fused"
        # nodes owned by the grid update: 8x8x7 (fused) / 8^3 cells per touched tile
        live = sim.debug_stats()["touched_tiles"] * (448 if fused else 512)
        # (1) every launch of one real frame (eager, the same launches the graph
        # replays, re-binning launches included), each kernel's begin/end stamped
        # by its own dispatch packet -- the interval rocprofv3's kernel trace
        # reports, so frame_ms / launches is rocprof's per-launch average
        masks, state["t"] = substep_masks(specs, state["t"], dt, spf)
        prof = sim.profile(dt, masks)
        names = ("k_fused", "k_grid_f", "binning") if fused else ("k_p2g", "k_grid", "k_g2p", "binning")
        # the fused pipeline runs spf + 1 k_fused launches per frame (the first is
        # P2G only, the last G2P only: together one substep's work)
        nl = {"k_fused": spf + 1, "k_grid_f": int(prof[3]) if fused and prof[3] > 0 else spf,
              "k_p2g": spf, "k_grid": spf, "k_g2p": spf}
        frame_prof = {k: prof[i] for i, k in enumerate(names)}
        # (2) steady state: hipEvents around 20 back-to-back launches of each kernel
        # on the current frame's inputs (no re-binning launches)
        kms = sim.time_kernels(dt, substep_masks(specs, state["t"], dt, 1)[0][0], reps=20)
        kern = {k: kms[i] for i, k in enumerate(names)}
        abytes = {k: v for k, v in algorithmic_bytes(n_local, sa.n_grid, sa.material).items() if k in kern}

    out.update({
        "sim_ms_per_frame": sim_ms,
        "sim_substeps_per_s": spf / (sim_ms / 1e3),
        "render_ms_per_frame": render_ms,
        "render_host_ms_per_frame": render_host_ms,
        "render_default_stream_first_ms": render_cold_ms,
        # per forward of the timed frames, on the render's stream beside the simulator
        "render_in_frame": render_in_frame,
        # particle scatters that left their chunk window (each makes the next k_grid_f sweep every tile):
        # since set_particles, and in the timed frames
        "escapes_since_start": escapes,
        "escapes_timed": escapes_timed,
        "rebin": sim.rebin_state() if hasattr(sim, "rebin_state") else None,
    })
    if kern is not None:
        # dominant kernel: the one with the most time per frame among those that
        # carry the reference's work
        dom = max(abytes, key=lambda k: frame_prof[k])
        frame_s = frame_prof[dom] * 1e-3
        avg_launch_s = frame_s / nl[dom]
        wl = {"config": args.config, "particles": args.particles, "n_grid": sa.n_grid, "material": sa.material}
        us = {k: frame_prof[k] / nl[k] * 1e3 for k in ("k_fused", "k_grid_f") if k in frame_prof}
        folded = fused and sim.folded
        kr = kernel_roofline(n_local, sa.n_grid, sa.material, live, us, wl, launches=nl, spf=spf,
                             fold=folded) if fused else {}
        # headline: the live-byte basis (bytes the kernel must move at least), not
        # SURVEY 8(d)'s dense n^3 sweep; the dense figure stays only as the
        # labelled contract fraction
        lbytes = algorithmic_bytes_live(n_local, live, sa.material, folded)[dom] if fused else abytes[dom]
        ach = lbytes / avg_launch_s / 1e9
        traffic = measured_traffic(dom, wl)
        out["kernels_ms_per_launch"] = {k: round(frame_prof[k] / nl[k], 5) for k in frame_prof if k in nl}
        out["kernels_ms_per_frame"] = {k: round(v, 4) for k, v in frame_prof.items()}
        out["kernels_ms_per_launch_steady"] = {k: round(v, 5) for k, v in kern.items()}
        out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic,
                           "traffic_frac": None if traffic is None else
                           round(traffic / avg_launch_s / 1e9 / HBM_PEAK_GBS, 4),
                           "avg_launch_us": round(avg_launch_s * 1e6, 2), "launches_per_frame": nl[dom],
                           "algorithmic_bytes_per_launch": lbytes,
                           "basis": "live bytes: 208 N particle-plane bytes (+ 8 N plastic) + 28 B x live nodes "
                                    "(56 B when k_fused folds the grid update in) (touched 8x8x7 tiles x 448) per "
                                    "launch; achieved = bytes / the kernel's average "
                                    "packet-stamped launch time over one eager frame (= rocprofv3's per-launch "
                                    "duration); traffic = PMC FETCH_SIZE + WRITE_SIZE per launch",
                           "pipeline": sim.pipeline + (" (grid update folded into k_fused)" if folded else ""),
                           "live_nodes": live,
                           "substep": kr.get("substep"),
                           # SURVEY 8(d)'s B_sub split per kernel with the dense n^3 grid the reference sweeps
                           # (utils.py:177-183, model.py:124-127): bytes this kernel never moves, kept only as
                           # the labelled contract figure
                           "frac_dense_contract": round(abytes[dom] / avg_launch_s / 1e9 / HBM_PEAK_GBS, 4),
                           "dense_contract_bytes_per_launch": abytes[dom],
                           "traffic_source_sha": source_sha()}
        out["kernels_roofline"] = kr
    if not args.no_extra_configs and world == 1:
        out["other_configs"] = other_configs(args, dev)
    if world > 1 and xp is not None and not args.no_multi_configs and not args.no_extra_configs:
        # the headline's scene and graphs are done with: free them first
        out["multi_gpu"] = multi_gpu_configs(args, dev, rank, world, xp, barrier, red_dev)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(scene, args, args.cpu_seconds)
    if slab:
        st = sim.stats()
        out["config"]["rank0_slab_planes"] = [st["lo"], st["hi"]]
        out["config"]["rank0_window_rects"] = sim.engine.slab_rects()
        out["config"]["slab_bounds"] = sim.bounds  # after any re-cuts (gsmpm_mpm_slab_set_rebalance, on by default)
        out["config"]["slab_recuts"] = sim.rebalances
    finish()


if __name__ == "__main__":
    main()
