"""Workgroup timeline of one k_grid_f launch on the bench scene at rest, split
by the chunk counts of the workgroup's tile (GPU diagnostic; the library must
be the stamps build: make -C csrc stamps, GSMPM_LIB=.../libgsmpm_stamps.so).

Runs FRAMES frames (default 13: the lego scene is at rest from frame 12 on,
profiles/chunk_hist/), then three profiled substeps, and reads the stamps of
the last k_grid_f launch: 0 start, 2 tile known, 3 cover record in LDS, 4
nodes stored, 1 end (s_memrealtime, 100 MHz); slot 5 the tile, 6 its own chunk
count | the largest chunk count among its 27 covers << 16, 7 the part.  Prints
when the workgroups end, relative to the launch's first start, by the largest
cover chunk count: whether the waves of the dense tiles end the launch.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gaussian-splatting-mpm_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
import bench
from gsmpm.bc import substep_masks
from gsmpm._lib import LIB, stream_of


class A:
    particles = int(os.environ.get('N', 100000))
    n_grid = int(os.environ.get('NG', 128))
    config = os.environ.get('CONFIG', 'lego.json')
    material = os.environ.get('MAT')


frames = int(os.environ.get('FRAMES', 13))
dev = torch.device('cuda:0')
scene = bench.build_scene(A, dev)
sim, specs = bench.make_sim(scene, dev)
sa = scene['sargs']
t = 0.0
for _ in range(frames):
    masks, t = substep_masks(specs, t, sa.substep_dt, sa.steps_per_frame)
    sim.step(sa.substep_dt, masks)
torch.cuda.synchronize()
print('stats', sim.debug_stats(), 'pipeline', sim.pipeline, 'frames', frames)
masks, t = substep_masks(specs, t, sa.substep_dt, sa.steps_per_frame)
ms = sim.profile(sa.substep_dt, masks[:3])
print('event ms K/grid/bins per 3 substeps', [round(float(m), 4) for m in ms])
buf = np.zeros((4, 8192, 8), np.uint64)
LIB.gsmpm_debug_stamps(buf.ctypes.data_as(ctypes.c_void_p), stream_of(dev))
g = buf[3].astype(np.int64)
g = g[g[:, 0] > 0]
t0 = g[:, 0].min()
ok = g[:, 2] > 0
g = g[ok]
print(f"k_grid_f: {len(ok)} WGs ({len(g)} with a tile); start spread {(g[:, 0].max() - t0) / 100:.2f} us; "
      f"last end {(g[:, 1].max() - t0) / 100:.2f} us")
own, cov = g[:, 6] & 0xffff, g[:, 6] >> 16
end = (g[:, 1] - t0) / 100
start = (g[:, 0] - t0) / 100
nodes = (g[:, 4] - g[:, 3]) / 100
print("by the largest chunk count among the tile's covers (own = the tile's own count):")
print("covers' max | WGs | start p50 | cover->stored p50 / p90 / max | end p50 / p90 / max (us after the first start)")
for c in sorted(set(cov.tolist())):
    m = cov == c
    p = lambda a, q: np.percentile(a[m], q)
    print(f"  {c:2d} | {m.sum():5d} | {p(start, 50):5.2f} | {p(nodes, 50):5.2f} / {p(nodes, 90):5.2f} / {nodes[m].max():5.2f} | "
          f"{p(end, 50):5.2f} / {p(end, 90):5.2f} / {end[m].max():5.2f}")
sp, de = cov <= 1, cov >= 3
if sp.any() and de.any():
    print(f"last end: single-chunk covers {end[sp].max():.2f} us, covers of >= 3 chunks {end[de].max():.2f} us; "
          f"p90 {np.percentile(end[sp], 90):.2f} / {np.percentile(end[de], 90):.2f}")
order = np.argsort(-end)[:10]
print("last 10 WGs to end: (end us, start us, cover->stored us, own chunks, covers' max, part)")
for i in order:
    print("   ", round(end[i], 2), round(start[i], 2), round(nodes[i], 2), int(own[i]), int(cov[i]), int(g[i, 7]))
ms2 = sim.time_kernels(sa.substep_dt, masks[3], reps=20)
print('time_kernels K/grid/bins', [round(float(m), 4) for m in ms2])
