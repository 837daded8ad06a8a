"""GPU diagnostic: what the rasterizer's depth and alpha maps cost on the lego
frame (100k Gaussians, 800x800, SH degree 3, precomputed covariances as
main.py passes them, after one simulated frame).  ROUNDS times, alternating:
REPS forwards with the maps off (k_render<false>), with depth only and with
both (k_render<true>), each timed by the in-frame timer
(gsmpm_raster_set_timing: events before and after k_render on the forward's
own stream).  Prints k_render's and the whole forward's mean time per variant
and round."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gaussian-splatting-mpm_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch  # noqa: E402

import bench  # noqa: E402
from gsmpm import raster  # noqa: E402
from gsmpm.bc import substep_masks  # noqa: E402


class A:
    particles = int(os.environ.get('N', 100000))
    n_grid = int(os.environ.get('NG', 128))
    config = os.environ.get('CONFIG', 'lego.json')
    material = None


REPS = int(os.environ.get('REPS', 50))
ROUNDS = int(os.environ.get('ROUNDS', 3))
dev = torch.device('cuda:0')
scene = bench.build_scene(A, dev)
sim, specs = bench.make_sim(scene, dev)
sa = scene['sargs']
masks, _ = substep_masks(specs, 0.0, sa.substep_dt, sa.steps_per_frame)
sim.step(sa.substep_dt, masks)
sim.postprocess()
cam, g, mask = scene['cam'], scene['g'], scene['mask']
means_r, covs_r = sim.world_outputs(float(scene['s']), [float(v) for v in scene['c'].reshape(-1).tolist()],
                                    render_space=True)
sh = g.get_features[mask].contiguous().detach()
op = g.get_opacity[mask].reshape(-1).contiguous().detach()
args = (means_r, op, cam.view_mat, cam.full_proj_mat, cam.cam_center, torch.zeros(3, device=dev), cam.height,
        cam.width, math.tan(cam.FovX * 0.5), math.tan(cam.FovY * 0.5))
kw = dict(sh_degree=3, shs=sh, cov3D_precomp=covs_r)
variants = [("maps off", dict()), ("depth only", dict(depth=True)), ("depth and alpha", dict(depth=True, alpha=True))]


def timed(more):
    for _ in range(3):
        raster.forward(*args, **kw, **more)
    torch.cuda.synchronize()
    raster.timing()
    raster.set_timing(True)
    for _ in range(REPS):
        raster.forward(*args, **kw, **more)
    raster.set_timing(False)
    kr, fw, n = raster.timing()
    return kr / n * 1e3, fw / n * 1e3


out = raster.forward(*args, **kw, depth=True, alpha=True)
print(f"lego frame: {means_r.shape[0]} Gaussians, {cam.width}x{cam.height}, num_rendered {out[0]}; "
      f"covered pixels (A >= 1/255) {float((out[4] >= 1 / 255).float().mean()):.3f}, A max {float(out[4].max()):.6f}")
for r in range(ROUNDS):
    for name, more in variants:
        kr, fw = timed(more)
        print(f"round {r}  {name:16s} k_render {kr:7.1f} us   forward {fw:7.1f} us   ({REPS} forwards, in-frame timer)",
              flush=True)
