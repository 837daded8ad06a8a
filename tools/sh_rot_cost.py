"""GPU diagnostic: what sh_rotations costs on the lego frame (100k Gaussians,
800x800, SH degree 3, precomputed covariances as main.py passes them).
REPS iterations of the rasterizer forward + backward without and with
sh_rotations = MPM_Simulator.sh_rotations(), and REPS calls of
gsmpm_mpm_sh_rotations with and without A, for
    rocprofv3 --kernel-trace --stats -- python tools/sh_rot_cost.py
(k_preprocess<false|true>, k_preprocess_bwd<false|true>, k_sh_rotations) and,
without the profiler, device-event times per call."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gaussian-splatting-mpm_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch  # noqa: E402

import bench  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from gsmpm.bc import substep_masks  # noqa: E402


class A:
    particles = int(os.environ.get('N', 100000))
    n_grid = int(os.environ.get('NG', 128))
    config = os.environ.get('CONFIG', 'lego.json')
    material = None


REPS = int(os.environ.get('REPS', 50))
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
st = GaussianRasterizationSettings(image_height=cam.height, image_width=cam.width,
                                   tanfovx=math.tan(cam.FovX * 0.5), tanfovy=math.tan(cam.FovY * 0.5),
                                   bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.view_mat,
                                   projmatrix=cam.full_proj_mat, sh_degree=3, campos=cam.cam_center,
                                   prefiltered=False, debug=False)
ras = GaussianRasterizer(st)
m3 = means_r.detach().clone().requires_grad_(True)
c6 = covs_r.detach().clone().requires_grad_(True)
sh = g.get_features[mask].contiguous().detach().clone().requires_grad_(True)
op = g.get_opacity[mask].reshape(-1, 1).contiguous().detach().clone().requires_grad_(True)
Q = sim.sh_rotations().detach().clone().requires_grad_(True)
target = torch.rand(3, cam.height, cam.width, device=dev)
turn = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]  # a quarter turn about z


def step(q):
    img, _ = ras(means3D=m3, means2D=None, shs=sh, colors_precomp=None, opacities=op, scales=None, rotations=None,
                 cov3D_precomp=c6, sh_rotations=q)
    (img - target).abs().mean().backward()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


out = torch.empty((sim.count, 3, 3), dtype=torch.float32, device=dev)
rows = [("forward + backward, sh_rotations=None", timed(lambda: step(None))),
        ("forward + backward, sh_rotations=particle_R", timed(lambda: step(Q))),
        ("gsmpm_mpm_sh_rotations(A=NULL)", timed(lambda: sim.sh_rotations(None, out))),
        ("gsmpm_mpm_sh_rotations(A)", timed(lambda: sim.sh_rotations(turn, out)))]
for name, us in rows:
    print(f"{name}: {us:.1f} us per call ({REPS} reps, device events around the loop)")
