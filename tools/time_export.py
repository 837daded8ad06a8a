"""Times the export pass (csrc/export.hip) on cuda:0: k_cov_to_scale_rot, k_sh_rotate (D = 3) and
gsmpm.export.deformed_model at 100,000 and 1,000,000 synthetic Gaussians (device events, median of
50 calls after 5 warm-up calls), and next to them what a saved frame costs anyway: the PNG encode
of the 800x800 frame of the 100,000 Gaussians (FrameWriter's work) and save_ply of the rows.
DESIGN.md 3.12 "Cost" quotes its output.

    python tools/time_export.py
"""
import io, os, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-mpm_amd"), os.path.join(ROOT, "tests")]
from gaussian_splatting.scene import GaussianModel
from gsmpm import raster
from gsmpm.export import cov_to_scale_rot, rotate_sh, deformed_model
from sh_rot_ref import random_rotations
from utils.render_utils import to8b
from test_gpu_raster import _camera
dev = torch.device("cuda:0")

def timed(fn, reps):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())

for n in (100_000, 1_000_000):
    g = GaussianModel(3, device=dev).init_synthetic(n, seed=1)
    rng = np.random.default_rng(1)
    cov = g.get_covariance().contiguous()
    Q = torch.from_numpy(random_rotations(rng, n).astype(np.float32)).to(dev)
    shs = g.get_features.contiguous()
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    ls, q = torch.empty((n, 3), device=dev), torch.empty((n, 4), device=dev)
    from gsmpm import _lib
    out = torch.empty_like(shs)
    st = _lib.stream_of(dev)
    k1 = timed(lambda: _lib.LIB.gsmpm_cov_to_scale_rot(_lib.ptr(cov), n, _lib.ptr(ls), _lib.ptr(q), None, st), 50)
    k2 = timed(lambda: _lib.LIB.gsmpm_sh_rotate(_lib.ptr(shs), _lib.ptr(Q), n, 3, 16, _lib.ptr(out), st), 50)
    dm = timed(lambda: deformed_model(g, mask, g.get_xyz, cov, sh_rotations=Q), 10)
    b1, b2 = n * (24 + 28), n * (192 * 2 + 36)
    print(f"n {n}: k_cov_to_scale_rot median {k1[0]:.4f} ms (min {k1[1]:.4f} max {k1[2]:.4f}), {b1 / k1[0] / 1e6:.0f} GB/s; "
          f"k_sh_rotate D3 median {k2[0]:.4f} ms (min {k2[1]:.4f} max {k2[2]:.4f}), {b2 / k2[0] / 1e6:.0f} GB/s; "
          f"deformed_model (both kernels + torch copies) {dm[0]:.3f} ms", flush=True)
    if n == 100_000:
        W = H = 800
        view, full, campos, tx, ty = _camera(W, H, 0.9)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        img = raster.forward(g.get_xyz, g.get_opacity, t(view), t(full), t(campos), t(np.zeros(3, np.float32)), H, W, tx, ty,
                             sh_degree=3, shs=shs, cov3D_precomp=cov)[1]
        frame = img.cpu().numpy().transpose(1, 2, 0)
        from PIL import Image
        ts = []
        for _ in range(10):
            t0 = time.perf_counter(); buf = io.BytesIO(); Image.fromarray(to8b(frame)).save(buf, format="PNG"); ts.append((time.perf_counter() - t0) * 1e3)
        print(f"PNG encode of the 800x800 frame of these Gaussians (FrameWriter's work): median {np.median(ts):.1f} ms, {buf.tell()} bytes", flush=True)
        path = os.path.join(tempfile.mkdtemp(), "point_cloud.ply")
        gd = deformed_model(g, mask, g.get_xyz, cov, sh_rotations=Q)
        torch.cuda.synchronize(); t0 = time.perf_counter(); gd.save_ply(path); print(f"save_ply of {n} rows: {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
