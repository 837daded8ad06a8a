"""The 3DGS export pass on the GPU (csrc/export.hip): k_cov_to_scale_rot and
k_sh_rotate against the float64 reference of tests/export_ref.py, the model
assembly (gsmpm.export.deformed_model) through save_ply / load_ply and the
rasterizer, and main.py --save_pcd --save_pcd_deformed.

Bounds: 4 e_cov and 4 e_sh, e_cov / e_sh the reference's own error once its
outputs are rounded to f32 (export_ref.reference_errors, measured and pinned
in test_export_ref.py); 1e-3 absolute on pixels (test_gpu_raster.py).
Measured on an MI355X: see the docstrings.
"""
from __future__ import annotations

import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import export_ref as E
from conftest import PKG
from test_gpu_raster import _camera

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 1000]
EPS32 = 2.0 ** -24
PIXEL_TOL = 1e-3     # the per-pixel forward tolerance of test_gpu_raster.py
# |render from cov3D_precomp + sh_rotations  -  render from the reference's exported scales /
# rotations / SH|, measured once on an MI355X for the scene of test_end_to_end_render: what the
# file format's f32 (log-scale, quaternion, SH) representation costs in pixels.
FORMAT_ROUNDOFF = 2.4e-7


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------- covariance -> scale, rotation --
@pytest.mark.parametrize("P", SIZES)
def test_cov_to_scale_rot(dev, P):
    """Measured (bound 4 e_cov = 3.50e-6): reconstruction 8.74e-7 at P = 1000 (= e_cov: the kernel's
    f64 result rounds to the reference's f32 values), eigenvalues 9.5e-7 lambda_max."""
    from gsmpm.export import cov_to_scale_rot
    e_cov = E.reference_errors()["e_cov"]
    cov, bad = E.covariance_inputs(P)
    t = _t(dev)
    ls_t, q_t, n_bad = cov_to_scale_rot(t(cov), return_bad=True)
    ls, q = ls_t.cpu().numpy(), q_t.cpu().numpy()
    ok = E.finite_rows(cov)
    assert ls.shape == (P, 3) and q.shape == (P, 4) and ls.dtype == q.dtype == np.float32
    assert np.isfinite(ls).all() and np.isfinite(q).all()
    assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() <= 4 * EPS32
    assert (q[:, 0] >= 0).all() and not np.signbit(q[:, 0]).any()
    assert (np.diff(ls, axis=1) <= 0).all()
    err = E.cov_error(cov, ls, q)
    lam = E.eigenvalues(cov)
    lmax = lam[:, :1]
    above = ok[:, None] & (lam > E.floor_of(lmax))
    eig = np.abs(np.exp(2 * ls.astype(np.float64)) - lam) / np.where(lmax > 0, lmax, 1.0)
    print(f"cov_to_scale_rot P {P}: reconstruction {np.nanmax(err) if np.isfinite(err).any() else 0:.3e}, "
          f"eigenvalues {eig[above].max() if above.any() else 0:.3e} (bound {4 * e_cov:.3e}); n_bad {n_bad}")
    assert not (np.nan_to_num(err) > 4 * e_cov).any(), np.nanargmax(err)
    assert not (eig[above] > 4 * e_cov).any()
    # the zero matrix: identity, the absolute floor
    zero = ok & (np.abs(cov).max(axis=1) == 0)
    assert (ls[zero] == np.float32(E.FLOOR_LOG_SCALE)).all() and (q[zero] == [1, 0, 0, 0]).all()
    # bad rows: identity quaternion, floor scale, counted
    assert n_bad == len(bad)
    assert (q[bad] == [1, 0, 0, 0]).all() and (ls[bad] == np.float32(E.FLOOR_LOG_SCALE)).all()
    # deterministic: a second call and a permutation of the rows give the same bits
    ls2, q2 = cov_to_scale_rot(t(cov))
    assert torch.equal(ls2, ls_t) and torch.equal(q2, q_t)
    perm = np.random.default_rng(P).permutation(P)
    ls3, q3 = cov_to_scale_rot(t(cov[perm]))
    assert np.array_equal(ls3.cpu().numpy(), ls[perm]) and np.array_equal(q3.cpu().numpy(), q[perm])


def test_cov_to_scale_rot_empty_and_counter_accumulates(dev):
    from gsmpm import _lib
    from gsmpm.export import cov_to_scale_rot
    ls, q, nb = cov_to_scale_rot(torch.empty((0, 6), device=dev), return_bad=True)
    assert ls.shape == (0, 3) and q.shape == (0, 4) and nb == 0
    cov, bad = E.covariance_inputs(300)
    c = _t(dev)(cov)
    ls, q = torch.empty((300, 3), device=dev), torch.empty((300, 4), device=dev)
    cnt = torch.full((1,), 5, dtype=torch.int64, device=dev)  # the kernel adds to the caller's counter
    for _ in range(2):
        _lib.check(_lib.LIB.gsmpm_cov_to_scale_rot(_lib.ptr(c), 300, _lib.ptr(ls), _lib.ptr(q), _lib.ptr(cnt),
                                                   _lib.stream_of(dev)), "gsmpm_cov_to_scale_rot")
    assert int(cnt.item()) == 5 + 2 * len(bad)


# ------------------------------------------------------------- SH rotation --
@pytest.mark.parametrize("D,M", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)])
@pytest.mark.parametrize("P", SIZES)
def test_sh_rotate(dev, P, D, M):
    """Measured at P = 1000, of max |shs|: D1 6.9e-9, D2 2.3e-8, D3 6.2e-8 (bounds 4 e_sh: 3.2e-8,
    2.4e-7, 7.7e-7; e_sh is set by the simulator's rotations, which these inputs do not contain)."""
    from gsmpm.export import rotate_sh
    e_sh = E.reference_errors()["e_sh"][D]
    shs, Q = E.sh_inputs(P, M), E.rotation_inputs(P)
    t = _t(dev)
    out_t = rotate_sh(t(shs), t(Q), D)
    out = out_t.cpu().numpy()
    K = (D + 1) ** 2
    assert out.shape == shs.shape and out.dtype == np.float32
    assert np.array_equal(out[:, 0], shs[:, 0]) and np.array_equal(out[:, K:], shs[:, K:])
    err = E.sh_error(D, shs, Q, out, E.check_directions())  # relative to max |shs| = 4.0 (row 0) for every P
    print(f"sh_rotate P {P} D {D} M {M}: {err:.3e} (bound {4 * e_sh:.3e})")
    assert err <= 4 * e_sh
    if D and P > 5:  # past the identity and the half turns: the coefficients do change
        assert np.abs(out[5:, 1:K] - shs[5:, 1:K]).max() > 1e-3
    # [P,9] is the same input; out may alias shs
    assert torch.equal(rotate_sh(t(shs), t(Q.reshape(P, 9)), D), out_t)


def sheared_block_rotations(dev, n=512):
    """Simulator.sh_rotations() of a jelly block in simple shear (v_x = 40 z) after 20 substeps:
    rotations of a few degrees with the orthogonality defect of the f32 polar decomposition."""
    from gsmpm.sim import Simulator
    rng = np.random.default_rng(3)
    x = rng.uniform(0.8, 1.2, size=(n, 3)).astype(np.float32)
    cov = np.tile(np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32), (n, 1))
    vol = np.full(n, (0.4 ** 3) / n, np.float32)
    sim = Simulator(n, n_grid=32, grid_extent=2.0, material="jelly", E=2e5, nu=0.3, density=200.0, gravity=(0, 0, 0),
                    device=dev)
    t = _t(dev)
    sim.set_particles(t(x), t(cov), t(vol))
    v = np.zeros((n, 3), np.float32)
    v[:, 0] = 40.0 * (x[:, 2] - 1.0)
    sim.set("v", t(v))
    sim.step(1e-4, [0] * 20)
    sim.postprocess()
    Q = sim.sh_rotations().cpu().numpy()
    sim.close()
    return Q


def test_sh_rotate_with_the_simulators_rotations(dev):
    """The Q the driver feeds: particle_R of a sheared block.  Measured: max |Q - I| 4.8e-2,
    orthogonality defect 1.16e-6 (the recorded set's), error 2.35e-7 of max |shs| against the
    bound 4 e_sh = 7.7e-7: with such a Q, Y_l(Q d) leaves band l by about the defect, and no
    coefficients reproduce it exactly; the reference's fit over 256 directions is at 1.9e-7."""
    from gsmpm.export import rotate_sh
    Q = sheared_block_rotations(dev)
    P = Q.shape[0]
    turn = float(np.abs(Q - np.eye(3, dtype=np.float32)).max())
    defect = E.orthogonality_defect(Q)
    shs = E.sh_inputs(P, 16)
    out = rotate_sh(_t(dev)(shs), _t(dev)(Q), 3).cpu().numpy()
    err = E.sh_error(3, shs, Q, out, E.check_directions())
    e_sh = E.reference_errors()["e_sh"][3]
    print(f"sh_rotate, simulator Q: max |Q - I| {turn:.2e}, orthogonality defect {defect:.2e} "
          f"(recorded set {E.orthogonality_defect(E.simulator_rotations()):.2e}); {err:.3e} (bound {4 * e_sh:.3e})")
    assert np.isfinite(Q).all() and turn > 1e-3  # the block did shear
    assert np.array_equal(out[:, 0], shs[:, 0])
    assert err <= 4 * e_sh


# -------------------------------------------------------------- end to end --
def _deformed_scene(dev, n=2000):
    """init_synthetic at SH degree 3, covariances F Sigma F^T with random F (det F > 0), moved
    means, random Q."""
    from gaussian_splatting.scene import GaussianModel
    g = GaussianModel(3, device=dev).init_synthetic(n, seed=4)
    rng = np.random.default_rng(4)
    F = np.eye(3) + 0.35 * rng.normal(size=(n, 3, 3))
    F[:, :, 0] *= np.sign(np.linalg.det(F))[:, None]
    S = E.sym3(g.get_covariance().cpu().numpy())
    cov6 = E.cov6_of(F @ S @ F.transpose(0, 2, 1)).astype(np.float32)
    means = (g.get_xyz.cpu().numpy() + rng.normal(0, 0.05, size=(n, 3))).astype(np.float32)
    Q = E.random_rotations(rng, n).astype(np.float32)
    return g, means, cov6, Q


def test_end_to_end_render(dev, tmp_path):
    """deformed_model -> save_ply -> load_ply, rendered from scales / rotations / SH alone (A),
    against the direct render from cov3D_precomp + sh_rotations (B) and the same path as A from
    the float64 reference's export (C).  Measured: A-C 2.4e-7, B-C 2.4e-7 (FORMAT_ROUNDOFF),
    A-B 3.0e-7."""
    from gaussian_splatting.scene import GaussianModel
    from gsmpm import raster
    from gsmpm.export import deformed_model
    g, means, cov6, Q = _deformed_scene(dev)
    n = means.shape[0]
    t = _t(dev)
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    gd = deformed_model(g, mask, t(means), t(cov6), sh_rotations=t(Q))
    path = str(tmp_path / "point_cloud.ply")
    gd.save_ply(path)
    ld = GaussianModel(3, device=dev)
    ld.load_ply(path)
    assert torch.equal(ld._scaling, gd._scaling) and torch.equal(ld._rotation, gd._rotation)
    assert torch.equal(ld.get_features, gd.get_features) and torch.equal(ld._opacity, g._opacity)
    W = H = 64
    view, full, campos, tx, ty = _camera(W, H, 0.9)
    cam = (t(view), t(full), t(campos), t(np.zeros(3, np.float32)), H, W, tx, ty)

    def by_parameters(m):
        return raster.forward(m.get_xyz, m.get_opacity, *cam, sh_degree=3, shs=m.get_features,
                              scales=m.get_scaling, rotations=m.get_rotation)[1]

    A = by_parameters(ld)
    B = raster.forward(t(means), g.get_opacity, *cam, sh_degree=3, shs=g.get_features, cov3D_precomp=t(cov6),
                       sh_rotations=t(Q))[1]
    ls, q = E.cov_to_scale_rot(cov6)
    ref = GaussianModel(3, device=dev)
    shs = E.rotate_sh(g.get_features.cpu().numpy(), Q, 3)
    ref._set(means, shs[:, :1], shs[:, 1:], g._opacity.cpu().numpy(), ls, q)
    C = by_parameters(ref)
    ac, bc, ab = (float((x - y).abs().max()) for x, y in ((A, C), (B, C), (A, B)))
    print(f"end to end: A-C {ac:.3e}, B-C {bc:.3e}, A-B {ab:.3e}; image max {float(B.max()):.3f}")
    assert float(B.max()) > 0.2                      # there is a picture
    assert float((B - raster.forward(t(means), g.get_opacity, *cam, sh_degree=3, shs=g.get_features,
                                     cov3D_precomp=t(cov6))[1]).abs().max()) > 1e-2  # and Q matters to it
    assert ac < PIXEL_TOL
    assert ab < FORMAT_ROUNDOFF + PIXEL_TOL


def _run_main(argv, monkeypatch, record):
    """main.py with the simulator's world_outputs and deformed_model recorded."""
    import main as drv
    real = getattr(drv.MPM_Simulator, "real", drv.MPM_Simulator)

    def spy(*a, **k):
        solver = real(*a, **k)
        inner = solver._sim.world_outputs

        def world_outputs(*wa, **wk):
            m, c = inner(*wa, **wk)
            record["world"].append((m.clone(), c.clone()))
            return m, c

        solver._sim.world_outputs = world_outputs
        return solver

    spy.real = real
    monkeypatch.setattr(drv, "MPM_Simulator", spy)
    buf = io.StringIO()
    with redirect_stdout(buf):
        drv.main(argv)
    return buf.getvalue()


def test_main_py_save_pcd_deformed(dev, tmp_path, monkeypatch):
    """main.py on the tiny scene of test_gpu_main_e2e.py (lego.json, 5,000 synthetic Gaussians,
    n_grid 64, 2 frames) with interior filling: --save_pcd --save_pcd_deformed --rotate_sh writes
    sources + filled rows whose covariances are the simulator's; --save_pcd alone writes the bytes
    the earlier code path writes.  Measured: 1,350 filled; covariance of the source rows 6.8e-7
    (bound 4 e_cov = 3.50e-6)."""
    from gaussian_splatting.scene import GaussianModel
    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        cfg = json.load(f)
    # uniformly scattered Gaussians have no shell; at a 48^3 fill grid and this threshold the holes
    # between them count as interior (about 1,350 cells by tests/fill_ref.py), which is all this test
    # needs of the filling: rows that are not in the trained model
    cfg["particle_filling"] = {"n_grid": 48, "density_threshold": 0.5, "support": 4, "per_cell": 1, "seed": 1}
    cfg_path = tmp_path / "lego-fill.json"
    cfg_path.write_text(json.dumps(cfg))
    common = ["--config_path", str(cfg_path), "--synthetic", "5000", "--n_grid", "64", "--num_frames", "2",
              "--save_pcd", "--save_pcd_interval", "1"]
    src = GaussianModel(3, device=dev).init_synthetic(5000, seed=0)
    bound = torch.tensor(np.array(cfg["mpm"]["sim_area"])).to(dev)  # float64, as main.py compares
    mask = torch.logical_and((src.get_xyz <= bound[1]).all(dim=1), (src.get_xyz >= bound[0]).all(dim=1))
    n_src = int(mask.sum())

    rec = {"world": []}
    out = str(tmp_path / "deformed")
    text = _run_main(common + ["--output_path", out, "--save_pcd_deformed", "--rotate_sh"], monkeypatch, rec)
    filled = int([ln for ln in text.splitlines() if ln.startswith("Number of filled particles: ")][0].split(": ")[1])
    assert f"Number of simulatable Gaussians: {n_src}" in text and filled > 0
    e_cov = E.reference_errors()["e_cov"]
    for fid in (1, 2):
        ld = GaussianModel(3, device=dev)
        ld.load_ply(os.path.join(out, "point_cloud", f"iteration_{fid}", "point_cloud.ply"))
        means, cov6 = rec["world"][fid - 1]
        assert ld.get_xyz.shape[0] == 5000 + filled and means.shape[0] == n_src + filled
        for f in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            assert torch.isfinite(getattr(ld, f)).all(), f
        assert torch.equal(ld.get_xyz[:5000][mask], means[:n_src]) and torch.equal(ld.get_xyz[5000:], means[n_src:])
        assert torch.equal(ld.get_xyz[:5000][~mask], src.get_xyz[~mask])
        assert torch.equal(ld._scaling[:5000][~mask], src._scaling[~mask])
        got = E.sym3(ld.get_covariance().cpu().numpy())
        got = np.concatenate([got[:5000][mask.cpu().numpy()], got[5000:]])
        want = E.sym3(cov6.cpu().numpy())
        err = np.abs(got - want).max(axis=(1, 2)) / np.linalg.norm(want, axis=(1, 2))
        print(f"main.py --save_pcd_deformed frame {fid}: {filled} filled; covariance {err.max():.3e} "
              f"(sources {err[:n_src].max():.3e}; bound {4 * e_cov:.3e})")
        assert err[:n_src].max() <= 4 * e_cov
    # --rotate_sh reached the file: the rest coefficients of the simulated rows moved, the dc did not
    assert torch.equal(ld._features_dc[:5000], src._features_dc)
    assert not torch.equal(ld._features_rest[:5000][mask], src._features_rest[mask])

    # without the flag: byte for byte what the code path before the flag writes
    rec2 = {"world": []}
    out2 = str(tmp_path / "plain")
    _run_main(common + ["--output_path", out2], monkeypatch, rec2)
    for fid in (1, 2):
        g2 = GaussianModel(3, device=dev)
        g2._set(*[t.detach().cpu().numpy() for t in (src._xyz, src._features_dc, src._features_rest, src._opacity,
                                                      src._scaling, src._rotation)])
        g2._xyz[mask] = rec2["world"][fid - 1][0][:n_src]
        want_path = str(tmp_path / f"want_{fid}.ply")
        g2.save_ply(want_path)
        with open(want_path, "rb") as a, open(os.path.join(out2, "point_cloud", f"iteration_{fid}",
                                                           "point_cloud.ply"), "rb") as b:
            assert a.read() == b.read()
