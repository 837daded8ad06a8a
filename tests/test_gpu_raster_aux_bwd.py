"""The rasterizer backward with the gradients of the depth and alpha maps
(gsmpm_raster_backward_aux; k_render_bwd<true>, k_preprocess_bwd<., true>) on
the GPU, through gsmpm.raster.backward, the drop-in's depth_alpha_grad and
extra.py's --lambda_alpha.

Reference: tests/raster_aux_bwd_ref.py (the oracle's colour backward for gC
plus the oracle's colour backward of a render of (z_i, 1, 0) over black for
(gD, gA), plus the chain through z_i), pinned against float64 autograd in
test_raster_aux_bwd_ref.py.  Comparison: the _close rule of
test_gpu_raster_bwd.py (2e-4 of the max; at most 0.1 % of the entries beyond
1e-3 and 0.01 % beyond 1e-2, per element relative to its own magnitude + 1e-3
of the max).  Scenes: `small` (800 Gaussians, 97x61, ragged tiles), `opaque`
(3,000, 64x48, lists longer than 512 and early stops) and `square` (2,000,
200x200) of test_gpu_raster_aux.py, over bg = 0.25.

Every test here fails without the feature.
"""
from __future__ import annotations

import math
import random

import numpy as np
import pytest
import torch

import raster_aux_bwd_ref as ABR
from test_gpu_raster_aux import _Case, _opaque_scene, _scene
from test_gpu_raster_bwd import _close

pytestmark = pytest.mark.gpu

BG = 0.25
_KEYS = ("means2D", "opacity", "means3D", "cov3D", "scales", "rotations", "colors", "sh")


class _BwdCase(_Case):
    """A scene of test_gpu_raster_aux over bg = 0.25 with its pixel weights
    (independent standard normals) and, computed once per (mode, which) and
    never modified, the reference gradients."""

    def __init__(self, dev, scene, W, H, seed):
        super().__init__(dev, scene, W, H, bg=BG)
        P = self.means.shape[0]
        rng = np.random.default_rng(seed)
        self.gC = rng.normal(0, 1, (3, H, W)).astype(np.float32)
        self.gD = rng.normal(0, 1, (H, W)).astype(np.float32)
        self.gA = rng.normal(0, 1, (H, W)).astype(np.float32)
        self.scales = np.exp(rng.normal(-3.2, 0.4, (P, 3))).astype(np.float32)
        self.rots = rng.normal(0, 1, (P, 4)).astype(np.float32)
        self.cols = rng.uniform(0, 1, (P, 3)).astype(np.float32)
        self._refs = {}

    def inputs(self, mode):
        """(kwargs of raster.forward, kwargs of the oracle) for "sh" (SH +
        cov3D_precomp) or "sr" (colors_precomp + scales / rotations)."""
        t = self.t
        if mode == "sh":
            return self.kw, dict(shs=self.shs, sh_degree=3, cov3D_precomp=self.c6)
        return (dict(colors_precomp=t(self.cols), scales=t(self.scales), rotations=t(self.rots)),
                dict(colors_precomp=self.cols, scales=self.scales, rotations=self.rots))

    def ref(self, mode="sh", which="CDA"):
        """Reference gradients for the weights named in `which` (C, D, A)."""
        if (mode, which) not in self._refs:
            g = ABR.backward(self.gC if "C" in which else None, self.gD if "D" in which else None,
                             self.gA if "A" in which else None, self.means, self.opa, self.view, self.full,
                             self.campos, np.full(3, BG, np.float32), self.W, self.H, self.tx, self.ty,
                             **self.inputs(mode)[1])
            for v in g.values():
                if v is not None:
                    v.setflags(write=False)
            self._refs[(mode, which)] = g
        return self._refs[(mode, which)]

    def run(self, mode="sh", which="CDA", maps_in_forward=True, via_rot=False):
        """Context forward + raster.backward on the GPU; returns the gradient dict."""
        from gsmpm import raster
        ctx = raster.RasterContext()
        out = raster.forward(*self.args, **self.inputs(mode)[0], context=ctx, return_args=True,
                             depth=maps_in_forward, alpha=maps_in_forward)
        a, keep = out[-2:]
        gC = self.t(self.gC) if "C" in which else torch.zeros((3, self.H, self.W), device=self.dev)
        if via_rot:
            return _backward_rot(ctx, keep, a, out[2], gC)
        return raster.backward(ctx, keep, a, out[2], gC, self.t(self.gD) if "D" in which else None,
                               self.t(self.gA) if "A" in which else None)


def _backward_rot(ctx, keep, a, radii, gC):
    """The colour backward through gsmpm_raster_backward_rot itself."""
    import ctypes
    from gsmpm._lib import LIB, check, ptr, stream_of
    dev, P = gC.device, a.P
    z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    g = {"means2D": z(P, 3), "colors": z(P, 3), "opacity": z(P), "means3D": z(P, 3), "cov3D": z(P, 6),
         "sh": z(P, a.M, 3) if keep["shs"] is not None else None,
         "scales": z(P, 3) if keep["scales"] is not None else None,
         "rotations": z(P, 4) if keep["rotations"] is not None else None, "sh_rotations": None}
    with torch.cuda.device(dev):
        check(LIB.gsmpm_raster_backward_rot(ctx.h, ctypes.byref(a), ptr(radii), ptr(gC.contiguous()),
                                            ptr(g["means2D"]), ptr(g["colors"]), ptr(g["opacity"]), ptr(g["means3D"]),
                                            ptr(g["cov3D"]), ptr(g["sh"]), ptr(g["scales"]), ptr(g["rotations"]), None,
                                            stream_of(dev)), "gsmpm_raster_backward_rot")
    return g


_CASES = {}


def _case(dev, name):
    if name not in _CASES:
        if name == "small":
            _CASES[name] = _BwdCase(dev, _scene(800, seed=800 + 97), 97, 61, seed=1)
        elif name == "square":
            _CASES[name] = _BwdCase(dev, _scene(2000, seed=2000 + 200), 200, 200, seed=2)
        elif name == "opaque":
            _CASES[name] = _BwdCase(dev, _opaque_scene(3000, seed=3000), 64, 48, seed=3)
    return _CASES[name]


def _compare(got, ref, label):
    n = 0
    for k in _KEYS:
        if ref.get(k) is None:
            continue
        assert got[k] is not None, k
        _close(got[k].cpu().numpy(), ref[k], f"{label}/{k}")
        n += 1
    assert n >= 5, n


def _same(g0, g1):
    assert set(g0) == set(g1)
    for k, v in g0.items():
        if v is None:
            assert g1[k] is None, k
        else:
            assert bool(torch.isfinite(v).all()), k
            assert torch.equal(v, g1[k]), k


@pytest.mark.parametrize("name,mode", [("small", "sh"), ("opaque", "sh"), ("square", "sh"), ("small", "sr")])
def test_parity_with_reference(dev, name, mode):
    """Colour, depth and alpha weights together: every gradient against the reference."""
    c = _case(dev, name)
    got = c.run(mode)
    ref = c.ref(mode)
    _compare(got, ref, f"{name}/{mode}")
    assert np.abs(ref["dz"]).max() > 0


@pytest.mark.parametrize("which", ["D", "A"])
def test_one_map_alone(dev, which):
    """gC = 0 and one map's gradient only: the geometric gradients match the
    reference, and nothing reaches the colours."""
    c = _case(dev, "small")
    for mode in ("sh",):
        got = c.run(mode, which)
        ref = c.ref(mode, which)
        for k in _KEYS[:6]:
            if ref.get(k) is not None:
                _close(got[k].cpu().numpy(), ref[k], f"small/{mode}/{which}/{k}")
        assert not bool(got["colors"].any())
        if got["sh"] is not None:
            assert not bool(got["sh"].any())
        assert bool(got["means3D"].abs().sum() > 0) and bool(got["opacity"].abs().sum() > 0)


@pytest.mark.parametrize("name", ["small", "opaque"])
def test_independent_of_the_forwards_request(dev, name):
    """A context forward that wrote no map, then a backward with map gradients:
    bit for bit the backward after a forward that wrote both."""
    c = _case(dev, name)
    _same(c.run(maps_in_forward=False), c.run(maps_in_forward=True))


@pytest.mark.parametrize("name", ["small", "opaque"])
def test_colour_path_unchanged(dev, name):
    """raster.backward with both map gradients None is the call through
    gsmpm_raster_backward_rot, bit for bit; gsmpm_raster_backward_aux with a
    zero map gradient runs the other kernels and agrees to rounding."""
    c = _case(dev, name)
    g_none = c.run(which="C")
    _same(g_none, c.run(which="C", via_rot=True))
    assert bool(g_none["means3D"].abs().sum() > 0)
    # the new entry point exists and is the one that takes the maps
    from gsmpm._lib import LIB
    assert hasattr(LIB, "gsmpm_raster_backward_aux")
    from gsmpm import raster
    ctx = raster.RasterContext()
    out = raster.forward(*c.args, **c.kw, context=ctx, return_args=True)
    g_zero = raster.backward(ctx, out[-1], out[-2], out[2], c.t(c.gC), torch.zeros((c.H, c.W), device=dev), None)
    for k, v in g_none.items():
        if v is not None:
            _close(g_zero[k].cpu().numpy(), v.cpu().numpy(), f"{name}/zero-map/{k}")


@pytest.mark.parametrize("mode", [("0", "0", "0"), ("1", "0", "0"), ("0", "1", "0"), ("0", "0", "1")])
def test_every_listed_pair_record_is_written_with_maps(dev, monkeypatch, mode):
    """GSMPM_RASTER_POISON=1 (every listed pair's record NaN before
    k_render_bwd) with map gradients: all outputs finite and bit-identical to
    the unpoisoned run, so k_render_bwd<true> writes the dz slot of every
    listed pair, the batches past a tile's last contributor included.  The
    binning variants of test_every_listed_pair_record_is_written, on the
    opaque scene (lists of more than two batches, early stops)."""
    render_mode, onesweep, wide = mode
    monkeypatch.setenv("GSMPM_RASTER_RENDER_MODE", render_mode)
    monkeypatch.setenv("GSMPM_RASTER_ONESWEEP", onesweep)
    monkeypatch.setenv("GSMPM_RASTER_WIDE_KEYS", wide)
    c = _case(dev, "opaque")
    outs = []
    for poison in ("0", "1"):
        monkeypatch.setenv("GSMPM_RASTER_POISON", poison)
        outs.append(c.run("sr"))
    _same(outs[1], outs[0])
    assert bool(outs[0]["means3D"].abs().sum() > 0)


def test_degenerate_frames(dev):
    """Every Gaussian behind the camera (K = 0): all-zero gradients; P = 0
    through the drop-in backpropagates nothing."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gsmpm import raster
    c = _case(dev, "small")
    t, W, H = c.t, c.W, c.H
    behind = np.tile(np.array([[0.0, 0.0, -10.0]], np.float32), (10, 1))
    bargs = [t(behind), t(np.ones((10, 1), np.float32)), *c.args[2:]]
    bkw = dict(colors_precomp=t(np.ones((10, 3), np.float32)),
               cov3D_precomp=t(np.tile(np.array([[1e-2, 0, 0, 1e-2, 0, 1e-2]], np.float32), (10, 1))))
    ctx = raster.RasterContext()
    out = raster.forward(*bargs, **bkw, context=ctx, return_args=True)
    assert int(out[2].abs().sum()) == 0
    g = raster.backward(ctx, out[-1], out[-2], out[2], t(c.gC), t(c.gD), t(c.gA))
    for k, v in g.items():
        if v is not None:
            assert v.numel() > 0 and not bool(v.any()), k
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tx, tanfovy=c.ty, bg=c.args[5],
                                       scale_modifier=1.0, viewmatrix=c.args[2], projmatrix=c.args[3], sh_degree=0,
                                       campos=c.args[4], prefiltered=False, debug=False)
    m = torch.zeros(0, 3, device=dev, requires_grad=True)
    img, radii, depth, alpha = GaussianRasterizer(st)(
        means3D=m, means2D=None, opacities=torch.zeros(0, 1, device=dev), colors_precomp=torch.zeros(0, 3, device=dev),
        cov3D_precomp=torch.zeros(0, 6, device=dev), return_depth_alpha=True, depth_alpha_grad=True)
    assert depth.requires_grad and alpha.requires_grad
    assert not bool(depth.any()) and not bool(alpha.any())
    (img.sum() + depth.sum() + alpha.sum()).backward()
    assert m.grad is None or m.grad.numel() == 0


def test_drop_in_keeps_the_maps_in_the_graph(dev):
    from diff_gaussian_rasterization import (GaussianRasterizationSettings, GaussianRasterizer,
                                             rasterize_gaussians)
    c = _case(dev, "small")
    st = GaussianRasterizationSettings(image_height=c.H, image_width=c.W, tanfovx=c.tx, tanfovy=c.ty, bg=c.args[5],
                                       scale_modifier=1.0, viewmatrix=c.args[2], projmatrix=c.args[3], sh_degree=3,
                                       campos=c.args[4], prefiltered=False, debug=False)
    m3 = c.args[0].clone().requires_grad_(True)
    opa = c.args[1].clone().requires_grad_(True)
    kw = dict(means3D=m3, means2D=None, opacities=opa, shs=c.kw["shs"], cov3D_precomp=c.kw["cov3D_precomp"])
    color, radii, depth, alpha = GaussianRasterizer(st)(**kw, return_depth_alpha=True, depth_alpha_grad=True)
    assert color.requires_grad and depth.requires_grad and alpha.requires_grad and not radii.requires_grad
    (alpha * c.t(c.gA)).sum().backward()
    ref = c.ref("sh", "A")
    _close(m3.grad.cpu().numpy(), ref["means3D"], "drop-in/alpha/means3D")
    _close(opa.grad.view(-1).cpu().numpy(), ref["opacity"], "drop-in/alpha/opacity")
    # all three outputs in one loss, the normalised depth formed by the caller
    m3.grad = opa.grad = None
    color, _, depth, alpha = GaussianRasterizer(st)(**kw, return_depth_alpha=True, depth_alpha_grad=True)
    ((color * c.t(c.gC)).sum() + (depth * c.t(c.gD)).sum() + (alpha * c.t(c.gA)).sum()).backward()
    _close(m3.grad.cpu().numpy(), c.ref("sh")["means3D"], "drop-in/all/means3D")
    nd = GaussianRasterizer(st)(**kw, return_depth_alpha=True, depth_alpha_grad=True)
    m3.grad = None
    (nd[2] / nd[3].clamp_min(1e-3)).sum().backward()
    assert bool(torch.isfinite(m3.grad).all()) and bool(m3.grad.abs().sum() > 0)
    # the flag alone is an error, on all three entry points' public two
    with pytest.raises(ValueError):
        GaussianRasterizer(st)(**kw, depth_alpha_grad=True)
    e = torch.Tensor([])
    with pytest.raises(ValueError):
        rasterize_gaussians(m3, None, c.kw["shs"], e, opa, e, e, c.kw["cov3D_precomp"], st, depth_alpha_grad=True)
    # a tensor passed positionally where sh_rotations is meant is still refused
    Q = torch.eye(3, device=dev).repeat(m3.shape[0], 1, 1)
    with pytest.raises(TypeError):
        rasterize_gaussians(m3, None, c.kw["shs"], e, opa, e, e, c.kw["cov3D_precomp"], st, Q)
    with pytest.raises(TypeError):
        rasterize_gaussians(m3, None, c.kw["shs"], e, opa, e, e, c.kw["cov3D_precomp"], st, True, Q)
    # without the new keyword the maps stay out of the graph
    out = GaussianRasterizer(st)(**kw, return_depth_alpha=True)
    assert not out[2].requires_grad and not out[3].requires_grad


def _extra_run(lambda_alpha):
    """extra.py's loop on the synthetic torus of test_extra_py_synthetic_training_loop
    (n = 3000, 64 x 64, 2 cameras, one iteration), seeded."""
    from argparse import ArgumentParser

    import extra
    from arguments import MPMParams
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    sim_args = MPMParams(ArgumentParser())
    sim_args.fitting = True
    sim_args.E, sim_args.nu = 3e5, 0.3

    class A:
        iters = 1
    args = A()
    if lambda_alpha is not None:
        args.lambda_alpha = lambda_alpha
    si = extra.SystemIndentifier("", "", sim_args, args, synthetic=dict(n=3000, E_true=1e5, size=64, n_cams=2))
    return si, si.train(log=lambda *_: None)


@pytest.fixture(scope="module")
def extra_runs(dev):
    return {k: _extra_run(k) for k in (None, 0.0, 1.0)}


def test_extra_py_silhouette_loss(extra_runs):
    """--lambda_alpha 1: the loop runs with the alpha map in the loss, every
    ground-truth camera carries its mask, and the term moves the fit."""
    import extra
    si, hist = extra_runs[1.0]
    assert len(hist) == extra.train_num_frames
    assert all(math.isfinite(h[2]) and math.isfinite(h[3]) and math.isfinite(h[4]) for h in hist)
    for frame in si.cameras_all:
        for cam in frame:
            a = cam.gt_alpha
            assert tuple(a.shape) == (64, 64) and not a.requires_grad
            assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
            assert bool((a > 0.5).any()) and bool((a == 0).any())  # covered and empty pixels
    assert hist[-1][3] != extra_runs[0.0][1][-1][3]


def test_extra_py_lambda_zero_is_the_colour_only_loop(extra_runs, dev):
    """lambda_alpha = 0 is the loop without the attribute.

    The request was: the two histories equal value for value.  That cannot be
    asked of the frames behind the differentiable MPM: its scatters bin by
    atomic ranks, so two runs of the very same code "can still differ in the
    last bits from run to run" (csrc/fit.hip; test_gpu_fit.py measured
    run-to-run spreads of the adjoints up to 2e-2).  Measured on the MI355X
    with this test as first written: frame 0 equal; frame 1 loss
    0.20004837214946747 and E 299996.1153687383 equal, nu 0.300000067146472
    against 0.30000004525088; later frames drift apart from there.  So the
    equality is asserted, value for value, where the code is deterministic
    and lambda_alpha could enter:
      * the history's iteration and frame columns, and the whole of frame 0
        (the appearance fit: render, loss, no MPM);
      * render() on the same state: a bare tensor (no maps requested, the
        colour-only kernels), bit-identical between the two objects, and so
        is every gradient of a loss on it;
      * no mask on the cameras.
    The frames behind the MPM are checked for what both runs must share:
    finite, and E moved."""
    si0, h0 = extra_runs[0.0]
    si_, h_ = extra_runs[None]
    assert si0.lambda_alpha == 0.0 and si_.lambda_alpha == 0.0
    assert len(h0) == len(h_) and [h[:2] for h in h0] == [h[:2] for h in h_]
    assert h0[0] == h_[0]
    for h in (h0, h_):
        assert all(math.isfinite(v) for row in h for v in row[2:]) and h[-1][3] != 3e5
    for si in (si0, si_):
        assert not any(hasattr(cam, "gt_alpha") for frame in si.cameras_all for cam in frame)
    cam = si_.cameras_all[3][1]
    w = torch.from_numpy(np.random.default_rng(7).normal(0, 1, (3, 64, 64)).astype(np.float32)).to(dev)
    grads = []
    for si in (si0, si_):
        means = si_.gaussians.get_xyz.detach().clone().requires_grad_(True)
        covs = si_.gaussians.get_covariance().detach().clone().requires_grad_(True)
        img = si.render(cam, si_.gaussians, means, covs)
        assert isinstance(img, torch.Tensor) and tuple(img.shape) == (3, 64, 64)
        for p in (si_.gaussians._features_dc, si_.gaussians._opacity):
            p.grad = None
        (img * w).sum().backward()
        grads.append([img.detach(), means.grad, covs.grad, si_.gaussians._features_dc.grad.clone(),
                      si_.gaussians._opacity.grad.clone()])
    for a, b in zip(*grads):
        assert bool(a.abs().sum() > 0) and torch.equal(a, b)
    # with the term on, the same call returns the alpha map too, in the graph
    out = extra_runs[1.0][0].render(cam, si_.gaussians, si_.gaussians.get_xyz, si_.gaussians.get_covariance())
    assert isinstance(out, tuple) and torch.equal(out[0], grads[0][0]) and out[1].requires_grad
