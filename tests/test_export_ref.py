"""CPU tests of the 3DGS export pass: the float64 reference (tests/export_ref.py)
is pinned by known answers, its own error after rounding to f32 is measured
(the GPU bounds of test_gpu_export.py are 4x these numbers; DESIGN.md 3.12
records them), and the parts of the feature that need no GPU are checked: the
C-ABI's argument validation, the committed SH tables, the flag and the config.

Measured here (printed by test_reference_error_after_f32_rounding):
  e_cov = 8.74e-7   the f32 rounding of the log-scales (half an ulp at 8..16 is
                    4.8e-7, twice that on lambda) and of the quaternion
  e_sh  = 8.1e-9 (D = 1), 6.1e-8 (D = 2), 1.93e-7 (D = 3) of max |shs|; for
          D >= 2 it is set by the recorded simulator rotations, which are off
          orthogonal by 1.16e-6 (on the f32-rounded rotations alone: 2.1e-8, 4.2e-8)
"""
from __future__ import annotations

import json
import os
import re
from argparse import ArgumentParser

import numpy as np
import pytest

import export_ref as E
from conftest import PKG
from sh_rot_ref import random_rotations

EPS32 = 2.0 ** -24


# ------------------------------------------------------------ SH reference --
def _rz(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def test_identity_rotation_is_the_identity_map():
    shs = E.sh_inputs(50, 16)
    out = E.rotate_sh(shs, np.tile(np.eye(3), (50, 1, 1)), 3)
    assert np.abs(out - shs).max() < 1e-13
    for X in E.band_maps(3, np.eye(3)[None]):
        assert np.abs(X[0] - np.eye(X.shape[1])).max() < 1e-13


@pytest.mark.parametrize("phi", [0.3, -1.1, 2.5])
def test_z_rotation_mixes_the_m_pairs(phi):
    """Q = a turn by phi about z: within band l the pair (l, -m), (l, +m) mixes by the angle
    m phi and nothing else does; m = 0 is untouched.  Band 1 is written out with its signs:
    sh(c, Q d) = -C1 (s x + c y) c_1 + C1 z c_2 - C1 (c x - s y) c_3, so c'_1 = c c_1 - s c_3,
    c'_3 = s c_1 + c c_3."""
    maps = E.band_maps(3, _rz(phi)[None])
    c, s = np.cos(phi), np.sin(phi)
    assert np.abs(maps[0][0] - np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])).max() < 1e-13
    for l, X in zip((1, 2, 3), maps):
        X = X[0]
        want = np.zeros_like(X)
        want[l, l] = 1.0
        for m in range(1, l + 1):
            i, j = l - m, l + m
            blk = X[np.ix_([i, j], [i, j])]
            assert abs(blk[0, 0] - np.cos(m * phi)) < 1e-13 and abs(blk[1, 1] - np.cos(m * phi)) < 1e-13
            assert abs(abs(blk[0, 1]) - abs(np.sin(m * phi))) < 1e-13 and abs(blk[0, 1] + blk[1, 0]) < 1e-13
            want[np.ix_([i, j], [i, j])] = blk
        assert np.abs(X - want).max() < 1e-13  # nothing outside the pairs


def test_reference_rotation_satisfies_its_contract_in_f64():
    rng = np.random.default_rng(1)
    Q = random_rotations(rng, 40)
    shs = E.sh_inputs(40, 16)
    for D in (1, 2, 3):
        assert E.sh_error(D, shs, Q, E.rotate_sh(shs, Q, D), E.check_directions()) < 1e-14
    out = E.rotate_sh(shs, Q, 1)
    assert np.array_equal(out[:, 0], shs[:, 0].astype(np.float64)) and np.array_equal(out[:, 4:], shs[:, 4:])


def test_sh_basis_is_the_rasterizers():
    """export_ref.sh_eval against tests/raster_torch_ref.py::_sh, the polynomial the GPU tests of the
    rasterizer are judged by."""
    import torch
    from raster_torch_ref import _sh
    rng = np.random.default_rng(2)
    shs, d = rng.normal(size=(30, 16, 3)), E.unit_directions(rng, 30)
    for D in (0, 1, 2, 3):
        want = _sh(D, torch.tensor(shs), torch.tensor(d)).numpy()
        assert np.abs(E.sh_eval(D, shs, d[:, None, :])[:, 0] - want).max() < 1e-14


# ----------------------------------------------------- covariance reference --
def test_diagonal_covariance_returns_its_own_entries():
    for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [1, 0, 2]):
        d = np.array([4.0, 0.25, 1e-6])[perm]
        cov = np.array([[d[0], 0, 0, d[1], 0, d[2]]])
        ls, q = E.cov_to_scale_rot(cov)
        assert np.allclose(np.exp(2 * ls[0]), [4.0, 0.25, 1e-6], rtol=1e-14)
        R = E.quat_to_rot(q)[0]
        assert np.abs(np.abs(R) - np.eye(3)[:, np.argsort(-d)]).max() < 1e-15  # a signed permutation
        assert abs(np.linalg.det(R) - 1.0) < 1e-14 and q[0, 0] >= 0
        assert np.abs(E.reconstruct(ls, q)[0] - np.diag(d)).max() < 1e-15


def test_reference_output_is_canonical_and_finite():
    cov, bad = E.covariance_inputs(E.N_MAX)
    ls, q = E.cov_to_scale_rot(cov)
    assert np.isfinite(ls).all() and (np.diff(ls, axis=1) <= 0).all()
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-15 and (q[:, 0] >= 0).all()
    assert np.abs(np.linalg.det(E.quat_to_rot(q)) - 1).max() < 1e-14
    assert (q[bad] == [1, 0, 0, 0]).all() and np.allclose(ls[bad], E.FLOOR_LOG_SCALE)
    ok = np.isfinite(E.cov_error(cov, ls, q))
    # exact in f64 but for the rows f32 rounding left indefinite: their clamped negative eigenvalue,
    # at most the rounding of the entries, is the error
    assert np.nanmax(E.cov_error(cov, ls, q)) < EPS32
    assert np.nanmedian(E.cov_error(cov, ls, q)) < 1e-14
    assert ok.sum() == E.N_MAX - len(bad) - 1           # every row but the bad two and the zero matrix


def test_get_covariance_of_a_model_built_from_the_reference_matches():
    """GaussianModel.get_covariance (f32 torch: exp, quaternion -> R, two products) of the reference's
    export against the input, in the e_cov metric.  The f32 evaluation adds a few roundings on top
    of the reference's own e_cov: two exp (<= 2 ulp each), R's entries (<= 4 ulp), two 3-term
    products; 16 eps covers them."""
    import torch
    from gaussian_splatting.scene import GaussianModel
    cov, bad = E.covariance_inputs(E.N_MAX)
    ls, q = E.cov_to_scale_rot(cov)
    g = GaussianModel(3, device="cpu")
    g._scaling, g._rotation = torch.tensor(ls, dtype=torch.float32), torch.tensor(q, dtype=torch.float32)
    got = g.get_covariance().numpy().astype(np.float64)
    S = E.sym3(np.where(E.finite_rows(cov)[:, None], cov, 0.0))
    nrm = np.linalg.norm(S, axis=(1, 2))
    use = E.finite_rows(cov) & (nrm > 1e-30)  # below: exp(log_scale)^2 leaves f32's normal range
    err = np.abs(E.sym3(got) - S).max(axis=(1, 2))[use] / nrm[use]
    print(f"get_covariance of the reference's export: max rel err {err.max():.3e}")
    assert err.max() < E.reference_errors()["e_cov"] + 16 * EPS32


def test_reference_error_after_f32_rounding():
    """e_cov and e_sh, the figures the GPU bounds are 4x of.  Sanity limits from the formats alone:
    e_cov <= 2 * half an ulp of a log-scale in [16, 32) (9.5e-7) + the quaternion's rounding through
    R S^2 R^T (a few eps) < 2.5e-6; e_sh <= 16 coefficients rounded by eps each, |Y_m| <= 1.1,
    plus l * the orthogonality defect of the f32 rotations in the set, < 2e-6."""
    e = E.reference_errors()
    defect = max(E.orthogonality_defect(E.rotation_inputs(E.N_MAX)), E.orthogonality_defect(E.simulator_rotations()))
    print(f"e_cov = {e['e_cov']:.3e}; e_sh = " + ", ".join(f"D{D}: {e['e_sh'][D]:.3e}" for D in (1, 2, 3)) +
          f"; orthogonality defect of the rotations {defect:.2e}")
    assert 1e-8 < e["e_cov"] < 2.5e-6
    assert all(1e-9 < e["e_sh"][D] < 2e-6 for D in (1, 2, 3))


# ------------------------------------------------------- the committed tables --
def _tables():
    txt = open(os.path.join(PKG, "csrc", "sh_rot_tables.inc")).read()
    out = {}
    for name, body in re.findall(r"double (k\w+)\[[^\]]*\] = \{([^}]*)\}", txt):
        out[name] = np.array([float(v) for v in body.replace("\n", " ").split(",") if v.strip()])
    return out


def test_committed_tables_invert_the_basis_at_unit_directions():
    t = _tables()
    for l, ns in ((1, 3), (2, 10), (3, 14)):
        n = 2 * l + 1
        d, pinv = t[f"kShDir{l}"].reshape(ns, 3), t[f"kShPinv{l}"].reshape(n, ns)
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
        A = E.sh_basis(l, d)[:, l * l:]
        assert np.abs(pinv @ A - np.eye(n)).max() < 1e-14
        assert np.abs(pinv - np.linalg.pinv(A)).max() < 1e-14
        assert np.linalg.cond(A) < 4.0


# ------------------------------------------------------------------ C-ABI --
def test_abi_validates_before_any_hip_call():
    """No GPU here: every call below must return from its argument checks.  The non-null
    pointers are never dereferenced."""
    import ctypes
    from gsmpm import _lib
    L, p = _lib.LIB, 0x1000
    bad_cov = [(None, 4, p, p), (p, 4, None, p), (p, 4, p, None), (p, -1, p, p)]
    for cov, n, ls, q in bad_cov:
        assert L.gsmpm_cov_to_scale_rot(cov, n, ls, q, None, None) == _lib.GSMPM_EINVAL
        assert "gsmpm_cov_to_scale_rot" in _lib.last_error()
    bad_sh = [(None, p, 4, 3, 16, p), (p, None, 4, 3, 16, p), (p, p, 4, 3, 16, None), (p, p, -1, 3, 16, p),
              (p, p, 4, -1, 16, p), (p, p, 4, 4, 25, p), (p, p, 4, 3, 15, p), (p, p, 4, 1, 3, p), (p, p, 4, 0, 0, p)]
    for shs, Q, n, D, M, out in bad_sh:
        assert L.gsmpm_sh_rotate(shs, Q, n, D, M, out, None) == _lib.GSMPM_EINVAL, (n, D, M)
        assert "gsmpm_sh_rotate" in _lib.last_error()
    # n == 0: success, nothing launched (a launch would fail without a device)
    assert L.gsmpm_cov_to_scale_rot(p, 0, p, p, None, None) == _lib.GSMPM_OK
    assert L.gsmpm_sh_rotate(p, p, 0, 3, 16, p, None) == _lib.GSMPM_OK
    assert L.gsmpm_sh_rotate(p, p, 0, 3, 15, p, None) == _lib.GSMPM_EINVAL  # the shape is still checked


def test_package_exports_the_module():
    import gsmpm
    from gsmpm import export
    assert "export" in gsmpm.__all__
    assert all(callable(getattr(export, f)) for f in ("cov_to_scale_rot", "rotate_sh", "deformed_model"))


# ----------------------------------------------------------- flag and config --
def test_save_pcd_deformed_flag_and_export_config():
    from arguments import FillingParams, RenderParams

    def parse(cfg, argv):
        parser = ArgumentParser()
        r = RenderParams(parser, cfg["render"])
        return r.extract(parser.parse_args(argv))

    with open(os.path.join(PKG, "configs", "lego.json")) as f:
        lego = json.load(f)
    assert parse(lego, []).save_pcd_deformed is False
    assert parse(lego, ["--save_pcd"]).save_pcd_deformed is False
    assert parse(lego, ["--save_pcd", "--save_pcd_deformed"]).save_pcd_deformed is True
    with open(os.path.join(PKG, "configs", "lego-export.json")) as f:
        cfg = json.load(f)
    r = parse(cfg, [])
    assert r.save_pcd is True and r.save_pcd_deformed is True and r.rotate_sh is True
    assert FillingParams(cfg.get("particle_filling")).extract() is not None
