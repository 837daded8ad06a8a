"""Float64 reference (torch on the CPU) of the differentiable MPM: the six
kernels of the fitting path written from the formulas (utils.py:56-76
compute_stress_from_F_opt, 136-174 p2g_opt, 177-183
grid_normalization_and_gravity + boundary_conditions.py:23-27, 284-347
g2p_opt, 349-362 compute_mu_lam_from_E_nu, 435-467 compute_cov_from_F_opt),
their adjoints taken with torch.autograd.grad kernel by kernel in the order
of solver.py:71-90, and the input classes shared by test_fit_ref_oracle.py and
test_gpu_fit_ref.py.

Nothing comes from oracle/ and nothing from device code.  Every sum, product
and division is float64.  Taken in f32 (as float64 values) is what the library
stores in f32: dx, inv_dx, dt, dt*g, the constants 1e-2, 1e-15, 0.49, the
learning rates, the cube's centre and half-size; and the discrete decisions:
the base cell int(f32(x * inv_dx) - 0.5f) and the cube's node predicate.

A reverse-mode kernel of the reference reads the adjoint fields of its
outputs and adds into the adjoint fields of its inputs; FitRef.backward does
exactly that with the accumulators it holds, so the reference's behaviours
are statements about what is a constant and what is cleared:
  * m is a constant in p2g and in the grid update (no mass adjoint);
  * v_in.grad += v_out.grad / m on every node with m > 1e-15, the nodes
    inside the fixed cube included: the cube only zeroes the forward v_out;
  * sign(J) and the clamped value are constants (no dJ term when |J| < 1e-2);
  * the grid accumulators are cleared by clear_grads alone;
  * mu_lam's product runs every substep on the accumulated gmu / glam;
  * cov's adjoint sees the six stored upper entries.
Four constructor flags flip one behaviour each (the mutation checks of
test_fit_ref_oracle.py).
"""
from __future__ import annotations

import math

import numpy as np
import torch

F32 = np.float32
T64 = torch.float64
STICKY_GROUND = ((1.0, 0.6, 1.0), (1.0, 0.1, 1.0))  # boundary_conditions.py:88-95
LEVELED = {"x": 3, "v": 3, "F": 9, "C": 9, "stress": 9}
_OFF = torch.tensor([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], dtype=torch.long)


def f32(a):
    """The f32 value(s) of `a`, as float64."""
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def t64(a, shape=None):
    t = torch.from_numpy(np.array(a, np.float64))
    return t if shape is None else t.reshape(shape)


# ------------------------------------------------------------- measures --
def field_err(a, r):
    """max|a - r| / max|r| (0 / 0 = 0)."""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    d, s = np.abs(a - r).max(), np.abs(r).max()
    return 0.0 if d == 0 else float(d / s) if s > 0 else math.inf


def elem_err(a, r, scale=None):
    """max over entries of |a - r| / (|r| + 1e-3 max|r|); `scale` replaces |r|
    (a sum's |terms|, for sums that cancel)."""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    s = np.abs(r) if scale is None else np.asarray(scale, np.float64).reshape(r.shape)
    d = np.abs(a - r)
    if d.max() == 0:
        return 0.0
    den = s + 1e-3 * s.max()
    return float((d / den).max()) if s.max() > 0 else math.inf


# ------------------------------------------------------------- geometry --
class Grid:
    """n_grid^3 nodes over grid_extent; `nodes`: None (all of them, dense
    arrays) or a sorted tensor of node ids the arrays are restricted to."""

    def __init__(self, n_grid, grid_extent=2.0, gravity=(0.0, -9.81, 0.0), cube=None):
        self.ng = int(n_grid)
        self.dx32, self.inv_dx32 = F32(grid_extent / n_grid), F32(n_grid / grid_extent)
        self.dx, self.inv_dx = float(self.dx32), float(self.inv_dx32)
        self.g32 = np.array(gravity, F32)
        self.cube = None if cube is None else (np.array(cube[0], F32), np.array(cube[1], F32))
        self.m_eps = float(F32(1e-15))

    def base(self, x):
        x32 = x.detach().numpy().astype(F32)
        gp = (x32 * self.inv_dx32).astype(F32)
        return torch.from_numpy((gp - F32(0.5)).astype(F32).astype(np.int64))  # truncation toward zero

    def in_cube(self, ids):
        """The f32 predicate |f32(i) * dx - c| < s on all axes, per node id."""
        if self.cube is None:
            return torch.zeros(len(ids), dtype=torch.bool)
        ids = np.asarray(ids, np.int64)
        ijk = np.stack([ids // (self.ng * self.ng), (ids // self.ng) % self.ng, ids % self.ng], 1)
        p = (ijk.astype(F32) * self.dx32).astype(F32)
        return torch.from_numpy((np.abs((p - self.cube[0][None]).astype(F32)) < self.cube[1][None]).all(1))

    def stencil(self, x):
        """weight [n, 27], grad weight [n, 27, 3], dpos in cells [n, 27, 3],
        dense node id [n, 27]; differentiable in x through fx."""
        base = self.base(x)
        fx = x * self.inv_dx - base
        w = torch.stack([0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1.0) ** 2, 0.5 * (fx - 0.5) ** 2], 1)  # [n, offset, axis]
        dw = torch.stack([fx - 1.5, -2.0 * (fx - 1.0), fx - 0.5], 1)
        a, b, c = _OFF[:, 0], _OFF[:, 1], _OFF[:, 2]
        wx, wy, wz = w[:, a, 0], w[:, b, 1], w[:, c, 2]
        dx_, dy_, dz_ = dw[:, a, 0], dw[:, b, 1], dw[:, c, 2]
        weight = wx * wy * wz
        gw = self.inv_dx * torch.stack([dx_ * wy * wz, wx * dy_ * wz, wx * wy * dz_], -1)
        dpos = _OFF[None].to(T64) - fx[:, None, :]
        node = base[:, None, :] + _OFF[None]
        assert int(node.min()) >= 0 and int(node.max()) < self.ng, "a stencil leaves the grid: the reference is undefined"
        lin = (node[..., 0] * self.ng + node[..., 1]) * self.ng + node[..., 2]
        return weight, gw, dpos, lin

    def touched(self, x):
        return torch.unique(self.stencil(x)[3])

    def size(self, nodes):
        return self.ng ** 3 if nodes is None else len(nodes)

    def index(self, lin, nodes):
        return lin if nodes is None else torch.searchsorted(nodes, lin)

    def ids(self, nodes):
        return np.arange(self.ng ** 3) if nodes is None else nodes.numpy()


# -------------------------------------------------------------- kernels --
def mu_lam(logE, y):
    E = torch.pow(torch.tensor(10.0, dtype=T64), logE)
    nu = float(F32(0.49)) / (1.0 + torch.exp(-y))
    return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))


def stress(F, mu, lam, clamp_has_dJ=False):
    """sigma = F S F^T / J, S = 2 mu E + lam tr(E) I, E = (F^T F - I) / 2,
    |J| < 1e-2 replaced by 1e-2 sign(J), a constant."""
    J = torch.linalg.det(F)
    c = float(F32(1e-2))
    clamped = J.detach().abs() < c
    held = c * torch.sign(J.detach())
    Jc = torch.where(clamped, J + (held - J).detach() if clamp_has_dJ else held, J)
    eye = torch.eye(3, dtype=T64)
    E = 0.5 * (F.transpose(1, 2) @ F - eye)
    tr = E.diagonal(dim1=1, dim2=2).sum(1)
    S = 2.0 * mu[:, None, None] * E + (lam * tr)[:, None, None] * eye
    return F @ S @ F.transpose(1, 2) / Jc[:, None, None]


def p2g(G, x, v, C, sig, mass, vol, dt, nodes=None):
    """v_in [nodes, 3], m [nodes]."""
    weight, gw, dpos, lin = G.stencil(x)
    idx = G.index(lin, nodes).reshape(-1)
    wm = weight * mass[:, None]
    cd = torch.einsum("nrc,nac->nar", C, dpos * G.dx)
    ef = -vol[:, None, None] * torch.einsum("nrc,nac->nar", sig, gw)
    term = wm[..., None] * (v[:, None, :] + cd) + dt * ef
    v_in = torch.zeros(G.size(nodes), 3, dtype=T64).index_add(0, idx, term.reshape(-1, 3))
    m = torch.zeros(G.size(nodes), dtype=T64).index_add(0, idx, wm.reshape(-1))
    return v_in, m


def grid(G, v_in, m, dt, nodes=None, bc_blocks_adjoint=False):
    """v_out = v_in / m + dt g where m > 1e-15, else 0; 0 inside the cube.
    The cube stores a constant over v_out: by default its adjoint is nothing,
    and the normalisation's adjoint still reaches v_in there."""
    live = m.detach() > G.m_eps
    dtg = t64(f32(F32(dt) * G.g32))
    safe = torch.where(live, m, torch.ones_like(m))
    v = torch.where(live[:, None], v_in / safe[:, None] + dtg, torch.zeros_like(v_in))
    inc = G.in_cube(G.ids(nodes))[:, None]
    if bc_blocks_adjoint:
        return torch.where(inc, torch.zeros_like(v), v)
    return v - (v * inc).detach()


def g2p(G, x, F, v_out, dt, nodes=None):
    """x1, v1, C1, F1 of level s + 1."""
    weight, gw, dpos, lin = G.stencil(x)
    gv = v_out[G.index(lin, nodes)]  # [n, 27, 3]
    nv = (gv * weight[..., None]).sum(1)
    nC = torch.einsum("nar,nac->nrc", gv * (weight * G.inv_dx * 4.0)[..., None], dpos)
    nF = torch.einsum("nar,nac->nrc", gv, gw)
    return x + dt * nv, nv, nC, (torch.eye(3, dtype=T64) + dt * nF) @ F


def g2p_scatter_terms(G, x, F, gx1, gv1, gC1, gF1, dt, nodes=None):
    """What g2p's adjoint adds to v_out.grad, node by node: (sum of the
    particles' terms, sum of their magnitudes).  The second is the scale an
    error of the first is relative to."""
    weight, gw, dpos, lin = G.stencil(x.detach())
    idx = G.index(lin, nodes).reshape(-1)
    g_nv = gv1 + dt * gx1
    g_nF = dt * gF1 @ F.detach().transpose(1, 2)
    term = (weight[..., None] * g_nv[:, None, :]
            + (weight * G.inv_dx * 4.0)[..., None] * torch.einsum("nrc,nac->nar", gC1, dpos)
            + torch.einsum("nrc,nac->nar", g_nF, gw)).reshape(-1, 3)
    z = torch.zeros(G.size(nodes), 3, dtype=T64)
    return z.index_add(0, idx, term), z.index_add(0, idx, term.abs())


def cov(F, init_cov):
    a = init_cov
    A = torch.stack([a[:, 0], a[:, 1], a[:, 2], a[:, 1], a[:, 3], a[:, 4], a[:, 2], a[:, 4], a[:, 5]], 1).reshape(-1, 3, 3)
    M = F @ A @ F.transpose(1, 2)
    return torch.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# ---------------------------------------------------------------- state --
class FitRef:
    """The levelled fields, every adjoint accumulator and the API of
    MPM_Simulator(fitting=True).  `sparse`: grid arrays live on the nodes the
    level's particles touch (one forward / backward pair; for grids too large
    for dense float64 arrays)."""

    def __init__(self, x, cov6, vol, *, n_grid, grid_extent=2.0, E=2e6, nu=0.4, density=1000.0,
                 gravity=(0.0, -9.81, 0.0), init_v=None, levels=31, ground_only=False, sparse=False,
                 mass_adjoint=False, bc_blocks_adjoint=False, clamp_has_dJ=False,
                 clear_grid_adjoints_each_substep=False):
        x = np.ascontiguousarray(x, F32).reshape(-1, 3)
        n, L = len(x), int(levels)
        self.n, self.L, self.sparse = n, L, sparse
        self.G = Grid(n_grid, grid_extent, gravity, STICKY_GROUND if ground_only else None)
        self.mass_adjoint, self.bc_blocks_adjoint = mass_adjoint, bc_blocks_adjoint
        self.clamp_has_dJ, self.clear_each = clamp_has_dJ, clear_grid_adjoints_each_substep
        z = lambda *s: torch.zeros(*s, dtype=T64)
        self.x = [z(n, 3) for _ in range(L)]
        self.v = [z(n, 3) for _ in range(L)]
        self.F = [z(n, 3, 3) for _ in range(L)]
        self.C = [z(n, 3, 3) for _ in range(L)]
        self.stress = [z(n, 3, 3) for _ in range(L)]
        self.x[0] = t64(x)
        if init_v is not None:
            self.v[0] = t64(np.asarray(init_v, F32), (n, 3))
        self.F[0] = torch.eye(3, dtype=T64).repeat(n, 1, 1)
        self.vol = t64(np.asarray(vol, F32), (n,))
        self.mass = t64(f32(F32(density) * np.asarray(vol, F32).reshape(n)))
        self.logE = t64(np.full(n, F32(math.log10(E))))
        self.y = t64(np.full(n, F32(-math.log(0.49 / nu - 1.0))))
        self.init_cov = t64(np.asarray(cov6, F32), (n, 6))
        self.cov = self.init_cov.clone()
        self.nodes = None
        self.m = self.v_in = self.v_out = None
        self.g_v_in = self.g_v_out = self.g_v_out_scale = None
        self.mu_lam()
        self.clear_grads()

    # -- state access, [n, w] float64 numpy out, anything f32-valued in
    def set(self, field, a, level=0):
        a = np.asarray(a, F32)
        if field in LEVELED or field in ("gx", "gv", "gF", "gC", "gstress"):
            w = LEVELED[field[1:] if field[0] == "g" else field]
            getattr(self, field)[level] = t64(a, (self.n, 3) if w == 3 else (self.n, 3, 3))
        else:
            setattr(self, field, t64(a, (self.n, 6) if field in ("gcov", "init_cov") else (self.n,)))

    def get(self, field, level=0):
        t = getattr(self, field)
        t = t[level] if isinstance(t, list) else t
        return t.detach().numpy().reshape(self.n, -1) if t.dim() > 1 else t.detach().numpy()

    def mu_lam(self):
        self.mu, self.lam = mu_lam(self.logE, self.y)

    # -- forward
    def _grid_of(self, dt, s, sig):
        if self.sparse:
            self.nodes = self.G.touched(self.x[s])
        v_in, m = p2g(self.G, self.x[s], self.v[s], self.C[s], sig, self.mass, self.vol, dt, self.nodes)
        v_out = grid(self.G, v_in, m, dt, self.nodes)
        self.m, self.v_in, self.v_out = m, v_in, v_out
        return v_out

    def forward(self, dt, s):
        dt = float(F32(dt))
        self.stress[s] = stress(self.F[s], self.mu, self.lam)
        v_out = self._grid_of(dt, s, self.stress[s])
        self.x[s + 1], self.v[s + 1], self.C[s + 1], self.F[s + 1] = g2p(self.G, self.x[s], self.F[s], v_out, dt, self.nodes)

    def postprocess_forward(self):
        self.cov = cov(self.F[self.L - 1], self.init_cov)

    # -- backward: each kernel's vector-Jacobian product, solver.py:71-90
    def backward(self, dt, s):
        """Returns the per-node scale of this substep's v_out.grad sum
        (also accumulated in g_v_out_scale)."""
        dt = float(F32(dt))
        v_out = self._grid_of(dt, s, self.stress[s])  # the redo of p2g + grid update with the stored stress
        G, nodes = self.G, self.nodes
        size = G.size(nodes)
        if self.g_v_in is None or self.clear_each:
            self.g_v_in, self.g_v_out = torch.zeros(size, 3, dtype=T64), torch.zeros(size, 3, dtype=T64)
            self.g_v_out_scale = torch.zeros(size, 3, dtype=T64)
        assert len(self.g_v_in) == size, "sparse: one backward per clear_grads (the node set follows the level)"
        grad = torch.autograd.grad
        # g2p_opt.grad
        x0, F0, vo = _leaf(self.x[s]), _leaf(self.F[s]), _leaf(v_out)
        cot = [self.gx[s + 1], self.gv[s + 1], self.gC[s + 1], self.gF[s + 1]]
        a, b, c = grad(g2p(G, x0, F0, vo, dt, nodes), [x0, F0, vo], cot)
        terms, scale = g2p_scatter_terms(G, self.x[s], self.F[s], *cot, dt, nodes)
        assert float((c - terms).abs().max()) <= 1e-12 * max(float(scale.max()), 1e-300)  # the explicit terms are the product
        self.gx[s] = self.gx[s] + a
        self.gF[s] = self.gF[s] + b
        self.g_v_out = self.g_v_out + c
        self.g_v_out_scale = self.g_v_out_scale + scale
        # grid_normalization_and_gravity.grad; BasicBC.apply.grad
        vi, mi = _leaf(self.v_in), _leaf(self.m)
        vo2 = grid(G, vi, mi if self.mass_adjoint else mi.detach(), dt, nodes, self.bc_blocks_adjoint)
        if self.mass_adjoint:
            a, g_m = grad(vo2, [vi, mi], self.g_v_out)
        else:
            (a,), g_m = grad(vo2, [vi], self.g_v_out), None
        self.g_v_in = self.g_v_in + a
        # p2g_opt.grad
        x0, v0, C0, S0 = _leaf(self.x[s]), _leaf(self.v[s]), _leaf(self.C[s]), _leaf(self.stress[s])
        v_in, m = p2g(G, x0, v0, C0, S0, self.mass, self.vol, dt, nodes)
        outs, cots = ([v_in, m], [self.g_v_in, g_m]) if self.mass_adjoint else ([v_in], [self.g_v_in])
        a, b, c, d = grad(outs, [x0, v0, C0, S0], cots)
        self.gx[s] = self.gx[s] + a
        self.gv[s] = self.gv[s] + b
        self.gC[s] = self.gC[s] + c
        self.gstress[s] = self.gstress[s] + d
        # compute_stress_from_F_opt.grad
        F0, mu, lam = _leaf(self.F[s]), _leaf(self.mu), _leaf(self.lam)
        a, b, c = grad(stress(F0, mu, lam, self.clamp_has_dJ), [F0, mu, lam], self.gstress[s])
        self.gF[s] = self.gF[s] + a
        self.gmu = self.gmu + b
        self.glam = self.glam + c
        # compute_mu_lam_from_E_nu.grad, on the accumulated gmu / glam
        e, y = _leaf(self.logE), _leaf(self.y)
        a, b = grad(list(mu_lam(e, y)), [e, y], [self.gmu, self.glam])
        self.glogE = self.glogE + a
        self.gy = self.gy + b
        return scale

    def postprocess_backward(self):
        F = _leaf(self.F[self.L - 1])
        (a,) = torch.autograd.grad(cov(F, self.init_cov), [F], self.gcov)
        self.gF[self.L - 1] = self.gF[self.L - 1] + a

    def set_grads(self, xyz_grad, cov_grad):
        self.gx[self.L - 1] = t64(np.asarray(xyz_grad, F32), (self.n, 3))
        self.gcov = t64(np.asarray(cov_grad, F32), (self.n, 6))

    def clear_grads(self):
        n, L = self.n, self.L
        z = lambda *s: torch.zeros(*s, dtype=T64)
        self.gx = [z(n, 3) for _ in range(L)]
        self.gv = [z(n, 3) for _ in range(L)]
        self.gF = [z(n, 3, 3) for _ in range(L)]
        self.gC = [z(n, 3, 3) for _ in range(L)]
        self.gstress = [z(n, 3, 3) for _ in range(L)]
        self.gmu, self.glam, self.glogE, self.gy, self.gcov = z(n), z(n), z(n), z(n), z(n, 6)
        self.g_v_in = self.g_v_out = self.g_v_out_scale = None

    def learn(self):
        """solver.py:92-108: SGD on adjoints clipped to [-1, 1]."""
        clip = lambda g: torch.where(g.abs() > 1.0, torch.sign(g), g)
        self.logE = self.logE - float(F32(0.8)) * clip(self.glogE)
        self.y = self.y - float(F32(1.6)) * clip(self.gy)

    def cycle_init(self):
        """model.py:216-223: the last level becomes level 0."""
        for k in LEVELED:
            f = getattr(self, k)
            f[0] = f[self.L - 1].clone()

    def grid_adjoint(self, which):
        """g_v_in / g_v_out / g_v_out_scale as numpy [nodes, 3] (zeros before the first backward)."""
        t = getattr(self, which)
        return np.zeros((self.G.size(self.nodes), 3)) if t is None else t.numpy()

    def grid_field(self, which):
        """mass [nodes] or v_in / v_out / v_in_grad / v_out_grad [nodes, 3], as the device's get_grid names them."""
        if which in ("v_in_grad", "v_out_grad"):
            return self.grid_adjoint({"v_in_grad": "g_v_in", "v_out_grad": "g_v_out"}[which])
        return {"mass": self.m, "v_in": self.v_in, "v_out": self.v_out}[which].detach().numpy()


# ---------------------------------------------------------- input classes --
DT = 1e-3
GRAV = (0.0, -9.81, 0.0)
MAT = dict(E=1e5, nu=0.3, density=1000.0)
EXT = 2.0
CLASSES = ("interior", "box", "clamp", "face", "dense", "corner", "ragged1", "ragged257", "ragged1003")
GRID_OF = {"interior": 16, "box": 32, "clamp": 16, "face": 16, "dense": 32, "corner": 32,
           "ragged1": 16, "ragged257": 16, "ragged1003": 16}
_SEED = {k: 100 + i for i, k in enumerate(CLASSES)}
FWD_FIELDS = ("x1", "v1", "C1", "F1", "stress", "mass", "v_in", "v_out", "mu", "lam")
BWD_FIELDS = ("gx", "gv", "gC", "gF", "gstress", "gmu", "glam", "glogE", "gy", "v_in_grad", "v_out_grad")
MODEL_ADJ = ("gmu", "glam", "glogE", "gy")
LEVEL_ADJ = ("gx", "gv", "gC", "gF", "gstress")


def volumes(x, n_grid, grid_extent=EXT):
    """Cell volume over the number of particles in the particle's cell (filling.py:27-42)."""
    dx = grid_extent / n_grid
    c = np.floor(np.asarray(x, np.float64) / dx).astype(np.int64)
    key = (c[:, 0] * n_grid + c[:, 1]) * n_grid + c[:, 2]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return (dx ** 3 / cnt[inv]).astype(F32)


class Case(dict):
    __getattr__ = dict.__getitem__


def make_case(name, n_grid=None):
    """The f32 inputs of one class: x, v, C, F at level s, per-particle logE
    and y, cov, vol, and the cotangents gx, gv, gF, gC seeded at level s + 1."""
    ng = GRID_OF[name] if n_grid is None else n_grid
    rng = np.random.default_rng(_SEED[name] + 1000 * ng)
    inv_dx = ng / EXT
    blob = lambda n: rng.uniform(0.8, 1.2, (n, 3)) + np.array([0.0, 0.2, 0.0])
    if name == "interior":
        x = blob(400)
    elif name.startswith("ragged"):
        x = blob(int(name[6:]))
    elif name == "box":
        x = blob(400) - np.array([0.0, 0.55, 0.0])  # y in [0.45, 0.85]: into the sticky ground's cube, y in (0.5, 0.7)
    elif name == "clamp":
        x = blob(399)
    elif name == "face":
        x = rng.uniform(0.8, 1.2, (399, 3))  # centred: the pushed-out particles below stay 3 cells from the faces
        gp = x * inv_dx
        k = np.arange(133)  # the first third: one coordinate a little inside a stencil change
        ax = k % 3
        delta = rng.uniform(1e-3, 1e-2, 133) * np.where(rng.random(133) < 0.5, 1.0, -1.0)
        h = np.floor(gp[k, ax]) + 0.5
        # the first 24 sit one cell outside the blob with generic other axes well inside a cell: their far
        # node plane is touched by nobody else and carries weight delta^2 / 2
        far = k < 24
        h[far] = np.where(delta[far] > 0, np.floor(gp[:, ax[far]].max(0)) + 1.5, np.floor(gp[:, ax[far]].min(0)) - 0.5)
        for a in range(3):
            other = far & (ax != a)
            gp[k[other], a] = np.floor(gp[k[other], a]) + rng.uniform(0.2, 0.8, other.sum())
        gp[k, ax] = h + delta
        x = gp / inv_dx
    elif name == "dense":
        x = rng.uniform(10.0, 12.0, (700, 3)) / inv_dx  # two cells wide, base cells 9..11: inside tile (1, 1, 1)
    elif name == "corner":
        x = rng.uniform(7.5, 9.5, (304, 3)) / inv_dx  # base cells 7 and 8 on every axis: the corner shared by 8 tiles
    else:
        raise KeyError(name)
    x = x.astype(F32)
    n = len(x)
    N = lambda *s: rng.standard_normal(s)
    F = (np.eye(3).reshape(1, 9) + 0.05 * N(n, 9)).astype(F32)
    if name == "clamp":
        # the first row scaled so that det F is the target: thirds at +0.008, -0.009 and as drawn (about 1)
        F3 = F.astype(np.float64).reshape(n, 3, 3)
        third = np.arange(n) % 3
        target = np.where(third == 0, 0.008, -0.009) * rng.uniform(0.97, 1.03, n)
        a = np.where(third == 2, 1.0, target / np.linalg.det(F3))
        F3[:, 0, :] *= a[:, None]
        F = F3.reshape(n, 9).astype(F32)
    c = Case(name=name, n_grid=ng, n=n, x=x, v=(0.5 * N(n, 3)).astype(F32), C=(0.5 * N(n, 9)).astype(F32), F=F,
             cov=(np.array([1e-3, 2e-4, 0, 1e-3, 1e-4, 1e-3]) * rng.uniform(0.5, 1.5, (n, 1))).astype(F32),
             vol=volumes(x, ng),
             logE=(math.log10(MAT["E"]) + rng.uniform(-0.5, 0.5, n)).astype(F32),
             y=(-math.log(0.49 / MAT["nu"] - 1.0) + rng.uniform(-0.5, 0.5, n)).astype(F32))
    spread = 10.0 ** rng.uniform(-3, 3, (n, 1)) if name == "dense" else 1.0
    for k, w in (("gx", 3), ("gv", 3), ("gF", 9), ("gC", 9)):
        g = N(n, w)
        c[k] = ((np.abs(g) if name == "dense" else g) * spread).astype(F32)
    return c


def new_ref(c, levels=2, **flags):
    return FitRef(c.x, c.cov, c.vol, n_grid=c.n_grid, grid_extent=EXT, gravity=GRAV, init_v=c.v, levels=levels,
                  ground_only=True, **MAT, **flags)


# ----------------------------------------- drivers, generic over the three --
# `sim` is FitRef or an adapter with its methods: set / get / grid_field /
# mu_lam / forward / backward / clear_grads / ...
def seed_state(sim, c, s=0):
    for k in ("x", "v", "C", "F"):
        sim.set(k, c[k], s)
    sim.set("logE", c.logE)
    sim.set("y", c.y)
    sim.mu_lam()


def seed_cotangents(sim, c, level):
    for k in ("gx", "gv", "gF", "gC"):
        sim.set(k, c[k], level)


def forward_fields(sim, s=0):
    out = {k + "1": sim.get(k, s + 1) for k in ("x", "v", "C", "F")}
    out["stress"] = sim.get("stress", s)
    out.update({k: sim.grid_field(k) for k in ("mass", "v_in", "v_out")})
    out.update(mu=sim.get("mu"), lam=sim.get("lam"))
    return out


def backward_fields(sim, levels):
    """Every level's adjoints ([level, n, w]), the model adjoints, both grid adjoint fields."""
    out = {k: np.stack([sim.get(k, l) for l in levels]) for k in LEVEL_ADJ}
    out.update({k: sim.get(k) for k in MODEL_ADJ})
    out.update({k: sim.grid_field(k) for k in ("v_in_grad", "v_out_grad")})
    return out


def one_substep(sim, c):
    """forward(0), then the cotangents at level 1 through `set` (on the
    device that drops the stored grid: the recompute path) and backward(0)."""
    seed_state(sim, c)
    sim.forward(DT, 0)
    fwd = forward_fields(sim)
    sim.clear_grads()
    seed_cotangents(sim, c, 1)
    sim.backward(DT, 0)
    return fwd, backward_fields(sim, (0,))


def three_substeps(sim, c, through_set_grads=False):
    """levels = 4: forward 0, 1, 2; seed level 3; backward 2, 1, 0, the
    adjoints collected after each."""
    seed_state(sim, c)
    for s in range(3):
        sim.forward(DT, s)
    fwd = {k + "3": sim.get(k, 3) for k in ("x", "v", "C", "F")}
    sim.clear_grads()
    if through_set_grads:
        sim.postprocess_forward()
        fwd["cov"] = sim.get("cov")
        sim.set_grads(c.gx, 100.0 * c.gF[:, :6])
        sim.postprocess_backward()
    else:
        seed_cotangents(sim, c, 3)
    steps = []
    for s in (2, 1, 0):
        sim.backward(DT, s)
        steps.append(backward_fields(sim, range(4)))
    return fwd, steps


def accumulation(sim, c):
    """Adjoints already present at level s and on the model before
    backward(s), then a second backward(s) without clear_grads."""
    seed_state(sim, c)
    sim.forward(DT, 0)
    sim.clear_grads()
    seed_cotangents(sim, c, 1)
    rng = np.random.default_rng(5)
    for k, w in (("gx", 3), ("gv", 3), ("gF", 9), ("gC", 9), ("gstress", 9)):
        sim.set(k, rng.standard_normal((c.n, w)).astype(F32), 0)
    sim.set("gmu", (1e-4 * rng.standard_normal(c.n)).astype(F32))
    sim.set("glam", (1e-4 * rng.standard_normal(c.n)).astype(F32))
    steps = []
    for _ in range(2):
        sim.backward(DT, 0)
        steps.append(backward_fields(sim, (0,)))
    return steps


def postprocess_path(sim, c):
    """levels = 2, no `set` between the passes: forward, cov, set_grads,
    cov's adjoint, backward (on the device: the grid stored by forward)."""
    seed_state(sim, c)
    sim.forward(DT, 0)
    sim.postprocess_forward()
    fwd = forward_fields(sim)
    fwd["cov"] = sim.get("cov")
    sim.clear_grads()
    sim.set_grads(c.gx, 100.0 * c.gF[:, :6])
    sim.postprocess_backward()
    gF1 = sim.get("gF", 1)
    sim.backward(DT, 0)
    bwd = backward_fields(sim, (0,))
    bwd["gF1"] = gF1
    return fwd, bwd


def compare(got, ref, scale=None):
    """{field: (field_err, elem_err)}; v_out_grad's elem_err is relative to `scale` (the |terms| sums)."""
    return {k: (field_err(got[k], ref[k]), elem_err(got[k], ref[k], scale if k == "v_out_grad" else None))
            for k in ref if k in got}


def worst(errs):
    """Field-wise maximum of several compare() results."""
    out = {}
    for e in errs:
        for k, (a, b) in e.items():
            out[k] = (max(a, out.get(k, (0, 0))[0]), max(b, out.get(k, (0, 0))[1]))
    return out


def within(errs, bounds):
    return [(k, e, bounds[k]) for k, e in errs.items() if e[0] > bounds[k][0] or e[1] > bounds[k][1]]
