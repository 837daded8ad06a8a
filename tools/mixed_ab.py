"""k_fused per launch, uniform against mixed mode (DESIGN.md "Mixed materials").

Lego 100k / 128^3, created as metal; `Simulator.time_kernels` (the G2P + P2G
launch, `reps` back to back between two events, state restored) for
  (a) the uniform simulator: k_fused<1, 3>;
  (b) mixed mode with every id metal: the cost of the fast path alone;
  (c) the `regions` layout: id = quartile of x (jelly, metal, sand, foam);
  (d) the `salt` layout: a random id per particle (the divergent worst case);
and, for (c), the uniform simulator of each material.  Each case is taken
`--rounds` times, interleaved, after one untimed warm-up; every timing is
printed, then min / median / max.

    python tools/mixed_ab.py [--n 100000] [--n_grid 128] [--rounds 5] [--reps 50]

--uniform-only takes (a) alone: the form that also runs on a commit from
before mixed mode, to check that a uniform scene's kernel did not change.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gaussian-splatting-mpm_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--n_grid", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm_substeps", type=int, default=20, help="substeps before timing (a deformed, loaded state)")
    ap.add_argument("--uniform-only", action="store_true", help="case (a) alone")
    a = ap.parse_args()
    import numpy as np
    import torch
    from gsmpm.sim import MATERIALS, Simulator
    from scenarios import lego_problem

    dev = torch.device("cuda:0")
    prob = lego_problem(a.n, a.n_grid)
    cfg = prob["cfg"]
    n = len(prob["x"])
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    x = prob["x"][:, 0]
    layouts = {
        "b_mixed_all_metal": np.full(n, 1.0, np.float32),
        "c_regions": np.clip(np.floor(4.0 * (x - x.min()) / (x.max() - x.min())), 0, 3).astype(np.float32),
        "d_salt": np.random.default_rng(5).integers(0, 4, size=n).astype(np.float32),
    }

    def make(material, ids=None):
        s = Simulator(n, n_grid=a.n_grid, material=material, E=cfg["E"], nu=cfg["nu"], density=cfg["density"],
                      gravity=cfg["gravity"])
        s.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
        b = s.add_fixed_cube([1.0, 1.2, 0.5], [1.0, 0.8, 0.3])
        s.add_plane_collider([0, 0, 0.4], [0, 0, 1])
        if ids is not None:
            s.set("material", t(ids))
        s.step(cfg["substep_dt"], [1 << b] * a.warm_substeps)
        return s, 1 << b

    sims = {"a_uniform_metal": make("metal")}
    if not a.uniform_only:
        for k, ids in layouts.items():
            sims[k] = make("metal", ids)
        for m in ("jelly", "sand", "foam"):
            sims["uniform_" + m] = make(m)
        assert sims["a_uniform_metal"][0].material_mode == 0 and sims["c_regions"][0].material_mode == 1
    dt = cfg["substep_dt"]
    for s, mask in sims.values():  # warm-up, untimed
        s.time_kernels(dt, mask, reps=a.reps)
    us = {k: [] for k in sims}
    for r in range(a.rounds):
        for k, (s, mask) in sims.items():
            us[k].append(1e3 * s.time_kernels(dt, mask, reps=a.reps)[0])
    print(json.dumps({"N": n, "n_grid": a.n_grid, "rounds": a.rounds, "reps": a.reps, "unit": "us per k_fused launch",
                      "material_codes": MATERIALS}))
    for k, v in us.items():
        print(f"{k:20s} " + " ".join(f"{q:8.2f}" for q in v) +
              f"   min {min(v):8.2f} median {statistics.median(v):8.2f} max {max(v):8.2f}")
    if a.uniform_only:
        return
    ua = us["a_uniform_metal"]
    spread = max(ua) - min(ua)
    print(f"(b) - (a) medians: {statistics.median(us['b_mixed_all_metal']) - statistics.median(ua):+.2f} us; "
          f"spread of (a): {spread:.2f} us; 5 % of (a): {0.05 * statistics.median(ua):.2f} us")


if __name__ == "__main__":
    main()
