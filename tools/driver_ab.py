"""k_fused per launch with particle drivers (DESIGN.md "Particle drivers").

Lego 100k / 128^3; `Simulator.time_kernels` (the G2P + P2G launch, `reps`
back to back between two events, state restored) for each material of
  (a) the plain handle: k_fused<MAT, 3>;
  (b) a handle that holds a driver with no driver active: k_fused_drv<MAT, 3>,
      whose cost over (a) is the uniform test of the mask;
  (c) the same handle with the twist of the top fifth active: the indirect
      load of the selection word in every lane, the record loop in a fifth.
Each case is taken `--rounds` times, interleaved, after one untimed warm-up;
every timing is printed, then min / median / max.

    python tools/driver_ab.py [--n 100000] [--n_grid 128] [--rounds 5] [--reps 50] [--materials metal,jelly,fluid]

--uniform-only takes (a) alone: the form that also runs on a commit from
before the drivers, which is what (b) and (c) are to be compared against.
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
    ap.add_argument("--materials", default="metal,jelly,fluid")
    ap.add_argument("--uniform-only", action="store_true", help="case (a) alone")
    a = ap.parse_args()
    import numpy as np
    import torch
    from gsmpm.sim import Simulator
    from scenarios import lego_problem

    dev = torch.device("cuda:0")
    prob = lego_problem(a.n, a.n_grid)
    cfg = prob["cfg"]
    n = len(prob["x"])
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    z = prob["x"][:, 2]
    zmax, z80 = float(z.max()), float(np.quantile(z, 0.8))

    def make(material, driver):
        s = Simulator(n, n_grid=a.n_grid, material=material, E=cfg["E"], nu=cfg["nu"], density=cfg["density"],
                      gravity=cfg["gravity"])
        s.set_particles(t(prob["x"]), t(prob["cov"]), t(prob["vol"]))
        b = s.add_fixed_cube([1.0, 1.2, 0.5], [1.0, 0.8, 0.3])
        s.add_plane_collider([0, 0, 0.4], [0, 0, 1])
        d = None
        if driver:
            d = s.add_driver("enforce_particle_rotation", center=[1.0, 1.0, zmax], size=[1.0, 1.0, zmax - z80],
                             point=[1.0, 1.0, 1.0], axis=[0.0, 0.0, 1.0], omega=3.0, along=0.05)
        s.step(cfg["substep_dt"], [1 << b] * a.warm_substeps)
        return s, b, d

    sims = {}
    for m in a.materials.split(","):
        s, b, _ = make(m, False)
        sims[f"{m} a_plain"] = (s, 1 << b)
        if not a.uniform_only:
            s, b, d = make(m, True)
            sel = int(s.driver_selection(d).sum())
            sims[f"{m} b_driver_idle"] = (s, 1 << b)
            sims[f"{m} c_twist_active({sel})"] = (s, (1 << b) | (1 << d))
    dt = cfg["substep_dt"]
    for s, mask in sims.values():  # warm-up, untimed
        s.time_kernels(dt, mask, reps=a.reps)
    us = {k: [] for k in sims}
    for r in range(a.rounds):
        for k, (s, mask) in sims.items():
            us[k].append(1e3 * s.time_kernels(dt, mask, reps=a.reps)[0])
    print(json.dumps({"N": n, "n_grid": a.n_grid, "rounds": a.rounds, "reps": a.reps, "unit": "us per k_fused launch"}))
    for k, v in us.items():
        print(f"{k:28s} " + " ".join(f"{q:8.2f}" for q in v) +
              f"   min {min(v):8.2f} median {statistics.median(v):8.2f} max {max(v):8.2f}")


if __name__ == "__main__":
    main()
