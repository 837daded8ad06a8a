"""Chunk histogram of the bench scene over its frames (CPU only).

Builds the scene bench.py times (seeded synthetic Gaussians, world2grid, the
config's fixed cubes and the ground plane), runs it on the CPU oracle's
OpenMP build frame by frame, and at the chosen frames bins the particles
into the fused pipeline's 8x8x7 tiles by base cell, as k_bin_all_f does: the
owner tiles, their <= 256-particle chunks, the tiles by chunk count, the
share of particles in tiles of >= 2 and >= 3 chunks, and vmax.  This is the
state k_grid_f's cover gather sees at each frame: a tile of c chunks makes
every node it covers sum c windows.

Usage: python tools/chunk_hist.py [--particles 100000] [--n_grid 128]
       [--config lego.json] [--frames 0,5,8,10,12,25] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

T = (8, 8, 7)  # kFT0..2
CHUNK = 256


def tile_stats(x, v, n_grid, extent):
    inv_dx = np.float32(n_grid / extent)
    base = (x.astype(np.float32) * inv_dx - np.float32(0.5)).astype(np.int64)  # truncation, as base_of()
    t3 = base // np.array(T)
    td = [(n_grid + T[d] - 1) // T[d] for d in range(3)]
    tid = (t3[:, 0] * td[1] + t3[:, 1]) * td[2] + t3[:, 2]
    counts = np.unique(tid, return_counts=True)[1]
    nch = (counts + CHUNK - 1) // CHUNK
    hist = np.bincount(nch)
    n = len(x)
    return {"tiles": len(counts), "chunks": int(nch.sum()),
            "by_chunks": {int(c): int(hist[c]) for c in range(1, len(hist)) if hist[c]},
            "ge2": float(counts[nch >= 2].sum()) / n, "ge3": float(counts[nch >= 3].sum()) / n,
            "max_per_tile": int(counts.max()), "vmax": float(np.abs(v).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--n_grid", type=int, default=128)
    ap.add_argument("--config", default="lego.json")
    ap.add_argument("--frames", default="0,5,8,10,12,25")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scenarios import build_oracle_sim, lego_problem, oracle_run
    frames = sorted(int(f) for f in a.frames.split(","))
    os.environ.setdefault("OMP_NUM_THREADS", str(len(os.sched_getaffinity(0))))
    prob = lego_problem(a.particles, a.n_grid, config=a.config)
    cfg = prob["cfg"]
    sim, imps, ops = build_oracle_sim(prob, jelly_quirk=not cfg.get("jelly_fcr", False), threaded="fast")
    dt, ext = cfg["substep_dt"], cfg["grid_extent"]
    spf = int(cfg["frame_dt"] / dt)  # arguments/__init__.py: steps_per_frame
    lines = [f"# {a.config}, {len(prob['x'])} particles, n_grid {a.n_grid}, seed 0; {spf} substeps a frame; "
             f"tiles {T[0]}x{T[1]}x{T[2]} by base cell, chunks of {CHUNK}",
             "frame | owner tiles | chunks | tiles by chunk count | particles in tiles of >= 2 chunks | >= 3 chunks | "
             "max per tile | vmax"]
    t, done, t0 = 0.0, 0, time.perf_counter()
    for f in frames:
        t = oracle_run(sim, imps, ops, dt, (f - done) * spf, t0=t)
        done = f
        s = tile_stats(sim.x, sim.v, a.n_grid, ext)
        by = ", ".join(f"{n} x {c}" for c, n in s["by_chunks"].items())
        lines.append(f"{f} | {s['tiles']} | {s['chunks']} | {by} | {100 * s['ge2']:.1f} % | {100 * s['ge3']:.1f} % | "
                     f"{s['max_per_tile']} | {s['vmax']:.3g}")
        print(lines[-1], f"   [{time.perf_counter() - t0:.0f} s]", flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
