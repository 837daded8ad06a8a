"""Chunk histogram of the bench scene over its frames (CPU only).

Builds the scene bench.py times (seeded synthetic Gaussians, world2grid, the
config's fixed cubes and the ground plane), runs it on the CPU oracle's
OpenMP build frame by frame, and at the chosen frames bins the particles
into the fused pipeline's 8x8x7 tiles by base cell, as k_bin_all_f does: the
owner tiles, their <= 256-particle chunks, the tiles by chunk count, the
share of particles in tiles of >= 2 and >= 3 chunks, and vmax.  This is the
state k_grid_f's cover gather sees at each frame: a tile of c chunks makes
every node it covers sum c windows.

A second table counts the window nodes a k_fused launch stores to the chunk
slots (16 B each).  A chunk's stencil box in window coordinates (w = base -
(tile T - 1), 12 x 12 x 11 nodes) spans max - min + 3 nodes per axis.  For the
chunks of multi-chunk ("dense") tiles: whole windows (chunks x 1,584, what
they stored until they got boxes), the tile's union box for every chunk, each
chunk's own box with the tile's particles in a seeded random order (bin order
is arbitrary within a tile) and with the tile's particles cut into chunks by
z-layer; for single-chunk tiles their box.  k_grid_f reads a dense tile's
chunks inside the union.

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


W = (12, 12, 11)  # kFW0..2
FWIN = W[0] * W[1] * W[2]


def box_stats(x, n_grid, extent, seed=0):
    """window nodes stored to the slots by one k_fused launch, by scheme (module docstring)"""
    inv_dx = np.float32(n_grid / extent)
    base = (x.astype(np.float32) * inv_dx - np.float32(0.5)).astype(np.int64)
    t3 = base // np.array(T)
    td = [(n_grid + T[d] - 1) // T[d] for d in range(3)]
    tid = (t3[:, 0] * td[1] + t3[:, 1]) * td[2] + t3[:, 2]
    wb = base - (t3 * np.array(T) - 1)  # window coordinate of the base cell
    order = np.argsort(tid, kind="stable")
    tiles, first, counts = np.unique(tid[order], return_index=True, return_counts=True)
    rng = np.random.default_rng(seed)
    vol = lambda w: int(np.prod(w.max(0) - w.min(0) + 3))
    chunks_of = lambda w: [w[i:i + CHUNK] for i in range(0, len(w), CHUNK)]
    out = {"dense_chunks": 0, "now": 0, "union": 0, "own": 0, "own_z": 0, "single": 0}
    unions = []
    for f, c in zip(first, counts):
        w = wb[order[f:f + c]]
        if c <= CHUNK:
            out["single"] += vol(w)
            continue
        nc = (c + CHUNK - 1) // CHUNK
        out["dense_chunks"] += nc
        out["now"] += nc * FWIN
        out["union"] += nc * vol(w)
        unions.append(tuple(int(e) for e in w.max(0) - w.min(0) + 3))
        out["own"] += sum(vol(q) for q in chunks_of(w[rng.permutation(c)]))
        out["own_z"] += sum(vol(q) for q in chunks_of(w[np.argsort(w[:, 2], kind="stable")]))
    if unions:
        u = sorted(unions, key=lambda b: b[0] * b[1] * b[2])[len(unions) // 2]
        out["median_union"] = f"{u[0] * u[1] * u[2]} ({u[0]}x{u[1]}x{u[2]})"
    else:
        out["median_union"] = "-"
    return out


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
    blines = ["", "# window nodes stored to the chunk slots per k_fused launch (16 B a node)",
              "frame | dense chunks | dense, whole windows (chunks x 1,584) | dense, tile's union box | "
              "dense, each chunk's own box (random order within tile) | own box, chunks cut by z-layer | "
              "single-chunk tiles (boxed) | median union box"]
    t, done, t0 = 0.0, 0, time.perf_counter()
    for f in frames:
        t = oracle_run(sim, imps, ops, dt, (f - done) * spf, t0=t)
        done = f
        s = tile_stats(sim.x, sim.v, a.n_grid, ext)
        by = ", ".join(f"{n} x {c}" for c, n in s["by_chunks"].items())
        lines.append(f"{f} | {s['tiles']} | {s['chunks']} | {by} | {100 * s['ge2']:.1f} % | {100 * s['ge3']:.1f} % | "
                     f"{s['max_per_tile']} | {s['vmax']:.3g}")
        print(lines[-1], f"   [{time.perf_counter() - t0:.0f} s]", flush=True)
        b = box_stats(sim.x, a.n_grid, ext)
        blines.append(f"{f} | {b['dense_chunks']} | {b['now']:,} | {b['union']:,} | {b['own']:,} | {b['own_z']:,} | "
                      f"{b['single']:,} | {b['median_union']}")
        print(blines[-1], flush=True)
    text = "\n".join(lines + blines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
