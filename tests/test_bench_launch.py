"""bench.py's rank bookkeeping (CPU): --gpus N starts N ranks itself when no
launcher did, refuses a launcher that started a different number, and the
JSON line's n_gpus / parallelism come from the ranks that actually ran
(`--dry-run`: the same launch path, gloo on the CPU, no GPU work)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    env["OMP_NUM_THREADS"] = "1"
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=240)


def _line(p):
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    return json.loads(lines[0])


def test_gpus_flag_starts_that_many_ranks():
    """The default N > 1 headline is north_star's design: one lego scene
    sharded by spatial slab over the N ranks (strong scaling)."""
    out = _line(_run(["--gpus", "2", "--dry-run"]))
    assert out["n_gpus"] == 2 and out["scaling"] == "strong"
    assert out["config"]["parallelism"] == "slab2"


def test_gpus_flag_slab_mode():
    for flag in (["--slab"], ["--multi", "slab"]):
        out = _line(_run(["--gpus", "2", "--dry-run"] + flag))
        assert out["n_gpus"] == 2 and out["scaling"] == "strong"
        assert out["config"]["parallelism"] == "slab2"
    out = _line(_run(["--gpus", "2", "--dp", "--dry-run"]))
    assert out["scaling"] == "weak" and out["config"]["parallelism"].startswith("dp2")


def test_default_is_one_rank():
    out = _line(_run(["--dry-run"]))
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "single"


def test_full_and_dump_outputs_flags_parse():
    out = _line(_run(["--full", "--dump-outputs", "unused", "--dry-run"]))
    assert out["n_gpus"] == 1 and out["dry_run"] is True


def test_dump_outputs_float32_and_seeded_sample(tmp_path, monkeypatch):
    """dump_outputs writes <name>.npy in float32; an array above its share of
    the byte budget is written as the same sorted sample of its elements on
    every call, and the files stay within the budget."""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("gsmpm_bench", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_BUDGET_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * 1000)  # 1000 elements per array
    big = torch.arange(30_000, dtype=torch.float64).reshape(100, 300)
    small = torch.arange(12, dtype=torch.int32).reshape(4, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a.max() > 20_000 and np.all(a == np.round(a))  # a spread of big's elements
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy())
    assert a.nbytes + s.nbytes <= 4 * 2 * 1000


def test_launcher_rank_count_must_match_flag():
    p = _run(["--gpus", "8", "--dry-run"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert "--gpus 8" in p.stderr and "WORLD_SIZE=1" in p.stderr
