"""tests/fluid_oracle.py adds a dispatch and one body, no other arithmetic: with
ids 0-3 it is tests/mixed_oracle.py bit for bit, and a fluid that never yields
is a metal that never yields.  (CPU only.)"""
import numpy as np
import pytest

from fluid_oracle import codes5, fluid_run
from mixed_oracle import mixed_run
from scenarios import build_oracle_sim

STEPS = 30
N = 4000


@pytest.fixture(scope="module")
def prob():
    from test_gpu_mixed import _problem  # lego_problem(4000, 48), the impulse moved to t = 0
    return _problem()


def _fluid(prob, yld, steps=STEPS, pv=0.008, yielded=None):
    ref, imps, ops = build_oracle_sim(prob, material="metal")
    ref.yield_stress[:] = np.float32(yld)
    ids = np.full(ref.n, 5.0, np.float32)
    fluid_run(ref, ids, imps, ops, prob["cfg"]["substep_dt"], steps, pv, yielded=yielded)
    return ref


def test_never_yielding_fluid_is_never_yielding_metal(prob):
    """Below the yield both return maps keep F = F_trial and both stresses are
    the StVK Kirchhoff stress of the same SVD: every field is equal, bit for bit."""
    from scenarios import oracle_run
    a, imps, ops = build_oracle_sim(prob, material="metal")
    a.yield_stress[:] = np.float32(1e9)
    oracle_run(a, imps, ops, prob["cfg"]["substep_dt"], STEPS)
    b = _fluid(prob, 1e9)
    assert a.n == N and np.abs(a.x - prob["x"]).max() > 1e-4  # the scene moved
    for k in ("x", "v", "C", "F_trial", "stress", "yield_stress"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_uniform_ids_reproduce_mixed_run(prob, code):
    dt = prob["cfg"]["substep_dt"]
    a, imps, ops = build_oracle_sim(prob, material="metal")
    b, _, _ = build_oracle_sim(prob, material="metal")
    ids = np.full(a.n, float(code), np.float32)
    mixed_run(a, ids, imps, ops, dt, STEPS)
    fluid_run(b, ids, imps, ops, dt, STEPS)
    for k in ("x", "v", "C", "F", "F_trial", "stress", "yield_stress"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_codes5():
    m = np.array([0.0, 1.0, 2.0, 3.0, 5.0, 4.0, 7.0, -1.0, 0.5, np.nan, 6.0], np.float32)
    assert codes5(m).tolist() == [0, 1, 2, 3, 5, 0, 0, 0, 0, 0, 0]


def test_both_branches(prob):
    """The scene exercises both branches of the return map.  Yield 2000: no row
    yields at substep 0 (F_trial = I) and part of them at substep 29 (measured:
    1014 of 4000).  At the default 0.005 most rows yield (measured: 3053 of
    4000 at substep 29): rounding in the SVD of the identity already exceeds it."""
    y = []
    ref = _fluid(prob, 2000.0, yielded=y)
    print("yield 2000: yielded rows at substep 0 / 29:", y[0], y[-1], "of", ref.n)
    assert len(y) == STEPS and y[0] == 0
    assert 0.05 * ref.n < y[-1] < 0.95 * ref.n
    assert np.array_equal(ref.yield_stress, np.full(ref.n, 2000.0, np.float32))  # the fluid never hardens
    y = []
    ref = _fluid(prob, 0.005, yielded=y)
    print("yield 0.005: yielded rows at substep 29:", y[-1], "of", ref.n)
    assert y[-1] > 0.5 * ref.n
    assert np.isfinite(ref.x).all() and np.isfinite(ref.F_trial).all()
