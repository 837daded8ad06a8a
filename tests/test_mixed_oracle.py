"""tests/mixed_oracle.py with uniform ids is OracleMPM.substep bit for bit, for
all four materials: the helper adds a dispatch and no arithmetic.  (CPU only.)"""
import numpy as np
import pytest

from mixed_oracle import material_codes, mixed_run
from scenarios import build_oracle_sim, lego_problem, oracle_run


@pytest.fixture(scope="module")
def prob():
    p = lego_problem(3000, 32)
    for d in p["cfg"]["boundary_conditions"]:  # an impulse inside the horizon, as test_impulse_window
        if d["type"] == "impulse":
            d["start_time"] = 0.0
            d["force"] = [-80.0, 0.0, 30.0]
    return p


@pytest.mark.parametrize("material,quirk", [("jelly", True), ("jelly", False), ("metal", True), ("sand", True),
                                            ("foam", True)])
def test_uniform_ids_reproduce_substep(prob, material, quirk):
    import oracle as O
    dt = prob["cfg"]["substep_dt"]
    a, imps, ops = build_oracle_sim(prob, material=material, jelly_quirk=quirk)
    b, _, _ = build_oracle_sim(prob, material=material, jelly_quirk=quirk)
    oracle_run(a, imps, ops, dt, 30)
    ids = np.full(a.n, float(O.MATERIALS[material]), np.float32)
    mixed_run(b, ids, imps, ops, dt, 30)
    assert np.abs(a.x - prob["x"]).max() > 1e-4  # the scene moved
    for k in ("x", "v", "C", "F", "F_trial", "stress", "yield_stress"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_material_codes():
    m = np.array([0.0, 1.0, 2.0, 3.0, 7.0, -1.0, 0.5, np.nan, 4.0], np.float32)
    assert material_codes(m).tolist() == [0, 1, 2, 3, 0, 0, 0, 0, 0]
