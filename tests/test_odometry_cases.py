"""CPU: the cases of tests/odometry_cases.py meet, on the oracle alone, the conditions tests/test_gpu_odometry.py relies on — key decisions clear of their thresholds,
key scans after the first, and a stability record within its cap — and step() from the loop's own state reproduces the loop."""
import numpy as np
import pytest

import odometry_cases as OC

NAMES = sorted(OC.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_shape(name):
    C = OC.make_case(name)
    assert C["scans"].shape == (OC.N_SCANS, OC.H * OC.W)
    nan = np.isnan(C["scans"]["x"])
    assert 0.002 < nan.mean() < 0.03 and nan.any(axis=1).all()          # about 1 % of the points, some in every scan
    assert np.allclose(np.diff(C["stamps"]), 1.0 / OC.SCAN_RATE) and abs(C["stamps"][0] - 100.2) < 1e-9
    assert np.isfinite(OC.scan_xyzi(C["scans"][0])[~nan[0]]).all()


@pytest.mark.parametrize("name", NAMES)
def test_key_decisions_clear_of_thresholds(name):
    R = OC.run(name)
    m = OC.key_margin(R["poses"])
    print("%s: key scans %s, smallest distance of a key decision from its threshold %.4g" % (name, R["keys"], m))
    assert R["keys"][0] == 0
    assert m >= OC.KEY_MARGIN


def test_key_scans_after_the_first():
    later = sum(len(OC.run(n)["keys"]) - 1 for n in NAMES)
    assert later >= 2
    assert all(len(OC.run(n)["keys"]) >= 2 for n in NAMES)      # every case rebuilds its map at least once


@pytest.mark.parametrize("name", NAMES)
def test_stability_record_within_cap(name):
    s, unstable = OC.stability(name)
    it = [r["iterations"] for r in OC.run(name)["steps"][1:]]
    print("%s: iterations %d..%d, s_k %.1e..%.1e, unstable steps %s" % (name, min(it), max(it), s[1:].min(), s[1:].max(), np.flatnonzero(unstable).tolist()))
    assert unstable.sum() <= OC.MAX_UNSTABLE[name]
    assert (s[1:][~unstable[1:]] <= OC.UNSTABLE_ABOVE).all()


def test_step_from_the_loops_state_is_the_loop():
    """step(map, guess, scan) builds its own aligner and reproduces the loop's record bit for bit (the oracle is deterministic)"""
    name, k = "lively", 5
    C, R = OC.make_case(name), OC.run(name)
    r = OC.step(R["maps"][R["n_map"][k]], OC.guess_of(R["poses"][k - 1]), OC.scan_xyzi(C["scans"][k]))
    assert np.array_equal(r["pose"], R["poses"][k]) and np.array_equal(r["p6"], R["steps"][k]["p6"])
    assert r["iterations"] == R["steps"][k]["iterations"] and r["n_src"] == R["steps"][k]["n_src"]


def test_guess_product_order():
    rng = np.random.default_rng(0)
    L, P = rng.standard_normal((4, 4)), rng.standard_normal((4, 4))
    assert np.abs(OC.guess_of(L, P).astype(np.float64) - L @ P).max() <= 1e-6
    assert np.array_equal(OC.guess_of(L), L.astype(np.float32))
