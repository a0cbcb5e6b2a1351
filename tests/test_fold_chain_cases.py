"""CPU: the cases of tests/fold_chain_cases.py are what they claim to be, and the oracle alone evaluates every one of them at both states (no unintended
range_error) — the premise of tests/test_gpu_fold_chain.py.  Also the closed form of the folded dense border block (lvi-exc_amd/csrc/lvx_fold.h, what k_fold_all
applies per entry) against the sequential in-place fold, in a stand-alone host program (tests/native/fold_host_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import fold_chain_cases as FC
import lvx
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _interval(P, t):
    return int(np.floor((t - P["t0"]) / P["dt"]))


def test_every_case_of_the_issue_is_built():
    assert len(set(FC.NAMES)) == len(FC.NAMES) == 13
    assert set(FC.LOCK_CASES.values()) >= {FC.TAU, 0, FC.TAU | lvx.LOCK_R3, FC.TAU | lvx.LOCK_LANDMARKS}


@pytest.mark.parametrize("name", FC.NAMES)
def test_premise_holds_and_the_oracle_evaluates(name):
    P, s, s2, locks, ex = FC.build(name)
    B = FC.base_problem()
    N, dt = P["n_knots"], P["dt"]
    assert (len(P["surf_t"]) > 0) == (name != "camsurf_only") and (len(P["cs_lm"]) > 0) == (name != "surfel_only")
    assert len(P["t_imu"]) > 0 and len(P["rep_lm"]) > 0
    assert not np.array_equal(s, s2) and np.abs(s - s2).max() <= 2.1e-3
    knot = P["t0"] + FC.HUB_KNOT * dt
    if name in FC.LOCK_CASES:
        assert locks == FC.LOCK_CASES[name]
    else:
        assert locks == FC.TAU
    if name in ("fallback_lists", "tmap_before_knot"):
        assert P["t_map"] == knot - 5e-6 and _interval(P, P["t_map"]) == FC.HUB_KNOT - 1
        assert np.count_nonzero(np.floor((P["surf_t"] - P["t0"]) / dt) == FC.HUB_KNOT) >= 10     # rows in the interval right behind t_map
        assert s[7 * N + 23] == (8e-6 if name == "fallback_lists" else B["state0"][7 * N + 23])
    elif name == "tmap_behind_knot":
        assert P["t_map"] == knot + 5e-6 and _interval(P, P["t_map"]) == FC.HUB_KNOT
    elif name == "tmap_mid_interval":
        assert abs((P["t_map"] - P["t0"]) / dt - (FC.HUB_KNOT + 0.5)) < 1e-9
    else:
        assert P["t_map"] == B["t_map"]
    if len(P["surf_t"]):
        assert P["surf_t"].min() > P["t_map"]
    if name == "lidar_poses":
        assert ex["poses"].n == 9 and (np.abs(ex["poses"].p_meas) >= 1e-3).all()
    else:
        assert ex["poses"] is None
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    n_rows = (3 if locks & lvx.LOCK_R3 else 6) * len(P["t_imu"]) +len(P["surf_t"]) + 2 * len(P["rep_lm"]) + len(P["cs_lm"]) + (3 * ex["poses"].n if ex["poses"] is not None else 0)
    for r in FC.oracle_results(name):
        assert r["residuals"].shape == (n_rows,)
        assert np.isfinite(r["residuals"]).all() and np.isfinite(r["cost"]) and r["cost"] > 0
        assert r["H"].shape == (o.tangent_size, o.tangent_size) and np.isfinite(r["H"]).all() and np.isfinite(r["g"]).all()
        # a locked position block leaves its three tangent entries of every knot without a column: the hub knots' among them (dead hub columns in the fold)
        dead = np.count_nonzero(np.diag(r["H"])[:6 * N] == 0.0)
        assert (dead >= 3 * N) == bool(locks & lvx.LOCK_R3), (dead, N)


def test_nonunit_hub_case_reaches_only_the_hub():
    P, s, k = FC.nonunit_hub_case()
    i0 = _interval(P, P["t_map"])
    assert i0 <= k <= i0 + 3 and len(P["t_imu"]) == 0 and len(P["rep_lm"]) == 0 and len(P["cs_lm"]) == 0 and len(P["surf_t"]) >= 100
    assert np.floor((P["surf_t"] - P["t0"]) / P["dt"]).min() > k                     # no surfel point's four knots hold the scaled one
    N = P["n_knots"]
    assert abs(np.linalg.norm(s[3 * N + 4 * k:3 * N + 4 * k + 4]) - 1.01) < 1e-12
    o = O.Oracle()
    lvx.load_problem(o, P, FC.TAU)
    with pytest.raises(ValueError):
        o.evaluate(s)


def test_closed_form_of_the_dense_fold_on_the_host(tmp_path):
    """C' = C + U^T C + C U + U^T C U entry by entry (fold_dense_entry) against the two sets' in-place row / column folds one after the other, on random symmetric
    blocks: shared and disjoint hub rows, dead columns, one set off.  Differences are rounding of sums of at most 12 + 12 + 144 products."""
    exe = str(tmp_path / "fold_host_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "fold_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fold_host_check: OK" in out.stdout
