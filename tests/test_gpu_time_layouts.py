"""GPU: the fused evaluators on irregular measurement-time layouts (tests/time_layout_cases.py) against the FP64 oracle — IMU dropouts longer than the accumulator
window, exact short holes, a burst of three batches inside one interval, streams sparse enough for the G *= 2 loop of ensure_layout, row counts around the batch size,
shuffled input with duplicate stamps, stamps on the knots, a non-zero IMU time offset; LiDAR bursts, rows only at the ends of the spline, row counts around the chunk
size, shuffled rows; shuffled reprojection blocks with unused / single-view landmarks.  A wrong ownership entry or flush count leaves band columns stale or counted
twice without crashing, so every case compares H entry by entry (block-scaled: an entry the oracle has as zero must BE zero), on the first pass and on its replay.

Tolerances are those of tests/test_gpu_eval.py::_compare, relative to the oracle's magnitudes: cost 1e-12, residuals 1e-11 max|r| (element by element: the input order
of the shuffled cases is part of the assertion), H 1e-10 max|H| and 1e-9 block-scaled, g 1e-10 max|g|.  Every comparison prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import lvx
import time_layout_cases as TL
from oracle import lm
from oracle import oracle as O
from test_gpu_eval import _assert_blockscaled
from test_gpu_jacobian_blocks import _check_records

pytestmark = pytest.mark.gpu

DET_CASES = ["imu_gap_long", "imu_burst", "imu_sparse", "surf_burst"]
RECORD_CASES = ["imu_gap_long", "imu_burst", "imu_shuffled_dups", "surf_burst", "rep_shuffled_unused"]
STEP_CASES = ["imu_gap_long", "imu_sparse"]


@functools.lru_cache(maxsize=2)
def _case(name):
    """(P, state, locks, expect, oracle result or None where the oracle throws range_error) — computed once per case and shared, never modified."""
    P, state, locks, ex = TL.build(name)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    try:
        ro = o.evaluate(state, normal_eq=True)
    except IndexError:
        ro = None
    assert (ro is None) == ex["oracle_raises"]          # as recorded by tests/test_time_layout_cases.py
    return P, state, locks, ex, ro


def _context(P, locks, det=False):
    g = lvx.Context(0)
    if det:
        g.set_switch("DETERMINISTIC", 1)
    lvx.load_problem(g, P, locks)
    return g


def _check(name, label, r, ro, g):
    d = np.sqrt(np.maximum(np.diag(ro["H"]), 0.0))
    sc = np.outer(d, d)
    dH = np.abs(r["H"] - ro["H"])
    fig = dict(cost=abs(r["cost"] - ro["cost"]) / abs(ro["cost"]), r=np.abs(r["residuals"] - ro["residuals"]).max() / np.abs(ro["residuals"]).max(),
               H=dH.max() / np.abs(ro["H"]).max(), Hblk=(dH[sc > 0] / sc[sc > 0]).max(), Hzero=dH[sc == 0].max(initial=0.0),
               g=np.abs(r["g"] - ro["g"]).max() / np.abs(ro["g"]).max())
    lo = g.layout()
    print("TIME_LAYOUT %s %s: cost %.2e r %.2e H %.2e H_blockscaled %.2e H_where_oracle_zero %.2e g %.2e exact_fallback %d fallback_rows %d"
          % (name, label, fig["cost"], fig["r"], fig["H"], fig["Hblk"], fig["Hzero"], fig["g"], lo["exact_fallback"], lo["fallback_rows"]))
    assert r["residuals"].shape == ro["residuals"].shape
    assert fig["cost"] <= 1e-12
    assert fig["r"] <= 1e-11
    assert fig["H"] <= 1e-10
    assert fig["g"] <= 1e-10
    _assert_blockscaled(r["H"], ro["H"])
    return lo


def _expect_range_error(g, state, **kw):
    with pytest.raises(lvx.LvxError) as ei:
        g.evaluate(state, normal_eq=True, **kw)
    assert ei.value.code == lvx.E_RANGE


@pytest.mark.parametrize("name", TL.NAMES)
def test_both_paths_match_the_oracle_twice(name):
    P, state, locks, ex, ro = _case(name)
    g = _context(P, locks)
    if ro is None:                                      # t + tau_imu leaves the sample's segment: range_error in the reference, LVX_E_RANGE here, on both paths
        _expect_range_error(g, state)
        _expect_range_error(g, state, jac=True)
        g.close()
        return
    # fused pass, its replay (the owned band columns are STORED over the first pass's values, not cleared), the per-segment kernels, the fused pass after them
    for label, jac in (("fused", False), ("fused_replay", False), ("per_segment", True), ("fused_after", False)):
        r = g.evaluate(state, jac=jac, normal_eq=True)
        lo = _check(name, label, r, ro, g)
        if not jac and not ex["tau_imu"]:
            assert lo["exact_fallback"] == 0 and lo["fallback_rows"] == 0
        if name == "imu_tau_ge_dt" and not jac:
            assert lo["exact_fallback"] == 1            # the ownership rule of k_imu_own assumes |tau_imu| < dt
    g.close()


@pytest.mark.parametrize("name", DET_CASES)
def test_deterministic_mode_matches_and_repeats(name):
    P, state, locks, ex, ro = _case(name)
    g = _context(P, locks, det=True)
    a = g.evaluate(state, normal_eq=True)
    lo = _check(name, "deterministic", a, ro, g)
    assert lo["exact_fallback"] == 0 and lo["fallback_rows"] == 0
    b = g.evaluate(state, normal_eq=True)
    g.close()
    h = _context(P, locks, det=True)                    # and on a fresh context
    c = h.evaluate(state, normal_eq=True)
    h.close()
    for r in (b, c):
        assert r["cost"] == a["cost"]
        assert np.array_equal(r["H"], a["H"]) and np.array_equal(r["g"], a["g"]) and np.array_equal(r["residuals"], a["residuals"])


@pytest.mark.parametrize("name", RECORD_CASES)
def test_jacobian_records_come_out_in_input_order(name):
    """k_imu_own<true> / k_family_mfma write the per-block records from the same schedule, at the row's INPUT position: against the debug rows of the per-segment kernels."""
    P, state, locks, ex, ro = _case(name)
    g = _context(P, locks)
    rb = g.evaluate(state, normal_eq=True, jac_blocks=True)
    lo = _check(name, "records_pass", rb, ro, g)
    assert lo["exact_fallback"] == 0 and lo["fallback_rows"] == 0
    _check_records(g, state, rb["jac_blocks"])
    g.close()


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_lm_step_on_a_band_with_unsupported_knots(name):
    """Knots no IMU sample touches are held by a few scalar surfel rows and the damping alone — a band the elimination plan of the solver has not seen.  One damped step
    (radius 1e4, Jacobi scaling) against numpy on the oracle's dense system and against the sequential band Cholesky, 1e-7 max|d| as tests/test_gpu_solver.py."""
    P, state, locks, ex, ro = _case(name)
    N, L = P["n_knots"], P["n_landmarks"]
    free = lm.free_tangent_indices(N, L, locks)
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(ro["H"])[free], 0)))
    d_ref, m_ref, _ = lm.solve_step(ro["H"], ro["g"], free, 1e4, scale)
    g = _context(P, locks)
    g.evaluate(state, normal_eq=True, dense=False)
    d, m = g.solve_step(1e4, True)
    fb = g.layout()["solver_fallbacks"]
    g.set_switch("SOLVER_SEQ", 1)
    g.evaluate(state, normal_eq=True, dense=False)
    ds, ms = g.solve_step(1e4, True)
    g.close()
    dmax = np.abs(d_ref).max()
    print("TIME_LAYOUT %s step: vs oracle %.2e vs sequential %.2e (sequential vs oracle %.2e) model cost change %.2e solver_fallbacks %d"
          % (name, np.abs(d - d_ref).max() / dmax, np.abs(d - ds).max() / dmax, np.abs(ds - d_ref).max() / dmax, abs(m - m_ref) / abs(m_ref), fb))
    assert np.abs(d - d_ref).max() <= 1e-7 * dmax
    assert np.abs(d - ds).max() <= 1e-7 * dmax
    assert fb == 0                                      # the default elimination did the work (a failed pivot sends the step to the sequential solver silently)
