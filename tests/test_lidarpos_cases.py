"""CPU: the LiDAR odometry position residual (lvx_resid.h: lidarpos_residual, built with g++) against the two yardsticks of tests/lidarpos_cases.py — the oracle's
dual-number rows of the converted surfel problem and a numpy restatement of the reference's functor — and its statistics record against numpy.

Bars.  Restatement against oracle rows: both are float64 chains of ~10 rotations / additions on quantities up to ~5 m: 1e-12 absolute (observed ~1e-14).  Host build
against the oracle: rows and Jacobian rows 1e-11 of the largest entry, the bar the suite holds the surfel rows to (tests/test_host_math.py, tests/test_gpu_eval.py)."""
import numpy as np
import pytest

import lidarpos_cases as lc
import traj_cases as tc
from oracle import oracle as O

LOCKS = {
    "tau_locked": lc.TAU,
    "tau_free": O.LOCK_CAM_TAU,
    "lidar_locked": lc.TAU | O.LOCK_LIDAR_Q | O.LOCK_LIDAR_P,
    "traj_locked": lc.TAU | O.LOCK_TRAJ,
}


def _t_start(P):
    return P["t0"] + 10.37 * P["dt"]


def _case(kind, n, **kw):
    P = lc.problem()
    return lc.Case(P, lc.pose_times(P, n, _t_start(P), kind), _t_start(P), **kw)


def _oracle_rows(P, case, state, locks):
    Q, sign = lc.converted_problem(P, case)
    o = tc.make_oracle(Q)
    o.set_locks(locks)
    r = o.evaluate(state, jac=True)
    r0 = lc.oracle_surfel_rows(o)
    rows = sign * r["residuals"][r0:r0 + 3 * case.n]
    J = sign[:, None] * O.dense_jacobian(r["jac_cols"], r["jac_vals"], o.tangent_size)[r0:r0 + 3 * case.n]
    return o, rows, J


@pytest.mark.parametrize("kind,n", [("spread", 40), ("dense", 16), ("hub", 9)])
def test_restatement_equals_converted_oracle_rows(kind, n):
    """The two YARDSTICKS against each other — the numpy restatement of the reference functor and the oracle's rows of the converted surfel problem, with the oracle's
    Jacobian against central differences of the restatement.  It runs no code of the library (it passes without lidarpos_residual): it is the check that the conversion the
    other tests rest on is right."""
    P = lc.problem()
    case = _case(kind, n)
    s = lc.perturbed_state(P)
    o, rows, J = _oracle_rows(P, case, s, lc.TAU)
    ref = lc.np_rows(o, s, P["n_knots"], case.t, case.p_meas, case.t_start, case.weight)
    err = np.abs(rows - ref).max()
    print("restatement vs converted oracle rows (%s): %.3e, max |r| %.3f" % (kind, err, np.abs(ref).max()))
    assert err <= 1e-12
    # the Jacobian of the converted rows against central differences of the restatement along random tangents (finite-difference limited: 1e-8)
    rng = np.random.default_rng(5)
    nt = o.tangent_size
    for _ in range(3):
        v = rng.standard_normal(nt)
        v[6 * P["n_knots"]:] = 0.0
        v[6 * P["n_knots"] + 8:6 * P["n_knots"] + 14] = rng.standard_normal(6)
        h = 1e-6
        fp = lc.np_rows(o, o.plus(s, h * v), P["n_knots"], case.t, case.p_meas, case.t_start, case.weight)
        fm = lc.np_rows(o, o.plus(s, -h * v), P["n_knots"], case.t, case.p_meas, case.t_start, case.weight)
        fd = (fp - fm) / (2 * h)
        assert np.abs(J @ v - fd).max() <= 1e-7 * max(1.0, np.abs(fd).max())


@pytest.mark.parametrize("lock_name", list(LOCKS))
@pytest.mark.parametrize("kind,n", [("spread", 40), ("dense", 16), ("hub", 9)])
def test_host_build_against_oracle(kind, n, lock_name):
    P = lc.problem()
    locks = LOCKS[lock_name]
    case = _case(kind, n)
    s = lc.perturbed_state(P)
    o, rows, J = _oracle_rows(P, case, s, locks)
    st, hr, hJ = lc.host_evaluate(P, s, case, locks)
    assert st == 0
    er, eJ = np.abs(hr - rows).max(), np.abs(hJ - J).max()
    print("host vs oracle (%s, %s): rows %.3e of %.3f, J %.3e of %.3f" % (kind, lock_name, er, np.abs(rows).max(), eJ, np.abs(J).max()))
    assert er <= 1e-11 * np.abs(rows).max()
    assert eJ <= 1e-11 * np.abs(J).max()
    if lock_name == "tau_free":
        assert np.abs(J[:, 6 * P["n_knots"] + 14]).max() > 0
    if lock_name == "lidar_locked":
        assert not hJ[:, 6 * P["n_knots"] + 8:6 * P["n_knots"] + 14].any()
    if lock_name == "traj_locked":
        assert not hJ[:, :6 * P["n_knots"]].any()


def test_exact_zero_block_against_restatement():
    """t_k = t_start, p_meas = 0: the residual is exactly zero whatever the state; the conversion does not cover it (a plane through the origin)."""
    P = lc.problem()
    case = _case("hub", 5)
    case.t = np.array([case.t_start]); case.p_meas = np.zeros((1, 3))
    s = lc.perturbed_state(P)
    st, hr, hJ = lc.host_evaluate(P, s, case, lc.TAU)
    assert st == 0
    ref = lc.np_rows(tc.make_oracle(P), s, P["n_knots"], case.t, case.p_meas, case.t_start, case.weight)
    assert np.abs(hr - ref).max() <= 1e-12 and np.abs(hr).max() <= 1e-12
    assert np.isfinite(hJ).all()


def test_out_of_range_time_reports_range():
    P = lc.problem()
    case = _case("spread", 4)
    case.t = case.t.copy(); case.t[-1] = tc.time_range(P)[1] + 1e-3
    st, _, _ = lc.host_evaluate(P, lc.perturbed_state(P), case, lc.TAU)
    assert st == 1   # RES_RANGE


@pytest.mark.parametrize("outliers", [0, 7])
def test_statistics_record_against_numpy(outliers):
    P = lc.problem()
    case = _case("spread", 130, outliers=outliers, seed=outliers)
    s = lc.perturbed_state(P, amp=1e-3)
    st, hr, _ = lc.host_evaluate(P, s, case, lc.TAU)
    assert st == 0
    ref = lc.np_stats(hr, case.weight, case.huber)
    st, got = lc.host_stats(P, s, case, lc.TAU)
    assert st == 0
    lc.assert_stats_close(got, ref)
    assert got["n_outliers"] >= outliers and (outliers > 0 or got["n_outliers"] == 0)
