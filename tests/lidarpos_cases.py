"""Shared by tests/test_lidarpos_cases.py (CPU) and tests/test_gpu_lidarpos.py: LiDAR odometry position blocks (lvx_set_lidar_poses) on the 98-knot problem of
tests/traj_cases.py, their conversion to surfel blocks the committed oracle evaluates, a numpy restatement of the reference's functor over Oracle.eval_pose, and
the g++ build of the residual header (tests/native/lidarpos_host_check.cpp) behind ctypes.

The conversion.  A position block (t_k, p_meas, weight w) equals three surfel blocks with p_L = 0, t_map = t_start, weight w and planes Pi_i = p_meas,i e_i: the
surfel row is w (n . p_M - d) with n = sign(p_meas,i) e_i and d = |p_meas,i|, i.e. sign(p_meas,i) times row i of the position block.  It needs every component of
p_meas away from zero (a plane through the origin has no closest-point form): the builder plants offsets so that |p_meas,i| >= 1e-3."""
import ctypes as C
import os
import subprocess

import numpy as np

import lvx
import synth
import traj_cases as tc
from oracle import oracle as O

ROOT = tc.ROOT
TAU = tc.TAU
HUBER = 5.0     # HuberLoss(5.0), lidar_position_measurement.h:26
WEIGHT = 1.0    # global_opt_pos_weight, calibration.hpp:68
_LIB = None


def problem():
    return tc.problem()


def perturbed_state(P, seed=3, amp=1e-2):
    """The problem's start state with every scalar moved by up to `amp` (quaternions renormalised, time offsets 0)."""
    N = P["n_knots"]
    rng = np.random.default_rng(seed)
    s = np.array(P["state0"], np.float64)
    s += amp * rng.uniform(-1.0, 1.0, s.size)
    q = s[3 * N:7 * N].reshape(N, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for o in (7 * N + 16, 7 * N + 24):
        s[o:o + 4] /= np.linalg.norm(s[o:o + 4])
    s[7 * N + 7] = 0.0; s[7 * N + 23] = 0.0; s[7 * N + 31] = 0.0
    s[7 * N:7 * N + 4] = [0, 0, 0, 1]; s[7 * N + 4:7 * N + 7] = 0.0
    return s


def np_measure(o, state, N, t, t_start):
    """v_L0Lk_L0 of lidar_position_measurement.h:29-60 (Measure up to its last subtraction) in numpy over Oracle.eval_pose: the position of the LiDAR at t in the LiDAR
    frame of t_start."""
    t = np.atleast_1d(np.asarray(t, np.float64))
    L = state[7 * N + 16:7 * N + 24]
    q_LtoI, p_LinI, tau = L[0:4], L[4:7], L[7]
    ek = o.eval_pose(state, t + tau)
    e0 = o.eval_pose(state, np.full(len(t), t_start + tau))
    q0c = synth.qconj(e0["quat"])
    p_IinL = synth.qrot(synth.qconj(q_LtoI), -p_LinI)
    v_I0Ik_I0 = synth.qrot(q0c, ek["pos"] - e0["pos"])
    v_L0I0_I0 = synth.qrot(q_LtoI, p_IinL)
    v_LkIk_I0 = synth.qrot(synth.qmul(q0c, ek["quat"]), np.broadcast_to(p_LinI, ek["pos"].shape))
    return synth.qrot(np.broadcast_to(synth.qconj(q_LtoI), ek["quat"].shape), v_I0Ik_I0 + v_L0I0_I0 + v_LkIk_I0)


def np_rows(o, state, N, t, p_meas, t_start, weight):
    """Error (:73) = weight * Measure, Measure = v_L0Lk_L0 - p_Lk_L0 (:63): rows [3 n]."""
    return (weight * (np_measure(o, state, N, t, t_start) - np.asarray(p_meas))).ravel()


def pose_times(P, n, t_start, kind="spread", seed=0):
    """n pose stamps, sorted, none within 1e-6 of a knot (there the oracle's single-time view answers for t - 1e-5, tests/traj_cases.py: oracle_retries).
    spread: 5 knot intervals apart from t_start on (wrapping inside the range when n is large: runs of equal keys);  dense: 4 per knot interval;
    hub: within 3 knots of the start time, one of them AT t_start (merged segments)."""
    dt = P["dt"]
    tmin, tmax = tc.time_range(P)
    rng = np.random.default_rng(100 + seed)
    if kind == "spread":
        span = int((tmax - t_start) / dt) - 1
        k = (5 * np.arange(n)) % span
        t = t_start + dt * (k + 0.15 + 0.7 * rng.uniform(0, 1, n))
    elif kind == "dense":
        t = t_start + 6 * dt + dt * (np.arange(n) // 4 + 0.1 + 0.2 * (np.arange(n) % 4) + 0.05 * rng.uniform(0, 1, n))
    else:
        t = np.concatenate([[t_start], t_start + dt * np.linspace(0.2, 3.3, n - 1)])
    t = np.sort(t)
    frac = (t - P["t0"]) / dt
    assert (t >= tmin).all() and (t < tmax).all() and (np.abs(frac - np.round(frac))[t != t_start] > 1e-4).all()
    return t


class Case:
    """n position blocks: times, measured positions (the true ones moved by `noise`, then pushed off zero), start time, weight, Huber."""

    def __init__(self, P, t, t_start, noise=0.02, seed=0, weight=WEIGHT, huber=HUBER, outliers=0):
        self.P, self.t, self.t_start, self.weight, self.huber = P, np.asarray(t, np.float64), float(t_start), weight, huber
        N = P["n_knots"]
        o = tc.make_oracle(P)
        rng = np.random.default_rng(200 + seed)
        pm = np_measure(o, np.asarray(P["state_true"], np.float64), N, self.t, t_start) + noise * rng.standard_normal((len(self.t), 3))
        small = np.abs(pm) < 1e-3
        pm[small] = np.where(pm[small] < 0, -1.0, 1.0) * (1e-3 + 5e-3 * rng.uniform(0, 1, int(small.sum())))
        self.outlier_idx = np.arange(0, 0)
        if outliers:
            self.outlier_idx = rng.choice(len(self.t), outliers, replace=False)
            d = rng.standard_normal((outliers, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
            pm[self.outlier_idx] += 10.0 * d
        assert (np.abs(pm) >= 1e-3).all()
        self.p_meas = pm

    @property
    def n(self):
        return len(self.t)


def converted_problem(P, case, keep_families=False):
    """The problem with the position blocks as 3 n surfel blocks (p_L = 0, planes p_meas,i e_i, t_map = t_start, no loss: the oracle's Huber acts per ROW, the
    block's acts on the norm of its three).  Returns (problem dict, sign[3 n]): oracle surfel row j = sign[j] * position row j."""
    Q = dict(P)
    n = case.n
    planes = np.zeros((3 * n, 3))
    planes[np.arange(3 * n), np.tile(np.arange(3), n)] = case.p_meas.ravel()
    Q["planes"] = planes
    Q["surf_pt"] = np.zeros((3 * n, 3))
    Q["surf_t"] = np.repeat(case.t, 3)
    Q["surf_plane"] = np.arange(3 * n, dtype=np.int32)
    Q["t_map"] = case.t_start
    Q["huber_surf"] = 0.0
    Q["w_surf"] = case.weight
    if not keep_families:
        Q["cs_lm"] = np.zeros(0, np.int32); Q["cs_plane"] = np.zeros(0, np.int32)
    return Q, np.sign(case.p_meas.ravel())


def oracle_surfel_rows(o):
    """Row range of the surfel family in the oracle's residual vector (gyro 3 n, accel 3 n, [prior], surfel)."""
    n_imu = len(o.P["t_imu"])
    return 6 * n_imu


def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "lidarpos_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "liblidarpos_host_check.so")
        deps = [src] + [os.path.join(ROOT, "lvi-exc_amd", "csrc", f) for f in ("lvx_math.h", "lvx_resid.h", "lvx_stats.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_evaluate(P, state, case, locks, mto=0.001):
    """(status, rows [3 n], dense J [3 n][n_tangent]) of the host build."""
    N, n = P["n_knots"], case.n
    s = np.ascontiguousarray(state, np.float64)
    t, pm = np.ascontiguousarray(case.t), np.ascontiguousarray(case.p_meas)
    res, cols, vals = np.zeros(3 * n), np.full((3 * n, 55), -1, np.int32), np.zeros((3 * n, 55))
    st = host_lib().lp_evaluate(_p(s), C.c_int(N), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_uint32(locks), C.c_double(mto), C.c_int(n), _p(t), _p(pm),
                                C.c_double(case.t_start), C.c_double(case.weight), _p(res), _p(cols), _p(vals))
    return st, res, O.dense_jacobian(cols, vals, 6 * N + 22)


ST_FIELDS = ("n_evaluated", "n_outliers", "cost")


def host_stats(P, state, case, locks, mto=0.001):
    N, n = P["n_knots"], case.n
    s = np.ascontiguousarray(state, np.float64)
    t, pm = np.ascontiguousarray(case.t), np.ascontiguousarray(case.p_meas)
    out = np.zeros(16)
    st = host_lib().lp_stats(_p(s), C.c_int(N), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_uint32(locks), C.c_double(mto), C.c_int(n), _p(t), _p(pm), C.c_double(case.t_start),
                             C.c_double(case.weight), C.c_double(case.huber), _p(out))
    return st, dict(n_evaluated=int(out[0]), n_outliers=int(out[1]), cost=out[2], sum=out[3:6].copy(), sum_abs=out[6:9].copy(), sum_sq=out[9:12].copy(), max_abs=out[12:15].copy())


def np_stats(rows, weight, huber):
    """The statistics record from the weighted rows [3 n] in numpy: raw error = row / weight, outliers and cost by the block norm (ceres::HuberLoss)."""
    r = np.asarray(rows).reshape(-1, 3)
    s = (r * r).sum(axis=1)
    out = s > huber * huber if huber > 0 else np.zeros(len(s), bool)
    rho = np.where(out, 2.0 * huber * np.sqrt(s) - huber * huber, s)
    e = r / weight
    return dict(n_evaluated=len(r), n_outliers=int(out.sum()), cost=float(0.5 * rho.sum()), sum=e.sum(axis=0), sum_abs=np.abs(e).sum(axis=0), sum_sq=(e * e).sum(axis=0),
                max_abs=np.abs(e).max(axis=0) if len(r) else np.zeros(3))


def assert_stats_close(got, ref, tol=1e-12):
    assert got["n_evaluated"] == ref["n_evaluated"] and got["n_outliers"] == ref["n_outliers"], (got, ref)
    assert abs(got["cost"] - ref["cost"]) <= tol * max(1.0, abs(ref["cost"]))
    for k in ("sum", "sum_abs", "sum_sq", "max_abs"):
        assert np.abs(np.asarray(got[k]) - ref[k]).max() <= tol * max(1.0, np.abs(ref["sum_abs"]).max(), np.abs(ref["sum_sq"]).max()), k


def np_huber_system(rows, J, huber):
    """cost, H = J^T J, g = J^T r of the robustified blocks from the PRE-LOSS rows [3 n] and Jacobian [3 n][nt]: every block scaled by sqrt(rho') = sqrt(huber / |r|)
    beyond the bound (ceres::HuberLoss + Corrector without the second-order term, as the evaluator applies it)."""
    r = np.asarray(rows).reshape(-1, 3)
    s = (r * r).sum(axis=1)
    out = s > huber * huber
    scale = np.where(out, np.sqrt(huber / np.sqrt(np.where(out, s, 1.0))), 1.0)
    rho = np.where(out, 2.0 * huber * np.sqrt(s) - huber * huber, s)
    sc = np.repeat(scale, 3)
    Js, rs = J * sc[:, None], rows * sc
    return float(0.5 * rho.sum()), Js.T @ Js, Js.T @ rs


def load_case(g, case):
    g.set_lidar_poses(case.t, case.p_meas, case.t_start, case.huber, case.weight)
