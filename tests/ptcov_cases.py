"""Cases, numpy restatements and probes of lvx_map_point_covariance, shared by tests/test_ptcov_host.py, tests/test_gpu_ptcov.py and the generator of the reference's own
accuracy, tests/golden/make_ptcov_ref.py.  Not a test module.

Definition (include/lvx.h): a LiDAR point p_L measured at t_k is carried into the LiDAR frame at t_map, p_M = T_L(t_map)^-1 T_L(t_k) p_L with T_L(t) the
LVX_FRAME_LIDAR pose at t + tau_L (LiDARSurfelPoint::reprojectPoint2map, lidar_surfel_point.h:34-69).  It depends on 55 tangent scalars (window_idx): the four knots
of the pose at t_k, the four of the pose at t_map, the LiDAR's theta, p, tau; window_cov = Sigma over them (trajcov_cases.reference_sigma), cov = J window_cov J^T."""
import numpy as np

import calib_cov_cases as CC
import lvx
import synth
import trajcov_cases as TC
from landmark_cov_cases import qrot

W = 55
TAUFREE = lvx.LOCK_CAM_TAU   # the second solve's mask with the LiDAR's time offset free: column 54 is live, the hub range is padded by the sensor's maximum offset
MASKS = dict(CC.MASKS, taufree=TAUFREE)
CASES = {CC.case_name(m, r, s): (m, r, s) for m in MASKS for r in CC.RADII for s in (True, False)}


def problem():
    return synth.make_problem(**CC.SMALL)


def window_indices(P, state, t):
    """the 55 tangent indices of a point measured at t (locks not applied: trajcov_cases.window_of drops the constant ones)"""
    N = P["n_knots"]
    tau = state[7 * N + 23]
    ik = int(np.floor((t + tau - P["t0"]) / P["dt"]))
    i0 = int(np.floor((P["t_map"] + tau - P["t0"]) / P["dt"]))
    return [6 * (ik + c // 6) + c % 6 for c in range(24)] + [6 * (i0 + c // 6) + c % 6 for c in range(24)] + [6 * N + 8 + b for b in range(7)]


def probe_times(P):
    """times whose windows the reference's own error is measured on: the first and the last interval, on a knot, inside the window of t_map"""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    return [t0 + 0.3 * dt, tmax - 0.4 * dt, t0 + 5 * dt, P["t_map"] + 0.05 * dt]


def lidar_pose(P, state, t):
    """(q x, y, z, w; p) of the LVX_FRAME_LIDAR pose at t (tau_L added here), from the numpy spline of synth"""
    N = P["n_knots"]
    sp = synth.Spline(P["t0"], P["dt"], state[:3 * N].reshape(N, 3), state[3 * N:7 * N].reshape(N, 4))
    e = sp.eval(np.array([t + state[7 * N + 23]]))
    return TC.qmul(e["quat"][0], state[7 * N + 16:7 * N + 20]), e["pos"][0] + qrot(e["quat"][0], state[7 * N + 20:7 * N + 23])


def chain(pose_k, pose_0, q_li, p_li, p_l):
    """lidar_surfel_point.h:34-69 with the TRAJECTORY poses (q, p) at the two times and the LiDAR's extrinsics, statement by statement"""
    conj = lambda q: np.array([-q[0], -q[1], -q[2], q[3]])
    p_i = qrot(q_li, p_l) + p_li
    p_temp = qrot(conj(pose_0[0]), qrot(pose_k[0], p_i) + pose_k[1] - pose_0[1])
    return qrot(conj(q_li), p_temp - p_li)


def map_point(P, state, t, p_l):
    """p_M by the reference's chain from the numpy spline"""
    N = P["n_knots"]
    sp = synth.Spline(P["t0"], P["dt"], state[:3 * N].reshape(N, 3), state[3 * N:7 * N].reshape(N, 4))
    tau = state[7 * N + 23]
    e = sp.eval(np.array([t + tau, P["t_map"] + tau]))
    return chain((e["quat"][0], e["pos"][0]), (e["quat"][1], e["pos"][1]), state[7 * N + 16:7 * N + 20], state[7 * N + 20:7 * N + 23], np.asarray(p_l, float))


def point_from_sensor_poses(qk, pk, q0, p0, p_l):
    """p_M = R_S0^T (R_Sk p_L + p_Sk - p_S0) from two LVX_FRAME_LIDAR poses"""
    return qrot(np.array([-q0[0], -q0[1], -q0[2], q0[3]]), qrot(qk, p_l) + pk - p0)


def fd_point_jacobian(point_fn, state, N, idx, plus=None, h=1e-3):
    """Central differences of point_fn(state) -> [3] by the tangent scalars idx at steps h and h / 2 and their Richardson extrapolation (h = 1e-5 s for a time offset, as
    trajcov_cases.fd_jacobian).  Returns (J_richardson [3, len(idx)], J_half)."""
    if plus is None:
        plus = lambda x, g, step: TC.plus_tangent(x, N, g, step)
    Jr = np.zeros((3, len(idx))); Jh = np.zeros((3, len(idx)))
    for c, g in enumerate(idx):
        if g < 0:
            continue
        hg = h * 1e-2 if g - 6 * N in (14, 21) else h
        d1 = (point_fn(plus(state, g, hg)) - point_fn(plus(state, g, -hg))) / (2 * hg)
        d2 = (point_fn(plus(state, g, hg / 2)) - point_fn(plus(state, g, -hg / 2))) / hg
        Jh[:, c] = d2
        Jr[:, c] = (4 * d2 - d1) / 3
    return Jr, Jh


def merge_columns(J, idx):
    """columns of J summed per unique tangent index (a scalar that stands in both knot groups moves the point by the sum); returns (J_u, unique idx, -1 dropped)"""
    uniq = sorted({int(g) for g in idx if g >= 0})
    Ju = np.zeros((J.shape[0], len(uniq)))
    for c, g in enumerate(idx):
        if g >= 0:
            Ju[:, uniq.index(int(g))] += J[:, c]
    return Ju, uniq


def sigma_max(cov):
    return float(np.sqrt(max(np.linalg.eigvalsh(cov)[-1], 0.0)))
