"""Cases, numpy restatements and probes of lvx_projection_covariance, shared by tests/test_projcov_host.py, tests/test_gpu_projcov.py and the generator of the
reference's own accuracy, tests/golden/make_projcov_ref.py.  Not a test module.

Definition (include/lvx.h): a map point x, given in the LiDAR frame at t_map, lands in the image taken at image_t at
    pt_G = R_L0 x + p_L0,   pt_C = R_C^T (pt_G - p_C),   uv = radtan projection of pt_C          (LIinitializer::RenderMap)
with (R_L0, p_L0) the LVX_FRAME_LIDAR pose at t_map + tau_L and (R_C, p_C) the LVX_FRAME_CAMERA pose at image_t + tau_C.  uv depends on 62 tangent scalars
(window_idx): the four knots of the camera pose, the camera's theta, p, tau, the four knots of the LiDAR pose, the LiDAR's theta, p, tau; window_cov = Sigma over
them (trajcov_cases.reference_sigma), pose_cov = J12 window_cov J12^T over (camera dp, dphi; LiDAR dp, dphi), cov_uv = A pose_cov A^T."""
import ctypes as C

import numpy as np

import calib_cov_cases as CC
import lvx
import synth
import trajcov_cases as TC
from landmark_cov_cases import qrot

W = 62
CAMTAUFREE = lvx.LOCK_LIDAR_TAU   # the second solve's mask with the camera's time offset free: column 30 is live (the counterpart of ptcov_cases.TAUFREE)
MASKS = dict(CC.MASKS, camtaufree=CAMTAUFREE)
CASES = {CC.case_name(m, r, s): (m, r, s) for m in MASKS for r in CC.RADII for s in (True, False)}
RADTAN = dict(synth.DEFAULT_CAMERA, k1=-0.11, k2=0.035, k3=-0.004, p1=7e-4, p2=-5e-4)   # all five distortion terms at work


def problem(camera=None):
    return synth.make_problem(camera=camera, **CC.SMALL)


def window_indices(P, state, image_t):
    """the 62 tangent indices of a map point in the image at image_t (locks not applied: trajcov_cases.window_of drops the constant ones)"""
    N = P["n_knots"]
    ic = int(np.floor((image_t + state[7 * N + 31] - P["t0"]) / P["dt"]))
    il = int(np.floor((P["t_map"] + state[7 * N + 23] - P["t0"]) / P["dt"]))
    return ([6 * (ic + c // 6) + c % 6 for c in range(24)] + [6 * N + 15 + b for b in range(7)] +
            [6 * (il + c // 6) + c % 6 for c in range(24)] + [6 * N + 8 + b for b in range(7)])


def probe_times(P):
    """image times whose windows the reference's own error is measured on: the first and the last interval, on a knot, t_map itself and just behind it"""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    return [t0 + 0.3 * dt, tmax - 0.4 * dt, t0 + 5 * dt, P["t_map"], P["t_map"] + 0.05 * dt]


def sensor_pose(P, state, t, frame):
    """(q x, y, z, w; p) of the LVX_FRAME_LIDAR / LVX_FRAME_CAMERA pose at t (the sensor's tau added here), from the numpy spline of synth"""
    N = P["n_knots"]
    o = 7 * N + (16 if frame == lvx.FRAME_LIDAR else 24)
    sp = synth.Spline(P["t0"], P["dt"], state[:3 * N].reshape(N, 3), state[3 * N:7 * N].reshape(N, 4))
    e = sp.eval(np.array([t + state[o + 7]]))
    return TC.qmul(e["quat"][0], state[o:o + 4]), e["pos"][0] + qrot(e["quat"][0], state[o + 4:o + 7])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def to_camera(pose_c, pose_l, x):
    """pt_C = R_C^T (R_L0 x + p_L0 - p_C)"""
    return qrot(qconj(pose_c[0]), qrot(pose_l[0], np.asarray(x, float)) + pose_l[1] - pose_c[1])


def project(cam, pt_c):
    """RenderMap's inline radtan projection (lvi_initialize_surfel_orb.cpp:766-779)"""
    x, y = pt_c[0] / pt_c[2], pt_c[1] / pt_c[2]
    r2 = x * x + y * y
    d = 1 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
    u = x * d + 2 * cam["p1"] * x * y + cam["p2"] * (r2 + 2 * x * x)
    v = y * d + cam["p1"] * (r2 + 2 * y * y) + 2 * cam["p2"] * x * y
    return np.array([cam["fx"] * u + cam["cx"], cam["fy"] * v + cam["cy"]])


def pixel(P, state, image_t, x):
    """uv of map point x in the image at image_t by the chain from the numpy spline"""
    return project(P["camera"], to_camera(sensor_pose(P, state, image_t, lvx.FRAME_CAMERA), sensor_pose(P, state, P["t_map"], lvx.FRAME_LIDAR), x))


def pixel_from_poses(cam, qc, pc, ql, pl, x):
    return project(cam, to_camera((qc, pc), (ql, pl), x))


def unproject(cam, uv, z):
    """pt_C at depth z whose projection is uv: the radtan model inverted by fixed-point iteration (converges for the mild distortion of the cases)"""
    mx, my = (uv[0] - cam["cx"]) / cam["fx"], (uv[1] - cam["cy"]) / cam["fy"]
    x, y = mx, my
    for _ in range(200):
        r2 = x * x + y * y
        d = 1 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
        x, y = (mx - 2 * cam["p1"] * x * y - cam["p2"] * (r2 + 2 * x * x)) / d, (my - cam["p1"] * (r2 + 2 * y * y) - 2 * cam["p2"] * x * y) / d
    return np.array([x * z, y * z, z])


def in_image_points(P, state, image_t, n, seed=31, margin=2.0):
    """n map points (float32 xyz) that land in the image at image_t: uv at least `margin` px inside, depth in [0.5, 10] m, carried back through the chain at `state`
    and rounded to float32 (which moves the pixel by about 1e-4 px).  Returns (xyz float32 [n, 3], uv picked [n, 2])."""
    cam = P["camera"]
    rng = np.random.default_rng(seed)
    qc, pc = sensor_pose(P, state, image_t, lvx.FRAME_CAMERA)
    ql, pl = sensor_pose(P, state, P["t_map"], lvx.FRAME_LIDAR)
    uv = np.stack([rng.uniform(margin, cam["cols"] - 1 - margin, n), rng.uniform(margin, cam["rows"] - 1 - margin, n)], axis=1)
    z = rng.uniform(0.5, 10.0, n)
    xyz = np.array([qrot(qconj(ql), qrot(qc, unproject(cam, uv[i], z[i])) + pc - pl) for i in range(n)])
    return xyz.astype(np.float32), uv


def fd_jacobian(fn, state, N, idx, plus=None, h=1e-3):
    """Central differences of fn(state) -> [m] by the tangent scalars idx at steps h and h / 2 and their Richardson extrapolation (h = 1e-5 s for a time offset, as
    trajcov_cases.fd_jacobian).  Returns (J_richardson [m, len(idx)], J_half)."""
    if plus is None:
        plus = lambda x, g, step: TC.plus_tangent(x, N, g, step)
    m = len(fn(state))
    Jr = np.zeros((m, len(idx))); Jh = np.zeros((m, len(idx)))
    for c, g in enumerate(idx):
        if g < 0:
            continue
        hg = h * 1e-2 if g - 6 * N in (14, 21) else h
        d1 = (fn(plus(state, g, hg)) - fn(plus(state, g, -hg))) / (2 * hg)
        d2 = (fn(plus(state, g, hg / 2)) - fn(plus(state, g, -hg / 2))) / hg
        Jh[:, c] = d2
        Jr[:, c] = (4 * d2 - d1) / 3
    return Jr, Jh


def rotmat(q):
    return np.stack([qrot(q, e) for e in np.eye(3)], axis=1)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def eig2(cov):
    """(largest eigenvalue, trace) of a symmetric 2 x 2 by numpy"""
    return float(np.linalg.eigvalsh(cov)[-1]), float(np.trace(cov))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the g++ build of lvx_projcov.h (tests/native/projcov_host_check.cpp) seen from Python
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Pinhole(C.Structure):
    """lvx_pinhole"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("readout", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double)]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_jacobian(host, cam, qc, pc, ql, pl, xyz):
    """pj_jacobian of the host check: (uv [2], A [2, 12], depth in the camera) of the float32 point xyz given the two sensor poses"""
    host.pj_jacobian.restype = C.c_double
    uv, A = np.zeros(2), np.zeros((2, 12))
    z = host.pj_jacobian(C.byref(cam), ptr(np.ascontiguousarray(qc)), ptr(np.ascontiguousarray(pc)), ptr(np.ascontiguousarray(ql)), ptr(np.ascontiguousarray(pl)),
                         ptr(np.ascontiguousarray(xyz, np.float32)), ptr(uv), ptr(A))
    return uv, A, z


def inside_image(P, pose_c, pose_l, xyz, z_min=0.1, z_max=15.0):
    """RenderMap's decision for one point in one image, from the numpy chain: in depth range and int(uv) on the sensor"""
    cam = P["camera"]
    pt = to_camera(pose_c, pose_l, np.asarray(xyz, np.float64))
    if not z_min <= pt[2] <= z_max:
        return False
    uv = project(cam, pt)
    return 0 <= int(uv[0]) <= cam["cols"] - 1 and 0 <= int(uv[1]) <= cam["rows"] - 1 and uv[0] > -1 and uv[1] > -1
