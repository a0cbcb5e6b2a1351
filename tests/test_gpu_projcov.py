"""lvx_projection_covariance on the device: the pixel covariance of LiDAR map points in the images, in the damped LM system at a stated radius, from the selected
inverse of the sequential factor (k_border_inv, k_band_selinv, then k_proj_poses, k_proj_hub with a wavefront per image and k_proj_cov with a lane per point), against
the float64 Cholesky inverse of the SAME damped system built from the device's own dense export, restricted to window_idx (tests/projcov_cases.py,
tests/trajcov_cases.py).

Window bar: calib_cov_cases.rel_err over the live rows of a window; a case may use 10 x the reference's own error against mpmath at 40 digits
(tests/golden/projcov_ref.npz, written by tests/golden/make_projcov_ref.py from the oracle's H), floor 1e-11 — the bar of the other four covariance tests.
cov_uv bar, built as tests/test_gpu_ptcov.py builds its own: against J_fd W_ref J_fd^T with J_fd from Context.plus + lvx.sample_trajectory in both frames + the numpy
projection (central differences, Richardson; columns per unique tangent index): 10 x (the change of that product between the two Richardson levels + the window bar
carried through |J|: tol (|J| d)_r (|J| d)_s / sqrt(cov_rr cov_ss), d = sqrt(diag W_ref)).
uv bar: 1e-12 of the image width against the numpy chain.  sigma^2 and sigma_max^2 against numpy: 16 ulp of the trace.
The reference's own error per case, the bar and the observed figures are printed by every test (-s).

Near t_map the pose-level terms cancel: the trajectory's part of the two poses is common to both and only the rig's relative pose moves the pixel.

Observed on one MI355X (SMALL: 44 knots).  Windows: 8.4e-13 .. 1.5e-12 at R 1e4 (reference's own 2.8e-13 .. 1.0e-12, bar 1e-11), 6.1e-9 .. 1.3e-8 at R 1e8 (own
3.3e-9 .. 8.3e-9, bar 3.3e-8 .. 8.3e-8), <= 2.5e-15 under the solve-3 mask; the two diagonal blocks of pose_cov are lvx_trajectory_covariance's cov bit for bit.
cov_uv against J_fd W_ref J_fd^T at R 1e4: 1.6e-12 (first interval) .. 3.2e-11 of sqrt(cov_rr cov_ss), the Richardson levels differ by 6.3e-7 .. 4.3e-6, carried window
bar 5.6e-11 .. 3.6e-9.  AT t_map and 0.05 dt behind it (all 24 knot scalars shared): 7.0e-12 .. 2.4e-11 relative, 2.6e-10 .. 1.9e-8 px^2 absolute at sigmas of 6 .. 28
px; two knots shared: 3.7e-12 .. 7.1e-12.  uv: <= 5.4e-16 of the width.  sigma^2, sigma_max^2 against numpy: <= 3.2e-16 of the trace.  Solve 3 against
A_cam Sigma_cam A_cam^T from lvx_calibration_covariance: 1.9e-12 .. 1.8e-11 (levels 2.6e-7 .. 2.5e-6).  The relative pose at t_map against lidar_in_camera_cov: 1.2e-14
(carried bar 9.9e-10): sigma of T_CL 6 .. 10 cm and 0.7 .. 1.0 degrees where the camera pose alone has 11 .. 31 cm.  The 240 projected points of the decision test
against the g++ build of lvx_projcov.h on the device's pose_cov: the same bits.  sigma at R 1e4 (solve2): 8 .. 28 px inside the measured span, 1.6e8 px in the first
knot interval, which no measurement reaches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import calib_cov_cases as CC
import lvx
import projcov_cases as JC
import synth
import trajcov_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "projcov_ref.npz")))
EPS = 2.0 ** -52
POINT_KEYS = ("uv", "cov", "sigma", "sigma_max", "image", "status")
IMAGE_KEYS = ("pose_cov", "window_cov", "window_idx", "image_valid")
_P = {}


def _problem(radtan=False):
    key = "radtan" if radtan else "small"
    if key not in _P:
        _P[key] = JC.problem(camera=JC.RADTAN if radtan else None)
    return _P[key]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _context(P, locks, switches=()):
    g = lvx.Context(0)
    for k, v in switches:
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _xyzi(xyz):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    out[:, 3] = 0.5
    return out


def _image_times(P):
    """the probe times, then the first instant, exactly on a knot, the intervals around t_map (windows that share 0 .. 4 knots with the window of t_map), a spread"""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    km = int(np.floor((P["t_map"] - t0) / dt))
    t = JC.probe_times(P) + [t0, np.nextafter(tmax, 0.0), t0 + (N - 4) * dt]
    t += [t0 + (km + k + 0.37) * dt for k in (-4, -3, -2, -1, 1, 2, 3, 4) if 0 <= km + k <= N - 4]
    t += list(np.random.default_rng(5).uniform(t0, tmax, 24 - len(t)))
    return np.array(t)


def _expected_idx(P, t, free):
    want = np.array(JC.window_indices(P, P["state0"], t))
    want[~np.isin(want, free)] = -1
    return want


def _same(a, b, keys, rows=None, where=""):
    for k in keys:
        if k in a or k in b:
            x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
            assert np.array_equal(x, y), (where, k)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("projcov") / "libprojcov_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, os.path.join(ROOT, "tests", "native", "projcov_host_check.cpp")])
    return C.CDLL(so)


# 1. windows: parity with the same damped system, and the two halves are lvx_trajectory_covariance's windows bit for bit
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("mask", list(JC.MASKS))
def test_windows_match_the_damped_system_and_trajectory_covariance(mask, radius, scaling):
    P = _problem()
    locks = JC.MASKS[mask]
    g = _context(P, locks)
    name = CC.case_name(mask, radius, scaling)
    tol = _tol(name)
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, scaling)
    t = _image_times(P)
    pts = _xyzi(JC.in_image_points(P, P["state0"], t[0], 3)[0])
    r = g.projection_covariance(pts, t, radius, scaling, window=True)
    assert r["image_valid"].all()
    tc = g.trajectory_covariance(t, lvx.FRAME_CAMERA, radius, scaling, window=True)
    tm = g.trajectory_covariance([P["t_map"]], lvx.FRAME_LIDAR, radius, scaling, window=True)
    assert tc["valid"].all() and tm["valid"].all()
    worst = 0.0
    for i in range(len(t)):
        want = _expected_idx(P, t[i], free)
        assert np.array_equal(r["window_idx"][i], want), (name, i)
        Wd = r["window_cov"][i]
        dead = want < 0
        assert not Wd[dead].any() and not Wd[:, dead].any()
        assert np.array_equal(Wd, Wd.T) and np.array_equal(r["pose_cov"][i], r["pose_cov"][i].T)
        worst = max(worst, TC.window_rel_err(Wd, TC.window_of(Sig, free, want)))
        assert np.array_equal(Wd[:31, :31], tc["window_cov"][i]) and np.array_equal(r["window_idx"][i][:31], tc["window_idx"][i])
        assert np.array_equal(Wd[31:, 31:], tm["window_cov"][0]) and np.array_equal(r["window_idx"][i][31:], tm["window_idx"][0])
        # the diagonal blocks of pose_cov are the two pose covariances, bit for bit: the other pose's columns of J12 are exact zeros in the same sums, in the same order
        assert np.array_equal(r["pose_cov"][i][:6, :6], tc["cov"][i]) and np.array_equal(r["pose_cov"][i][6:, 6:], tm["cov"][0]), (name, i)
    print("%-28s window err %.3e (reference's own %.3e, allowed %.3e)" % (name, worst, float(REF_ERR[name]), tol))
    assert worst <= tol
    if mask == "solve3":   # the trajectory and the LiDAR are constant: only the camera's theta and p are left
        assert g.layout()["n_band"] == 0
        assert (r["window_idx"][:, :24] == -1).all() and (r["window_idx"][:, 30:] == -1).all() and (r["window_idx"][:, 24:30] >= 0).all()
        assert not r["pose_cov"][:, 6:, :].any()
    if mask == "camtaufree":
        assert (r["window_idx"][:, 30] == 6 * P["n_knots"] + 21).all() and (np.einsum("nii->ni", r["window_cov"])[:, 30] > 0).all()
    g.close()


# 2. cov_uv against finite-difference Jacobians, uv, the summaries
def _fd_case(P, g, radius, tol, Sig, free, image_t, n_pts, seed):
    """one image alone: every point of the constructor is status 2.  Returns the figures of the worst point."""
    N, nt = P["n_knots"], g.tangent_size
    xyz = JC.in_image_points(P, P["state0"], image_t, n_pts, seed=seed)[0]
    r = g.projection_covariance(_xyzi(xyz), [image_t], radius, True, window=True)
    assert r["image_valid"].all() and (r["status"] == 2).all() and (r["image"] == 0).all()
    idx = r["window_idx"][0]
    uniq = sorted({int(k) for k in idx if k >= 0})

    def plus(state, k, h):
        d = np.zeros(nt); d[k] = h
        return g.plus(state, d)

    def pixels(state):
        c = lvx.sample_trajectory(g, state, [image_t], lvx.FRAME_CAMERA, fields=("position", "orientation"))
        l = lvx.sample_trajectory(g, state, [P["t_map"]], lvx.FRAME_LIDAR, fields=("position", "orientation"))
        return np.concatenate([JC.pixel_from_poses(P["camera"], c["orientation"][0], c["position"][0], l["orientation"][0], l["position"][0], p.astype(np.float64)) for p in xyz])
    Jr, Jh = JC.fd_jacobian(pixels, P["state0"], N, uniq, plus=plus)
    Wr = TC.window_of(Sig, free, uniq)
    out = dict(err=0.0, level=0.0, carried=0.0, uv=0.0, summ=0.0, abs=0.0, sigma=None, shared=len(idx[idx >= 0]) - len(uniq))
    for i in range(n_pts):
        Ji, Jhi = Jr[2 * i:2 * i + 2], Jh[2 * i:2 * i + 2]
        cov_r, cov_h = Ji @ Wr @ Ji.T, Jhi @ Wr @ Jhi.T
        s = np.sqrt(np.diag(cov_r))
        level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
        jd = np.abs(Ji) @ np.sqrt(np.diag(Wr))
        carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
        err = np.abs((r["cov"][i] - cov_r) / np.outer(s, s)).max()
        assert err <= 10 * (level + carried), (image_t, i, err, level, carried)
        uverr = np.abs(r["uv"][i] - JC.pixel(P, P["state0"], image_t, xyz[i].astype(np.float64))).max() / P["camera"]["cols"]
        assert uverr <= 1e-12
        ev, tr = JC.eig2(r["cov"][i])
        serr = max(abs(r["sigma_max"][i] ** 2 - ev), np.abs(r["sigma"][i] ** 2 - np.diag(r["cov"][i])).max()) / tr
        assert serr <= 16 * EPS
        assert np.array_equal(r["cov"][i], r["cov"][i].T) and r["sigma_max"][i] >= r["sigma"][i].max()
        if err >= out["err"]:
            out.update(err=err, level=level, carried=carried, abs=np.abs(r["cov"][i] - cov_r).max(), sigma=r["sigma"][i])
        out["uv"], out["summ"] = max(out["uv"], uverr), max(out["summ"], serr)
    return out


@pytest.mark.parametrize("mask", ["solve1", "solve2", "camtaufree"])
def test_pixel_covariance_against_finite_differences(mask):
    """Images in the first interval, inside the measured span, AT t_map (all four knots shared with the window of t_map), 0.05 dt behind it and two intervals before
    it (two knots shared).  At and next to t_map the trajectory's part of the two poses cancels: what is left is the rig's relative pose, and the absolute error of
    cov_uv printed below is that of the cancelling terms."""
    P = _problem()
    locks, radius = JC.MASKS[mask], 1e4
    g = _context(P, locks)
    name = CC.case_name(mask, radius, True)
    tol = _tol(name)
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, True)
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    assert P["state0"][7 * N + 23] == 0.0 and P["state0"][7 * N + 31] == 0.0
    km = int(np.floor((P["t_map"] - t0) / dt))
    times = [t0 + 0.3 * dt, t0 + 27.6 * dt, P["t_map"], P["t_map"] + 0.05 * dt, t0 + (km - 2 + 0.37) * dt]
    live = 24 + 24 + int((np.isin(np.arange(6 * N + 8, 6 * N + 22), free)).sum())
    for k, t in enumerate(times):
        o = _fd_case(P, g, radius, tol, Sig, free, t, 3, seed=40 + k)
        assert o["shared"] == (0, 0, 24, 24, 12)[k]
        print("%s image_t %.4f: cov err %.3e (absolute %.3e px^2)  Richardson level %.3e  window bar carried %.3e  uv err %.3e  summaries %.3e  sigma %s px  shared scalars %d of %d" %
              (name, t, o["err"], o["abs"], o["level"], o["carried"], o["uv"], o["summ"], o["sigma"], o["shared"], live))
    g.close()


# 3. independent routes
def test_solve3_is_the_calibration_covariance_of_the_camera(host):
    """Trajectory and LiDAR constant: uv moves with the camera's theta and p alone, and cov_uv = A_cam Sigma_cam A_cam^T with Sigma_cam from lvx_calibration_covariance
    of the same context and radius — another kernel on another route through the factor.  At image_t = t_map under the second solve's mask the relative-pose part of
    pose_cov is the covariance of the rig's LiDAR-in-camera extrinsic, lidar_in_camera_cov of the same calibration covariance."""
    P = _problem()
    N, radius = P["n_knots"], 1e4
    g = _context(P, CC.SOLVE3)
    tol = _tol(CC.case_name("solve3", radius, True))
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    cc = g.calibration_covariance(radius, True)
    cam_cols = [6 * N + c for c in range(15, 21)]
    Scam = cc["cov"][15:21, 15:21]
    nt = g.tangent_size
    for k, image_t in enumerate((P["t0"] + 11.4 * P["dt"], P["t_map"])):
        xyz = JC.in_image_points(P, P["state0"], image_t, 3, seed=60 + k)[0]
        r = g.projection_covariance(_xyzi(xyz), [image_t], radius, True, window=True)
        assert (r["status"] == 2).all() and sorted(int(i) for i in r["window_idx"][0] if i >= 0) == cam_cols

        def plus(state, kk, h):
            d = np.zeros(nt); d[kk] = h
            return g.plus(state, d)
        pix = lambda state: np.concatenate([JC.pixel(P, state, image_t, p.astype(np.float64)) for p in xyz])
        Jr, Jh = JC.fd_jacobian(pix, P["state0"], N, cam_cols, plus=plus)
        for i in range(3):
            Ji, Jhi = Jr[2 * i:2 * i + 2], Jh[2 * i:2 * i + 2]
            cov_r, cov_h = Ji @ Scam @ Ji.T, Jhi @ Scam @ Jhi.T
            s = np.sqrt(np.diag(cov_r))
            level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
            jd = np.abs(Ji) @ np.sqrt(np.diag(Scam))
            carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
            err = np.abs((r["cov"][i] - cov_r) / np.outer(s, s)).max()
            print("solve3 image_t %.4f point %d: cov err %.3e  Richardson level %.3e  carried %.3e  sigma %s px" % (image_t, i, err, level, carried, r["sigma"][i]))
            assert err <= 10 * (level + carried)
    g.close()
    # the rig's relative pose
    g = _context(P, CC.SOLVE2)
    tol = _tol(CC.case_name("solve2", radius, True))
    x = P["state0"]
    assert x[7 * N + 23] == 0.0 and x[7 * N + 31] == 0.0
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    cc = g.calibration_covariance(radius, True)
    want = np.zeros((6, 6))
    host.pj_lidar_in_camera_cov(np.ascontiguousarray(cc["cov"]).ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), C.c_int(N), want.ctypes.data_as(C.c_void_p))
    xyz = JC.in_image_points(P, x, P["t_map"], 1, seed=70)[0]
    r = g.projection_covariance(_xyzi(xyz), [P["t_map"]], radius, True)
    qc, pc = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_CAMERA)
    ql, pl = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_LIDAR)
    Rt = JC.rotmat(qc).T
    M = np.zeros((6, 12))   # (dp, dphi) of T_CL = T_C^-1 T_L by the pose errors of the two poses
    M[:3, 0:3], M[:3, 3:6], M[:3, 6:9] = -Rt, Rt @ JC.skew(pl - pc), Rt
    M[3:, 3:6], M[3:, 9:12] = -Rt, Rt
    Pc = r["pose_cov"][0]
    got = M @ Pc @ M.T
    s = np.sqrt(np.diag(want))
    jd = np.abs(M) @ np.sqrt(np.diag(Pc))
    carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
    err = np.abs((got - want) / np.outer(s, s)).max()
    print("relative pose at t_map: err %.3e  carried %.3e  sigma of T_CL (m, rad) %s  sigma of the camera pose alone %s" % (err, carried, s, np.sqrt(np.diag(Pc))[:6]))
    assert err <= 10 * carried
    g.close()


# 4. decisions are lvx_render_map_d's
def _decision_cloud(P, times, n_in=120):
    """257 points: in-image sets of images 1 and 2, then NaN coordinates, points behind the camera, beyond z_max, outside the image; shuffled"""
    x = P["state0"]
    ql, pl = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_LIDAR)
    parts = [JC.in_image_points(P, x, times[k], n_in, seed=80 + k)[0] for k in (1, 2)]
    rng = np.random.default_rng(17)
    from landmark_cov_cases import qrot
    qc, pc = JC.sensor_pose(P, x, times[1], lvx.FRAME_CAMERA)
    back = lambda pt_c: qrot(JC.qconj(ql), qrot(qc, pt_c) + pc - pl)
    behind = [back(JC.unproject(P["camera"], [rng.uniform(100, 1100), rng.uniform(100, 600)], -rng.uniform(1, 5))) for _ in range(5)]
    far = [back(JC.unproject(P["camera"], [rng.uniform(100, 1100), rng.uniform(100, 600)], rng.uniform(17, 30))) for _ in range(5)]
    outside = [back(np.array([rng.choice([-1, 1]) * rng.uniform(25, 40), rng.uniform(-1, 1), rng.uniform(1, 4)])) for _ in range(4)]
    nan = np.array([[np.nan, 1, 2], [1, np.nan, 2], [1, 2, np.nan]])
    xyz = np.concatenate([parts[0], parts[1], np.array(behind + far + outside, np.float32), nan.astype(np.float32)])
    assert len(xyz) == 257
    order = rng.permutation(257)
    kind = np.concatenate([np.full(n_in, 1), np.full(n_in, 2), np.full(5, -1), np.full(5, -2), np.full(4, -3), np.full(3, -4)])[order]
    return _xyzi(xyz[order]), kind


def test_status_and_image_are_the_decisions_of_render_map_d(host):
    import torch
    P = _problem(radtan=True)
    cam = P["camera"]
    g = _context(P, CC.SOLVE2)
    x = P["state0"]
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    times = np.array([P["t0"] - 1.0, P["t_map"], P["t0"] + 25.2 * P["dt"]])   # image 0 lies before the spline
    cloud, kind = _decision_cloud(P, times)
    r = g.projection_covariance(cloud, times, 1e4)
    assert list(r["image_valid"]) == [False, True, True] and not r["pose_cov"][0].any() and r["pose_cov"][1].any()
    dev = torch.device("cuda:0")
    img_d = torch.zeros((3, cam["rows"], cam["cols"]), dtype=torch.uint8, device=dev)
    out_d = torch.full((257 * 16,), 7, dtype=torch.uint8, device=dev)
    cloud_d = torch.from_numpy(cloud).to(dev)
    torch.cuda.synchronize()
    valid, ncol = lvx.render_map_d(g, x, P["t_map"], img_d.data_ptr(), 3, cam["cols"], times, out_d.data_ptr(), map_d_ptr=cloud_d.data_ptr(), n=257)
    rec = out_d.cpu().numpy().view(lvx.POINT_XYZRGB)
    assert list(valid) == [False, True, True]
    assert np.array_equal(r["status"] == 2, rec["a"] == 255) and ncol == (r["status"] == 2).sum()
    kept = (rec["x"] == cloud[:, 0]) & (rec["y"] == cloud[:, 1]) & (rec["z"] == cloud[:, 2])
    zero = (rec["x"] == 0) & (rec["y"] == 0) & (rec["z"] == 0)
    assert np.array_equal(r["status"] >= 1, kept) and np.array_equal(r["status"] == 0, zero)
    # by construction
    assert (r["status"][kind > 0] == 2).all() and (r["status"][(kind == -1) | (kind == -2) | (kind == -4)] == 0).all() and (r["status"][kind == -3] == 1).all()
    off = r["status"] < 2
    assert (r["image"][off] == -1).all() and not r["uv"][off].any() and not r["cov"][off].any() and not r["sigma"][off].any() and not r["sigma_max"][off].any()
    assert (r["image"][kind == 1] == 1).all() and np.isin(r["image"][kind == 2], (1, 2)).all() and (r["image"][kind == 2] == 2).sum() > 10
    # the lowest valid image that holds the point, and the record against the g++ build of the same header on the device's pose_cov (all five radtan terms at work)
    poses = {k: JC.sensor_pose(P, x, times[k], lvx.FRAME_CAMERA) for k in (1, 2)}
    ql, pl = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_LIDAR)
    hc = JC.Pinhole(**{k: cam[k] for k, _ in JC.Pinhole._fields_})
    worst = 0.0
    for i in np.nonzero(r["status"] == 2)[0]:
        first = [k for k in (1, 2) if JC.inside_image(P, poses[k], (ql, pl), cloud[i, :3])][0]
        assert r["image"][i] == first
        uv, A, _ = JC.host_jacobian(host, hc, poses[first][0], poses[first][1], ql, pl, cloud[i, :3])
        Pc = r["pose_cov"][first]
        bound = 64 * 24 * EPS * (np.abs(A) @ np.abs(Pc) @ np.abs(A).T)
        worst = max(worst, (np.abs(r["cov"][i] - A @ Pc @ A.T) / bound).max())
        assert np.abs(r["uv"][i] - uv).max() <= 1e-12 * cam["cols"]
    print("257 points: %d projected, %d outside, %d skipped; cov against the host header on the device's pose_cov: %.3f of 64 * 24 eps |A| |P| |A|^T" %
          ((r["status"] == 2).sum(), (r["status"] == 1).sum(), (r["status"] == 0).sum(), worst))
    assert worst <= 1.0
    # 32 images run; 0 and 33 are argument errors
    t32 = np.concatenate([times, np.linspace(P["t0"] + 2 * P["dt"], P["t0"] + 30 * P["dt"], 29)])
    r32 = g.projection_covariance(cloud, t32, 1e4)
    assert r32["image_valid"][1:].all() and not r32["image_valid"][0]
    _same(r32, r, ("uv", "cov", "sigma", "sigma_max", "image", "status"), rows=(r["status"] == 2, r["status"] == 2), where="32 images")
    assert np.array_equal(r32["pose_cov"][:3], r["pose_cov"])
    for bad in (0, 33):
        with pytest.raises(lvx.LvxError) as e:
            g.projection_covariance(cloud, np.full(bad, P["t_map"]), 1e4)
        assert e.value.code == lvx.E_ARG
    g.close()


# 5. shapes, bits, forms
def _raw_scans(P, S=3, H=4, W=64):
    """a small organised recording inside the spline: points on the walls of a room, stamps behind t_map"""
    rng = np.random.default_rng(23)
    raw = np.zeros((S, H, W), dtype=lvx.POINT_XYZIT)
    az = np.linspace(-np.pi, np.pi, W, endpoint=False)
    for s in range(S):
        for h in range(H):
            d = 4.0 / np.maximum(np.abs(np.cos(az)), np.abs(np.sin(az)))
            raw["x"][s, h], raw["y"][s, h], raw["z"][s, h] = d * np.cos(az), d * np.sin(az), -0.5 + 0.3 * h + 0.01 * rng.normal(size=W)
            raw["timestamp"][s, h] = P["t_map"] + 0.05 * s + 0.04 * np.arange(W) / W
    return raw


def test_bits_do_not_depend_on_the_batch_the_position_or_the_form():
    """n = 1 .. 257 are prefixes of one shuffled cloud (around the wavefront and the workgroup of 256); a permutation; single points; without the optional arrays; the
    _d form; the _d form on the scans of the last data association (map_xyzi4_d == NULL) against the same cloud handed over."""
    import torch
    P = _problem(radtan=True)
    g = _context(P, CC.SOLVE2)
    x = P["state0"]
    raw = _raw_scans(P)
    dev = torch.device("cuda:0")
    times = np.array([P["t0"] - 1.0, P["t_map"], P["t0"] + 25.2 * P["dt"]])
    td = torch.from_numpy(times).to(dev)

    def device_call(map_ptr, n, n_out):
        o = dict(uv=torch.full((n_out, 2), 7.0, dtype=torch.float64, device=dev), cov=torch.full((n_out, 4), 7.0, dtype=torch.float64, device=dev),
                 sigma=torch.full((n_out, 2), 7.0, dtype=torch.float64, device=dev), sigma_max=torch.full((n_out,), 7.0, dtype=torch.float64, device=dev),
                 image=torch.full((n_out,), 7, dtype=torch.int32, device=dev))
        im = dict(pose_cov=torch.full((3, 144), 7.0, dtype=torch.float64, device=dev), window_cov=torch.full((3, 62 * 62), 7.0, dtype=torch.float64, device=dev),
                  window_idx=torch.full((3, 62), 7, dtype=torch.int32, device=dev))
        status, iv = torch.full((n_out,), 7, dtype=torch.uint8, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.projection_covariance_d(map_ptr, n, td.data_ptr(), 3, {k: v.data_ptr() for k, v in im.items()}, iv.data_ptr(), {k: v.data_ptr() for k, v in o.items()}, status.data_ptr(), radius=1e4)
        g.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got.update({k: v.cpu().numpy() for k, v in im.items()})
        got["cov"] = got["cov"].reshape(n_out, 2, 2); got["pose_cov"] = got["pose_cov"].reshape(3, 12, 12); got["window_cov"] = got["window_cov"].reshape(3, 62, 62)
        got["status"], got["image_valid"] = status.cpu().numpy(), iv.cpu().numpy().astype(bool)
        return got
    # before any association the NULL cloud is a state error
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    with pytest.raises(lvx.LvxError) as e:
        g.projection_covariance_d(None, 0, td.data_ptr(), 3, {}, td.data_ptr(), {}, td.data_ptr())
    assert e.value.code == lvx.E_STATE
    lvx.set_scans(g, raw, raw.shape[1], raw.shape[2])
    lvx.data_association(g, x, P["t_map"])
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    cloud, kind = _decision_cloud(P, times)
    full = g.projection_covariance(cloud, times, 1e4, window=True)
    assert (full["status"] == 2).sum() == 240 and np.isfinite(full["cov"]).all() and (full["sigma_max"][full["status"] == 2] > 0).all()
    for n in (1, 63, 64, 65, 255, 256, 257):
        part = g.projection_covariance(cloud[:n], times, 1e4, window=True)
        _same(part, {k: full[k][:n] for k in POINT_KEYS}, POINT_KEYS, where="prefix %d" % n)
        _same(part, full, IMAGE_KEYS, where="prefix %d" % n)
    perm = np.random.default_rng(77).permutation(257)
    _same(g.projection_covariance(cloud[perm], times, 1e4), {k: full[k][perm] for k in POINT_KEYS}, POINT_KEYS, where="permutation")
    for i in (0, 100, 256):
        _same(g.projection_covariance(cloud[i:i + 1], times, 1e4), {k: full[k][i:i + 1] for k in POINT_KEYS}, POINT_KEYS, where="alone %d" % i)
    lean = g.projection_covariance(cloud, times, 1e4, lean=True)
    _same(lean, full, ("image", "status", "image_valid"), where="lean")
    assert "uv" not in lean and "pose_cov" not in lean
    # the images in another order: a point's record follows its image
    swapped = g.projection_covariance(cloud, times[[2, 1, 0]], 1e4)
    only2 = (full["image"] == 2)
    assert (swapped["image"][only2] == 0).all()
    _same(swapped, full, ("uv", "cov", "sigma", "sigma_max", "status"), rows=(only2, only2), where="swapped")
    assert np.array_equal(swapped["pose_cov"][0], full["pose_cov"][2])
    # the device form
    cloud_d = torch.from_numpy(cloud).to(dev)
    _same(device_call(cloud_d.data_ptr(), 257, 257), full, POINT_KEYS + IMAGE_KEYS, where="_d")
    # the scans of the last association
    n_res = raw.size
    res = device_call(None, 0, n_res)
    scans = np.ascontiguousarray(lvx.get_scans_in_map(g, raw.shape[0], raw.shape[1], raw.shape[2]).reshape(-1, 4))
    want = g.projection_covariance(scans, times, 1e4, window=True)
    _same(res, want, POINT_KEYS + IMAGE_KEYS, where="resident cloud")
    print("resident cloud: %d points, %d projected, %d outside" % (n_res, (res["status"] == 2).sum(), (res["status"] == 1).sum()))
    assert (res["status"] == 2).sum() > 0
    g.close()


# 6. errors, each writing nothing
def test_errors_are_codes_and_a_failed_call_writes_nothing():
    import torch
    P = _problem()
    N = P["n_knots"]
    g = _context(P, CC.SOLVE2)
    times = np.array([P["t_map"], P["t0"] + 25.2 * P["dt"]])
    cloud = _xyzi(JC.in_image_points(P, P["state0"], times[0], 5)[0])
    n = 5
    with pytest.raises(lvx.LvxError) as e:
        g.projection_covariance(cloud, times)
    assert e.value.code == lvx.E_STATE   # no evaluation
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    cov, status, pcv, iv = np.full((n, 4), 7.0), np.full(n, 7, np.uint8), np.full((2, 144), 7.0), np.full(2, 7, np.int32)
    intact = lambda: (cov == 7.0).all() and (status == 7).all() and (pcv == 7.0).all() and (iv == 7).all()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(h=g, opt=None, pts=cloud, t=times, n_images=2, n_pts=n, img=True, out=True, iv_=iv, st_=status):
        o = opt if opt is not None else h._proj_options(1e8, True, None, None)
        im = lvx.ProjCovImages(pcv.ctypes.data, None, None, iv_.ctypes.data if iv_ is not None else None)
        rec = lvx.ProjCov(None, cov.ctypes.data, None, None, None, st_.ctypes.data if st_ is not None else None)
        return h._l.lvx_projection_covariance(h._h, C.byref(o), C.c_int(n_pts), vp(pts), C.c_int(n_images), vp(t), C.byref(im) if img else None, C.byref(rec) if out else None)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(reserved=1), dict(z_min=2.0, z_max=1.0)):
        o = g._proj_options(1e8, True, None, None)
        for k, v in kw.items():
            setattr(o, k, v)
        assert call(opt=o) == lvx.E_ARG
    assert call(pts=None) == lvx.E_ARG and call(t=None) == lvx.E_ARG and call(img=False) == lvx.E_ARG and call(out=False) == lvx.E_ARG
    assert call(iv_=None) == lvx.E_ARG and call(st_=None) == lvx.E_ARG and call(n_pts=0) == lvx.E_ARG and call(n_images=0) == lvx.E_ARG and call(n_images=33) == lvx.E_ARG
    assert intact()
    seen = []

    def allreduce(buf, op):
        seen.append(call())
    g.solve_step_shared(1e4, allreduce)
    assert seen and all(c == lvx.E_STATE for c in seen) and intact()   # a context of a joint solve
    # a declared pivot failure: LVX_E_NOTPD, the pre-filled arrays intact (host form), nothing written and the code at lvx_synchronize (_d form)
    g.set_switch("TEST_BAD_PIVOT", 1)
    assert call() == lvx.E_NOTPD and intact()
    dev = torch.device("cuda:0")
    t_d, p_d = torch.from_numpy(times).to(dev), torch.from_numpy(cloud).to(dev)
    cov_d, st_d = torch.full((n, 4), 7.0, dtype=torch.float64, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    pc_d, iv_d = torch.full((2, 144), 7.0, dtype=torch.float64, device=dev), torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dcall = lambda h=g: h.projection_covariance_d(p_d.data_ptr(), n, t_d.data_ptr(), 2, dict(pose_cov=pc_d.data_ptr()), iv_d.data_ptr(), dict(cov=cov_d.data_ptr()), st_d.data_ptr())
    dintact = lambda: bool((cov_d == 7.0).all()) and bool((st_d == 7).all()) and bool((pc_d == 7.0).all()) and bool((iv_d == 7).all())
    dcall()
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NOTPD and dintact()
    g.synchronize()   # reported once
    g.set_switch("TEST_BAD_PIVOT", 0)
    assert call() == lvx.OK and (status == 2).all() and (iv == 1).all() and (cov != 7.0).all()   # the context is as usable as before
    g.close()
    cov[:], status[:], pcv[:], iv[:] = 7.0, 7, 7.0, 7
    # no surfel / camera-surfel family has set t_map; and no camera
    Pn = synth.make_problem(**CC.ND)
    gn = _context(Pn, CC.ND_LOCKS)
    gn.evaluate(Pn["state0"], normal_eq=True, dense=False, residuals=False)
    tn = Pn["t0"] + np.array([0.1, 0.2])
    assert call(h=gn, t=tn) == lvx.E_STATE and intact()
    gn.close()
    gc = lvx.Context(0)
    gc.set_spline(Pn["t0"], Pn["dt"], Pn["n_knots"])
    gc.set_imu(Pn["t_imu"], Pn["gyro"], Pn["acc"], Pn["w_gyro"], Pn["w_acc"])
    gc.set_locks(CC.ND_LOCKS)
    gc.evaluate(Pn["state0"], normal_eq=True, dense=False, residuals=False)
    assert call(h=gc, t=tn) == lvx.E_STATE and "camera" in gc._l.lvx_last_error(gc._h).decode() and intact()
    gc.close()
    # the window of t_map in the band: camera-surfel rows alone lay the hub knots around t_map + tau_C; a LOCKED tau_L of three knot intervals moves the LiDAR's
    # pose at t_map onto band knots (the locked-tau_L case of tests/test_gpu_ptcov.py)
    Pc = synth.make_problem(seed=14, duration=0.4, n_surfel=0, n_landmarks=12, n_camsurf=5)
    Nc, dtc = Pc["n_knots"], Pc["dt"]
    xc = Pc["state0"].copy()
    gb = _context(Pc, CC.SOLVE2)
    tb = np.array([Pc["t_map"], Pc["t0"] + 20.1 * dtc])
    gb.evaluate(xc, normal_eq=True, dense=False, residuals=False)
    cb = _xyzi(JC.in_image_points(Pc, xc, tb[0], 5)[0])
    ok = gb.projection_covariance(cb, tb, 1e8)   # tau_L = 0: the window of t_map is the hub's
    assert ok["image_valid"].all() and (ok["status"] == 2).all() and (ok["sigma_max"] > 0).all()
    xc[7 * Nc + 23] = 3 * dtc
    gb.evaluate(xc, normal_eq=True, dense=False, residuals=False)
    assert call(h=gb, pts=cb, t=tb) == lvx.E_STATE and intact()
    tb_d, cb_d = torch.from_numpy(tb).to(dev), torch.from_numpy(cb).to(dev)
    torch.cuda.synchronize()
    gb.projection_covariance_d(cb_d.data_ptr(), n, tb_d.data_ptr(), 2, dict(pose_cov=pc_d.data_ptr()), iv_d.data_ptr(), dict(cov=cov_d.data_ptr()), st_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        gb.synchronize()
    assert e.value.code == lvx.E_STATE and dintact()
    gb.close()


# 7. host: Calibrator::ProjectionUncertainty over the map of a calibrated sequence
def test_calibrator_reports_the_pixel_uncertainty_of_the_map(tmp_path):
    """The noise-free 6 s sequence of tests/test_gpu_pipeline.py.  The map cloud through Calibrator::ProjectionUncertainty with two image times: projected points with
    finite positive sigmas, sigma_max >= every axis sigma and <= their root sum of squares, and FormatProjectionUncertainty's line."""
    import build as lvx_build
    from test_gpu_pipeline import _write
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "projcov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "projcov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin = str(tmp_path / "seq.bin")
    _write(pin, S, refine_iterations=1, lvi=0, camsurf=0)
    r = subprocess.run([exe, pin, "20"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    head = lines[0].split()
    n, n_proj, radius = int(head[2]), int(head[4]), float(head[6])
    assert radius == 1e8 and n > 100 and n_proj > 50
    assert lines[1].startswith("[Map] pixel std (px): median")
    rows = [ln.split()[1:] for ln in lines if ln.startswith("P ")]
    assert len(rows) == n_proj
    for row in rows:
        image, sig, smax = int(row[1]), np.array([float.fromhex(v) for v in row[4:6]]), float.fromhex(row[6])
        assert image in (0, 1) and np.isfinite(sig).all() and (sig > 0).all() and smax >= sig.max() and smax <= np.sqrt((sig ** 2).sum()) * (1 + 1e-12)
    print(lines[1])
