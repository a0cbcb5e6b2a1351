"""CPU checks behind lvx_projection_covariance (no GPU): the 2 x 12 pixel Jacobian, the 2 x 2 sandwich and eigenvalue, the decision chain and the LiDAR-in-camera
covariance of lvi-exc_amd/csrc/lvx_projcov.h (g++ build with -ffp-contract=off: tests/native/projcov_host_check.cpp).

Jacobian bar: 10 x the largest difference between the two Richardson levels (central differences at h / 2 and their extrapolation with h; h = 1e-4 m / rad on the
pose errors dp, dphi of the two poses), relative to the largest entry of the row, through the numpy restatement of the chain (projcov_cases), with the default
pinhole camera and with all five radtan terms at work.  Observed: the levels differ by <= 7.1e-9 of the row, |A - extrapolation| <= 9.8e-12 of it.
uv bar: 1e-12 of the image size against the numpy chain; observed <= 4e-16.
Sandwich bar: both sides are float64 sums of 12 products two stages deep: 8 * 24 eps (|A| |P| |A|^T).  Eigenvalue bar: 16 ulp of the trace against numpy.linalg.eigvalsh.
lidar_in_camera_cov bar: against J_fd Sigma J_fd^T with J_fd the Richardson central differences of T_CL = T_CI^-1 T_LI through trajcov_cases.plus_tangent: 10 x the
change of that product between the two Richardson levels, relative to sqrt(c_rr c_ss); observed 1.1e-12 against a level of 1.2e-7.  Sandwich: <= 0.011 of its bound; eigenvalue: <= 2.2e-16 of the trace."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import projcov_cases as JC
import trajcov_cases as TC
from landmark_cov_cases import qrot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("projcov") / "libprojcov_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, os.path.join(ROOT, "tests", "native", "projcov_host_check.cpp")])
    lib = C.CDLL(so)
    lib.pj_jacobian.restype = C.c_double
    lib.pj_eig_max.restype = C.c_double
    return lib


@pytest.fixture(scope="module", params=["pinhole", "radtan"])
def problem(request):
    return JC.problem(camera=JC.RADTAN if request.param == "radtan" else None)


_p = JC.ptr


def _cam(P):
    return JC.Pinhole(**{k: P["camera"][k] for k, _ in JC.Pinhole._fields_})


def _moved(q, p, d6):
    """the pose after the pose error (dp, dphi): p + dp, Exp(dphi) R"""
    return TC.qplus(q, 0.5 * d6[3:]), p + d6[:3]


def test_struct_layouts_match_the_ctypes_mirrors(host):
    out = (C.c_longlong * 22)()
    host.pj_layout(out)
    o, i, r = lvx.ProjCovOptions, lvx.ProjCovImages, lvx.ProjCov
    want = [C.sizeof(o), o.radius.offset, o.jacobi_scaling.offset, o.reserved.offset, o.z_min.offset, o.z_max.offset,
            C.sizeof(i), i.pose_cov.offset, i.window_cov.offset, i.window_idx.offset, i.valid.offset,
            C.sizeof(r), r.uv.offset, r.cov.offset, r.sigma.offset, r.sigma_max.offset, r.image.offset, r.status.offset,
            lvx.PROJ_COV_W, lvx.KERNEL_PROJ_HUB, lvx.KERNEL_PROJ_COV, len(lvx.KERNEL_NAMES_EXT)]
    assert list(out) == want
    assert lvx.KERNEL_NAMES_EXT[lvx.KERNEL_PROJ_HUB] == "proj_hub" and lvx.KERNEL_NAMES_EXT[lvx.KERNEL_PROJ_COV] == "proj_cov"


def test_pixel_jacobian_against_central_differences(host, problem):
    P = problem
    cam = _cam(P)
    x = P["state0"]
    t0, dt = P["t0"], P["dt"]
    worst_level = worst_err = worst_uv = 0.0
    for image_t in (t0 + 7.3 * dt, P["t_map"], t0 + 30.6 * dt):
        qc, pc = JC.sensor_pose(P, x, image_t, lvx.FRAME_CAMERA)
        ql, pl = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_LIDAR)
        pts, _ = JC.in_image_points(P, x, image_t, 6, seed=int(image_t * 1000) % 97)
        for xyz in pts:
            uv, A, z = JC.host_jacobian(host, cam, qc, pc, ql, pl, xyz)
            want = JC.pixel_from_poses(P["camera"], qc, pc, ql, pl, xyz.astype(np.float64))
            worst_uv = max(worst_uv, np.abs(uv - want).max() / P["camera"]["cols"])
            assert 0.5 - 1e-3 <= z <= 10 + 1e-3

            def f(d12):
                a, b = _moved(qc, pc, d12[:6]), _moved(ql, pl, d12[6:])
                return JC.pixel_from_poses(P["camera"], a[0], a[1], b[0], b[1], xyz.astype(np.float64))
            h = 1e-4
            Jr, Jh = np.zeros((2, 12)), np.zeros((2, 12))
            for c in range(12):
                e = np.zeros(12); e[c] = h
                d1 = (f(e) - f(-e)) / (2 * h)
                d2 = (f(e / 2) - f(-e / 2)) / h
                Jh[:, c] = d2; Jr[:, c] = (4 * d2 - d1) / 3
            scale = np.abs(Jr).max(axis=1, keepdims=True)
            level = (np.abs(Jr - Jh) / scale).max()
            err = (np.abs(A - Jr) / scale).max()
            worst_level, worst_err = max(worst_level, level), max(worst_err, err)
            assert err <= 10 * level, (image_t, xyz, err, level)
    print("A: Richardson levels differ by <= %.3e of the row, |A - extrapolation| <= %.3e; uv err %.3e of the width" % (worst_level, worst_err, worst_uv))
    assert worst_uv <= 1e-12
    if P["camera"]["k1"] != 0.0:   # the distortion terms matter at this bar: the pinhole Jacobian of the same point misses it
        plain = JC.Pinhole(**{k: (0.0 if k in ("k1", "k2", "k3", "p1", "p2") else P["camera"][k]) for k, _ in JC.Pinhole._fields_})
        _, A0, _ = JC.host_jacobian(host, plain, qc, pc, ql, pl, xyz)
        assert (np.abs(A0 - Jr) / scale).max() > 1e3 * 10 * level


def test_sandwich_and_eigenvalue_against_numpy(host):
    rng = np.random.default_rng(3)
    worst_c = worst_e = 0.0
    for k in range(200):
        A = rng.normal(size=(2, 12)) * 10.0 ** rng.uniform(-2, 3)
        B = rng.normal(size=(12, 12 if k % 3 else 1)) * 10.0 ** rng.uniform(-6, 0, (12, 1))
        Pm = B @ B.T
        cov, lam = np.zeros(4), np.zeros(1)
        host.pj_sandwich(_p(np.ascontiguousarray(A)), _p(np.ascontiguousarray(Pm)), _p(cov), _p(lam))
        cov = cov.reshape(2, 2)
        want = A @ Pm @ A.T
        bound = 8 * 24 * EPS * (np.abs(A) @ np.abs(Pm) @ np.abs(A).T)
        assert np.array_equal(cov, cov.T) and (np.abs(cov - want) <= bound).all()
        worst_c = max(worst_c, (np.abs(cov - want) / bound).max())
        ev, tr = JC.eig2(cov)
        worst_e = max(worst_e, abs(lam[0] - ev) / tr)
        assert abs(lam[0] - ev) <= 16 * EPS * tr
    for cov in ([4.0, 0.0, 0.0, 4.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [3.0, 0.0, 0.0, 1e-300], [2.0, -1.5, -1.5, 9.0]):
        c = np.array(cov)
        ev, tr = JC.eig2(c.reshape(2, 2))
        assert abs(host.pj_eig_max(_p(c)) - ev) <= 16 * EPS * tr
    print("sandwich: <= %.3f of the bound; eigenvalue: <= %.3e of the trace" % (worst_c, worst_e))


def test_decisions_of_the_chain(host, problem):
    """the in-image constructor gives status 2 at the lowest valid image that holds the point; NaN, behind the camera and beyond z_max are skipped; in depth range
    but off the sensor is status 1; an invalid map pose skips everything"""
    P = problem
    cam = _cam(P)
    x, t0, dt = P["state0"], P["t0"], P["dt"]
    times = [t0 + 3.3 * dt, P["t_map"], t0 + 25.2 * dt]
    poses = [JC.sensor_pose(P, x, t, lvx.FRAME_CAMERA) for t in times]
    ql, pl = JC.sensor_pose(P, x, P["t_map"], lvx.FRAME_LIDAR)
    qc, pc = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    pts, uv_pick = JC.in_image_points(P, x, times[2], 40, seed=8)
    back = lambda pt_c: qrot(JC.qconj(ql), qrot(poses[2][0], pt_c) + poses[2][1] - pl)
    extra = np.array([[np.nan, 1, 1], back(JC.unproject(P["camera"], [300.0, 200.0], -2.0)), back(JC.unproject(P["camera"], [300.0, 200.0], 16.0)),
                      back(np.array([30.0, 0.0, 3.0]))], np.float32)
    xyzi = np.zeros((44, 4), np.float32); xyzi[:40, :3] = pts; xyzi[40:, :3] = extra

    def run(valid, map_valid=1):
        st, im, uv = np.zeros(44, np.uint8), np.zeros(44, np.int32), np.zeros((44, 2))
        host.pj_decide(C.byref(cam), C.c_int(3), _p(qc), _p(pc), _p(np.array(valid, np.int32)), _p(ql), _p(pl), C.c_int(map_valid), C.c_double(0.1), C.c_double(15.0),
                       C.c_int(44), _p(xyzi), _p(st), _p(im), _p(uv))
        return st, im, uv
    st, im, uv = run([0, 0, 1])
    assert (st[:40] == 2).all() and (im[:40] == 2).all() and np.abs(uv[:40] - uv_pick).max() < 1e-2
    assert list(st[40:]) == [0, 0, 0, 1] and (im[40:] == -1).all() and not uv[40:].any()
    st_all, im_all, uv_all = run([1, 1, 1])
    assert (st_all[:40] == 2).all() and (im_all[:40] <= 2).all()
    for i in range(40):   # the lowest valid image whose numpy chain holds the point
        first = [k for k in range(3) if JC.inside_image(P, poses[k], (ql, pl), xyzi[i, :3])][0]
        assert im_all[i] == first
        assert np.abs(uv_all[i] - JC.pixel_from_poses(P["camera"], poses[first][0], poses[first][1], ql, pl, xyzi[i, :3].astype(np.float64))).max() <= 1e-12 * P["camera"]["cols"]
    st0, im0, _ = run([1, 1, 1], map_valid=0)
    assert not st0.any() and (im0 == -1).all()


def test_lidar_in_camera_covariance_against_finite_differences(host, problem):
    P = problem
    N = P["n_knots"]
    x = P["state0"].copy()
    x[7 * N + 16:7 * N + 20] = TC.qplus(x[7 * N + 16:7 * N + 20], np.array([0.2, -0.1, 0.3]))   # well away from the identity
    x[7 * N + 20:7 * N + 23] += [0.3, -0.2, 0.1]

    def t_cl(state):
        ql, pl, qc, pc = state[7 * N + 16:7 * N + 20], state[7 * N + 20:7 * N + 23], state[7 * N + 24:7 * N + 28], state[7 * N + 28:7 * N + 31]
        return TC.qmul(JC.qconj(qc), ql), qrot(JC.qconj(qc), pl - pc)
    cols = [6 * N + c for c in (8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20)]
    Jr, Jh = TC.fd_jacobian(t_cl, x, N, cols)
    rng = np.random.default_rng(12)
    B = rng.normal(size=(22, 22)) * 10.0 ** rng.uniform(-4, -2, (22, 1))
    Sig = B @ B.T
    sub = Sig[np.ix_([c - 6 * N for c in cols], [c - 6 * N for c in cols])]
    cov_r, cov_h = Jr @ sub @ Jr.T, Jh @ sub @ Jh.T
    got = np.zeros((6, 6))
    host.pj_lidar_in_camera_cov(_p(np.ascontiguousarray(Sig)), _p(x), C.c_int(N), _p(got))
    s = np.sqrt(np.diag(cov_r))
    level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
    err = np.abs((got - cov_r) / np.outer(s, s)).max()
    print("lidar_in_camera_cov: err %.3e, Richardson level %.3e" % (err, level))
    assert np.array_equal(got, got.T) and err <= 10 * level
