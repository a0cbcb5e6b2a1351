"""CPU checks behind lvx_map_point_covariance (no GPU): the map point, its 3 x 55 Jacobian and the factored covariance of lvi-exc_amd/csrc/lvx_ptcov.h (g++ build:
tests/native/ptcov_host_check.cpp).

Jacobian bar: 10 x the largest difference between the two Richardson levels (central differences at h / 2 and their extrapolation with h) through
trajcov_cases.plus_tangent, as tests/test_lmcov_host.py sets it; h = 1e-3 in tangent units, 1e-5 s for the time offset.  A time inside the window of t_map repeats
tangent indices in both knot groups (all four knots; one knot in the cases u0 and tau): there the columns are summed per unique index on both sides.  Observed: the
levels differ by 1.7e-9 (inside the window of t_map, where the point hardly moves) .. 9.0e-7 (the rotation columns, which carry the lever |p_L| = 9 m),
|J - extrapolation| <= 5.5e-9.
Point bar: 1e-12 |p_M| against the reference's chain (lidar_surfel_point.h:34-69) restated statement by statement in numpy on synth's spline; observed <= 7.2e-15.
Factored covariance bar: both sides are float64 sums of at most 55 + 31 + 6 products per entry, five stages deep: 8 * 92 eps (|J| |W| |J|^T)_rs = 1.6e-13; observed
3e-16 .. 1.3e-14.  sigma_max / var_dir bar: 16 eps trace(cov) (cyclic Jacobi and LAPACK both return eigenvalues to a few eps of the norm); observed 8.7e-16."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import ptcov_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
P_L = np.array([7.5, -4.0, 3.0])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ptcov") / "libptcov_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", so, os.path.join(ROOT, "tests", "native", "ptcov_host_check.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def problem():
    return PC.problem()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(host, P, x, t, p_l=P_L):
    J = np.zeros((3, PC.W)); idx = np.zeros(PC.W, np.int32); Pm = np.zeros(3)
    st = host.pc_jacobian(_p(np.ascontiguousarray(x)), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_double(P["t_map"]), C.c_double(t),
                          _p(np.ascontiguousarray(p_l, float)), _p(J), _p(idx), _p(Pm))
    return st, J, idx, Pm


def _case(P, where):
    """(state, t_k): tt = t_k + tau_L is what the name says"""
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    x = P["state0"].copy()
    if where == "tau":
        x[7 * N + 23] = 7e-4
    tau = x[7 * N + 23]
    tt = {"inner": t0 + 20.41 * dt, "u0": t0 + 9 * dt + 1e-3 * dt, "u_near_1": t0 + 7 * dt + dt * (1 - 1e-9), "i0_first": t0 + 0.37 * dt, "i0_last": t0 + (N - 4) * dt + 0.63 * dt,
          "tau": t0 + 15.2 * dt, "hub": P["t_map"] + tau + 0.05 * dt}[where]
    return x, tt - tau


CASES = ["inner", "u0", "u_near_1", "i0_first", "i0_last", "tau", "hub"]


@pytest.mark.parametrize("where", CASES)
def test_jacobian_against_central_differences_and_point_against_the_chain(host, problem, where):
    P = problem
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    x, t = _case(P, where)
    st, J, idx, Pm = _call(host, P, x, t)
    assert st == 0
    assert list(idx) == PC.window_indices(P, x, t)
    ik, i0 = idx[0] // 6, idx[24] // 6
    if where == "i0_first":
        assert ik == 0
    if where == "i0_last":
        assert ik == N - 4
    if where == "hub":
        assert ik == i0 and list(idx[:24]) == list(idx[24:48])
    shared = 6 * max(0, 4 - abs(int(ik) - int(i0)))   # scalars that stand in both knot groups ("u0" and "tau" share one knot with the window of t_map, "hub" all four)

    def point(state):
        s, _, _, p = _call(host, P, state, t)
        assert s == 0
        return p
    Ju, uniq = PC.merge_columns(J, idx)
    assert len(uniq) == 55 - shared and (shared > 0) == (where in ("u0", "tau", "hub"))
    Jr, Jh = PC.fd_point_jacobian(point, x, N, uniq)
    level = np.abs(Jr - Jh).max()
    err = np.abs(Ju - Jr).max()
    want = PC.map_point(P, x, t, P_L)
    perr = np.abs(Pm - want).max() / np.linalg.norm(want)
    print("%-9s: Richardson levels differ by %.3e, |J - J_fd| = %.3e; point error %.3e of |p_M| = %.3f" % (where, level, err, perr, np.linalg.norm(want)))
    assert err <= 10 * level
    assert perr <= 1e-12
    if where == "tau":
        assert np.abs(J[:, 54]).max() > 0.1   # the point moves with the time offset (m / s)


def test_jacobian_reports_range_and_unit_norm(host, problem):
    P = problem
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    x = P["state0"]
    tau = x[7 * N + 23]
    for t in (t0 + (N - 3) * dt - tau, float("nan"), t0 - 1e-3 - tau):
        assert _call(host, P, x, t)[0] == 1
    far = 12 if abs(P["t_map"] - (t0 + 12 * dt)) > 6 * dt else 30
    y = x.copy()
    y[3 * N + 4 * far:3 * N + 4 * far + 4] *= 1.001
    assert _call(host, P, y, t0 + (far - 1.5) * dt - tau)[0] == 2 and _call(host, P, y, t0 + (far + 4.5 if far + 8 < N - 4 else far - 8.5) * dt - tau)[0] == 0


@pytest.mark.parametrize("where", ["inner", "tau", "hub", "i0_last"])
def test_factored_covariance_is_j_w_jt(host, problem, where):
    """what k_pt_hub / k_point_cov compute (C00, B0, T = Gk [Wkk | B0], pt_cov_assemble) against J W J^T with the dense 3 x 55 Jacobian, on a random symmetric
    positive definite window whose rows span six decades (position, rotation and calibration scalars do)"""
    P = problem
    x, t = _case(P, where)
    st, J, idx, _ = _call(host, P, x, t)
    assert st == 0
    rng = np.random.default_rng(CASES.index(where))
    G = rng.uniform(-1, 1, (PC.W, PC.W))
    d = 10.0 ** rng.uniform(-6, 0, PC.W)
    Wn = (G @ G.T + PC.W * np.eye(PC.W)) * np.outer(d, d)
    Wn = (Wn + Wn.T) / 2
    cov = np.zeros((3, 3))
    rc = host.pc_factored(_p(np.ascontiguousarray(x)), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_double(P["t_map"]), C.c_double(t), _p(P_L), _p(Wn), _p(cov))
    assert rc == 0
    ref = J @ Wn @ J.T
    bound = np.abs(J) @ np.abs(Wn) @ np.abs(J).T
    err = (np.abs(cov - ref) / bound).max()
    print("%-8s: |cov - J W J^T| / (|J| |W| |J|^T) = %.3e (allowed %.3e); sigma %s" % (where, err, 8 * 92 * EPS, np.sqrt(np.diag(cov))))
    assert err <= 8 * 92 * EPS and np.array_equal(cov, cov.T)


def test_sigma_max_and_var_dir_against_numpy(host):
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(40):
        A = rng.uniform(-1, 1, (3, 3)) * 10.0 ** rng.uniform(-4, 0, 3)
        cov = A @ A.T if k else np.zeros((3, 3))
        if k == 1:
            cov = np.diag([4e-6, 1e-6, 9e-6])
        if k == 2:
            cov = np.outer([1e-3, 2e-3, -1e-3], [1e-3, 2e-3, -1e-3])   # rank one
        cov = (cov + cov.T) / 2
        dirn = rng.uniform(-1, 1, 3); dirn /= np.linalg.norm(dirn)
        out = np.zeros(2)
        host.pc_summaries(_p(np.ascontiguousarray(cov)), _p(dirn), _p(out))
        tr = max(np.trace(cov), 1e-300)
        worst = max(worst, abs(out[0] ** 2 - PC.sigma_max(cov) ** 2) / tr, abs(out[1] - dirn @ cov @ dirn) / tr)
    print("sigma_max^2 / var_dir: worst error %.3e of the trace (allowed %.3e)" % (worst, 16 * EPS))
    assert worst <= 16 * EPS


def test_struct_layout_matches_the_ctypes_mirrors(host):
    out = (C.c_longlong * 14)()
    host.pc_layout(out)
    o, r = lvx.PointCovOptions, lvx.PointCov
    assert list(out) == [C.sizeof(o), o.radius.offset, o.jacobi_scaling.offset, o.reserved.offset,
                         C.sizeof(r), r.point.offset, r.cov.offset, r.sigma.offset, r.sigma_max.offset, r.var_dir.offset, r.window_cov.offset, r.window_idx.offset, r.valid.offset,
                         lvx.PT_COV_W]
