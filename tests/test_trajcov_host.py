"""CPU checks behind lvx_trajectory_covariance (no GPU): the pose Jacobian of lvi-exc_amd/csrc/lvx_trajcov.h (g++ build: tests/native/trajcov_host_check.cpp) against
central differences of the pose through EigenQuaternionParameterization::Plus; the selected inverse restated in numpy from the factor layout of the sequential route
(tests/trajcov_cases.py: column by column, and in k_band_selinv's panel order with its ring) against a float64 inverse; the layout of the call's two structs.

Jacobian bar: 10 x the largest difference between the two Richardson levels (central differences at h / 2 and their extrapolation with h), h = 1e-3 in tangent units
and 1e-5 s for a time offset.  Observed: in the spline's own frame the levels differ by 2e-11 .. 9e-11 and |J - extrapolation| <= 2.5e-13; in a sensor frame by 3e-8 ..
5e-8 (the time-offset column) and |J - extrapolation| <= 3.5e-9 (the rounding of that column's differences, eps |p| / 1e-5).
Selected inverse bar: both sides are float64 eliminations of a random factor with diagonal in [1, 2] and up to 86 off-diagonal entries in [-1, 1] per column, whose
inverse entries span six decades: 1e-9 of sqrt(S_ii S_jj); observed 2e-16 .. 1.9e-10 (the largest at nb = 40, bw = 23, 46 border rows; the larger of the column-by-column form and
the panel form)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
import trajcov_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("trajcov") / "libtrajcov_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", so, os.path.join(ROOT, "tests", "native", "trajcov_host_check.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def problem():
    P = synth.make_problem(seed=14, duration=0.4, n_surfel=0, n_landmarks=0, n_camsurf=0)
    x = P["state0"].copy()
    N = P["n_knots"]
    x[7 * N + 23], x[7 * N + 31] = 6.5e-4, -8e-4   # sensor time offsets that are not zero
    return P, x


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _jac(host, P, x, frame, t):
    J = np.zeros((6, TC.W)); idx = np.zeros(TC.W, np.int32)
    st = host.tc_jacobian(_p(x), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(frame), C.c_double(t), _p(J), _p(idx))
    return st, J, idx


def _pose_fn(host, P, frame, t):
    def fn(state):
        s = np.ascontiguousarray(state)
        q = np.zeros(4); p = np.zeros(3); i0 = C.c_int(0); u = C.c_double(0)
        assert host.tc_pose(_p(s), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(frame), C.c_double(t), _p(q), _p(p), C.byref(i0), C.byref(u)) == 0
        return q, p
    return fn


def _times(P):
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    return {"u0_i0first": t0, "u_near_1": t0 + 7 * dt + dt * (1 - 1e-9), "u0_inner": t0 + 11 * dt, "i0_last": t0 + (N - 4) * dt + 0.63 * dt, "inner": t0 + 20.41 * dt}


@pytest.mark.parametrize("frame", [lvx.FRAME_TRAJECTORY, lvx.FRAME_LIDAR, lvx.FRAME_CAMERA])
@pytest.mark.parametrize("where", ["u0_i0first", "u_near_1", "u0_inner", "i0_last", "inner"])
def test_jacobian_against_central_differences(host, problem, frame, where):
    P, x = problem
    N = P["n_knots"]
    t = _times(P)[where]
    if frame != lvx.FRAME_TRAJECTORY and where == "u0_i0first":
        t = t - x[7 * N + (23 if frame == lvx.FRAME_LIDAR else 31)] + 2e-5   # the evaluation time t + tau at u = 1e-3 of the first interval: the differences by tau stay inside the spline
    st, J, idx = _jac(host, P, x, frame, t)
    assert st == 0
    tau = 0.0 if frame == lvx.FRAME_TRAJECTORY else x[7 * N + (23 if frame == lvx.FRAME_LIDAR else 31)]
    i0 = int(np.floor((t + tau - P["t0"]) / P["dt"]))
    want = [6 * (i0 + c // 6) + c % 6 for c in range(24)] + ([-1] * 7 if frame == lvx.FRAME_TRAJECTORY else [6 * N + (8 if frame == lvx.FRAME_LIDAR else 15) + b for b in range(7)])
    assert list(idx) == want
    if where == "u0_i0first":
        assert i0 == 0
    if where == "i0_last":
        assert i0 == N - 4
    Jr, Jh = TC.fd_jacobian(_pose_fn(host, P, frame, t), x, N, idx)   # the tau column moves the evaluation time: free or locked, the column is the same derivative
    level = np.abs(Jr - Jh).max()
    err = np.abs(J - Jr).max()
    print("frame %d %-11s Richardson levels differ by %.3e, |J - J_fd| = %.3e" % (frame, where, level, err))
    assert err <= 10 * level
    if frame == lvx.FRAME_TRAJECTORY:
        assert not J[:, 24:].any()


def test_jacobian_reports_range_and_unit_norm(host, problem):
    P, x = problem
    N = P["n_knots"]
    assert _jac(host, P, x, 0, P["t0"] + (N - 3) * P["dt"])[0] == 1 and _jac(host, P, x, 0, float("nan"))[0] == 1 and _jac(host, P, x, 0, P["t0"] - 1e-9)[0] == 1
    y = x.copy()
    y[3 * N + 4 * 12:3 * N + 4 * 12 + 4] *= 1.001
    assert _jac(host, P, y, 0, P["t0"] + 10.5 * P["dt"])[0] == 2 and _jac(host, P, y, 0, P["t0"] + 20.5 * P["dt"])[0] == 0


@pytest.mark.parametrize("nbd", [0, 1, 22, 46])
@pytest.mark.parametrize("bw", [0, 3, 23, 64])
@pytest.mark.parametrize("nb", [1, 15, 16, 17, 40])
def test_selected_inverse_restated(nb, bw, nbd):
    """random SPD band + border systems: the scalar recurrence on the padded pattern and the panel order of the kernel, both from (Lb, Z, S), against numpy's inverse;
    then the ord[] gather of a window that mixes band positions, border slots and constants."""
    rng = np.random.default_rng(1000 * nb + 10 * bw + nbd)
    A, Lb, Z, S = TC.random_system(rng, nb, bw, nbd)
    Sig = np.linalg.inv(A)
    d = np.sqrt(np.diag(Sig))
    band, zb, cc = TC.selinv_scalar(Lb, Z, S, nb, bw, nbd)
    sigb, zb2, cc2 = TC.selinv_panels(Lb, Z, S, nb, bw, nbd)
    worst = 0.0
    for j in range(nb):
        for dd in range(min(max(bw, 23), nb - 1 - j) + 1):
            ref = Sig[j + dd, j]
            worst = max(worst, abs(band[j, dd] - ref) / (d[j] * d[j + dd]))
            if dd < 24:
                worst = max(worst, abs(sigb[j, dd] - ref) / (d[j] * d[j + dd]))
        for r in range(nbd):
            worst = max(worst, abs(zb[r, j] - Sig[nb + r, j]) / (d[j] * d[nb + r]), abs(zb2[r, j] - Sig[nb + r, j]) / (d[j] * d[nb + r]))
    if nbd:
        worst = max(worst, np.abs((cc - Sig[nb:, nb:]) / np.outer(d[nb:], d[nb:])).max())
    print("nb %d bw %d nbd %d: max error %.3e" % (nb, bw, nbd, worst))
    assert worst <= 1e-9
    # gather: up to 24 consecutive band positions, border slots, a constant
    lo = int(rng.integers(0, max(nb - 23, 1)))
    pos = list(range(lo, min(lo + 24, nb))) + [None] + [-1 - r for r in range(min(nbd, 7))]
    s = rng.uniform(0.5, 1.5, nb + nbd)
    Wn = TC.gather(pos, sigb, zb2, cc2, s, nb)
    live = [k for k, p in enumerate(pos) if p is not None]
    g = np.array([pos[k] if pos[k] >= 0 else nb - 1 - pos[k] for k in live])
    ref = Sig[np.ix_(g, g)] * np.outer(s[g], s[g])
    assert np.abs((Wn[np.ix_(live, live)] - ref) / np.outer(d[g] * s[g], d[g] * s[g])).max() <= 1e-9
    dead = pos.index(None)
    assert not Wn[dead].any() and not Wn[:, dead].any() and np.array_equal(Wn, Wn.T)


def test_selected_inverse_stops_at_the_lowest_position():
    rng = np.random.default_rng(3)
    nb, bw, nbd = 70, 23, 5
    A, Lb, Z, S = TC.random_system(rng, nb, bw, nbd)
    Sig = np.linalg.inv(A)
    sigb, zb, _ = TC.selinv_panels(Lb, Z, S, nb, bw, nbd, lowest=41)
    assert np.isnan(sigb[:32]).all() and np.isnan(zb[:, :32]).all()   # the panel of position 41 starts at 32
    for j in range(32, nb):
        for dd in range(min(23, nb - 1 - j) + 1):
            assert abs(sigb[j, dd] - Sig[j + dd, j]) <= 1e-9 * np.sqrt(Sig[j, j] * Sig[j + dd, j + dd])
    assert np.abs(zb[:, 32:] - Sig[nb:, 32:nb]).max() <= 1e-9 * np.abs(Sig).max()


def test_struct_layout_matches_the_ctypes_mirrors(host):
    out = (C.c_longlong * 10)()
    host.tc_layout(out)
    o, r = lvx.TrajCovOptions, lvx.TrajCov
    assert list(out) == [C.sizeof(o), o.radius.offset, o.jacobi_scaling.offset, o.reserved.offset,
                         C.sizeof(r), r.cov.offset, r.sigma.offset, r.window_cov.offset, r.window_idx.offset, r.valid.offset]
