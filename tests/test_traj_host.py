"""Trajectory queries without a GPU: the C ABI exports the five calls and refuses a NULL context; the per-sample math the kernels run (lvi-exc_amd/csrc/lvx_traj.h, built
here with g++ -O2 -ffp-contract=off) against the oracle (Oracle.eval_pose, Oracle.evaluate) on the cases of tests/traj_cases.py; the pose-error pass against a numpy
restatement; PublishTrajectory's sampling loop and the LOAM pose file round trip of lvi-exc_amd/host/lvx_calibrate.hpp.
Bars (traj_cases.py): position 1e-12, quaternion 1e-13, derivatives and predicted readings 1e-11, pose errors 1e-11."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
import traj_cases as tc


def test_library_exports_the_trajectory_calls():
    l = lvx.lib()
    for name in ("lvx_sample_trajectory", "lvx_sample_trajectory_d", "lvx_predict_imu", "lvx_predict_imu_d", "lvx_compare_poses"):
        assert hasattr(l, name), name
    assert C.sizeof(lvx.TrajSamples) == 6 * 8 and C.sizeof(lvx.ErrSummary) == 32 and C.sizeof(lvx.PoseErrors) == 8 + 4 * 32
    assert (lvx.FRAME_TRAJECTORY, lvx.FRAME_LIDAR, lvx.FRAME_CAMERA, lvx.ALIGN_NONE, lvx.ALIGN_FIRST) == (0, 1, 2, 0, 1)
    s, e = lvx.TrajSamples(), lvx.PoseErrors()
    assert l.lvx_sample_trajectory(None, None, C.c_int(0), C.c_int(1), None, C.byref(s)) == lvx.E_ARG
    assert l.lvx_sample_trajectory_d(None, None, C.c_int(0), C.c_int(1), None, C.byref(s)) == lvx.E_ARG
    assert l.lvx_predict_imu(None, None, C.c_int(1), None, None, None, None) == lvx.E_ARG
    assert l.lvx_predict_imu_d(None, None, C.c_int(1), None, None, None, None) == lvx.E_ARG
    assert l.lvx_compare_poses(None, None, C.c_int(0), C.c_int(1), None, None, None, C.c_int(0), C.byref(e), None, None) == lvx.E_ARG


@pytest.fixture(scope="module")
def scene():
    P = tc.problem()
    return dict(P=P, o=tc.make_oracle(P))


POSE_KIN = ("position", "orientation", "velocity", "angular_velocity")


@pytest.mark.parametrize("which", ["state_true", "state0"])
def test_spline_frame_matches_the_oracle(scene, which):
    """All five fields at 1000 unsorted times plus t0, the last double below MaxTime, every knot with its neighbouring doubles; MaxTime, MaxTime + 5e-6, t0 - 1e-9, NaN
    and +-inf are invalid with zeros written.  The oracle is asked only for the valid ones.  At about 70 of the knot stamps — the last double below MaxTime among them —
    Oracle.eval_pose itself answers for t - 1e-5 (tc.oracle_retries), which a query by definition does not: tc.check_fields says how those are held."""
    P, o = scene["P"], scene["o"]
    s = P[which]
    t, ok = tc.query_times(P, 1000, 7)
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok)
    assert 20 < len(retried) < 100
    got, st = tc.host_sample(P, s, t_all)
    assert np.array_equal(got["valid"][:n0], ok) and got["valid"][n0:].all() and st == 1
    for f in lvx.TRAJ_FIELDS:
        assert not got[f][:n0][~ok].any()
    tc.check_fields(got, tc.oracle_spline(o, s), P, t_all, ok, retried, n0, tc.BARS, which)


@pytest.mark.parametrize("n_knots", [4, 5])
def test_one_and_two_intervals(scene, n_knots):
    P = scene["P"]
    N = P["n_knots"]
    s = P["state_true"]
    s2 = np.concatenate([s[:3 * n_knots], s[3 * N:3 * N + 4 * n_knots], s[7 * N:7 * N + 32]])
    t, ok = tc.query_times(P, 65, 9, n_knots)
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok, n_knots)
    got, st = tc.host_sample(P, s2, t_all, 0, n_knots)
    assert np.array_equal(got["valid"][:n0], ok) and got["valid"][n0:].all()
    tc.check_fields(got, tc.oracle_spline(tc.spline_oracle(P, n_knots), s2), P, t_all, ok, retried, n0, tc.BARS, "%d knots" % n_knots, n_knots)


@pytest.mark.parametrize("frame", [lvx.FRAME_LIDAR, lvx.FRAME_CAMERA])
def test_sensor_frames_match_the_composition(scene, frame):
    """Sensor pose, velocity of the sensor origin v + w x (R p_S) and w composed in numpy from the oracle at t + tau_S; tau_S = +-3e-4 moves the samples within 3e-4 of
    either end across the validity test."""
    P, o = scene["P"], scene["o"]
    N = P["n_knots"]
    t = tc.sensor_times(P)
    for tau in (None, 3e-4, -3e-4):
        s = tc.with_sensor_tau(P, P["state_true"], frame, tau)
        ok = tc.is_valid(P, t + tc.sensor_slots(s, N, frame)[2])
        got, _ = tc.host_sample(P, s, t, frame)
        assert np.array_equal(got["valid"], ok)
        tc.assert_sensor_tau_moves_the_ends(ok, tau)
        tc.check_fields(got, tc.oracle_sensor(o, P, s, frame), P, t, ok, np.zeros(0, int), len(t), {f: tc.BARS[f] for f in POSE_KIN}, "frame %d tau %s" % (frame, tau))


@pytest.mark.parametrize("which", ["state_true", "state0"])
@pytest.mark.parametrize("tau_dt", [0.0, 0.3, -0.3])
def test_predicted_imu_matches_the_oracle_rows(scene, which, tau_dt):
    """meas - r / w from Oracle.evaluate at the problem's 600 stamps: gyro bar 1e-11 / w_gyro, accel bar 1e-11 / w_acc — the rows are held at 1e-11 AFTER the weight.
    Repeated with tau_imu = +-0.3 dt in the state; the stamps stay inside the range.  One stamp in eight lies on a knot: 21 of them are stamps at which the oracle's
    row is the model at t - 1e-5 (tc.check_fields)."""
    P, o = scene["P"], scene["o"]
    N = P["n_knots"]
    s = P[which].copy()
    s[7 * N + 7] = tau_dt * P["dt"]
    t, ok = P["t_imu"], np.ones(len(P["t_imu"]), bool)
    if tau_dt != 0.0:
        with pytest.raises(IndexError):   # (why tc.oracle_imu hands the oracle the offset in the stamps)
            o.evaluate(s)
        assert not tc.oracle_retries(P, t + s[7 * N + 7]).any()
        t_all, retried, n0 = t, np.zeros(0, int), len(t)
    else:
        t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok)
        assert len(retried) == 21
    g, a, valid, st = tc.host_predict_imu(P, s, t_all)
    assert valid.all() and st == 0
    tc.check_fields({"gyro": g, "acc": a}, tc.oracle_imu(P, s), P, t_all, ok, retried, n0, tc.imu_bars(P), "imu %s tau %.1f dt" % (which, tau_dt))


def test_nonunit_control_quaternion_invalidates_its_windows(scene):
    """One SO3 control point scaled by 1.001: exactly the in-range samples whose four-knot window holds that point are invalid; the oracle evaluates the other times
    without an error and they meet the bars."""
    P, o = scene["P"], scene["o"]
    s, t, ok, hit = tc.nonunit_case(P, P["state_true"])
    assert hit.sum() > 20
    with pytest.raises(IndexError):
        o.eval_pose(s, t[hit][:1])
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok & ~hit)
    got, st = tc.host_sample(P, s, t_all)
    assert st == 3 and np.array_equal(got["valid"][:n0], ok & ~hit) and got["valid"][n0:].all()
    for f in lvx.TRAJ_FIELDS:
        assert not got[f][~got["valid"]].any()
    tc.check_fields(got, tc.oracle_spline(o, s), P, t_all, ok & ~hit, retried, n0, tc.BARS, "non-unit", grid_ok=lambda g: ~tc.nonunit_window(P, g))   # the oracle evaluates them: no error
    g, a, okI, stI = tc.host_predict_imu(P, s, P["t_imu"])
    hitI = tc.nonunit_window(P, P["t_imu"])
    assert stI == 2 and np.array_equal(okI, ~hitI) and not g[hitI].any() and not a[hitI].any()


def _lidar_poses(scene, t):
    P, o = scene["P"], scene["o"]
    ok = tc.is_valid(P, t + tc.sensor_slots(P["state_true"], P["n_knots"], lvx.FRAME_LIDAR)[2])
    q, p = np.zeros((len(t), 4)), np.zeros((len(t), 3))
    e = tc.oracle_sensor(o, P, P["state_true"], lvx.FRAME_LIDAR)(t[ok])
    q[ok], p[ok] = e["orientation"], e["position"]
    return q, p, ok


@pytest.mark.parametrize("n", [1, 2, 257])
def test_pose_error_math_matches_the_restatement(scene, n):
    """Oracle LiDAR poses against references with planted errors (1 mm - 1 m, 1 mrad - 1 rad, one unique largest each, non-unit quaternion norms); for n = 257 two stamps
    in the middle are out of range, so a relative pair bridges the gap.  The planted rotation angle IS the absolute rotation error; argmax is exact."""
    P = scene["P"]
    tmin, tmax = tc.time_range(P)
    t = np.linspace(tmin + 0.01, tmax - 0.01, n)
    if n == 257:
        t[100], t[101] = tmax + 1.0, tmin - 1.0
    Tq, Tp, ok = _lidar_poses(scene, t)
    assert ok.sum() == (n - 2 if n == 257 else n)
    qr, pr, it, ir = tc.planted_reference(np.random.default_rng(n), Tq, Tp, ok)
    qr[~ok], pr[~ok] = [0.3, 0.1, -0.2, 0.7], [1.0, 2.0, 3.0]
    ref0, ref1 = tc.np_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_NONE), tc.np_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_FIRST)
    got0, got1 = tc.host_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_NONE), tc.host_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_FIRST)
    tc.assert_errors_close(got0, ref0)
    tc.assert_errors_close(got1, ref1)
    assert got0["abs_trans"]["argmax"] == it and got0["abs_rot"]["argmax"] == ir and abs(got0["abs_trans"]["max"] - 1.0) < 1e-11 and abs(got0["abs_rot"]["max"] - 1.0) < 1e-11
    assert got0["rel_trans"]["n"] == ok.sum() - 1
    for k in ("rel_trans", "rel_rot"):
        assert got0[k] == got1[k]   # the same bits under both alignments
    # the reference moved rigidly on the left: ALIGN_FIRST undoes it, ALIGN_NONE reports metres
    G = (synth.q_from_rotvec(np.array([0.4, -0.7, 1.1])), np.array([3.0, -2.0, 5.0]))
    qg, pg = synth.qmul(np.broadcast_to(G[0], Tq.shape), Tq) * 1.7, synth.qrot(np.broadcast_to(G[0], Tq.shape), Tp) + G[1]
    qg[~ok] = [0, 0, 0, 1]
    a1, a0 = tc.host_pose_errors(Tq, Tp, ok, qg, pg, lvx.ALIGN_FIRST), tc.host_pose_errors(Tq, Tp, ok, qg, pg, lvx.ALIGN_NONE)
    assert max(a1["abs_trans"]["max"], a1["abs_rot"]["max"]) <= 1e-11 and a0["abs_trans"]["mean"] > 1.0 and a0["abs_rot"]["mean"] > 0.5
    assert max(a1["rel_trans"]["max"], a1["rel_rot"]["max"]) <= 1e-11
    z = tc.host_pose_errors(Tq, Tp, np.zeros(n, bool), qr, pr, lvx.ALIGN_FIRST)
    assert z["n_valid"] == 0 and all(z[k] == {"rmse": 0.0, "mean": 0.0, "max": 0.0, "argmax": 0, "n": 0} for k in ("abs_trans", "abs_rot", "rel_trans", "rel_rot"))


def test_sample_times_and_pose_file(tmp_path):
    """SampleTimes is the reference's loop `t = begin; while (t < end) { ...; t += step; }` (lvi_initialize_surfel_orb.cpp:875-891): the accumulated sum, so 0.05 over 1.5 s
    gives 31 samples (30 additions of 0.05 stay below 101.5), not 30.  WritePoseFile -> ReadPoseGT: the doubles are equal exactly."""
    libdir = os.path.join(tc.ROOT, "lvi-exc_amd")
    exe, path = str(tmp_path / "traj_host_demo"), str(tmp_path / "poses.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(tc.ROOT, "tests", "native", "traj_host_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def loop(b, e, step):
        out, t = [], b
        while t < e:
            out.append(t)
            t += step
        return out
    want = []
    for b, e, step in ((100.0, 101.5, 0.05), (100.0, 100.5, 0.07), (100.0, 100.0, 0.05), (0.1, 0.1 + 3 * 0.3, 0.3)):
        ts = loop(b, e, step)
        want.append("times %d %s %s" % (len(ts), "%.17g" % (ts[0] if ts else 0.0), "%.17g" % (ts[-1] if ts else 0.0)))
    lines = r.stdout.splitlines()
    assert lines[:4] == want and lines[0].startswith("times 31 100 ") and lines[1].startswith("times 8 ") and lines[2] == "times 0 0 0"
    assert lines[4] == "roundtrip 3 1"
    assert len(open(path).read().splitlines()) == 3 and open(path).readline().split()[0] == "1403636579763555584"
