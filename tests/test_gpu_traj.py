"""Trajectory queries on the device (lvi-exc_amd/csrc/lvx_traj.hip): lvx_sample_trajectory in the spline's and the sensors' frames against the oracle (Oracle.eval_pose),
lvx_predict_imu against the oracle's gyroscope / accelerometer rows, lvx_compare_poses against a numpy restatement, the _d variants and repeated calls bit for bit, the
error codes, and the C++ free functions of lvx_calibrate.hpp against the Python binding.  Problem, cases and bars: tests/traj_cases.py (position 1e-12, quaternion
1e-13, derivatives and predicted readings 1e-11, pose errors 1e-11).  Every test prints its maxima."""
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
import traj_cases as tc

pytestmark = pytest.mark.gpu
POSE_KIN = ("position", "orientation", "velocity", "angular_velocity")


@pytest.fixture(scope="module")
def scene():
    """One problem, its oracle, one context with the problem loaded (read-only)."""
    P = tc.problem()
    g = lvx.Context(0)
    lvx.load_problem(g, P, tc.TAU)
    yield dict(P=P, g=g, o=tc.make_oracle(P))
    g.close()


def _same_bits(a, b, keys):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


@pytest.mark.parametrize("which", ["state_true", "state0"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_all_fields_match_the_oracle(scene, n, which):
    """n unsorted times plus t0, the last double below MaxTime and every knot with its neighbouring doubles (sizes around the wavefront and the workgroup); MaxTime,
    MaxTime + 5e-6, t0 - 1e-9, NaN and +-inf are invalid with zeros written.  The oracle is asked only for the valid ones; at the knot stamps where Oracle.eval_pose
    itself answers for t - 1e-5, see tc.check_fields."""
    P, g, o = scene["P"], scene["g"], scene["o"]
    s = P[which]
    t, ok = tc.query_times(P, n, 100 + n)
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok)
    got = lvx.sample_trajectory(g, s, t_all)
    assert np.array_equal(got["valid"][:n0], ok) and got["valid"][n0:].all()
    for f in lvx.TRAJ_FIELDS:
        assert not got[f][:n0][~ok].any()
    tc.check_fields(got, tc.oracle_spline(o, s), P, t_all, ok, retried, n0, tc.BARS, "n=%d %s" % (n, which))


@pytest.mark.parametrize("n_knots", [4, 5])
def test_one_and_two_intervals(scene, n_knots):
    """Splines of 4 and 5 control points: a context with nothing but lvx_set_spline."""
    P = scene["P"]
    N = P["n_knots"]
    s = P["state_true"]
    s2 = np.concatenate([s[:3 * n_knots], s[3 * N:3 * N + 4 * n_knots], s[7 * N:7 * N + 32]])
    t, ok = tc.query_times(P, 65, 9, n_knots)
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok, n_knots)
    g = lvx.Context(0)
    try:
        g.set_spline(P["t0"], P["dt"], n_knots)
        got = lvx.sample_trajectory(g, s2, t_all)
    finally:
        g.close()
    assert np.array_equal(got["valid"][:n0], ok) and got["valid"][n0:].all()
    tc.check_fields(got, tc.oracle_spline(tc.spline_oracle(P, n_knots), s2), P, t_all, ok, retried, n0, tc.BARS, "%d knots" % n_knots, n_knots)


def test_single_fields_device_pointers_and_repeats_are_the_same_bits(scene):
    """Every field requested alone (other pointers NULL), the _d variant on device buffers (with the state passed and with the resident state of set_state) and a second
    call give the bits of the all-fields call.  1000 + knots + invalid stamps."""
    import torch
    P, g = scene["P"], scene["g"]
    s = np.ascontiguousarray(P["state0"], np.float64)
    t, ok = tc.query_times(P, 1000, 5)
    keys = lvx.TRAJ_FIELDS + ("valid",)
    full = lvx.sample_trajectory(g, s, t)
    assert _same_bits(full, lvx.sample_trajectory(g, s, t), keys)
    for f in lvx.TRAJ_FIELDS:
        one = lvx.sample_trajectory(g, s, t, fields=(f,))
        assert sorted(one) == sorted([f, "valid"]) and _same_bits(full, one, (f, "valid")), f
    dev = torch.device("cuda:0")
    n = len(t)
    t_d, s_d = torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev)
    g.set_state(s)
    for state_ptr in (s_d.data_ptr(), None):
        out = {f: torch.full((n, 4 if f == "orientation" else 3), 7.0, dtype=torch.float64, device=dev) for f in lvx.TRAJ_FIELDS}
        valid = torch.full((n,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        lvx.sample_trajectory_d(g, t_d.data_ptr(), n, {f: out[f].data_ptr() for f in out}, valid.data_ptr(), lvx.FRAME_TRAJECTORY, state_ptr)
        g.synchronize()
        got = {f: out[f].cpu().numpy() for f in out}
        got["valid"] = valid.cpu().numpy().astype(bool)
        assert _same_bits(full, got, keys)
    # lvx_predict_imu: two calls and the _d variant
    gy, ac, vi = lvx.predict_imu(g, s, t)
    gy2, ac2, vi2 = lvx.predict_imu(g, s, t)
    assert gy.tobytes() == gy2.tobytes() and ac.tobytes() == ac2.tobytes() and np.array_equal(vi, vi2) and np.array_equal(vi, ok)
    gd, ad = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    vd = torch.zeros((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lvx.predict_imu_d(g, t_d.data_ptr(), n, gd.data_ptr(), ad.data_ptr(), vd.data_ptr(), s_d.data_ptr())
    g.synchronize()
    assert gd.cpu().numpy().tobytes() == gy.tobytes() and ad.cpu().numpy().tobytes() == ac.tobytes() and np.array_equal(vd.cpu().numpy().astype(bool), vi)


@pytest.mark.parametrize("frame", [lvx.FRAME_LIDAR, lvx.FRAME_CAMERA])
def test_sensor_frames(scene, frame):
    """Pose and valid bit for bit lvx_evaluate_lidar_pose / lvx_evaluate_camera_pose; pose, velocity v + w x (R p_S) and w against the composition in numpy from the
    oracle; tau_S = +-3e-4 in the state moves the samples within 3e-4 of either end across the validity test; acceleration in a sensor frame is LVX_E_ARG."""
    P, g, o = scene["P"], scene["g"], scene["o"]
    N = P["n_knots"]
    t = tc.sensor_times(P)
    pose_fn = lvx.eval_lidar_pose if frame == lvx.FRAME_LIDAR else lvx.eval_camera_pose
    for tau in (None, 3e-4, -3e-4):
        s = tc.with_sensor_tau(P, P["state_true"], frame, tau)
        ok = tc.is_valid(P, t + tc.sensor_slots(s, N, frame)[2])
        got = lvx.sample_trajectory(g, s, t, frame, POSE_KIN)
        assert np.array_equal(got["valid"], ok)
        tc.assert_sensor_tau_moves_the_ends(ok, tau)
        q, p, v = pose_fn(g, s, t)
        assert np.array_equal(v, ok) and q[ok].tobytes() == got["orientation"][ok].tobytes() and p[ok].tobytes() == got["position"][ok].tobytes()
        for f in POSE_KIN:
            assert not got[f][~ok].any()
        pose_only = lvx.sample_trajectory(g, s, t, frame, ("position", "orientation"))
        assert _same_bits(got, pose_only, ("position", "orientation", "valid"))
        tc.check_fields(got, tc.oracle_sensor(o, P, s, frame), P, t, ok, np.zeros(0, int), len(t), {f: tc.BARS[f] for f in POSE_KIN}, "frame %d tau %s" % (frame, tau))
    with pytest.raises(lvx.LvxError) as e:
        lvx.sample_trajectory(g, P["state_true"], t, frame, ("acceleration",))
    assert e.value.code == lvx.E_ARG


def test_argument_and_state_errors(scene):
    import ctypes as C
    P, g = scene["P"], scene["g"]
    s, t = np.ascontiguousarray(P["state_true"]), np.array([P["t_start"]])
    with pytest.raises(lvx.LvxError) as e:
        lvx.sample_trajectory(g, s, t, 3)
    assert e.value.code == lvx.E_ARG
    smp, valid = lvx.TrajSamples(), np.zeros(1, np.int32)
    args = (g._h, s.ctypes.data_as(C.c_void_p), C.c_int(0))
    assert g._l.lvx_sample_trajectory(*args, C.c_int(1), t.ctypes.data_as(C.c_void_p), C.byref(smp)) == lvx.E_ARG          # NULL valid
    assert g._l.lvx_sample_trajectory(*args, C.c_int(1), t.ctypes.data_as(C.c_void_p), None) == lvx.E_ARG                  # NULL out
    smp.valid = valid.ctypes.data
    assert g._l.lvx_sample_trajectory(*args, C.c_int(0), t.ctypes.data_as(C.c_void_p), C.byref(smp)) == lvx.E_ARG          # n <= 0
    assert g._l.lvx_predict_imu(g._h, s.ctypes.data_as(C.c_void_p), C.c_int(1), t.ctypes.data_as(C.c_void_p), None, None, None) == lvx.E_ARG
    assert g._l.lvx_compare_poses(g._h, s.ctypes.data_as(C.c_void_p), C.c_int(1), C.c_int(1), t.ctypes.data_as(C.c_void_p), None, None, C.c_int(0), None, None, None) == lvx.E_ARG
    fresh = lvx.Context(0)
    try:
        for call in (lambda: lvx.sample_trajectory(fresh, s, t), lambda: lvx.predict_imu(fresh, s, t), lambda: lvx.compare_poses(fresh, s, 0, t, [[0, 0, 0, 1.0]], [[0, 0, 0.0]])):
            with pytest.raises(lvx.LvxError) as e:
                call()
            assert e.value.code == lvx.E_STATE
    finally:
        fresh.close()


@pytest.mark.parametrize("which", ["state_true", "state0"])
@pytest.mark.parametrize("tau_dt", [0.0, 0.3, -0.3])
def test_predicted_imu_matches_the_oracle_rows(scene, which, tau_dt):
    """meas - r / w from Oracle.evaluate at the problem's 600 stamps: gyro bar 1e-11 / w_gyro, accel bar 1e-11 / w_acc.  Repeated with tau_imu = +-0.3 dt written into the
    state; the stamps stay inside the range.  (tc.oracle_imu: how the oracle is given the offset; tc.check_fields: the 21 knot stamps at which its row is the model at
    t - 1e-5.)"""
    P, g = scene["P"], scene["g"]
    N = P["n_knots"]
    s = P[which].copy()
    s[7 * N + 7] = tau_dt * P["dt"]
    t, ok = P["t_imu"], np.ones(len(P["t_imu"]), bool)
    if tau_dt != 0.0:
        assert not tc.oracle_retries(P, t + s[7 * N + 7]).any()
        t_all, retried, n0 = t, np.zeros(0, int), len(t)
    else:
        t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok)
    gy, ac, valid = lvx.predict_imu(g, s, t_all)
    assert valid.all()
    tc.check_fields({"gyro": gy, "acc": ac}, tc.oracle_imu(P, s), P, t_all, ok, retried, n0, tc.imu_bars(P), "imu %s tau %.1f dt" % (which, tau_dt))


def test_nonunit_control_quaternion(scene):
    """One SO3 control point scaled by 1.001: the call returns LVX_E_NONUNIT_QUAT, exactly the in-range samples whose four-knot window holds that point are invalid (zeros),
    the others meet the bars (tests/test_traj_host.py shows first that the oracle evaluates them without an error).  The _d variant reports through lvx_synchronize, once."""
    import torch
    P, g, o = scene["P"], scene["g"], scene["o"]
    s, t, ok, hit = tc.nonunit_case(P, P["state_true"])
    t_all, retried, n0 = tc.with_oracle_stamps(P, t, ok & ~hit)
    with pytest.raises(lvx.LvxError) as e:
        lvx.sample_trajectory(g, s, t_all)
    assert e.value.code == lvx.E_NONUNIT_QUAT
    got = e.value.partial
    assert np.array_equal(got["valid"][:n0], ok & ~hit) and got["valid"][n0:].all()
    for f in lvx.TRAJ_FIELDS:
        assert not got[f][~got["valid"]].any()
    tc.check_fields(got, tc.oracle_spline(o, s), P, t_all, ok & ~hit, retried, n0, tc.BARS, "non-unit", grid_ok=lambda x: ~tc.nonunit_window(P, x))
    assert lvx.sample_trajectory(g, P["state_true"], t)["valid"].sum() == ok.sum()   # the flag does not outlive the call
    with pytest.raises(lvx.LvxError) as e:
        lvx.predict_imu(g, s, P["t_imu"])
    hitI = tc.nonunit_window(P, P["t_imu"])
    gy, ac, vi = e.value.partial
    assert e.value.code == lvx.E_NONUNIT_QUAT and np.array_equal(vi, ~hitI) and not gy[hitI].any() and not ac[hitI].any() and gy[~hitI].all()
    # LiDAR frame: the pose comes from lvx_pose.h, which reports the same windows
    ttL = t + tc.sensor_slots(s, P["n_knots"], lvx.FRAME_LIDAR)[2]
    with pytest.raises(lvx.LvxError) as e:
        lvx.sample_trajectory(g, s, t, lvx.FRAME_LIDAR, ("position", "orientation"))
    assert e.value.code == lvx.E_NONUNIT_QUAT and np.array_equal(e.value.partial["valid"], tc.is_valid(P, ttL) & ~tc.nonunit_window(P, ttL))
    dev = torch.device("cuda:0")
    t_d, s_d = torch.from_numpy(t).to(dev), torch.from_numpy(s).to(dev)
    pos, valid = torch.zeros((len(t), 3), dtype=torch.float64, device=dev), torch.zeros((len(t),), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lvx.sample_trajectory_d(g, t_d.data_ptr(), len(t), {"position": pos.data_ptr()}, valid.data_ptr(), lvx.FRAME_TRAJECTORY, s_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NONUNIT_QUAT and np.array_equal(valid.cpu().numpy().astype(bool), ok & ~hit)
    g.synchronize()   # reported once


def _lidar_reference(scene, t):
    P, o = scene["P"], scene["o"]
    ok = tc.is_valid(P, t + tc.sensor_slots(P["state_true"], P["n_knots"], lvx.FRAME_LIDAR)[2])
    q, p = np.zeros((len(t), 4)), np.zeros((len(t), 3))
    q[:, 3] = 1.0
    e = tc.oracle_sensor(o, P, P["state_true"], lvx.FRAME_LIDAR)(t[ok])
    q[ok], p[ok] = e["orientation"], e["position"]
    return q, p, ok


@pytest.mark.parametrize("n", [1, 2, 257])
def test_compare_poses(scene, n):
    """The reference is the oracle's LiDAR poses moved by planted errors (1 mm - 1 m, 1 mrad - 1 rad, one unique largest in each) and scaled by non-unit quaternion norms;
    for n = 257 two stamps in the middle are out of range, so n_valid < n and a relative pair bridges the gap.  Per-pose errors and the four summaries 1e-11 against
    tc.np_pose_errors on the oracle's poses; argmax exact; relative summaries the same bits under both alignments; a rigidly moved reference; n_valid = 0; a repeat."""
    P, g = scene["P"], scene["g"]
    s = P["state_true"]
    tmin, tmax = tc.time_range(P)
    t = np.linspace(tmin + 0.0101, tmax - 0.0101, n)
    if n == 257:
        t[100], t[101] = tmax + 1.0, tmin - 1.0
    Tq, Tp, ok = _lidar_reference(scene, t)
    assert ok.sum() == (n - 2 if n == 257 else n)
    qr, pr, it, ir = tc.planted_reference(np.random.default_rng(n), Tq, Tp, ok)
    qr[~ok], pr[~ok] = [0.3, 0.1, -0.2, 0.7], [1.0, 2.0, 3.0]
    got0, got1 = lvx.compare_poses(g, s, lvx.FRAME_LIDAR, t, qr, pr, lvx.ALIGN_NONE), lvx.compare_poses(g, s, lvx.FRAME_LIDAR, t, qr, pr, lvx.ALIGN_FIRST)
    tc.assert_errors_close(got0, tc.np_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_NONE))
    tc.assert_errors_close(got1, tc.np_pose_errors(Tq, Tp, ok, qr, pr, lvx.ALIGN_FIRST))
    assert got0["n_valid"] == ok.sum() and got0["abs_trans"]["argmax"] == it and got0["abs_rot"]["argmax"] == ir
    assert abs(got0["abs_trans"]["max"] - 1.0) <= tc.BAR_E and abs(got0["abs_rot"]["max"] - 1.0) <= tc.BAR_E and got0["rel_trans"]["n"] == ok.sum() - 1
    assert got0["rel_trans"] == got1["rel_trans"] and got0["rel_rot"] == got1["rel_rot"]   # the same bits under both alignments
    assert not got0["abs_trans_n"][~ok].any() and not got0["abs_rot_n"][~ok].any()
    rep = lvx.compare_poses(g, s, lvx.FRAME_LIDAR, t, qr, pr, lvx.ALIGN_FIRST)
    assert all(rep[k] == got1[k] for k in ("n_valid", "abs_trans", "abs_rot", "rel_trans", "rel_rot")) and rep["abs_trans_n"].tobytes() == got1["abs_trans_n"].tobytes()
    # the reference moved rigidly on the left: ALIGN_FIRST undoes it, ALIGN_NONE reports metres
    G = (synth.q_from_rotvec(np.array([0.4, -0.7, 1.1])), np.array([3.0, -2.0, 5.0]))
    qg, pg = synth.qmul(np.broadcast_to(G[0], Tq.shape), Tq) * 1.7, synth.qrot(np.broadcast_to(G[0], Tq.shape), Tp) + G[1]
    a1, a0 = lvx.compare_poses(g, s, lvx.FRAME_LIDAR, t, qg, pg, lvx.ALIGN_FIRST), lvx.compare_poses(g, s, lvx.FRAME_LIDAR, t, qg, pg, lvx.ALIGN_NONE)
    print("rigidly moved reference, ALIGN_FIRST: max abs %.3e m %.3e rad" % (a1["abs_trans"]["max"], a1["abs_rot"]["max"]))
    assert max(a1["abs_trans"]["max"], a1["abs_rot"]["max"]) <= tc.BAR_E and a0["abs_trans"]["mean"] > 1.0 and a0["abs_rot"]["mean"] > 0.5
    zero = {"rmse": 0.0, "mean": 0.0, "max": 0.0, "argmax": 0, "n": 0}
    z = lvx.compare_poses(g, s, lvx.FRAME_LIDAR, np.full(n, tmax + 2.0), qr, pr, lvx.ALIGN_FIRST)   # LVX_OK
    assert z["n"] == n and z["n_valid"] == 0 and all(z[k] == zero for k in ("abs_trans", "abs_rot", "rel_trans", "rel_rot")) and not z["abs_trans_n"].any()


def test_cpp_free_functions_print_what_python_returns(scene, tmp_path):
    """tests/native/traj_demo.cpp: SampleTrajectory and ComparePoses of lvx_calibrate.hpp on a context of its own, the same state, stamps and poses — to the last digit."""
    P = scene["P"]
    g = scene["g"]
    N = P["n_knots"]
    assert len(P["state_true"]) == 7 * N + 32
    libdir = os.path.join(tc.ROOT, "lvi-exc_amd")
    exe, data = str(tmp_path / "traj_demo"), str(tmp_path / "traj.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(tc.ROOT, "tests", "native", "traj_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    tmin, tmax = tc.time_range(P)
    rng = np.random.default_rng(77)
    for frame in (lvx.FRAME_TRAJECTORY, lvx.FRAME_LIDAR):
        s = P["state0"]
        t = np.concatenate([rng.uniform(tmin, tmax, 40), [tmax, tmin]])
        stamps = np.round(np.concatenate([np.linspace(tmin + 0.05, tmax - 0.05, 12), [tmax + 1.0]]) * 1e9).astype(np.int64)
        tp = stamps.astype(np.float64) * 1e-9
        q = rng.standard_normal((len(tp), 4))
        p = rng.standard_normal((len(tp), 3))
        poses = np.column_stack([stamps.astype(np.float64), p, q[:, 3], q[:, :3]])
        assert np.array_equal(poses[:, 0].astype(np.int64), stamps)
        with open(data, "wb") as f:
            f.write(np.concatenate([[N, P["t0"], P["dt"], frame, lvx.ALIGN_FIRST, len(t), len(tp)], s, t, poses.ravel()]).astype(np.float64).tobytes())
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        fields = ("position", "velocity", "acceleration", "angular_velocity", "orientation") if frame == 0 else ("position", "velocity", "angular_velocity", "orientation")
        smp = lvx.sample_trajectory(g, s, t, frame, fields)
        want = ["sample %d " % smp["valid"][i] + " ".join("%.17g" % x for f in fields for x in smp[f][i]) for i in range(len(t))]
        c = lvx.compare_poses(g, s, frame, tp, q, p, lvx.ALIGN_FIRST)
        want.append("errors %d %d" % (c["n"], c["n_valid"]))
        want += ["summary %.17g %.17g %.17g %d %d" % (c[k]["rmse"], c[k]["mean"], c[k]["max"], c[k]["argmax"], c[k]["n"]) for k in ("abs_trans", "abs_rot", "rel_trans", "rel_rot")]
        want += ["abs %.17g %.17g" % (a, b) for a, b in zip(c["abs_trans_n"], c["abs_rot_n"])]
        assert c["n_valid"] == 12 and r.stdout.splitlines() == want
