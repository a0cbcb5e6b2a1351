"""GPU: LiDAR odometry position blocks (lvx_set_lidar_poses) through the C ABI against the oracle's converted problem (tests/lidarpos_cases.py: three surfel blocks
with p_L = 0 and planes p_meas,i e_i per position block; the oracle's surfel row is sign(p_meas,i) times the block's row i, so J^T J, J^T r and the cost are the same).

Bars are the ones tests/test_gpu_eval.py holds the surfel family to: residual rows 1e-11 of the largest residual, cost 1e-12 relative, Jacobian rows 1e-9 of the
largest entry, H and g 1e-10 of their largest entry and every H entry 1e-9 of sqrt(H_ii H_jj); one damped step 1e-7 of the largest step entry
(tests/test_gpu_solver.py); converged extrinsics 1e-6 rad / 1e-4 m (tests/test_gpu_converge_oracle.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lidarpos_cases as lc
import lvx
import stages
import synth
import traj_cases as tc
from oracle import lm
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TAU = lc.TAU


def _t_start(P):
    return P["t0"] + 10.37 * P["dt"]


@functools.lru_cache(maxsize=None)
def _case(kind, n, outliers=0, seed=0):
    P = lc.problem()
    return lc.Case(P, lc.pose_times(P, n, _t_start(P), kind, seed), _t_start(P), outliers=outliers, seed=seed)


@functools.lru_cache(maxsize=None)
def _state(amp=1e-2):
    s = lc.perturbed_state(lc.problem(), amp=amp)
    s.setflags(write=False)
    return s


def _pair(P, case, locks):
    """(oracle of the converted problem, sign of its surfel rows, context with the position blocks)."""
    Q, sign = lc.converted_problem(P, case)
    o = tc.make_oracle(Q)
    o.set_locks(locks)
    g = lvx.Context(0)
    lvx.load_problem(g, P, locks)
    lc.load_case(g, case)
    return o, sign, g


def _row_sign(o, sign, n_rows):
    s = np.ones(n_rows)
    r0 = lc.oracle_surfel_rows(o)
    s[r0:r0 + len(sign)] = sign
    return s


def _assert_blockscaled(Hg, Ho, tol=1e-9):
    d = np.sqrt(np.maximum(np.diag(Ho), 0.0))
    scale = np.outer(d, d)
    bad = np.abs(Hg - Ho) > tol * scale + 1e-300
    assert not bad.any(), "worst entry-scaled error %.3e" % (np.abs(Hg - Ho)[bad] / np.maximum(scale[bad], 1e-300)).max()


def _compare(o, sign, g, state, tag):
    ro = o.evaluate(state, jac=True, normal_eq=True)
    nt = o.tangent_size
    sg = _row_sign(o, sign, len(ro["residuals"]))
    r_ref = sg * ro["residuals"]
    J_ref = sg[:, None] * O.dense_jacobian(ro["jac_cols"], ro["jac_vals"], nt)
    rs, Hs, gs = np.abs(r_ref).max(), np.abs(ro["H"]).max(), np.abs(ro["g"]).max()
    r0, m = lc.oracle_surfel_rows(o), len(sign)
    for jac in (True, False):   # the debug Jacobian takes the per-segment kernels for every family; without it the fused IMU kernel runs beside the position blocks
        rg = g.evaluate(state, jac=jac, normal_eq=True)
        assert rg["residuals"].shape == r_ref.shape
        e = dict(rows=np.abs(rg["residuals"] - r_ref).max() / rs, cost=abs(rg["cost"] - ro["cost"]) / abs(ro["cost"]), H=np.abs(rg["H"] - ro["H"]).max() / Hs,
                 g=np.abs(rg["g"] - ro["g"]).max() / gs)
        # the position rows against THEIR largest entry (the weighted IMU rows are two orders larger)
        e["pose_rows"] = np.abs(rg["residuals"][r0:r0 + m] - r_ref[r0:r0 + m]).max() / np.abs(r_ref[r0:r0 + m]).max()
        if jac:
            Jg = O.dense_jacobian(rg["jac_cols"], rg["jac_vals"], nt)
            e["J"] = np.abs(Jg - J_ref).max() / np.abs(J_ref).max()
            e["pose_J"] = np.abs(Jg[r0:r0 + m] - J_ref[r0:r0 + m]).max() / np.abs(J_ref[r0:r0 + m]).max()
        print("%s jac=%d: %s" % (tag, jac, ", ".join("%s %.2e" % kv for kv in e.items())))
        assert e["rows"] <= 1e-11 and e["cost"] <= 1e-12 and e["H"] <= 1e-10 and e["g"] <= 1e-10 and e.get("J", 0.0) <= 1e-9
        assert e["pose_rows"] <= 1e-11 and e.get("pose_J", 0.0) <= 1e-9
        _assert_blockscaled(rg["H"], ro["H"])
    return ro, rg, r_ref, J_ref


@pytest.mark.parametrize("kind,n", [("spread", 1), ("spread", 63), ("spread", 64), ("spread", 65), ("spread", 130), ("dense", 16), ("hub", 9)])
def test_rows_jacobian_cost_and_normal_equations_against_the_converted_oracle(kind, n):
    P = lc.problem()
    case = _case(kind, n)
    o, sign, g = _pair(P, case, TAU)
    try:
        r0, total = g.lidar_pose_rows()
        assert g.family_rows()[-1] == r0 == 6 * len(P["t_imu"]) and total == r0 + 3 * n == g.layout()["n_residuals"]
        _compare(o, sign, g, _state(), "%s n=%d" % (kind, n))
        if kind == "hub":   # merged segments: the block AT t_start has both poses on the same four knots (two local columns per tangent index)
            assert case.t[0] == case.t_start and g.layout()["exact_fallback"] == 0
    finally:
        g.close()


def test_huber_acts_on_the_block_norm():
    """Planted 10 m outliers (block norm > 5) and blocks moved by 4.8 m (just inside): cost, H and g against numpy built from the oracle's PRE-LOSS rows with the
    block-norm scale sqrt(5 / |r|); n_outliers from the statistics call."""
    P = lc.problem()
    base = _case("spread", 65, outliers=6, seed=2)
    case = lc.Case(P, base.t, base.t_start)
    case.p_meas = base.p_meas.copy()
    inside = np.setdiff1d(np.arange(case.n), base.outlier_idx)[:5]
    case.p_meas[inside, 0] += 4.8
    s = _state(1e-3)
    o, sign, g = _pair(P, case, TAU)
    try:
        ro = o.evaluate(s, jac=True)
        r0 = lc.oracle_surfel_rows(o)
        rows = sign * ro["residuals"][r0:]
        J = sign[:, None] * O.dense_jacobian(ro["jac_cols"], ro["jac_vals"], o.tangent_size)[r0:]
        norms = np.linalg.norm(rows.reshape(-1, 3), axis=1)
        assert (norms[base.outlier_idx] > 5.0).all() and (norms[inside] > 4.5).all() and (norms[inside] < 5.0).all() and (norms > 5.0).sum() == 6
        o_imu = tc.make_oracle(P)
        ri = o_imu.evaluate(s, normal_eq=True)
        c_lp, H_lp, g_lp = lc.np_huber_system(rows, J, case.huber)
        H_ref, g_ref, c_ref = ri["H"] + H_lp, ri["g"] + g_lp, ri["cost"] + c_lp
        rg = g.evaluate(s, normal_eq=True)
        e = (abs(rg["cost"] - c_ref) / c_ref, np.abs(rg["H"] - H_ref).max() / np.abs(H_ref).max(), np.abs(rg["g"] - g_ref).max() / np.abs(g_ref).max())
        print("huber: cost %.2e H %.2e g %.2e; pose share of the cost %.3f" % (e + (c_lp / c_ref,)))
        assert e[0] <= 1e-12 and e[1] <= 1e-10 and e[2] <= 1e-10
        _assert_blockscaled(rg["H"], H_ref)
        assert np.abs(rg["residuals"][r0:] - rows).max() <= 1e-11 * np.abs(rows).max()   # the rows stay pre-loss
        st = g.lidar_pose_statistics(s)
        assert st["n_blocks"] == case.n == st["n_evaluated"] and st["n_outliers"] == 6
        lc.assert_stats_close(st, lc.np_stats(rows, case.weight, case.huber), tol=1e-11)
        st2 = g.lidar_pose_statistics(s)
        assert all(np.array_equal(st[k], st2[k]) for k in st)   # fixed order: identical bits
    finally:
        g.close()


@pytest.mark.parametrize("name,locks", [("lidar_locked", TAU | lvx.LOCK_LIDAR_Q | lvx.LOCK_LIDAR_P), ("traj_locked", TAU | lvx.LOCK_TRAJ), ("tau_free", lvx.LOCK_CAM_TAU)])
def test_lock_masks(name, locks):
    P = lc.problem()
    N = P["n_knots"]
    case = _case("spread", 65)
    o, sign, g = _pair(P, case, locks)
    try:
        ro, rg, _, J_ref = _compare(o, sign, g, _state(), name)
        rj = g.evaluate(_state(), jac=True, normal_eq=True)
        Jg = O.dense_jacobian(rj["jac_cols"], rj["jac_vals"], o.tangent_size)
        dead = {"lidar_locked": np.arange(6 * N + 8, 6 * N + 15), "traj_locked": np.concatenate([np.arange(6 * N), [6 * N + 14]]), "tau_free": np.arange(0)}[name]
        assert not Jg[:, dead].any() and not rj["H"][dead].any() and not rj["H"][:, dead].any() and not rj["g"][dead].any()
        if name == "tau_free":
            r0 = lc.oracle_surfel_rows(o)
            assert np.abs(Jg[r0:, 6 * N + 14]).max() > 0 and rj["H"][6 * N + 14, 6 * N + 14] > 0
    finally:
        g.close()


@functools.lru_cache(maxsize=None)
def _mixed_problem():
    return synth.make_problem(seed=7, duration=1.5, n_surfel=300, n_planes=8, n_landmarks=20, n_camsurf=6)


def _mixed_case(P, n=40):
    return lc.Case(P, lc.pose_times(P, n, P["t_map"], "spread", 1), P["t_map"])


def test_mixed_pass_with_surfels_reprojection_and_camera_surfels():
    """Poses beside all six families at an equal t_map: the old families' rows, family_rows() and H contributions are unchanged; H with poses = the oracle's H of the
    problem without them + J^T J of the pose rows (from the converted oracle).  A different start time: LVX_E_ARG."""
    P = _mixed_problem()
    case = _mixed_case(P)
    s = P["state0"]
    g = lvx.Context(0)
    try:
        lvx.load_problem(g, P, TAU)
        r1 = g.evaluate(s, normal_eq=True)
        rows1, n1 = g.family_rows(), g.layout()["n_residuals"]
        lc.load_case(g, case)
        r2 = g.evaluate(s, normal_eq=True)
        assert g.family_rows() == rows1 and g.lidar_pose_rows() == (n1, n1 + 3 * case.n)
        assert np.array_equal(r2["residuals"][:n1], r1["residuals"])
        Q, sign = lc.converted_problem(P, case)
        oq = tc.make_oracle(Q)
        rq = oq.evaluate(s, jac=True)
        q0 = lc.oracle_surfel_rows(oq)
        rows = sign * rq["residuals"][q0:q0 + 3 * case.n]
        J = sign[:, None] * O.dense_jacobian(rq["jac_cols"], rq["jac_vals"], oq.tangent_size)[q0:q0 + 3 * case.n]
        assert np.linalg.norm(rows.reshape(-1, 3), axis=1).max() < 5.0
        ro = tc.make_oracle(P).evaluate(s, normal_eq=True)
        H_ref, g_ref = ro["H"] + J.T @ J, ro["g"] + J.T @ rows
        Hs = np.abs(H_ref).max()
        print("mixed: |H2 - (H_oracle + H_poses)| %.2e, |(H2 - H_poses) - H1| %.2e of max |H|" % (np.abs(r2["H"] - H_ref).max() / Hs, np.abs(r2["H"] - J.T @ J - r1["H"]).max() / Hs))
        assert np.abs(r2["residuals"][n1:] - rows).max() <= 1e-11 * np.abs(rows).max()
        assert np.abs(r2["H"] - H_ref).max() <= 1e-10 * Hs and np.abs(r2["g"] - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
        assert np.abs(r2["H"] - J.T @ J - r1["H"]).max() <= 1e-10 * Hs
        assert abs(r2["cost"] - ro["cost"] - 0.5 * rows @ rows) <= 1e-12 * r2["cost"]
        _assert_blockscaled(r2["H"], H_ref)
        g.set_lidar_poses(case.t, case.p_meas, np.nextafter(case.t_start, np.inf), case.huber, case.weight)
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(s)
        assert ei.value.code == lvx.E_ARG
        g.set_lidar_poses(np.zeros(0), np.zeros((0, 3)), case.t_start)
        r3 = g.evaluate(s, normal_eq=True)
        assert g.layout()["n_residuals"] == n1 and np.array_equal(r3["residuals"], r1["residuals"])
    finally:
        g.close()


def test_poses_with_reprojection_blocks_only():
    """What the four-argument trajInitFromLVIdata assembles: IMU + position + reprojection blocks, no surfel map — directly against the converted oracle."""
    P = dict(_mixed_problem())
    P["surf_pt"], P["surf_t"], P["surf_plane"] = P["surf_pt"][:0], P["surf_t"][:0], P["surf_plane"][:0]
    P["cs_lm"], P["cs_plane"] = P["cs_lm"][:0], P["cs_plane"][:0]
    case = _mixed_case(P)
    Q, sign = lc.converted_problem(P, case)
    o = tc.make_oracle(Q)
    g = lvx.Context(0)
    try:
        lvx.load_problem(g, P, TAU)
        lc.load_case(g, case)
        s = P["state0"]
        ro = o.evaluate(s, normal_eq=True)
        rg = g.evaluate(s, normal_eq=True)
        # rows: gyro, accel, (surfel = converted | reprojection) in the oracle; gyro, accel, reprojection, poses on the device
        q0, m = lc.oracle_surfel_rows(o), 3 * case.n
        r_ref = np.concatenate([ro["residuals"][:q0], ro["residuals"][q0 + m:], sign * ro["residuals"][q0:q0 + m]])
        assert np.abs(rg["residuals"] - r_ref).max() <= 1e-11 * max(np.abs(r_ref).max(), 100.0)   # pixel coordinates up to 1e3 (tests/test_gpu_eval.py: res_floor)
        assert abs(rg["cost"] - ro["cost"]) <= 1e-12 * ro["cost"]
        assert np.abs(rg["H"] - ro["H"]).max() <= 1e-10 * np.abs(ro["H"]).max() and np.abs(rg["g"] - ro["g"]).max() <= 1e-10 * np.abs(ro["g"]).max()
        _assert_blockscaled(rg["H"], ro["H"])
    finally:
        g.close()


def test_solve_step_matches_dense():
    P = lc.problem()
    case = _case("spread", 65)
    locks = stages.stage_locks("TrajFromLidarPose")
    o, sign, g = _pair(P, case, locks)
    try:
        s = _state()
        ro = o.evaluate(s, normal_eq=True)
        g.evaluate(s, normal_eq=True, dense=False)
        d_gpu, m_gpu = g.solve_step(1e4, True)
        free = lm.free_tangent_indices(P["n_knots"], 0, locks)
        scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(ro["H"])[free], 0)))
        d_ref, m_ref, _ = lm.solve_step(ro["H"], ro["g"], free, 1e4, scale)
        print("solve step: %.2e of the largest entry" % (np.abs(d_gpu - d_ref).max() / np.abs(d_ref).max()))
        assert np.abs(d_gpu - d_ref).max() <= 1e-7 * np.abs(d_ref).max()
        assert abs(m_gpu - m_ref) <= 1e-8 * abs(m_ref)
    finally:
        g.close()


def _qang(a, b):
    d = synth.qmul(a, synth.qconj(b))
    return 2 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


def _perturbed_extrinsics(P):
    """The start state with the LiDAR extrinsics 3 degrees / 5 cm off the planted ones."""
    N = P["n_knots"]
    s = np.array(P["state0"], np.float64)
    t = np.array(P["state_true"], np.float64)
    s[7 * N + 16:7 * N + 20] = synth.qmul(t[7 * N + 16:7 * N + 20], synth.q_from_rotvec(np.deg2rad(3.0) * np.array([0.6, -0.64, 0.48])))
    s[7 * N + 20:7 * N + 23] = t[7 * N + 20:7 * N + 23] + 0.05 * np.array([0.48, 0.6, -0.64])
    s[7 * N + 23] = 0.0
    return s


def _stamped_case(P, n=40):
    """Poses on integer-nanosecond stamps (a LOAM pose file), the first one AT the start time."""
    t = lc.pose_times(P, n, _t_start(P), "spread", 4)
    stamp = np.concatenate([[int(round(_t_start(P) * 1e9))], np.round(t * 1e9).astype(np.int64)]).astype(np.int64)
    tt = stamp.astype(np.float64) * 1e-9
    return stamp, lc.Case(P, tt, tt[0], noise=1e-3, seed=9)


def _check_converged(P, o, free, s0, x_gpu, acc_gpu, term_gpu, it_gpu, tag):
    N = P["n_knots"]
    xo, so = lm.lm_solve(o, s0, free, max_iterations=50, n_knots=N, n_landmarks=0)
    print("%s: %d iterations, termination %s, accepted %s" % (tag, it_gpu, term_gpu, list(acc_gpu)))
    assert it_gpu == so["iterations"] and term_gpu == so["termination"] and list(acc_gpu) == list(so["accepted"])
    ug, uo, ut = synth.unpack_state(x_gpu, N, 0), synth.unpack_state(xo, N, 0), synth.unpack_state(P["state_true"], N, 0)
    e_q, e_p = _qang(ug["lidar"][:4], uo["lidar"][:4]), np.abs(ug["lidar"][4:7] - uo["lidar"][4:7]).max()
    print("%s: extrinsics vs oracle LM %.2e rad %.2e m; vs planted %.2e rad %.2e m" % (tag, e_q, e_p, _qang(ug["lidar"][:4], ut["lidar"][:4]), np.abs(ug["lidar"][4:7] - ut["lidar"][4:7]).max()))
    assert e_q <= 1e-6 and e_p <= 1e-4
    return xo


def test_traj_init_from_lidar_pose_by_lm_solve():
    P = lc.problem()
    _, case = _stamped_case(P)
    locks = stages.stage_locks("TrajFromLidarPose")
    o, sign, g = _pair(P, case, locks)
    try:
        s0 = _perturbed_extrinsics(P)
        free = lm.free_tangent_indices(P["n_knots"], 0, locks)
        assert g.lidar_pose_statistics(s0)["n_outliers"] == 0
        xg, sg = g.lm_solve(s0, max_iterations=50)
        assert g.lidar_pose_statistics(xg)["n_outliers"] == 0
        _check_converged(P, o, free, s0, xg, sg["accepted"], sg["termination"], sg["iterations"], "lm_solve")
        assert sg["final_cost"] < sg["initial_cost"]
    finally:
        g.close()


def _offset_case(P, tau, n=40):
    """Poses measured tau seconds late: the positions are the planted trajectory's at t + tau (planted LiDAR offset tau in the generating state)."""
    N = P["n_knots"]
    _, case = _stamped_case(P, n)
    st = np.array(P["state_true"], np.float64)
    st[7 * N + 23] = tau
    rng = np.random.default_rng(31)
    pm = lc.np_measure(tc.make_oracle(P), st, N, case.t, case.t_start) + 1e-3 * rng.standard_normal((case.n, 3))
    small = np.abs(pm) < 1e-3
    pm[small] = np.where(pm[small] < 0, -1.0, 1.0) * 2e-3
    case.p_meas = pm
    return case


@pytest.mark.parametrize("tau", [4e-4, 3e-3])
def test_traj_init_from_lidar_pose_with_a_free_time_offset(tau):
    """trajInitFromLidarPose with opt_time_offset: the LiDAR offset is a bounded parameter block of the problem (LiDARPositionMeasurement::AddToEstimator adds the LiDAR
    to it), so the solve is constrained in Ceres' sense — projected start point and gradient norm, projected line search — as oracle/lm.py runs it on the converted
    problem (its surfel blocks make the offset part of the problem there).  Planted offsets inside the bound (0.4 ms of 1 ms) and three times beyond it."""
    P = lc.problem()
    N = P["n_knots"]
    case = _offset_case(P, tau)
    locks = stages.stage_locks("TrajFromLidarPose", opt_time_offset=True)
    assert not locks & lvx.LOCK_LIDAR_TAU
    o, sign, g = _pair(P, case, locks)
    try:
        s0 = _perturbed_extrinsics(P)
        free = lm.free_tangent_indices(N, 0, locks)
        assert 6 * N + 14 in free
        xg, sg = g.lm_solve(s0, max_iterations=50)
        xo = _check_converged(P, o, free, s0, xg, sg["accepted"], sg["termination"], sg["iterations"], "free offset %g" % tau)
        print("free offset: tau_L device %.6e oracle %.6e (planted %.1e, bound 1e-3)" % (xg[7 * N + 23], xo[7 * N + 23], tau))
        assert abs(xg[7 * N + 23] - xo[7 * N + 23]) <= 1e-9 and abs(xg[7 * N + 23]) <= 1e-3
        assert g.lidar_pose_statistics(xg)["n_outliers"] == 0
    finally:
        g.close()


def test_traj_init_from_lidar_pose_by_the_calibrator(tmp_path):
    """Calibrator::RunLidarPoses in a compiled C++ program: Solve #0, then trajInitFromLidarPose on a pose file; the second stage against oracle/lm.py from the state
    the first one left."""
    P = lc.problem()
    N = P["n_knots"]
    assert P["w_gyro"] == 28.0 and P["w_acc"] == 18.0   # CalibrateOptions' defaults
    stamp, full = _stamped_case(P)
    # the pose file: the first pose is the odometry's origin, and the whole file sits in another frame (q_a, t_a) — RunLidarPoses re-expresses it in the first pose's
    p_L0 = full.p_meas.copy(); p_L0[0] = 0.0
    q_a = synth.q_from_rotvec(np.array([0.3, -0.2, 0.5])); t_a = np.array([1.5, -2.0, 0.7])
    p_file = synth.qrot(np.broadcast_to(q_a, (full.n, 4)), p_L0) + t_a
    pose_file = str(tmp_path / "loam_poses.txt")
    synth.write_loam_pose_file(pose_file, stamp, p_file, np.tile([q_a[3], q_a[0], q_a[1], q_a[2]], (full.n, 1)))
    # the block AT the start time measures p = 0 there: its rows and Jacobian vanish identically, and the conversion cannot express it — the oracle's problem leaves it out
    case = lc.Case(P, full.t[1:], full.t_start)
    case.p_meas = full.p_meas[1:].copy()
    s0 = _perturbed_extrinsics(P)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([P["t0"], P["dt"], float(N)])]
    for a in (s0, P["t_imu"], P["gyro"], P["acc"]):
        a = np.ascontiguousarray(a, np.float64).ravel()
        parts += [np.array([float(a.size)]), a]
    np.concatenate(parts).tofile(pin)
    libdir = os.path.join(tc.ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "lidarpos_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(tc.ROOT, "tests", "native", "lidarpos_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, pin, pout, pose_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    st = [l.split() for l in lines if l.startswith("stage")]
    assert [w[1] for w in st] == ["initialSO3TrajWithGyro", "trajInitFromLidarPose"]
    iters, term, n_poses, out_before, out_after = (int(v) for v in st[1][2:7])
    assert n_poses == full.n == case.n + 1 and out_before == 0 and out_after == 0
    accepted = [int(v) for v in [l for l in lines if l.startswith("accepted")][1].split()[1:]]
    x = np.fromfile(pout).reshape(2, -1)
    locks = stages.stage_locks("TrajFromLidarPose")
    Q, _ = lc.converted_problem(P, case)
    o = tc.make_oracle(Q)
    o.set_locks(locks)
    free = lm.free_tangent_indices(N, 0, locks)
    _check_converged(P, o, free, x[0], x[1], accepted, lvx.LM_TERMINATION[term], iters, "Calibrator")


def test_range_and_argument_errors():
    P = lc.problem()
    case = _case("spread", 9)
    s = _state()
    g = lvx.Context(0)
    try:
        lvx.load_problem(g, P, TAU)
        n0 = g.layout()["n_residuals"]
        t_bad = case.t.copy(); t_bad[3] = tc.time_range(P)[1] + 1e-3
        g.set_lidar_poses(t_bad, case.p_meas, case.t_start)
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(s)
        assert ei.value.code == lvx.E_RANGE
        rc, st = g.lidar_pose_statistics(s, raw=True)
        assert rc == lvx.E_RANGE and st["n_blocks"] == 9 and st["n_evaluated"] == 8
        lc.load_case(g, case)
        assert g.layout()["n_residuals"] == n0 + 27
        g.evaluate(s)
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(s, jac_blocks=True)
        assert ei.value.code == lvx.E_ARG
        g.set_switch("DETERMINISTIC", 1)
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(s)
        assert ei.value.code == lvx.E_ARG
        g.set_switch("DETERMINISTIC", 0)
        g.set_lidar_poses(np.zeros(0), np.zeros((0, 3)), case.t_start)
        assert g.layout()["n_residuals"] == n0 and g.lidar_pose_rows() == (n0, n0)
        g.evaluate(s, jac_blocks=True)
        assert g.lidar_pose_statistics(s)["n_blocks"] == 0
    finally:
        g.close()


def test_a_pass_without_poses_launches_nothing_new():
    """The position kernel has an id of its own beyond the 17 of kernel_ms(): launched once per pass with poses, never without."""
    P = lc.problem()
    g = lvx.Context(0)
    try:
        lvx.load_problem(g, P, TAU)
        g.set_profiling(True); g.kernel_ms_ext()
        g.evaluate(_state(), normal_eq=True, dense=False)
        _, n_without = g.kernel_ms_ext()
        lc.load_case(g, _case("spread", 9))
        g.evaluate(_state(), normal_eq=True, dense=False)
        _, n_with = g.kernel_ms_ext()
        assert n_without[lvx.KERNEL_LIDAR_POS] == 0 and n_with[lvx.KERNEL_LIDAR_POS] == 1
        assert list(n_with[:17]) == list(n_without[:17]) and len(g.kernel_ms()[0]) == 17
    finally:
        g.close()
