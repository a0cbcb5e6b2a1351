"""lvx_trajectory_covariance on the device: the covariance of trajectory poses in the damped LM system at a stated radius, from the selected inverse of the sequential
factor (k_border_inv, k_band_selinv, k_pose_cov), against the float64 Cholesky inverse of the SAME damped system built from the device's own dense export, restricted
to window_idx (tests/trajcov_cases.py).

Window bar: calib_cov_cases.rel_err over the live rows of a window; a case may use 10 x the reference's own error against mpmath at 40 digits
(tests/golden/trajcov_ref.npz, written by tests/golden/make_trajcov_ref.py from the oracle's H), floor 1e-11.
Pose covariance bar: against J_fd W_ref J_fd^T with J_fd from Context.plus + lvx.sample_trajectory (central differences, Richardson): 10 x (the change of that product
between the two Richardson levels + the window bar carried through |J|: tol (|J| d)_r (|J| d)_s / sqrt(cov_rr cov_ss), d = sqrt(diag W_ref)).
The reference's own error per case, the bar and the observed figures are printed by every test (-s) and recorded in docs/HISTORY.md."""
import os

import numpy as np
import pytest

import calib_cov_cases as CC
import lvx
import synth
import trajcov_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "trajcov_ref.npz")))
FRAMES = (lvx.FRAME_TRAJECTORY, lvx.FRAME_LIDAR, lvx.FRAME_CAMERA)
_P = {}


def _problem(key="small"):
    if key not in _P:
        _P[key] = synth.make_problem(**CC.SMALL) if key == "small" else (synth.make_problem(**CC.ND) if key == "nd" else TC.r3_problem())
    return _P[key]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _context(P, locks, switches=(), r3=False):
    g = lvx.Context(0)
    for k, v in switches:
        g.set_switch(k, v)
    if r3:
        TC.load_r3(g, P)
    else:
        lvx.load_problem(g, P, locks)
    return g


def _check_windows(g, P, locks, radius, scaling, tol, label, frames=FRAMES):
    """evaluate, export, reference; every frame's windows over trajcov_cases.query_times.  Returns {frame: record}, Sigma_ref, free."""
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, scaling)
    t = TC.query_times(P)
    out = {}
    for frame in frames:
        r = g.trajectory_covariance(t, frame, radius, scaling, window=True)
        assert r["valid"][:-2].all() and not r["valid"][-2:].any()
        assert not r["cov"][-2:].any() and not r["sigma"][-2:].any() and not r["window_cov"][-2:].any() and (r["window_idx"][-2:] == -1).all()
        worst = 0.0
        for i in range(len(t) - 2):
            want = np.array(TC.window_indices(P, t[i], frame))
            want[~np.isin(want, free)] = -1
            assert np.array_equal(r["window_idx"][i], want), (label, frame, i)
            Wr = TC.window_of(Sig, free, want)
            dead = want < 0
            assert not r["window_cov"][i][dead].any() and not r["window_cov"][i][:, dead].any()
            assert np.array_equal(r["window_cov"][i], r["window_cov"][i].T) and np.array_equal(r["cov"][i], r["cov"][i].T)
            worst = max(worst, TC.window_rel_err(r["window_cov"][i], Wr))
        assert np.array_equal(r["sigma"], np.sqrt(np.einsum("nii->ni", r["cov"])))
        print("%-28s frame %d: window err %.3e (allowed %.3e)" % (label, frame, worst, tol))
        assert worst <= tol
        out[frame] = r
    return out, Sig, free, t


# 1. parity with the same damped system
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("mask", ["solve1", "solve2", "solve3"])
def test_windows_match_the_damped_system(mask, radius, scaling):
    P = _problem()
    locks = CC.MASKS[mask]
    g = _context(P, locks)
    name = CC.case_name(mask, radius, scaling)
    out, Sig, free, t = _check_windows(g, P, locks, radius, scaling, _tol(name), name)
    if mask == "solve3":   # the trajectory is constant: no band, the pose moves with the sensor's extrinsics only
        assert g.layout()["n_band"] == 0
        assert not out[lvx.FRAME_TRAJECTORY]["cov"].any() and not out[lvx.FRAME_TRAJECTORY]["window_cov"].any()
        c = g.calibration_covariance(radius, scaling)
        blk = c["cov"][15:21, 15:21]
        for i in range(len(t) - 2):
            Wd = out[lvx.FRAME_CAMERA]["window_cov"][i]
            assert not Wd[:24].any() and CC.rel_err(Wd[24:30, 24:30], blk) <= _tol(name)
    g.close()


def test_plan_of_the_solver_is_ignored():
    """SOLVER_ND = 1 plans the leaves + separators elimination for lvx_solve_step; the call takes the sequential factor all the same (84 knots, nb = 504: 31 panels + 8)."""
    P = _problem("nd")
    for radius in CC.RADII:
        g = _context(P, CC.ND_LOCKS, (("SOLVER_ND", 1),))
        name = CC.case_name("nd", radius, True)
        _check_windows(g, P, CC.ND_LOCKS, radius, True, _tol(name), name)
        lo = g.layout()
        assert lo["n_band"] == 6 * P["n_knots"] == 504 and lo["solver_fallbacks"] == 0
        g.close()


def test_band_narrower_than_a_window():
    """LVX_LOCK_R3, gyro + prior: three scalars per knot, the factor's own half-bandwidth below 23 — the recurrence runs on the padded pattern."""
    P = _problem("r3")
    for radius in CC.RADII:
        g = _context(P, TC.R3_LOCKS, r3=True)
        name = CC.case_name("r3", radius, True)
        _check_windows(g, P, TC.R3_LOCKS, radius, True, _tol(name), name, frames=(lvx.FRAME_TRAJECTORY, lvx.FRAME_LIDAR))
        assert g.layout()["bandwidth"] < 23
        g.close()


# 2. the pose covariance against finite-difference Jacobians
@pytest.mark.parametrize("mask", ["solve1", "solve2"])
def test_pose_covariance_against_finite_differences(mask):
    P = _problem()
    locks, radius = CC.MASKS[mask], 1e4
    g = _context(P, locks)
    name = CC.case_name(mask, radius, True)
    tol = _tol(name)
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, True)
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    nt = g.tangent_size
    times = [t0 + 0.3 * dt, t0 + 17 * dt, P["t_map"]]

    def plus(state, k, h):
        d = np.zeros(nt); d[k] = h
        return g.plus(state, d)
    for frame in FRAMES:
        r = g.trajectory_covariance(times, frame, radius, True, window=True)
        for i, t in enumerate(times):
            idx = r["window_idx"][i]

            def pose(state):
                s = lvx.sample_trajectory(g, state, [t], frame, fields=("position", "orientation"))
                return s["orientation"][0], s["position"][0]
            Jr, Jh = TC.fd_jacobian(pose, P["state0"], N, idx, plus=plus)
            Wr = TC.window_of(Sig, free, idx)
            cov_r, cov_h = Jr @ Wr @ Jr.T, Jh @ Wr @ Jh.T
            s = np.sqrt(np.diag(cov_r))
            level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
            jd = np.abs(Jr) @ np.sqrt(np.diag(Wr))
            carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
            err = np.abs((r["cov"][i] - cov_r) / np.outer(s, s)).max()
            print("%s frame %d t %.4f: cov err %.3e  Richardson level %.3e  window bar carried %.3e  sigma %s" % (name, frame, t, err, level, carried, r["sigma"][i]))
            assert err <= 10 * (level + carried)
    g.close()


# 3. bits
def test_bits_do_not_depend_on_the_batch_the_call_or_the_form():
    """n = 1, 63, 64, 65 are prefixes of one query list (unsorted, the invalid ones last): the same bits, whatever the lowest band position lets the sweep skip; two calls;
    the _d form."""
    import torch
    P = _problem()
    g = _context(P, CC.SOLVE2)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    t = TC.query_times(P)
    full = g.trajectory_covariance(t, lvx.FRAME_LIDAR, 1e4, window=True)
    for n in (1, 63, 64, 65):
        r = g.trajectory_covariance(t[:n], lvx.FRAME_LIDAR, 1e4, window=True)
        for k in ("cov", "sigma", "window_cov", "window_idx", "valid"):
            assert np.array_equal(r[k], full[k][:n]), (n, k)
    again = g.trajectory_covariance(t, lvx.FRAME_LIDAR, 1e4, window=True)
    for k in again:
        assert np.array_equal(again[k], full[k]), k
    lean = g.trajectory_covariance(t, lvx.FRAME_LIDAR, 1e4)   # without the window arrays
    assert np.array_equal(lean["cov"], full["cov"]) and np.array_equal(lean["sigma"], full["sigma"]) and "window_cov" not in lean
    dev = torch.device("cuda:0")
    n = len(t)
    t_d = torch.from_numpy(t).to(dev)
    o = dict(cov=torch.full((n, 36), 7.0, dtype=torch.float64, device=dev), sigma=torch.full((n, 6), 7.0, dtype=torch.float64, device=dev),
             window_cov=torch.full((n, 961), 7.0, dtype=torch.float64, device=dev), window_idx=torch.full((n, 31), 7, dtype=torch.int32, device=dev))
    valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.trajectory_covariance_d(t_d.data_ptr(), n, {k: v.data_ptr() for k, v in o.items()}, valid.data_ptr(), lvx.FRAME_LIDAR, 1e4)
    g.synchronize()
    assert np.array_equal(o["cov"].cpu().numpy().reshape(n, 6, 6), full["cov"]) and np.array_equal(o["sigma"].cpu().numpy(), full["sigma"])
    assert np.array_equal(o["window_cov"].cpu().numpy().reshape(n, 31, 31), full["window_cov"]) and np.array_equal(o["window_idx"].cpu().numpy(), full["window_idx"])
    assert np.array_equal(valid.cpu().numpy().astype(bool), full["valid"])
    g.close()


# 4. no side effects
def test_call_leaves_the_normal_equations_and_the_next_step_alone():
    P = _problem()
    g = _context(P, CC.SOLVE2, (("DETERMINISTIC", 1),))
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    d0, m0 = g.solve_step(1e4)
    ck0 = g.normal_eq_checksum()
    r = g.trajectory_covariance(TC.query_times(P), lvx.FRAME_CAMERA, 1e8)
    assert r["valid"].sum() == 63 and (r["sigma"][r["valid"]] > 0).all()
    assert g.normal_eq_checksum() == ck0
    d1, m1 = g.solve_step(1e4)
    assert np.array_equal(d0, d1) and m0 == m1
    g.trajectory_covariance([P["t_map"]], lvx.FRAME_TRAJECTORY, 1e4, jacobi_scaling=False)
    d2, m2 = g.solve_step(1e4)
    assert np.array_equal(d0, d2) and m0 == m2 and g.normal_eq_checksum() == ck0
    g.close()


# 5. errors
def test_errors_are_codes_and_a_lost_pivot_writes_nothing():
    import torch
    P = _problem()
    g = _context(P, CC.SOLVE2)
    t = TC.query_times(P)[:5]
    with pytest.raises(lvx.LvxError) as e:
        g.trajectory_covariance(t)
    assert e.value.code == lvx.E_STATE
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(frame=3)):
        with pytest.raises(lvx.LvxError) as e:
            g.trajectory_covariance(t, **kw)
        assert e.value.code == lvx.E_ARG
    seen = []

    def allreduce(buf, op):
        try:
            g.trajectory_covariance(t)
            seen.append(None)
        except lvx.LvxError as err:
            seen.append(err.code)
    g.solve_step_shared(1e4, allreduce)
    assert seen and all(c == lvx.E_STATE for c in seen)
    # a declared pivot failure: LVX_E_NOTPD, the pre-filled arrays intact (host form), nothing written and the code at lvx_synchronize (_d form)
    g.set_switch("TEST_BAD_PIVOT", 1)
    n = len(t)
    cov, sigma, valid = np.full((n, 36), 7.0), np.full((n, 6), 7.0), np.full(n, 7, np.uint8)
    rec = lvx.TrajCov(cov.ctypes.data, sigma.ctypes.data, None, None, valid.ctypes.data)
    opt = g._cov_options(lvx.TrajCovOptions, g._l.lvx_traj_cov_default_options, 1e8, True)
    import ctypes as C
    rc = g._l.lvx_trajectory_covariance(g._h, C.byref(opt), C.c_int(0), C.c_int(n), t.ctypes.data_as(C.c_void_p), C.byref(rec))
    assert rc == lvx.E_NOTPD and (cov == 7.0).all() and (sigma == 7.0).all() and (valid == 7).all()
    dev = torch.device("cuda:0")
    t_d = torch.from_numpy(t).to(dev)
    cov_d, valid_d = torch.full((n, 36), 7.0, dtype=torch.float64, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.trajectory_covariance_d(t_d.data_ptr(), n, dict(cov=cov_d.data_ptr()), valid_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NOTPD and bool((cov_d == 7.0).all()) and bool((valid_d == 7).all())
    g.synchronize()   # reported once
    g.set_switch("TEST_BAD_PIVOT", 0)
    assert g.trajectory_covariance(t)["valid"].all()   # the context is as usable as before
    g.close()


def test_non_unit_control_quaternion_invalidates_its_windows():
    """Knot 20 fails logq's unit check.  Where the evaluation itself reports it there are no normal equations to work on and the call returns that error; where the
    evaluation passes (no row reads the knot), the windows that hold it are invalid, the call returns LVX_E_NONUNIT_QUAT and the rest is filled."""
    P = _problem("nd")
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    g = _context(P, CC.ND_LOCKS)
    x = P["state0"].copy()
    x[3 * N + 4 * 20:3 * N + 4 * 20 + 4] *= 1.001
    t = np.array([t0 + 2.5 * dt, t0 + 18.5 * dt, t0 + 40.5 * dt])
    try:
        g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    except lvx.LvxError as err:
        assert err.code == lvx.E_NONUNIT_QUAT
        with pytest.raises(lvx.LvxError) as e:
            g.trajectory_covariance(t)
        assert e.value.code in (lvx.E_NONUNIT_QUAT, lvx.E_STATE)
    else:
        with pytest.raises(lvx.LvxError) as e:
            g.trajectory_covariance(t)
        assert e.value.code == lvx.E_NONUNIT_QUAT
        r = e.value.partial
        assert list(r["valid"]) == [True, False, True] and not r["cov"][1].any() and (r["sigma"][[0, 2]] > 0).all()
    g.close()


# 6. host: Calibrator with CalibrateOptions::trajectory_covariance_step
def test_calibrator_attaches_pose_sigmas_and_ends_at_the_same_state(tmp_path):
    """The noise-free 6 s sequence of tests/test_gpu_pipeline.py, three stages.  With the option at 0.05 s every stage report carries finite, positive
    sigmas at its valid samples — in the CAMERA frame, the one frame in which every stage has something free (the third stage locks the trajectory and the LiDAR: its
    LiDAR-frame pose is a constant and the call returns exact zeros for it, which the LiDAR-frame run below checks) and the two lines of FormatTrajectoryUncertainty; the final state is the one of the run with the option off, bit for bit.  Both runs
    take LVX_DETERMINISTIC = 1: in the default mode the evaluation's atomics add in timing order and two runs of the SAME options already differ in the last
    bits (measured: four runs, four states; deterministic: four runs, option on and off, one state)."""
    import subprocess
    import build as lvx_build
    from test_gpu_pipeline import _write
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "trajcov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "trajcov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin = str(tmp_path / "seq.bin")
    _write(pin, S, refine_iterations=1, lvi=1, camsurf=1)
    runs = {}
    for step in ("0.05 2", "0", "0.05 1"):
        r = subprocess.run([exe, pin] + step.split(), capture_output=True, text=True, env=dict(os.environ, LVX_DETERMINISTIC="1"))
        assert r.returncode == 0, r.stderr
        runs[step] = r.stdout
    on, off, lidar = runs["0.05 2"], runs["0"], runs["0.05 1"]
    assert on.split("STATE")[1] == off.split("STATE")[1] == lidar.split("STATE")[1]
    blocks = [b.strip().splitlines() for b in on.split("STATE")[0].split("END\n") if b.strip()]
    assert [b[0].split()[1] for b in blocks] == ["BatchOptimization", "trajInitFromLVIdata", "trajInitFromLVIdata+lm_splane"]
    for b in blocks:
        head = b[0].split()
        has, n, n_valid, radius = int(head[3]), int(head[5]), int(head[7]), float(head[9])
        lo = np.array([float(v) for v in b[1].split()[1:]]); hi = np.array([float(v) for v in b[2].split()[1:]])
        assert has == 1 and radius == 1e8 and n >= 100 and 0.9 * n <= n_valid <= n
        assert np.isfinite(hi).all() and (lo > 0).all() and (hi >= lo).all()
        assert b[3].startswith("[Trajectory] position std (m): worst") and b[4].startswith("[Trajectory] rotation std (deg): worst")
        print(head[1], "\n".join(b[3:5]))
    assert all("has 0 n 0" in ln for ln in off.splitlines() if ln.startswith("STAGE"))
    lb = [b.strip().splitlines() for b in lidar.split("STATE")[0].split("END\n") if b.strip()]
    for k, b in enumerate(lb):
        lo = np.array([float(v) for v in b[1].split()[1:]]); hi = np.array([float(v) for v in b[2].split()[1:]])
        assert int(b[0].split()[3]) == 1 and ((lo > 0).all() if k < 2 else not hi.any())
