"""lvx_landmark_covariance on the device: the variance of a landmark's inverse depth, its covariance with the reference pose and the covariance of the map point in the
damped LM system at a stated radius — the landmark formula on the selected inverse of the sequential factor (k_band_selinv's wide band store, k_lc_lowest,
k_landmark_cov) — against the float64 Cholesky inverse of the SAME damped system (calib_cov_cases.damped_system) built from the device's own dense export, restricted to
window_idx (tests/landmark_cov_cases.py).

Window bar: calib_cov_cases.rel_err, max |a - ref| / sqrt(ref_ii ref_jj), over the live rows of a window: 10 x the reference's own error against mpmath at 40 digits
(tests/golden/landmark_cov_ref.npz, written by tests/golden/make_landmark_cov_ref.py from the oracle's H), floor 1e-11.  The margin covers two float64 eliminations in
different orders, as the other two covariance tests argue.
Point covariance bar (the construction of tests/test_gpu_trajcov.py's cov check): against J_fd W_ref J_fd^T with J_fd from Context.plus + lvx.sample_trajectory + numpy
(central differences, Richardson): 10 x (the change of that product between the two Richardson levels + the window bar carried through |J|).
Point bar: 1e-12 relative against the numpy restatement from lvx.sample_trajectory's camera-frame pose.
The reference's own error per case, the bar and the observed figures are printed by every test (-s).  First MI355X run (reference's own error -> observed, over all
landmarks of the case; scaled / plain where both run):
    SMALL solve2   R 1e4  6.7e-13 / 4.7e-13 -> 1.5e-12 / 1.3e-12      R 1e8  8.6e-09 / 2.7e-09 -> 9.0e-09 / 9.7e-09
    SMALL solve3   (no band)  9e-16 .. 2.6e-15 -> 1.1e-15 .. 3.5e-15
    70 tracks      R 1e4  4.2e-13 -> 8.2e-13      R 1e8  4.0e-09 -> 5.2e-09      (band 288, half-bandwidth 77, landmark rows 78 wide)
    hub            R 1e4  4.4e-13 -> 9.0e-13      R 1e8  3.0e-09 -> 1.8e-08
    no rows        R 1e4  5.5e-13 -> 1.1e-12      R 1e8  6.2e-09 -> 1.4e-08
    SOLVER_ND, 6   R 1e4  5.8e-13 -> 1.9e-12      R 1e8  4.5e-09 -> 8.0e-09
point: <= 1.6e-14 relative.  point_cov (landmarks 0, 4, 11; R 1e4): 6.1e-13 .. 1.2e-12 observed, Richardson levels 1.1e-7 .. 5.2e-7, carried window bar 1.8e-11 .. 4.6e-11."""
import ctypes as C
import os

import numpy as np
import pytest

import calib_cov_cases as CC
import landmark_cov_cases as LC
import lvx
import trajcov_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "landmark_cov_ref.npz")))
KEYS = ("var_rho", "sigma_rho", "point", "point_cov", "window_cov", "window_idx", "valid")
_P = {}


def _problem(key="small"):
    if key not in _P:
        _P[key] = LC.problem(key)
    return _P[key]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _context(P, locks, switches=()):
    g = lvx.Context(0)
    for k, v in switches:
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _camera_pose(g, P, state, l):
    s = lvx.sample_trajectory(g, state, [LC.ref_time(P, l)], lvx.FRAME_CAMERA, fields=("position", "orientation"))
    assert s["valid"][0]
    return s["orientation"][0], s["position"][0]


def _check_windows(g, P, locks, radius, scaling, name):
    """evaluate, export, reference; every landmark's window, variance and point.  Returns the record, Sigma_ref, free."""
    tol = _tol(name)
    x = P["state0"]
    H = g.evaluate(x, normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, scaling)
    r = g.landmark_covariance(radius, scaling)
    assert r["valid"].all()
    worst = worst_pt = 0.0
    for l in range(P["n_landmarks"]):
        want = np.array(LC.window_indices(P, x, l))
        want[~np.isin(want, free)] = -1
        assert np.array_equal(r["window_idx"][l], want), (name, l)
        Wd, Wr = r["window_cov"][l], TC.window_of(Sig, free, want)
        dead = want < 0
        assert not Wd[dead].any() and not Wd[:, dead].any()
        assert np.array_equal(Wd, Wd.T) and np.array_equal(r["point_cov"][l], r["point_cov"][l].T)
        assert r["var_rho"][l] == Wd[0, 0] and r["sigma_rho"][l] == np.sqrt(Wd[0, 0])
        worst = max(worst, TC.window_rel_err(Wd, Wr))
        pt = LC.point_from_pose(P, x, l, *_camera_pose(g, P, x, l))
        worst_pt = max(worst_pt, np.abs(r["point"][l] - pt).max() / np.abs(pt).max())
    print("%-28s window err %.3e (allowed %.3e, reference's own %.3e)  point err %.3e  sigma_rho %.3e .. %.3e" % (
        name, worst, tol, float(REF_ERR[name]), worst_pt, r["sigma_rho"].min(), r["sigma_rho"].max()))
    assert worst <= tol
    assert worst_pt <= 1e-12
    return r, Sig, free


# 1. parity with the same damped system
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("mask", ["solve2", "solve3"])
def test_windows_match_the_damped_system(mask, radius, scaling):
    P = _problem()
    locks = CC.MASKS[mask]
    g = _context(P, locks)
    r, _, _ = _check_windows(g, P, locks, radius, scaling, "small_" + CC.case_name(mask, radius, scaling))
    if mask == "solve3":   # the trajectory is constant: no band, the window holds rho and the camera's extrinsics only
        assert g.layout()["n_band"] == 0 and (r["window_idx"][:, 1:25] == -1).all() and (r["window_idx"][:, 25:31] >= 0).all()
    g.close()


@pytest.mark.parametrize("radius", CC.RADII)
def test_short_tracks(radius):
    """70 landmarks of 3 views over 0.6 s: the narrowest band such tracks leave (three frames 0.05 s apart reach nine knots)."""
    P = _problem("tracks")
    g = _context(P, CC.SOLVE2)
    _check_windows(g, P, CC.SOLVE2, radius, True, "tracks_" + CC.case_name("lm", radius, True))
    lo = g.layout()
    print("tracks: band %d, half-bandwidth %d, landmark row width %d" % (lo["n_band"], lo["bandwidth"], lo["lm_row_width"]))
    assert lo["bandwidth"] >= 23
    g.close()


@pytest.mark.parametrize("radius", CC.RADII)
def test_reference_frame_at_the_hub(radius):
    """Landmark HUB_LM's reference view lies at t_map: its window and its row hold hub knots, which are border slots."""
    P = _problem("hub")
    g = _context(P, CC.SOLVE2)
    r, _, _ = _check_windows(g, P, CC.SOLVE2, radius, True, "hub_" + CC.case_name("lm", radius, True))
    lo = g.layout()
    knots = r["window_idx"][LC.HUB_LM][1:25:6] // 6
    assert lo["n_hub_knots"] > 0 and ((knots >= lo["hub_knot0"]) & (knots < lo["hub_knot0"] + lo["n_hub_knots"])).any()
    g.close()


@pytest.mark.parametrize("radius", CC.RADII)
def test_landmark_without_rows_reports_the_damping(radius):
    P = _problem("norows")
    g = _context(P, CC.SOLVE2)
    r, _, _ = _check_windows(g, P, CC.SOLVE2, radius, True, "norows_" + CC.case_name("lm", radius, True))
    l = LC.NOROWS_LM
    assert r["valid"][l] and abs(r["var_rho"][l] / (radius / 1e-6) - 1.0) <= 1e-15 and not r["window_cov"][l][0, 1:].any()
    assert (np.diag(r["window_cov"][l])[1:25] > 0).all()   # the pose block of its window is the trajectory's
    g.close()


def test_plan_of_the_solver_is_ignored():
    """SOLVER_ND = 1 plans the leaves + separators elimination for lvx_solve_step; the call takes the sequential factor all the same."""
    P = _problem("nd6")
    for radius in CC.RADII:
        g = _context(P, CC.ND_LOCKS, (("SOLVER_ND", 1),))
        _check_windows(g, P, CC.ND_LOCKS, radius, True, "nd6_" + CC.case_name("lm", radius, True))
        lo = g.layout()
        assert lo["n_band"] == 6 * P["n_knots"] == 504 and lo["solver_fallbacks"] == 0
        g.close()


def test_locked_landmarks_are_invalid():
    P = _problem()
    g = _context(P, CC.SOLVE1)   # LVX_LOCK_LANDMARKS
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    r = g.landmark_covariance(1e4)
    assert not r["valid"].any() and (r["window_idx"] == -1).all()
    for k in ("var_rho", "sigma_rho", "point", "point_cov", "window_cov"):
        assert not r[k].any(), k
    g.close()


# 2. the point covariance against finite-difference Jacobians
def test_point_covariance_against_finite_differences():
    P = _problem()
    locks, radius = CC.SOLVE2, 1e4
    g = _context(P, locks)
    name = "small_" + CC.case_name("solve2", radius, True)
    tol = _tol(name)
    x = P["state0"]
    N, nt = P["n_knots"], g.tangent_size
    H = g.evaluate(x, normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, N, P["n_landmarks"], locks, radius, True)
    r = g.landmark_covariance(radius)

    def plus(state, k, h):
        d = np.zeros(nt); d[k] = h
        return g.plus(state, d)
    for l in (0, 4, 11):
        idx = r["window_idx"][l]
        point = lambda state: LC.point_from_pose(P, state, l, *_camera_pose(g, P, state, l))
        Jr = np.zeros((3, LC.W)); Jh = np.zeros((3, LC.W))
        for c, k in enumerate(idx):
            if k < 0:
                continue
            h = 1e-3 * x[7 * N + 32 + l] if c == 0 else (1e-5 if k == 6 * N + 21 else 1e-3)
            d1 = (point(plus(x, k, h)) - point(plus(x, k, -h))) / (2 * h)
            d2 = (point(plus(x, k, h / 2)) - point(plus(x, k, -h / 2))) / h
            Jh[:, c] = d2; Jr[:, c] = (4 * d2 - d1) / 3
        Wr = TC.window_of(Sig, free, idx)
        cov_r, cov_h = Jr @ Wr @ Jr.T, Jh @ Wr @ Jh.T
        s = np.sqrt(np.diag(cov_r))
        level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
        jd = np.abs(Jr) @ np.sqrt(np.diag(Wr))
        carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
        err = np.abs((r["point_cov"][l] - cov_r) / np.outer(s, s)).max()
        print("%s landmark %d: point_cov err %.3e  Richardson level %.3e  window bar carried %.3e  point sigma %s m" % (name, l, err, level, carried, s))
        assert err <= 10 * (level + carried)
    g.close()


# 3. bits
def test_bits_do_not_depend_on_the_batch_the_call_or_the_form():
    """ids unsorted and repeated; n = 1, 11, 12 are prefixes of one list: the same bits, whatever the lowest band position lets the sweep skip; a second call; the call
    without the window arrays; the _d form."""
    import torch
    P = _problem()
    g = _context(P, CC.SOLVE2)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    every = g.landmark_covariance(1e4)
    ids = np.array([7, 3, 11, 3, 0, 9, 5, 10, 1, 8, 2, 7], np.int32)
    full = g.landmark_covariance(1e4, ids=ids)
    for k in KEYS:
        assert np.array_equal(full[k], every[k][ids]), k
    for n in (1, 11, 12):
        r = g.landmark_covariance(1e4, ids=ids[:n])
        for k in KEYS:
            assert np.array_equal(r[k], full[k][:n]), (n, k)
    again = g.landmark_covariance(1e4, ids=ids)
    for k in KEYS:
        assert np.array_equal(again[k], full[k]), k
    lean = g.landmark_covariance(1e4, ids=ids, window=False)
    assert "window_cov" not in lean and "window_idx" not in lean
    for k in ("var_rho", "sigma_rho", "point", "point_cov", "valid"):
        assert np.array_equal(lean[k], full[k]), k
    dev = torch.device("cuda:0")
    n = len(ids)
    ids_d = torch.from_numpy(ids).to(dev)
    o = dict(var_rho=torch.full((n,), 7.0, dtype=torch.float64, device=dev), sigma_rho=torch.full((n,), 7.0, dtype=torch.float64, device=dev),
             point=torch.full((n, 3), 7.0, dtype=torch.float64, device=dev), point_cov=torch.full((n, 9), 7.0, dtype=torch.float64, device=dev),
             window_cov=torch.full((n, 1024), 7.0, dtype=torch.float64, device=dev), window_idx=torch.full((n, 32), 7, dtype=torch.int32, device=dev))
    valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.landmark_covariance_d(ids_d.data_ptr(), n, {k: v.data_ptr() for k, v in o.items()}, valid.data_ptr(), 1e4)
    g.synchronize()
    for k in KEYS[:-1]:
        assert np.array_equal(o[k].cpu().numpy().reshape(full[k].shape), full[k]), k
    assert np.array_equal(valid.cpu().numpy().astype(bool), full["valid"])
    g.close()


# 4. no side effects
def test_call_leaves_the_normal_equations_the_next_step_and_the_pose_covariance_alone():
    P = _problem()
    g = _context(P, CC.SOLVE2, (("DETERMINISTIC", 1),))
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    d0, m0 = g.solve_step(1e4)
    ck0 = g.normal_eq_checksum()
    t = TC.query_times(P)
    tc0 = g.trajectory_covariance(t, lvx.FRAME_CAMERA, 1e8, window=True)
    r = g.landmark_covariance(1e8)
    assert r["valid"].all() and (r["sigma_rho"] > 0).all()
    assert g.normal_eq_checksum() == ck0
    tc1 = g.trajectory_covariance(t, lvx.FRAME_CAMERA, 1e8, window=True)
    for k in tc0:
        assert np.array_equal(tc0[k], tc1[k]), k
    d1, m1 = g.solve_step(1e4)
    assert np.array_equal(d0, d1) and m0 == m1
    g.landmark_covariance(1e4, jacobi_scaling=False, ids=[11])
    d2, m2 = g.solve_step(1e4)
    assert np.array_equal(d0, d2) and m0 == m2 and g.normal_eq_checksum() == ck0
    g.close()


# 5. errors
def _raw(g, opt, n, ids, rec):
    return g._l.lvx_landmark_covariance(g._h, C.byref(opt) if opt is not None else None, C.c_int(n), ids.ctypes.data_as(C.c_void_p) if ids is not None else None,
                                        C.byref(rec) if rec is not None else None)


def test_errors_are_codes_and_a_lost_pivot_writes_nothing():
    import torch
    P = _problem()
    L = P["n_landmarks"]
    g = _context(P, CC.SOLVE2)
    with pytest.raises(lvx.LvxError) as e:
        g.landmark_covariance()
    assert e.value.code == lvx.E_STATE
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(ids=[]), dict(ids=list(range(L)) + [0]), dict(ids=[0, L]), dict(ids=[-1])):
        with pytest.raises(lvx.LvxError) as e:
            g.landmark_covariance(**kw)
        assert e.value.code == lvx.E_ARG, kw
    var, valid = np.full(L, 7.0), np.full(L, 7, np.uint8)
    rec = lvx.LandmarkCov(var.ctypes.data, None, None, None, None, None, valid.ctypes.data)
    opt = g._cov_options(lvx.LandmarkCovOptions, g._l.lvx_landmark_cov_default_options, 1e8, True)
    assert g._l.lvx_landmark_covariance(None, C.byref(opt), C.c_int(L), None, C.byref(rec)) == lvx.E_ARG
    assert _raw(g, None, L, None, rec) == lvx.E_ARG and _raw(g, opt, L, None, None) == lvx.E_ARG
    assert _raw(g, opt, L, None, lvx.LandmarkCov(var.ctypes.data, None, None, None, None, None, None)) == lvx.E_ARG
    bad = g._cov_options(lvx.LandmarkCovOptions, g._l.lvx_landmark_cov_default_options, 1e8, True); bad.reserved = 1
    assert _raw(g, bad, L, None, rec) == lvx.E_ARG
    assert (var == 7.0).all() and (valid == 7).all()
    seen = []

    def allreduce(buf, op):
        try:
            g.landmark_covariance()
            seen.append(None)
        except lvx.LvxError as err:
            seen.append(err.code)
    g.solve_step_shared(1e4, allreduce)
    assert seen and all(c == lvx.E_STATE for c in seen)
    # a declared pivot failure: LVX_E_NOTPD, the pre-filled arrays intact (host form), nothing written and the code at lvx_synchronize (_d form)
    g.set_switch("TEST_BAD_PIVOT", 1)
    assert _raw(g, opt, L, None, rec) == lvx.E_NOTPD and (var == 7.0).all() and (valid == 7).all()
    dev = torch.device("cuda:0")
    var_d, valid_d = torch.full((L,), 7.0, dtype=torch.float64, device=dev), torch.full((L,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.landmark_covariance_d(None, L, dict(var_rho=var_d.data_ptr()), valid_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NOTPD and bool((var_d == 7.0).all()) and bool((valid_d == 7).all())
    g.synchronize()   # reported once
    g.set_switch("TEST_BAD_PIVOT", 0)
    assert _raw(g, opt, L, None, rec) == lvx.OK and (valid == 1).all() and (var > 0).all()   # the context is as usable as before; only var_rho and valid were asked for
    g.close()


# 6. host: Calibrator with CalibrateOptions::landmark_covariance
def test_calibrator_attaches_landmark_sigmas_and_ends_at_the_same_state(tmp_path):
    """The noise-free 6 s sequence of tests/test_gpu_pipeline.py, three stages.  With the option on, every stage whose landmarks are free (the second and the third) carries one
    record — finite, positive sigmas at its valid landmarks and the line of FormatLandmarkUncertainty — and the surfel stage, which holds them constant, carries none; the final state is the one of
    the run with the option off, bit for bit.  Both runs take LVX_DETERMINISTIC = 1, the only mode in which two runs agree."""
    import subprocess
    import build as lvx_build
    import synth
    from test_gpu_pipeline import _write
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "landmark_cov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "landmark_cov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin = str(tmp_path / "seq.bin")
    _write(pin, S, refine_iterations=1, lvi=1, camsurf=1)
    runs = {}
    for flag in ("1", "0"):
        r = subprocess.run([exe, pin, flag], capture_output=True, text=True, env=dict(os.environ, LVX_DETERMINISTIC="1"))
        assert r.returncode == 0, r.stderr
        runs[flag] = r.stdout
    on, off = runs["1"], runs["0"]
    assert on.split("STATE")[1] == off.split("STATE")[1]
    blocks = [b.strip().splitlines() for b in on.split("STATE")[0].split("END\n") if b.strip()]
    assert [b[0].split()[1] for b in blocks] == ["BatchOptimization", "trajInitFromLVIdata", "trajInitFromLVIdata+lm_splane"]
    has = []
    for b in blocks:
        head = b[0].split()
        h, n, n_valid, radius = int(head[3]), int(head[5]), int(head[7]), float(head[9])
        has.append(h)
        if not h:
            assert n == 0
            continue
        lo, hi = float(b[1].split()[1]), float(b[1].split()[2])
        assert radius == 1e8 and n == len(S["lm_t0"]) and 0.9 * n <= n_valid <= n and 0 < lo <= hi and np.isfinite(hi)
        assert b[2].startswith("[Landmarks] relative depth std: median")
        print(head[1], b[2])
    assert has == [0, 1, 1]   # lvx_host::StageLocks: the surfel stage holds the landmarks constant, the two that follow estimate them
    assert all("has 0 n 0" in ln for ln in off.splitlines() if ln.startswith("STAGE"))
