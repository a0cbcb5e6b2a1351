"""lvx_calibration_covariance on the device: the covariance of the calibration scalars in the damped LM system at a stated radius, and the spectrum of their scaled
marginal information, against a float64 numpy Cholesky of the SAME damped system built from the device's own dense export (tests/calib_cov_cases.py).

Tolerance of the covariance: measure max |cov - ref| / sqrt(ref_ii ref_jj); a case may use 10 x the reference's own error against mpmath at 40 digits
(tests/golden/calib_cov_ref.npz, written by tests/golden/make_calib_cov_ref.py from the oracle's H), floor 1e-11: two float64 eliminations in different orders.
Reference's own error, the bound it gives, and the figure observed on the first MI355X run (default route):
    case                      reference vs mpmath   allowed     observed
    solve1 R 1e4  scaled / plain   3.7e-13 / 1.8e-12   1e-11 / 1.8e-11   2.0e-12 / 1.4e-12
    solve1 R 1e8  scaled / plain   7.7e-10 / 1.8e-09   7.7e-09 / 1.8e-08 1.6e-09 / 3.5e-09
    solve2 R 1e4  scaled / plain   5.7e-13 / 4.5e-13   1e-11 / 1e-11     4.3e-12 / 1.1e-12
    solve2 R 1e8  scaled / plain   2.1e-09 / 2.4e-09   2.1e-08 / 2.4e-08 5.2e-09 / 5.4e-09
    solve3 R 1e4  scaled / plain   4.8e-14 / 8.6e-15   1e-11 / 1e-11     7.7e-14 / 4.8e-15
    solve3 R 1e8  scaled / plain   1.7e-13 / 5.3e-14   1e-11 / 1e-11     8.7e-14 / 2.0e-13
    leaves + separators (512 free scalars, 3 leaves) R 1e4 / 1e8, scaled: 5.8e-13 / 1.4e-09, allowed 1e-11 / 1.4e-08, observed 5.9e-13 / 2.0e-09
    the other routes (uniform chain, sequential, per-landmark elimination, sequential redo) stay within 1.5 x the default route's figure;
    solve3 at radius 1e8 against 1e10: 1.0e-05 (bound 1e-4); camera free against locked, the other scalars: 7.5e-15 (bound 1e-9)
Spectrum: both sides form T by a float64 elimination whose absolute error is of order n eps |T| (n ~ 300: 1e-13 |T|), so an eigenvalue is held to
tol_case * lambda + 1e-12 * lambda_max.  An eigenvector is compared through |v . v_ref| only where its eigenvalue is separated from both neighbours by more than 1e-6 of
the larger; there a perturbation of that size turns it by at most angle = (perturbation) / gap (Davis-Kahan), and 1 - |v . v_ref| <= (4 angle)^2 / 2 is asserted (both
sides carry the perturbation, and a factor 2 of room) wherever angle <= 0.05, i.e. where that arithmetic determines the vector at all."""
import os

import numpy as np
import pytest

import calib_cov_cases as CC
import lvx
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "calib_cov_ref.npz")))
_P = {}


def _problem(key="small"):
    if key not in _P:
        _P[key] = synth.make_problem(**(CC.SMALL if key == "small" else CC.ND))
    return _P[key]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _context(P, locks, switches=()):
    g = lvx.Context(0)
    for k, v in switches:
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _compare(g, P, locks, radius, scaling, tol, label):
    """evaluate, export, call, reference; asserts covariance, constants, scale and spectrum.  Returns the record."""
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    r = g.calibration_covariance(radius, scaling)
    ref = CC.reference(H, P["n_knots"], P["n_landmarks"], locks, radius, scaling)
    cidx = ref["cidx"]
    assert list(r["free_index"]) == list(cidx) and r["radius"] == radius and r["n_hub_eliminated"] == g.layout()["n_border"] - 22
    cov = r["cov"][np.ix_(cidx, cidx)]
    err = CC.rel_err(cov, ref["cov"])
    w, V = np.linalg.eigh(ref["T"])
    eig_err = np.abs(r["info_eig"] - w) / (tol * w + 1e-12 * w[-1])
    print("%-34s cov err %.3e (allowed %.3e)  eig err / allowed %.3f  sweeps %d  eig %.3e .. %.3e" % (label, err, tol, eig_err.max(), r["sweeps"], r["info_eig"][0], r["info_eig"][-1]))
    assert err <= tol
    const = np.setdiff1d(np.arange(22), cidx)
    assert not r["cov"][const, :].any() and not r["cov"][:, const].any() and not r["sigma"][const].any()
    assert np.array_equal(r["sigma"], np.sqrt(np.diag(r["cov"])))
    assert np.abs(r["scale"][cidx] / ref["scale"] - 1).max() <= 4 * np.finfo(float).eps
    assert (r["info_eig"] > 0).all() and (np.diff(r["info_eig"]) >= 0).all()
    assert eig_err.max() <= 1.0
    n = len(w)
    assert np.abs(r["info_vec"].T @ r["info_vec"] - np.eye(n)).max() <= 1e-13
    for k in range(n):
        nb = [j for j in (k - 1, k + 1) if 0 <= j < n]
        if all(abs(w[k] - w[j]) > 1e-6 * max(w[k], w[j]) for j in nb):
            angle = max((tol * max(w[k], w[j]) + 1e-12 * w[-1]) / abs(w[k] - w[j]) for j in nb) if nb else 0.0
            if angle <= 0.05:
                assert 1 - abs(r["info_vec"][:, k] @ V[:, k]) <= 0.5 * (4 * angle) ** 2 + 1e-13, (label, k, angle)
    return r


# 1. parity with the same damped system, default elimination route (the uniform chain at this size)
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("mask", ["solve1", "solve2", "solve3"])
def test_parity_with_the_damped_system(mask, radius, scaling):
    P = _problem()
    g = _context(P, CC.MASKS[mask])
    name = CC.case_name(mask, radius, scaling)
    _compare(g, P, CC.MASKS[mask], radius, scaling, _tol(name), name)
    assert g.layout()["solver_fallbacks"] == 0
    g.close()


# 2. every elimination route
ROUTES = {"chain": (("SOLVER_ND", 0),), "seq": (("SOLVER_SEQ", 1),), "schur_one": (("TEST_LM_SCHUR_ONE", 1),), "redo": (("TEST_BAD_PIVOT", 1),)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("mask", ["solve1", "solve2", "solve3"])
def test_every_elimination_route(mask, route):
    """SOLVER_ND = 0: the uniform chain; SOLVER_SEQ = 1: the sequential band Cholesky; TEST_LM_SCHUR_ONE: one workgroup per landmark; TEST_BAD_PIVOT: a pivot failure is
    declared after the chain, the call repeats the elimination sequentially as lvx_solve_step does.  (solve3 has no band: its routes differ in the landmark kernel only.)"""
    P = _problem()
    for radius in CC.RADII:
        g = _context(P, CC.MASKS[mask], ROUTES[route])
        name = CC.case_name(mask, radius, True)
        _compare(g, P, CC.MASKS[mask], radius, True, _tol(name), route + " " + name)
        lo = g.layout()
        if route == "redo":
            assert lo["solver_fallbacks"] == (1 if lo["n_band"] > 0 else 0)
        if route == "schur_one" and not (CC.MASKS[mask] & lvx.LOCK_LANDMARKS):
            assert lo["lm_elim_kernel"] == 2
        g.close()


@pytest.mark.parametrize("radius", CC.RADII)
def test_leaves_and_separators_route(radius):
    P = _problem("nd")
    g = _context(P, CC.ND_LOCKS, (("SOLVER_ND", 1),))
    name = CC.case_name("nd", radius, True)
    _compare(g, P, CC.ND_LOCKS, radius, True, _tol(name), name)
    lo = g.layout()
    assert lo["solver_separators"] >= 2 and lo["solver_leaves"] == lo["solver_separators"] + 1 and lo["solver_fallbacks"] == 0 and lo["n_border"] == 22
    g.close()


# 3. independence from the prior where the data decide
def test_locked_trajectory_result_does_not_depend_on_the_radius():
    P = _problem()
    g = _context(P, CC.SOLVE3)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    a, b = g.calibration_covariance(1e8), g.calibration_covariance(1e10)
    idx = a["free_index"]
    d = CC.rel_err(b["cov"][np.ix_(idx, idx)], a["cov"][np.ix_(idx, idx)])
    print("solve3: radius 1e8 -> 1e10 changes the covariance by %.3e" % d)
    assert d <= 1e-4
    g.close()


# 4. unobserved directions are reported, not hidden
def test_unobserved_camera_extrinsics_show_in_the_spectrum():
    """No landmark, so no row touches the camera: with its extrinsics free the six slots c = 15 .. 20 carry nothing but the LM floor 1e-6 / radius.  They are exact
    (the slots are decoupled: no rotation reaches them) and the rest of the record is that of the run with the camera locked: the same 14 x 14 block (bit for bit out of
    the same elimination) decomposed among 20 instead of 14 — Jacobi is accurate to n eps kappa(B), B the block scaled to unit diagonal (kappa < 1e5): 1e-9 with room."""
    P = synth.make_problem(seed=14, duration=0.4, n_surfel=200, n_planes=10, n_landmarks=0, n_camsurf=0)
    radius = 1e8
    rec = {}
    for key, locks in (("free", CC.TAU), ("locked", CC.TAU | lvx.LOCK_CAM_Q | lvx.LOCK_CAM_P)):
        g = _context(P, locks, (("DETERMINISTIC", 1),))
        g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
        rec[key] = g.calibration_covariance(radius)
        g.close()
    f, l = rec["free"], rec["locked"]
    assert list(f["free_index"]) == list(range(14)) + list(range(15, 21)) and list(l["free_index"]) == list(range(14))
    assert np.abs(f["info_eig"][:6] / (1e-6 / radius) - 1).max() <= 1e-10
    cam = np.isin(f["free_index"], np.arange(15, 21))
    assert not f["info_vec"][~cam, :6].any() and not f["info_vec"][cam, 6:].any()
    assert np.abs(f["info_eig"][6:] / l["info_eig"] - 1).max() <= 1e-9
    d = CC.rel_err(f["cov"][:14, :14], l["cov"][:14, :14])
    print("camera free vs locked: covariance of the other scalars differs by %.3e" % d)
    assert d <= 1e-9
    assert np.abs(np.diag(f["cov"])[15:21] / (radius / 1e-6) - 1).max() <= 1e-10 and not f["cov"][15:21, :15].any()


# 5. locks
ALL_BUT_BIASES = lvx.LOCK_TRAJ | lvx.LOCK_LIDAR_Q | lvx.LOCK_LIDAR_P | CC.TAU | lvx.LOCK_CAM_Q | lvx.LOCK_CAM_P | lvx.LOCK_LANDMARKS


@pytest.mark.parametrize("locks", [CC.SOLVE1, CC.SOLVE2, CC.SOLVE3, 0, ALL_BUT_BIASES, CC.TAU | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS])
def test_free_index_follows_the_lock_mask(locks):
    P = _problem()
    g = _context(P, locks)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    r = g.calibration_covariance(1e4)
    _, _, cidx = CC.free_sets(P["n_knots"], P["n_landmarks"], locks)
    assert list(r["free_index"]) == list(cidx) and len(r["info_eig"]) == len(cidx)
    const = np.setdiff1d(np.arange(22), cidx)
    assert not r["cov"][const, :].any() and not r["cov"][:, const].any() and not r["sigma"][const].any()
    assert (r["sigma"][cidx] > 0).all() and np.all(np.isfinite(r["cov"]))
    g.close()


# 6. no side effects
def test_call_leaves_the_normal_equations_and_the_next_step_alone():
    P = _problem()
    g = _context(P, CC.SOLVE2, (("DETERMINISTIC", 1),))
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    d0, m0 = g.solve_step(1e4)
    ck0 = g.normal_eq_checksum()
    r = g.calibration_covariance(1e8)
    assert r["sweeps"] >= 1
    assert g.normal_eq_checksum() == ck0
    d1, m1 = g.solve_step(1e4)
    assert np.array_equal(d0, d1) and m0 == m1
    g.calibration_covariance(1e4, jacobi_scaling=False)
    d2, m2 = g.solve_step(1e4)
    assert np.array_equal(d0, d2) and m0 == m2 and g.normal_eq_checksum() == ck0
    g.close()


# 7. errors
def test_errors_are_codes_with_a_text_never_a_result():
    P = _problem()
    g = _context(P, CC.SOLVE2)
    with pytest.raises(lvx.LvxError) as e:
        g.calibration_covariance()
    assert e.value.code == lvx.E_STATE
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(max_sweeps=0)):
        with pytest.raises(lvx.LvxError) as e:
            g.calibration_covariance(**kw)
        assert e.value.code == lvx.E_ARG
    with pytest.raises(lvx.LvxError) as e:
        g.calibration_covariance(max_sweeps=1)
    assert e.value.code == lvx.E_NOTPD and "not converged after 1 sweeps" in str(e.value) and "sqrt(t_pp t_qq) =" in str(e.value)
    assert g.calibration_covariance()["sweeps"] > 1   # the context is as usable as before
    # a joint transport: inside the reduction callback of a shared step the context takes part in a joint solve
    seen = []

    def allreduce(buf, op):
        try:
            g.calibration_covariance()
            seen.append(None)
        except lvx.LvxError as err:
            seen.append(err.code)
    g.solve_step_shared(1e4, allreduce)
    assert seen and all(c == lvx.E_STATE for c in seen)
    g.close()


# 8. host: Calibrator with CalibrateOptions::covariance
STAGE_OF = {"BatchOptimization": "TrajFromSurfel", "Refinement": "TrajFromSurfel", "trajInitFromLVIdata": "TrajFromLVI", "trajInitFromLVIdata+lm_splane": "TrajFromLVILandmarksOnly"}


def test_calibrator_reports_a_record_per_stage(tmp_path):
    """The noise-free 6 s sequence of tests/test_gpu_pipeline.py (the truth is a fixed point: one association round), three stages with three lock masks.  Every
    stage's record has the free set of the stage's locks, and the lines of FormatCalibrationUncertainty (%.6e) carry the record's numbers: 2 sigma 180 / pi degrees for a
    rotation, sigma metres for a translation, the smallest eigenvalue and the scalar its eigenvector is largest at."""
    import subprocess
    import build as lvx_build
    import stages
    from test_gpu_pipeline import _write
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "calib_cov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "calib_cov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin = str(tmp_path / "seq.bin")
    _write(pin, S, refine_iterations=1, lvi=1, camsurf=1)
    r = subprocess.run([exe, pin], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blocks = [b.strip().splitlines() for b in r.stdout.split("END\n") if b.strip()]
    assert [b[0].split()[1] for b in blocks] == ["BatchOptimization", "trajInitFromLVIdata", "trajInitFromLVIdata+lm_splane"]
    for b in blocks:
        head = b[0].split()
        name, has, n_free, radius = head[1], int(head[3]), int(head[5]), float(head[7])
        free = [int(v) for v in head[9:]]
        sigma = np.array([float(v) for v in b[1].split()[1:]])
        eig = np.array([float(v) for v in b[2].split()[1:]])
        vec0 = np.array([float(v) for v in b[3].split()[1:]])
        _, _, cidx = CC.free_sets(S["n_knots"], len(S["lm_t0"]), stages.stage_locks(STAGE_OF[name]))
        assert has == 1 and radius == 1e8 and n_free == len(cidx) and free == list(cidx) and len(eig) == n_free
        assert (sigma[cidx] > 0).all() and not np.delete(sigma, cidx).any() and (eig > 0).all()
        lines = {ln.split()[0]: ln for ln in b[4:]}
        for tag, c0 in (("[LiDAR]", 8), ("[Camera]", 15)):
            if not any(c0 <= c < c0 + 6 for c in cidx):
                assert tag not in lines
                continue
            num = [float(v.rstrip(";")) for v in lines[tag].replace("(deg):", " ").replace("(m):", " ").split() if v[0].isdigit()]
            assert len(num) == 6
            want = np.concatenate([2 * sigma[c0:c0 + 3] * 180 / np.pi, sigma[c0 + 3:c0 + 6]])
            assert np.allclose(num, want, rtol=1e-6, atol=0)
        sp = lines["[Spectrum]"]
        assert abs(float(sp.split("eigenvalue:")[1].split()[0]) / eig[0] - 1) <= 1e-6 and float(sp.split("(radius")[1].split(")")[0]) == 1e8
        dom = free[int(np.argmax(np.abs(vec0)))]
        assert sp.rstrip().endswith("(c = %d)" % dom)
        print(name, "\n".join(b[4:]))
