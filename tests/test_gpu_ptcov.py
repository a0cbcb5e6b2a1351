"""lvx_map_point_covariance on the device: the covariance of LiDAR points carried into the map frame, in the damped LM system at a stated radius, from the selected
inverse of the sequential factor (k_border_inv, k_band_selinv, then k_pt_hub and k_point_cov with a lane per point), against the float64 Cholesky inverse of the SAME
damped system built from the device's own dense export, restricted to window_idx (tests/ptcov_cases.py, tests/trajcov_cases.py).

Window bar: calib_cov_cases.rel_err over the live rows of a window; a case may use 10 x the reference's own error against mpmath at 40 digits
(tests/golden/ptcov_ref.npz, written by tests/golden/make_ptcov_ref.py from the oracle's H), floor 1e-11 — the bar of the other three covariance tests.
Point covariance bar, built as tests/test_gpu_trajcov.py builds its own: against J_fd W_ref J_fd^T with J_fd from Context.plus + lvx.sample_trajectory in the LiDAR
frame (central differences, Richardson; columns per unique tangent index): 10 x (the change of that product between the two Richardson levels + the window bar carried
through |J|: tol (|J| d)_r (|J| d)_s / sqrt(cov_rr cov_ss), d = sqrt(diag W_ref)).
Point bar: 1e-12 |p_M| against the reference's chain restated in numpy.
The reference's own error per case, the bar and the observed figures are printed by every test (-s).

Observed on one MI355X (SMALL: 44 knots, nb = 216 .. 234, 52 border scalars).  Windows: 1.4e-12 .. 1.5e-12 at R 1e4 (reference's own 2.8e-13 .. 7.8e-13, bar 1e-11),
9.5e-9 .. 1.3e-8 at R 1e8 (own 3.3e-9 .. 8.5e-9, bar 3.3e-8 .. 8.5e-8), exact zeros under the solve-3 mask.  cov against J_fd W_ref J_fd^T at R 1e4: 6.4e-13 (first
interval) .. 9.0e-9 (0.001 s after t_map, where the four pose-level terms cancel to a sigma of 0.2 mm) of sqrt(cov_rr cov_ss), the Richardson levels differ by
9.5e-8 .. 4.0e-7, carried window bar 5.1e-11 .. 1.2e-8.  point: <= 8.6e-15 |p_M|.  sigma_max^2 and var_dir against numpy: <= 2.7e-16 of the trace.  Against
J W_dev J^T with the g++ Jacobian, all 24 points of the window test: <= 3.8e-15 of (|J| |W| |J|^T); the point AT t_map: diagonal (2.9e-19, 3.6e-18, -3.8e-19) for an
exact 0.  sigma at R 1e4 (solve2): 0.2 mm next to t_map, 5 .. 45 mm inside the measured span, 7e5 m in the first knot interval, which no measurement reaches."""
import ctypes as C
import os

import numpy as np
import pytest

import calib_cov_cases as CC
import lvx
import ptcov_cases as PC
import synth
import trajcov_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "ptcov_ref.npz")))
KEYS = ("point", "cov", "sigma", "sigma_max", "var_dir", "window_cov", "window_idx", "valid")
SEL_K = list(range(24)) + list(range(48, 55))   # rows of the 55 that are the pose window at t
SEL_0 = list(range(24, 55))                     # ... at t_map
_P = {}


def _problem():
    if "small" not in _P:
        _P["small"] = PC.problem()
    return _P["small"]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _context(P, locks, switches=()):
    g = lvx.Context(0)
    for k, v in switches:
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _times(P, n, seed=5):
    """n valid times: the first and the last interval, on knots, at t_map, in every interval around it (windows that share 0 .. 4 knots with the window of t_map), a
    spread; shuffled"""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    km = int(np.floor((P["t_map"] - t0) / dt))
    t = [t0, t0 + 0.3 * dt, np.nextafter(tmax, 0.0), tmax - 0.4 * dt, t0 + 5 * dt, P["t_map"], P["t_map"] + 0.05 * dt]
    t += [t0 + (km + k + 0.37) * dt for k in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5) if 0 <= km + k <= N - 4]
    rng = np.random.default_rng(seed)
    t = np.array(t[:n] + list(rng.uniform(t0, tmax, max(n - len(t), 0))))
    rng.shuffle(t)
    return t


def _points(n, seed=9):
    """float32-representable coordinates, so that the xyzi form reads the same values"""
    return np.random.default_rng(seed).uniform(-10, 10, (n, 3)).astype(np.float32).astype(np.float64)


def _dirs(n, seed=3):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _same(a, b, keys=KEYS, rows=None, where=""):
    for k in keys:
        if k in a or k in b:
            x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
            assert np.array_equal(x, y), (where, k)


def _expected_idx(P, t, free):
    want = np.array(PC.window_indices(P, P["state0"], t))
    want[~np.isin(want, free)] = -1
    return want


# 1. parity with the same damped system
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("mask", list(PC.MASKS))
def test_windows_match_the_damped_system(mask, radius, scaling):
    P = _problem()
    locks = PC.MASKS[mask]
    g = _context(P, locks)
    name = CC.case_name(mask, radius, scaling)
    tol = _tol(name)
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, scaling)
    t = _times(P, 24)
    pts, dirs = _points(len(t)), _dirs(len(t))
    r = g.map_point_covariance(pts, t, dirs, radius, scaling, window=True)
    assert r["valid"].all()
    worst = 0.0
    for i in range(len(t)):
        want = _expected_idx(P, t[i], free)
        assert np.array_equal(r["window_idx"][i], want), (name, i)
        Wd = r["window_cov"][i]
        dead = want < 0
        assert not Wd[dead].any() and not Wd[:, dead].any()
        assert np.array_equal(Wd, Wd.T) and np.array_equal(r["cov"][i], r["cov"][i].T)
        worst = max(worst, TC.window_rel_err(Wd, TC.window_of(Sig, free, want)))
    assert np.array_equal(r["sigma"], np.sqrt(np.maximum(np.einsum("nii->ni", r["cov"]), 0.0)))   # (a point measured AT t_map does not move: its terms cancel to rounding)
    print("%-24s window err %.3e (reference's own %.3e, allowed %.3e)" % (name, worst, float(REF_ERR[name]), tol))
    assert worst <= tol
    if mask == "solve3":   # the trajectory and the LiDAR are constant: every point is valid and does not move
        assert g.layout()["n_band"] == 0
        assert not r["cov"].any() and not r["sigma"].any() and not r["sigma_max"].any() and not r["var_dir"].any() and (r["window_idx"] == -1).all()
        want = np.array([PC.map_point(P, P["state0"], t[i], pts[i]) for i in range(len(t))])
        assert (np.abs(r["point"] - want).max(axis=1) <= 1e-12 * np.linalg.norm(want, axis=1)).all()
    else:
        assert np.isfinite(r["cov"]).all() and (r["sigma"][np.abs(t - P["t_map"]) > P["dt"]] > 0).all()
    if mask == "taufree":
        assert (r["window_idx"][:, 54] == 6 * P["n_knots"] + 14).all() and (np.einsum("nii->ni", r["window_cov"])[:, 54] > 0).all()
    g.close()


# 2. the two pose windows are lvx_trajectory_covariance's, bit for bit
@pytest.mark.parametrize("mask", ["solve2", "taufree"])
def test_rows_are_the_windows_of_trajectory_covariance(mask):
    P = _problem()
    g = _context(P, PC.MASKS[mask])
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    t = _times(P, 40)
    for radius, scaling in ((1e4, True), (1e8, False)):
        r = g.map_point_covariance(_points(len(t)), t, None, radius, scaling, window=True)
        tk = g.trajectory_covariance(t, lvx.FRAME_LIDAR, radius, scaling, window=True)
        tm = g.trajectory_covariance([P["t_map"]], lvx.FRAME_LIDAR, radius, scaling, window=True)
        assert r["valid"].all() and tk["valid"].all() and tm["valid"].all()
        assert np.array_equal(r["window_cov"][:, SEL_K][:, :, SEL_K], tk["window_cov"]) and np.array_equal(r["window_idx"][:, SEL_K], tk["window_idx"])
        for i in range(len(t)):
            assert np.array_equal(r["window_cov"][i][np.ix_(SEL_0, SEL_0)], tm["window_cov"][0]) and np.array_equal(r["window_idx"][i][SEL_0], tm["window_idx"][0])
    g.close()


# 3. the point, its covariance against finite-difference Jacobians, the summaries
@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("mask", ["solve1", "solve2", "taufree"])
def test_point_covariance_against_finite_differences(mask, valu):
    """valu: the plain per-lane product (switch PTCOV_VALU) that tools/ptcov_profile.py times beside the MFMA tiles is held to the same bar"""
    P = _problem()
    locks, radius = PC.MASKS[mask], 1e4
    g = _context(P, locks, (("PTCOV_VALU", 1),) if valu else ())
    name = CC.case_name(mask, radius, True)
    tol = _tol(name)
    H = g.evaluate(P["state0"], normal_eq=True, residuals=False)["H"]
    Sig, free = TC.reference_sigma(H, P["n_knots"], P["n_landmarks"], locks, radius, True)
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    km = int(np.floor((P["t_map"] - t0) / dt))
    nt = g.tangent_size
    times = np.array([t0 + 0.3 * dt, t0 + 27.6 * dt, P["t_map"] + 0.05 * dt, t0 + (km - 2 + 0.37) * dt])   # the last two: all four / two knots shared with the window of t_map
    pts, dirs = _points(len(times), 21), _dirs(len(times), 22)

    def plus(state, k, h):
        d = np.zeros(nt); d[k] = h
        return g.plus(state, d)
    r = g.map_point_covariance(pts, times, dirs, radius, True, window=True)
    assert r["valid"].all()
    for i, t in enumerate(times):
        idx = r["window_idx"][i]
        uniq = sorted({int(k) for k in idx if k >= 0})
        assert len(uniq) == (idx >= 0).sum() - (0, 0, 24, 12)[i]
        if mask == "taufree":
            assert idx[54] == 6 * N + 14

        def point(state):
            s = lvx.sample_trajectory(g, state, [t, P["t_map"]], lvx.FRAME_LIDAR, fields=("position", "orientation"))
            return PC.point_from_sensor_poses(s["orientation"][0], s["position"][0], s["orientation"][1], s["position"][1], pts[i])
        Jr, Jh = PC.fd_point_jacobian(point, P["state0"], N, uniq, plus=plus)
        if mask == "taufree":
            assert np.abs(Jr[:, uniq.index(6 * N + 14)]).max() > 1e-3   # the point moves with tau_L
        Wr = TC.window_of(Sig, free, uniq)
        cov_r, cov_h = Jr @ Wr @ Jr.T, Jh @ Wr @ Jh.T
        s = np.sqrt(np.diag(cov_r))
        level = np.abs((cov_h - cov_r) / np.outer(s, s)).max()
        jd = np.abs(Jr) @ np.sqrt(np.diag(Wr))
        carried = tol * (np.outer(jd, jd) / np.outer(s, s)).max()
        err = np.abs((r["cov"][i] - cov_r) / np.outer(s, s)).max()
        want = PC.map_point(P, P["state0"], t, pts[i])
        perr = np.abs(r["point"][i] - want).max() / np.linalg.norm(want)
        tr = np.trace(r["cov"][i])
        serr = abs(r["sigma_max"][i] ** 2 - PC.sigma_max(r["cov"][i]) ** 2) / tr
        verr = abs(r["var_dir"][i] - dirs[i] @ r["cov"][i] @ dirs[i]) / tr
        print("%s t %.4f: cov err %.3e  Richardson level %.3e  window bar carried %.3e  point err %.3e  sigma_max err %.3e  var_dir err %.3e  sigma %s" %
              (name, t, err, level, carried, perr, serr, verr, r["sigma"][i]))
        assert err <= 10 * (level + carried)
        assert perr <= 1e-12
        assert serr <= 16 * 2.0 ** -52 and verr <= 16 * 2.0 ** -52
    g.close()


# 4. shapes, bits
def test_bits_do_not_depend_on_the_batch_the_position_or_the_form():
    """n = 1 .. 257 are prefixes of one shuffled list; 257 points in one interval; one point in each interval; single points; a permutation; without the optional
    arrays; the _d form and the xyzi form (float32-representable coordinates)."""
    import torch
    P = _problem()
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    g = _context(P, CC.SOLVE2)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    rng = np.random.default_rng(77)
    t = _times(P, 257)
    pts, dirs = _points(257), _dirs(257)
    full = g.map_point_covariance(pts, t, dirs, 1e4, window=True)
    assert full["valid"].all() and np.isfinite(full["cov"]).all() and (full["sigma_max"][np.abs(t - P["t_map"]) > dt] > 0).all()
    for n in (1, 15, 16, 17, 63, 64, 65, 257):
        _same(g.map_point_covariance(pts[:n], t[:n], dirs[:n], 1e4, window=True), {k: v[:n] for k, v in full.items()}, where="prefix %d" % n)
    perm = rng.permutation(257)
    _same(g.map_point_covariance(pts[perm], t[perm], dirs[perm], 1e4, window=True), {k: v[perm] for k, v in full.items()}, where="permutation")
    for i in (0, 100, 256):
        _same(g.map_point_covariance(pts[i:i + 1], t[i:i + 1], dirs[i:i + 1], 1e4, window=True), {k: v[i:i + 1] for k, v in full.items()}, where="alone %d" % i)
    lean = g.map_point_covariance(pts, t, None, 1e4)
    _same(lean, full, keys=("point", "cov", "sigma", "sigma_max", "valid"), where="lean")
    assert "var_dir" not in lean and "window_cov" not in lean
    # 257 points of one interval (one staging, five wavefronts) and the same points alone / shuffled among other intervals
    t1 = t0 + (20 + rng.uniform(0, 1, 257)) * dt
    one = g.map_point_covariance(pts, t1, dirs, 1e4, window=True)
    assert one["valid"].all() and (one["window_idx"][:, 0] == 6 * 20).all()
    mix_t, mix_p, mix_d = np.concatenate([t1[:40], t[:100]]), np.concatenate([pts[:40], pts[:100]]), np.concatenate([dirs[:40], dirs[:100]])
    order = rng.permutation(140)
    mixed = g.map_point_covariance(mix_p[order], mix_t[order], mix_d[order], 1e4, window=True)
    inv = np.argsort(order)
    _same({k: v[inv][:40] for k, v in mixed.items()}, {k: v[:40] for k, v in one.items()}, where="one interval among others")
    _same({k: v[inv][40:] for k, v in mixed.items()}, {k: v[:100] for k, v in full.items()}, where="others among one interval")
    # one point in each interval, descending
    te = t0 + (np.arange(N - 3)[::-1] + 0.5) * dt
    each = g.map_point_covariance(pts[:N - 3], te, dirs[:N - 3], 1e4, window=True)
    assert each["valid"].all() and list(each["window_idx"][:, 0] // 6) == list(range(N - 3))[::-1]
    _same(g.map_point_covariance(pts[7:8], te[7:8], dirs[7:8], 1e4, window=True), {k: v[7:8] for k, v in each.items()}, where="each alone")
    # the device forms
    dev = torch.device("cuda:0")
    n = 257
    t_d, p_d, d_d = torch.from_numpy(t).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(dirs).to(dev)
    xyzi = np.concatenate([pts, np.full((n, 1), 0.5)], axis=1).astype(np.float32)
    assert np.array_equal(xyzi[:, :3].astype(np.float64), pts)
    x_d = torch.from_numpy(xyzi).to(dev)
    for form in ("d", "xyzi"):
        o = dict(point=torch.full((n, 3), 7.0, dtype=torch.float64, device=dev), cov=torch.full((n, 9), 7.0, dtype=torch.float64, device=dev),
                 sigma=torch.full((n, 3), 7.0, dtype=torch.float64, device=dev), sigma_max=torch.full((n,), 7.0, dtype=torch.float64, device=dev),
                 var_dir=torch.full((n,), 7.0, dtype=torch.float64, device=dev), window_cov=torch.full((n, 3025), 7.0, dtype=torch.float64, device=dev),
                 window_idx=torch.full((n, 55), 7, dtype=torch.int32, device=dev))
        valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        if form == "d":
            g.map_point_covariance_d(p_d.data_ptr(), t_d.data_ptr(), n, {k: v.data_ptr() for k, v in o.items()}, valid.data_ptr(), d_d.data_ptr(), radius=1e4)
        else:
            g.map_point_covariance_d(x_d.data_ptr(), t_d.data_ptr(), n, {k: v.data_ptr() for k, v in o.items()}, valid.data_ptr(), xyzi=True, radius=1e4)
        g.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["cov"] = got["cov"].reshape(n, 3, 3); got["window_cov"] = got["window_cov"].reshape(n, 55, 55); got["valid"] = valid.cpu().numpy().astype(bool)
        if form == "xyzi":
            assert (got.pop("var_dir") == 7.0).all()   # no directions: not written
        _same(got, full, keys=tuple(got), where=form)
    g.close()


# 5. validity
def test_invalid_points_leave_their_neighbours_alone():
    P = _problem()
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    g = _context(P, CC.SOLVE2)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    t = _times(P, 70)
    pts, dirs = _points(70), _dirs(70)
    clean = g.map_point_covariance(pts, t, dirs, 1e4, window=True)
    bad_t, bad_p = t.copy(), pts.copy()
    bad_t[3] = tmax; bad_t[17] = np.nan; bad_t[64] = t0 - 1e-6
    bad_p[5, 1] = np.nan; bad_p[66, 2] = np.inf
    bad = [3, 5, 17, 64, 66]
    r = g.map_point_covariance(bad_p, bad_t, dirs, 1e4, window=True)
    ok = np.setdiff1d(np.arange(70), bad)
    assert not r["valid"][bad].any() and r["valid"][ok].all()
    for k in ("point", "cov", "sigma", "sigma_max", "var_dir", "window_cov"):
        assert not r[k][bad].any(), k
    assert (r["window_idx"][bad] == -1).all()
    _same({k: v[ok] for k, v in r.items()}, {k: v[ok] for k, v in clean.items()}, where="neighbours")
    g.close()


# 6. errors
def test_errors_are_codes_and_a_failed_call_writes_nothing():
    import torch
    P = _problem()
    g = _context(P, CC.SOLVE2)
    t, pts = _times(P, 5), _points(5)
    with pytest.raises(lvx.LvxError) as e:
        g.map_point_covariance(pts, t)
    assert e.value.code == lvx.E_STATE
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    for kw in (dict(radius=0.0), dict(radius=-1.0)):
        with pytest.raises(lvx.LvxError) as e:
            g.map_point_covariance(pts, t, **kw)
        assert e.value.code == lvx.E_ARG
    with pytest.raises(lvx.LvxError) as e:
        g.map_point_covariance(np.zeros((0, 3)), np.zeros(0))
    assert e.value.code == lvx.E_ARG
    n = len(t)
    cov, valid = np.full((n, 9), 7.0), np.full(n, 7, np.uint8)
    opt = g._cov_options(lvx.PointCovOptions, g._l.lvx_point_cov_default_options, 1e8, True)
    args = lambda rec, o=opt, pp=pts, tt=t: (g._h, C.byref(o), C.c_int(n), pp.ctypes.data_as(C.c_void_p) if pp is not None else None,
                                             tt.ctypes.data_as(C.c_void_p) if tt is not None else None, None, C.byref(rec))
    rec = lvx.PointCov(None, cov.ctypes.data, None, None, None, None, None, valid.ctypes.data)
    bad_opt = g._cov_options(lvx.PointCovOptions, g._l.lvx_point_cov_default_options, 1e8, True); bad_opt.reserved = 1
    assert g._l.lvx_map_point_covariance(*args(rec, o=bad_opt)) == lvx.E_ARG
    assert g._l.lvx_map_point_covariance(*args(rec, pp=None)) == lvx.E_ARG and g._l.lvx_map_point_covariance(*args(rec, tt=None)) == lvx.E_ARG
    assert g._l.lvx_map_point_covariance(*args(lvx.PointCov(None, cov.ctypes.data, None, None, None, None, None, None))) == lvx.E_ARG
    assert (cov == 7.0).all() and (valid == 7).all()
    seen = []

    def allreduce(buf, op):
        try:
            g.map_point_covariance(pts, t)
            seen.append(None)
        except lvx.LvxError as err:
            seen.append(err.code)
    g.solve_step_shared(1e4, allreduce)
    assert seen and all(c == lvx.E_STATE for c in seen)
    # a declared pivot failure: LVX_E_NOTPD, the pre-filled arrays intact (host form), nothing written and the code at lvx_synchronize (_d form)
    g.set_switch("TEST_BAD_PIVOT", 1)
    assert g._l.lvx_map_point_covariance(*args(rec)) == lvx.E_NOTPD and (cov == 7.0).all() and (valid == 7).all()
    dev = torch.device("cuda:0")
    t_d, p_d = torch.from_numpy(t).to(dev), torch.from_numpy(pts).to(dev)
    cov_d, valid_d = torch.full((n, 9), 7.0, dtype=torch.float64, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.map_point_covariance_d(p_d.data_ptr(), t_d.data_ptr(), n, dict(cov=cov_d.data_ptr()), valid_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NOTPD and bool((cov_d == 7.0).all()) and bool((valid_d == 7).all())
    g.synchronize()   # reported once
    g.set_switch("TEST_BAD_PIVOT", 0)
    assert g.map_point_covariance(pts, t)["valid"].all()   # the context is as usable as before
    g.close()


def test_no_hub_and_a_hub_window_in_the_band_are_state_errors():
    """Without surfel / camera-surfel rows nothing has set t_map.  With camera-surfel rows alone the hub knots lie around t_map + tau_C; a LOCKED tau_L of three knot
    intervals moves the LiDAR's pose at t_map onto band knots, whose cross terms with a point's knots are off the factor's pattern: the call refuses, writes nothing."""
    import torch
    Pn = synth.make_problem(**CC.ND)
    g = _context(Pn, CC.ND_LOCKS)
    g.evaluate(Pn["state0"], normal_eq=True, dense=False, residuals=False)
    with pytest.raises(lvx.LvxError) as e:
        g.map_point_covariance(_points(3), Pn["t0"] + np.array([0.1, 0.2, 0.3]))
    assert e.value.code == lvx.E_STATE
    g.close()
    Pc = synth.make_problem(seed=14, duration=0.4, n_surfel=0, n_landmarks=12, n_camsurf=5)
    N, dt = Pc["n_knots"], Pc["dt"]
    x = Pc["state0"].copy()
    g = _context(Pc, CC.SOLVE2)
    t, pts = Pc["t0"] + np.array([3.3, 20.1, 30.7]) * dt, _points(3)
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    r = g.map_point_covariance(pts, t)   # tau_L = 0: the window of t_map is the hub's
    assert r["valid"].all() and (r["sigma"] > 0).all()
    x[7 * N + 23] = 3 * dt
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    n = 3
    cov, valid = np.full((n, 9), 7.0), np.full(n, 7, np.uint8)
    rec = lvx.PointCov(None, cov.ctypes.data, None, None, None, None, None, valid.ctypes.data)
    opt = g._cov_options(lvx.PointCovOptions, g._l.lvx_point_cov_default_options, 1e8, True)
    rc = g._l.lvx_map_point_covariance(g._h, C.byref(opt), C.c_int(n), pts.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None, C.byref(rec))
    assert rc == lvx.E_STATE and (cov == 7.0).all() and (valid == 7).all()
    dev = torch.device("cuda:0")
    t_d, p_d = torch.from_numpy(t).to(dev), torch.from_numpy(pts).to(dev)
    cov_d, valid_d = torch.full((n, 9), 7.0, dtype=torch.float64, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.map_point_covariance_d(p_d.data_ptr(), t_d.data_ptr(), n, dict(cov=cov_d.data_ptr()), valid_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_STATE and bool((cov_d == 7.0).all()) and bool((valid_d == 7).all())
    g.close()


# 7. host: Calibrator::MapPointCovariance over a raw scan
def test_calibrator_carries_a_raw_scan_into_the_map_with_its_sigmas(tmp_path):
    """The noise-free 6 s sequence of tests/test_gpu_pipeline.py, the surfel stage alone.  Every 7th point of raw scan 20 through Calibrator::MapPointCovariance (the
    existing getter lvx_get_scans_raw, then the host form): valid points with finite positive sigmas, sigma_max >= every axis sigma, p_M against the reference's chain
    restated in numpy at the final state (1e-12 |p_M|), the same bits for the same points in reverse order, and FormatMapPointUncertainty's line."""
    import subprocess
    import build as lvx_build
    from test_gpu_pipeline import _write
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "ptcov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "ptcov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin = str(tmp_path / "seq.bin")
    _write(pin, S, refine_iterations=1, lvi=0, camsurf=0)
    scan, step = 20, 7
    r = subprocess.run([exe, pin, str(scan), str(step)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    head = lines[0].split()
    n, n_valid, radius = int(head[2]), int(head[4]), float(head[6])
    assert radius == 1e8 and n > 100 and n_valid == n
    assert lines[1].startswith("[Map] point std (mm): median")
    rows = [ln.split()[1:] for ln in lines if ln.startswith("P ")]
    assert len(rows) == n and "REVERSED 1" in lines
    state = np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith("STATE")][0].split()[1:]])
    Pd = dict(t0=S["t0"], dt=S["dt"], n_knots=S["n_knots"], t_map=S["t_map"])
    sc = S["scans"][scan]
    worst = 0.0
    for row in rows:
        k = int(row[0])
        assert k % step == 0 and int(row[1]) == 1
        pm, sig, smax = np.array([float.fromhex(v) for v in row[2:5]]), np.array([float.fromhex(v) for v in row[5:8]]), float.fromhex(row[8])
        assert np.isfinite(sig).all() and (sig > 0).all() and smax >= sig.max() and smax <= np.sqrt((sig ** 2).sum()) * (1 + 1e-12)
        p_l = np.array([sc["x"][k], sc["y"][k], sc["z"][k]], np.float32).astype(np.float64)
        want = PC.map_point(Pd, state, sc["timestamp"][k], p_l)
        worst = max(worst, np.abs(pm - want).max() / np.linalg.norm(want))
    print(lines[1], "point err %.3e" % worst)
    assert worst <= 1e-12
