"""CPU checks behind lvx_landmark_covariance (no GPU): the map point and its 3 x 32 Jacobian of lvi-exc_amd/csrc/lvx_lmcov.h (g++ build:
tests/native/lmcov_host_check.cpp) against central differences through EigenQuaternionParameterization::Plus; the landmark formula restated in numpy on the selected
inverse of random band + border systems (tests/landmark_cov_cases.py: k_band_selinv's panel order with its wide band store, k_landmark_cov's read) against a float64
inverse of the full system; the layout of the call's two structs.

Jacobian bar: 10 x the largest difference between the two Richardson levels (central differences at h / 2 and their extrapolation with h), as tests/test_trajcov_host.py
sets it; h = 1e-3 in tangent units, 1e-5 s for the time offset, 1e-3 rho for the inverse depth.  Observed: the levels differ by 1.6e-6 .. 1.8e-6 (the rotation columns, which
carry the lever |y_h / rho|), |J - extrapolation| <= 4.2e-9.
Formula bar: both sides are float64 eliminations of a random factor with diagonal in [1, 2]: 1e-9 of sqrt(S_ii S_jj), the bar of the selected inverse's own test;
observed 4e-15 .. 4.6e-10 (the largest at nb = 40, bw = 64, 46 border rows)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import landmark_cov_cases as LC
import lvx
import synth
import trajcov_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADTAN = dict(synth.DEFAULT_CAMERA, k1=-0.17, k2=0.03, p1=1e-3, p2=-5e-4, k3=0.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lmcov") / "liblmcov_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", so, os.path.join(ROOT, "tests", "native", "lmcov_host_check.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def problem():
    P = synth.make_problem(seed=14, duration=0.4, n_surfel=0, n_landmarks=4, n_camsurf=0)
    x = P["state0"].copy()
    x[7 * P["n_knots"] + 31] = -8e-4   # a camera time offset that is not zero
    return P, x


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cam10(cam):
    return np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "readout")], float)


def _call(host, P, x, cam, l, uv, t0_ref):
    J = np.zeros((3, LC.W)); idx = np.zeros(LC.W, np.int32); Pw = np.zeros(3); yh = np.zeros(3)
    st = host.lc_jacobian(_p(np.ascontiguousarray(x)), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), _p(_cam10(cam)), C.c_int(cam["rows"]),
                          C.c_int(cam["cols"]), C.c_int(l), C.c_double(uv[0]), C.c_double(uv[1]), C.c_double(t0_ref), _p(J), _p(idx), _p(Pw), _p(yh))
    return st, J, idx, Pw, yh


def _plus(P, x, g, h):
    N = P["n_knots"]
    if g >= 6 * N + 22:
        y = np.array(x, float); y[7 * N + 32 + (g - 6 * N - 22)] += h
        return y
    return TC.plus_tangent(x, N, g, h)


@pytest.mark.parametrize("radtan", [False, True])
@pytest.mark.parametrize("where", ["u0_i0first", "u_near_1", "i0_last", "inner"])
def test_jacobian_against_central_differences(host, problem, where, radtan):
    P, x = problem
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    cam = RADTAN if radtan else P["camera"]
    l, uv = 2, np.array([911.0, 203.0])
    row = uv[1] * cam["readout"] / cam["rows"]
    tau = x[7 * N + 31]
    tt = {"u0_i0first": t0 + 1e-3 * dt, "u_near_1": t0 + 7 * dt + dt * (1 - 1e-9), "i0_last": t0 + (N - 4) * dt + 0.63 * dt, "inner": t0 + 20.41 * dt}[where]   # t_ref, offset included
    t0_ref = tt - tau - row
    st, J, idx, Pw, yh = _call(host, P, x, cam, l, uv, t0_ref)
    assert st == 0
    i0 = int(np.floor(((t0_ref + tau) + row - t0) / dt))
    assert list(idx) == [6 * N + 22 + l] + [6 * (i0 + c // 6) + c % 6 for c in range(24)] + [6 * N + 15 + b for b in range(7)]
    if where == "u0_i0first":
        assert i0 == 0
    if where == "i0_last":
        assert i0 == N - 4
    assert np.allclose(yh, LC.unproject(cam, uv), rtol=0, atol=1e-15)
    if radtan:
        assert np.abs(yh[:2] - LC.unproject(P["camera"], uv)[:2]).max() > 1e-3   # the iteration moved the ray

    def point(state):
        s, _, _, p, _ = _call(host, P, state, cam, l, uv, t0_ref)
        assert s == 0
        return p
    rho = x[7 * N + 32 + l]
    Jr = np.zeros((3, LC.W)); Jh = np.zeros((3, LC.W))
    for c, g in enumerate(idx):
        h = 1e-3 * rho if c == 0 else (1e-5 if g == 6 * N + 21 else 1e-3)
        d1 = (point(_plus(P, x, g, h)) - point(_plus(P, x, g, -h))) / (2 * h)
        d2 = (point(_plus(P, x, g, h / 2)) - point(_plus(P, x, g, -h / 2))) / h
        Jh[:, c] = d2; Jr[:, c] = (4 * d2 - d1) / 3
    level = np.abs(Jr - Jh).max()
    err = np.abs(J - Jr).max()
    print("%-11s radtan %d: Richardson levels differ by %.3e, |J - J_fd| = %.3e" % (where, radtan, level, err))
    assert err <= 10 * level
    # the point against the spline restated in numpy (synth.Spline)
    assert np.abs(J[:, 0] + (Pw - _cam_origin(P, x, tt)) / rho).max() <= 1e-12 * np.abs(J[:, 0]).max()   # column 0 = -(P - p_C) / rho


def _cam_origin(P, x, tt):
    """p_C(tt) = p(tt) + R(tt) p_CI from the numpy spline of synth"""
    N = P["n_knots"]
    sp = synth.Spline(P["t0"], P["dt"], x[:3 * N].reshape(N, 3), x[3 * N:7 * N].reshape(N, 4))
    e = sp.eval(np.array([tt]))
    return e["pos"][0] + LC.qrot(e["quat"][0], x[7 * N + 28:7 * N + 31])


def test_jacobian_reports_range_and_unit_norm(host, problem):
    P, x = problem
    N, t0, dt = P["n_knots"], P["t0"], P["dt"]
    cam = P["camera"]
    uv = np.array([640.0, 0.0])
    tau = x[7 * N + 31]
    assert _call(host, P, x, cam, 0, uv, t0 + (N - 3) * dt - tau)[0] == 1 and _call(host, P, x, cam, 0, uv, float("nan"))[0] == 1 and _call(host, P, x, cam, 0, uv, t0 - 1e-3)[0] == 1
    y = x.copy()
    y[3 * N + 4 * 12:3 * N + 4 * 12 + 4] *= 1.001
    assert _call(host, P, y, cam, 0, uv, t0 + 10.5 * dt)[0] == 2 and _call(host, P, y, cam, 0, uv, t0 + 20.5 * dt)[0] == 0


def _landmarks(rng, nb, bw, nbd):
    """rows over (band, border): one that starts at position 0, one that ends at nb, one whose band part ends at nb and that reaches into the border, one on the border
    alone; zeros inside the windows.  Returns [(positions, values)] with positions >= 0 band, < 0 border slot."""
    wl = min(bw + 1, nb)
    rows = []

    def band(lo):
        pos = [p for p in range(lo, lo + wl) if rng.uniform() < 0.7]
        return pos or [lo]
    bord = [-1 - r for r in sorted(rng.choice(nbd, 6, replace=False))]
    if nb:
        rows.append(band(0))
        rows.append(band(nb - wl))
        rows.append(band(nb - wl) + bord)
        rows.append(band((nb - wl) // 2) + bord[:2])
    rows.append(bord)
    return [(pos, list(rng.uniform(-1, 1, len(pos)))) for pos in rows]


@pytest.mark.parametrize("nbd", [22, 46])
@pytest.mark.parametrize("bw", [23, 64])
@pytest.mark.parametrize("nb", [0, 16, 40])
def test_landmark_formula_restated(nb, bw, nbd):
    """The REDUCED system (band + border, trajcov_cases.random_system) with its selected inverse in the kernel's panel order and wide store; landmarks with scaled rows
    e_l and pivots d_l are put back in front of it: A_full = [[diag d, e], [e^T, A + sum e_l^T e_l / d_l]], whose inverse numpy forms.  Jacobi scales are random, so the
    unscaling is exercised: the device's inputs are the UNSCALED row e / (s_l s_x) and w_l = s_l^2 / d_l."""
    rng = np.random.default_rng(7000 * nb + 10 * bw + nbd)
    bw_eff = min(bw, max(nb - 1, 0))
    A, Lb, Z, S = TC.random_system(rng, nb, bw_eff, nbd)
    n = nb + nbd
    sigw, zb, cc = LC.selinv_wide(Lb, Z, S, nb, bw_eff, nbd)
    rows = _landmarks(rng, nb, bw_eff, nbd)
    nl = len(rows)
    col = lambda p: p if p >= 0 else nb - 1 - p
    E = np.zeros((nl, n)); d = rng.uniform(0.5, 2.0, nl)
    for k, (pos, val) in enumerate(rows):
        E[k, [col(p) for p in pos]] = val
    full = np.zeros((nl + n, nl + n))
    full[:nl, :nl] = np.diag(d); full[:nl, nl:] = E; full[nl:, :nl] = E.T
    full[nl:, nl:] = A + E.T @ np.diag(1.0 / d) @ E
    s_x = rng.uniform(0.5, 1.5, n); s_l = rng.uniform(0.5, 1.5, nl)
    s_all = np.concatenate([s_l, s_x])
    Sig = np.linalg.inv(full) * np.outer(s_all, s_all)
    dd = np.sqrt(np.diag(Sig))
    worst = 0.0
    for k, (pos, val) in enumerate(rows):
        lo = min([p for p in pos if p >= 0], default=0)
        win = list(range(lo, min(lo + 24, nb))) + [None] + [-1 - r for r in range(nbd - 7, nbd)]   # a pose window inside the row's reach, a constant, the last border slots
        e_unscaled = [v / (s_l[k] * s_x[col(p)]) for p, v in zip(pos, val)]
        Wn = LC.landmark_block(pos, e_unscaled, s_l[k] ** 2 / d[k], win, s_x, nb, sigw, zb, cc)
        live = [m for m, p in enumerate(win) if p is not None]
        g = np.array([k] + [nl + col(win[m]) for m in live])
        sel = np.array([0] + [1 + m for m in live])
        ref = Sig[np.ix_(g, g)]
        worst = max(worst, np.abs((Wn[np.ix_(sel, sel)] - ref) / np.outer(dd[g], dd[g])).max())
        dead = 1 + win.index(None)
        assert not Wn[dead].any() and not Wn[:, dead].any() and np.array_equal(Wn, Wn.T)
    print("nb %d bw %d nbd %d: %d landmarks, max error %.3e" % (nb, bw, nbd, nl, worst))
    assert worst <= 1e-9


def test_wide_store_agrees_with_the_narrow_one_and_stops_at_the_lowest_position():
    rng = np.random.default_rng(3)
    nb, bw, nbd = 70, 40, 5
    A, Lb, Z, S = TC.random_system(rng, nb, bw, nbd)
    sigb, zb0, _ = TC.selinv_panels(Lb, Z, S, nb, bw, nbd)
    sigw, zb, _ = LC.selinv_wide(Lb, Z, S, nb, bw, nbd)
    assert sigw.shape[1] == 49 and np.array_equal(sigw[:, :24], sigb, equal_nan=True) and np.array_equal(zb, zb0)   # the same values, stored twice
    Sig = np.linalg.inv(A)
    for j in range(nb):
        for dd in range(min(48, nb - 1 - j) + 1):
            assert abs(sigw[j, dd] - Sig[j + dd, j]) <= 1e-9 * np.sqrt(Sig[j, j] * Sig[j + dd, j + dd])
    part, _, _ = LC.selinv_wide(Lb, Z, S, nb, bw, nbd, lowest=41)
    assert np.isnan(part[:32]).all() and np.array_equal(part[32:], sigw[32:], equal_nan=True)


def test_struct_layout_matches_the_ctypes_mirrors(host):
    out = (C.c_longlong * 13)()
    host.lc_layout(out)
    o, r = lvx.LandmarkCovOptions, lvx.LandmarkCov
    assert list(out) == [C.sizeof(o), o.radius.offset, o.jacobi_scaling.offset, o.reserved.offset,
                         C.sizeof(r), r.var_rho.offset, r.sigma_rho.offset, r.point.offset, r.point_cov.offset, r.window_cov.offset, r.window_idx.offset, r.valid.offset,
                         lvx.LM_COV_W]
