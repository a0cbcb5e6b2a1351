"""Shared by tests/test_rotinit_host.py and tests/test_gpu_rotinit.py: a numpy float64 restatement of InertialInitializer::EstimateRotation written from the reference
source (src/lvi_exc/src/core/inertial_initializer.cpp:26-81 — it stacks the A_j and runs np.linalg.svd; it never calls lvi-exc_amd/csrc/lvx_rotinit.h), odometry built from
the true state of traj_cases.problem() with a planted mounting rotation, the cases, the bars and the g++ build of the header (tests/native/rotinit_host_check.cpp) behind
ctypes.  The spline orientations of the restatement come from traj_cases.host_sample, which tests/test_traj_host.py pins to the oracle.

Bars.  The ten sums have <= 256 terms of O(1) each, the restatement's SVD and the Jacobi solver are backward stable: eigenvalues (squared singular values) are held at
1e-12 lambda_max absolute — squares, because for exact data sigma_min is about 1e-15 and carries no digits.  The quaternion is an eigenvector whose neighbour is
lambda[2] - lambda[3] away: the angle between the two estimates is held at 2e-12 lambda_max / (lambda[2] - lambda[3]) rad, from the restatement's own spectrum; the data
are chosen so that this ratio is at most 1e3 wherever a quaternion is compared."""
import ctypes as C
import os
import subprocess

import numpy as np

import lvx
import synth
import traj_cases as tc

ROOT = tc.ROOT
Q_LTOI = synth.q_from_rotvec(np.array([1.3, -1.9, 1.4]))   # |rotvec| = 2.69 rad, away from every axis
GAP_RATIO_MAX = 1e3
_LIB = None


def planted_angle():
    return float(np.linalg.norm([1.3, -1.9, 1.4]))


def stamps(P, n, on_knots, lo=0.0, hi=None):
    """n increasing stamps inside the valid range: on the 0.02 s knots (as 10 Hz stamps are) or off them."""
    tmin, tmax = tc.time_range(P)
    hi = (tmax - tmin) if hi is None else hi
    if on_knots:
        k = np.unique(np.round(np.linspace(lo / P["dt"], hi / P["dt"] - 1, n)).astype(int))
        assert len(k) == n, "more stamps than knots"
        return P["t0"] + k * P["dt"]
    return tmin + np.linspace(lo + 0.0013, hi - 0.0017, n)


def odometry(P, t, late=0.0, q_LtoI=Q_LTOI):
    """Odometry quaternions (x, y, z, w) of a sensor mounted with q_LtoI, relative to its first pose: q'_k = q_L(t_0)* q_L(t_k), q_L(t) = q(t + late) q_LtoI with q the TRUE
    spline.  late: the pose recorded under the stamp t belongs to the spline time t + late.  A stamp outside the spline gets a fixed unrelated quaternion."""
    t = np.asarray(t, np.float64)
    smp, _ = tc.host_sample(P, P["state_true"], t + late)
    ok = smp["valid"]
    q = np.tile(np.array([0.3, -0.2, 0.5, 0.6]), (len(t), 1))
    qL = synth.qmul(smp["orientation"][ok], np.broadcast_to(q_LtoI, (int(ok.sum()), 4)))
    q[ok] = synth.qmul(np.broadcast_to(synth.qconj(qL[0]), qL.shape), qL)
    return q


def _left(q):
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def _right(q):
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def _angle(q):
    return 2.0 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3]))


def np_estimate(P, state, t, q, n_poses=None, tau=0.0, huber_deg=1.0, min_pairs=15, min_sigma=0.25, n_knots=None, skip=None):
    """EstimateRotation on the first n_poses odometry poses with the stamps shifted by tau.  Returns a dict: n_poses, n_pairs, n_skipped, ok, sigma (4, zeros below
    min_pairs), lam = sigma^2, x (q_ItoS, w >= 0; identity below min_pairs), weights (huber per counted pair).  skip: a predicate on evaluation times that are to be
    treated as a non-unit window."""
    t, q = np.asarray(t, np.float64), np.asarray(q, np.float64)
    n = len(t) if n_poses is None else n_poses
    tmin, tmax = tc.time_range(P, n_knots)
    tt = t[:n] + tau
    with np.errstate(invalid="ignore"):
        inside = (tt >= tmin) & (tt < tmax)
    qs = np.zeros((n, 4))
    if inside.any():
        smp, _ = tc.host_sample(P, state, tt[inside], n_knots=n_knots)
        qs[inside] = smp["orientation"]
        bad = ~smp["valid"]
    else:
        bad = np.zeros(0, bool)
    nonunit = np.zeros(n, bool)
    nonunit[np.flatnonzero(inside)[bad]] = True
    if skip is not None:
        assert np.array_equal(nonunit, inside & skip(tt))
    else:
        assert not nonunit.any()
    qn = q[:n] / np.linalg.norm(q[:n], axis=1, keepdims=True)
    A, w, skipped = [], [], 0
    for j in range(1, n):
        i = j - 1
        if not (tt[j] < tmax) or not np.isfinite(tt[j]):   # :39-40
            break
        if not inside[i] or not inside[j] or nonunit[i] or nonunit[j]:   # the documented deviation: skipped and counted, where Evaluate would throw
            skipped += 1
            continue
        d_imu = synth.qmul(synth.qconj(qs[i]), qs[j])
        d_sen = synth.qmul(synth.qconj(qn[i]), qn[j])
        if d_sen[3] < 0:
            d_sen = -d_sen   # Matrix3d -> Quaterniond yields w >= 0 for trace > 0
        delta = 180.0 / np.pi * abs(_angle(d_sen) - _angle(d_imu))
        h = 1.0 / delta * huber_deg if delta > huber_deg else 1.0
        A.append(h * (_left(d_sen) - _right(d_imu)))
        w.append(h)
    out = {"n_poses": n, "n_pairs": len(A), "n_skipped": skipped, "ok": 0, "sigma": np.zeros(4), "lam": np.zeros(4), "x": np.array([0.0, 0.0, 0.0, 1.0]), "weights": np.array(w)}
    if len(A) < min_pairs:
        return out
    _, s, Vt = np.linalg.svd(np.vstack(A), full_matrices=False)
    x = Vt[3] / np.linalg.norm(Vt[3])
    out.update(sigma=s, lam=s * s, x=-x if x[3] < 0 else x, ok=int(s[2] > min_sigma))
    return out


def gap_ratio(ref):
    return ref["lam"][0] / (ref["lam"][2] - ref["lam"][3])


def check_record(rec, ref, tag=""):
    """One record (a numpy void of lvx.ROTINIT_DTYPE) against the restatement: counts and ok exact, eigenvalues and quaternion within the bars.  Returns the two worst
    figures as fractions of their bars."""
    assert (int(rec["n_poses"]), int(rec["n_pairs"]), int(rec["n_skipped"]), int(rec["ok"])) == (ref["n_poses"], ref["n_pairs"], ref["n_skipped"], ref["ok"]), (tag, rec, ref)
    if ref["n_pairs"] == 0 or not ref["lam"].any():
        assert not np.asarray(rec["sigma"]).any() and np.array_equal(rec["q_ItoS_xyzw"], [0, 0, 0, 1]), (tag, rec)
        return 0.0, 0.0
    lam_max = ref["lam"][0]
    e_lam = float(np.abs(np.asarray(rec["sigma"]) ** 2 - ref["lam"]).max())
    x = np.asarray(rec["q_ItoS_xyzw"])
    assert x[3] >= 0 and abs(np.linalg.norm(x) - 1) < 1e-14, (tag, x)
    ratio = gap_ratio(ref)
    assert ratio <= GAP_RATIO_MAX, (tag, ratio)
    s = 1.0 if x @ ref["x"] >= 0 else -1.0
    ang = float(2.0 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(s * x - ref["x"]))))
    bar_l, bar_q = 1e-12 * lam_max, 2e-12 * ratio
    print("%s lambda: max |got - ref| = %.3e (bar %.3e)   angle(got, ref) = %.3e rad (bar %.3e)   sigma = %s" % (tag, e_lam, bar_l, ang, bar_q, np.asarray(rec["sigma"])))
    assert e_lam <= bar_l, (tag, e_lam, bar_l)
    assert ang <= bar_q, (tag, ang, bar_q)
    return e_lam / bar_l, ang / bar_q


_REFS = {}


def reference(name):
    """The restatement of every record of a case, [n_tau][n_prefix] dicts: computed once."""
    if name not in _REFS:
        c = cases()[name]
        pl = [len(c["t"])] if c["prefix_len"] is None else list(c["prefix_len"])
        ta = [0.0] if c["tau"] is None else list(c["tau"])
        opt = c["opt"]
        o = dict(huber_deg=1.0, min_pairs=15, min_sigma=0.25) if opt is None else dict(huber_deg=opt.huber_deg, min_pairs=opt.min_pairs, min_sigma=opt.min_sigma)
        _REFS[name] = [[np_estimate(c["P"], c["state"], c["t"], c["q"], n, tv, **o) for n in pl] for tv in ta]
    return _REFS[name]


def check_refs(res, first_ok, refs, tag=""):
    """Every record of a call and first_ok against restatement records [n_tau][n_prefix].  Returns the worst fractions of the two bars."""
    assert res.shape == (len(refs), len(refs[0])) and len(first_ok) == len(refs), (tag, res.shape)
    worst = np.zeros(2)
    for a, row in enumerate(refs):
        for b, ref in enumerate(row):
            worst = np.maximum(worst, check_record(res[a, b], ref, "%s [%d][%d] n=%d" % (tag, a, b, ref["n_poses"])))
        oks = [b for b, ref in enumerate(row) if ref["ok"]]
        assert first_ok[a] == (oks[0] if oks else -1), (tag, a, first_ok[a], oks)
    return worst


def check_case(name, res, first_ok):
    return check_refs(res, first_ok, reference(name), name)


def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "rotinit_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "librotinit_host_check.so")
        deps = [src] + [os.path.join(ROOT, "lvi-exc_amd", "csrc", f) for f in ("lvx_math.h", "lvx_resid.h", "lvx_traj.h", "lvx_rotinit.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_estimate(P, state, t, q, prefix_len=None, tau=None, opt=None, n_knots=None):
    """The g++ build of the header: (results [n_tau][n_prefix], first_ok, status) — status 0, 2 (a non-unit control quaternion) or -1 (a bad prefix list)."""
    N = P["n_knots"] if n_knots is None else n_knots
    t, q = np.ascontiguousarray(t, np.float64), np.ascontiguousarray(q, np.float64).reshape(-1, 4)
    pl = None if prefix_len is None else np.ascontiguousarray(prefix_len, np.int32)
    ta = None if tau is None else np.ascontiguousarray(tau, np.float64)
    n_prefix, n_tau = (0 if pl is None else len(pl)), (0 if ta is None else len(ta))
    res, first = np.zeros((max(n_tau, 1), max(n_prefix, 1)), lvx.ROTINIT_DTYPE), np.zeros(max(n_tau, 1), np.int32)
    h, mp, ms = (1.0, 15, 0.25) if opt is None else (opt.huber_deg, opt.min_pairs, opt.min_sigma)
    st = host_lib().rh_estimate(_p(np.ascontiguousarray(state, np.float64)), C.c_int(N), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(len(t)), _p(t), _p(q), C.c_int(n_prefix), _p(pl),
                                C.c_int(n_tau), _p(ta), C.c_double(h), C.c_int(mp), C.c_double(ms), _p(res), _p(first))
    return res, first, st


def options(huber_deg=1.0, min_pairs=15, min_sigma=0.25):
    o = lvx.RotInitOptions()
    o.huber_deg, o.min_pairs, o.reserved, o.min_sigma = huber_deg, min_pairs, 0, min_sigma
    return o


# ---- the cases: name -> dict(P, t, q, prefix_len, tau, opt); built once, read-only ----
_CASES = None
_LONG = None
SHIFT_TRUE = 0.03
SHIFTS = np.round(np.arange(-6, 7) * 0.01, 2)
LONG_PREFIXES = [1, 16, 20, 24, 36, 40, 60]   # sigma[2] of the restatement: 0.116, 0.147, 0.176 | 0.335, 0.382, 0.499 (10 Hz, about 0.8 rad/s): the fifth is the first to pass


def long_problem():
    """The same generator as traj_cases.problem(), 6 s long (323 knots): long enough for sigma[2] to cross the reference's 0.25 at 10 Hz.  Read-only."""
    global _LONG
    if _LONG is None:
        _LONG = synth.make_problem(seed=41, duration=6.0, n_surfel=0, n_planes=1, n_landmarks=0)
        assert _LONG["n_knots"] == 323
    return _LONG


def with_planted_step(q, m, deg):
    """Odometry whose step m - 1 -> m turns deg degrees further about its own axis: its rotation angle, and nothing else, differs from the spline's by deg."""
    q = np.array(q, np.float64)
    d = synth.qmul(synth.qconj(q[m - 1]), q[m])
    if d[3] < 0:
        d = -d
    ax = d[:3] / np.linalg.norm(d[:3])
    d2 = synth.qmul(d, synth.q_from_rotvec(ax * np.deg2rad(deg)))
    rest = synth.qmul(np.broadcast_to(synth.qconj(q[m]), q[m:].shape), q[m:])
    q[m:] = synth.qmul(np.broadcast_to(synth.qmul(q[m - 1], d2), rest.shape), rest)
    return q


def with_tail(P, t):
    """Two stamps before MinTime in front; behind: MaxTime, a stamp past it, then a finite in-range stamp (which the break must keep out) and NaN."""
    tmin, tmax = tc.time_range(P)
    t2 = np.concatenate([[tmin - 0.05, tmin - 0.02], t, [tmax, tmax + 0.3, 0.5 * (tmin + tmax), np.nan]])
    return t2, odometry(P, t2)


def case(P, t, q, prefix_len=None, tau=None, opt=None):
    return dict(P=P, state=P["state_true"], t=t, q=q, prefix_len=prefix_len, tau=tau, opt=opt)


def cases():
    global _CASES
    if _CASES is None:
        P, PL = tc.problem(), long_problem()
        rng = np.random.default_rng(5)
        c = {}
        for n in (3, 17, 65, 257):
            for on in (True, False):
                if on and n > 90:
                    continue   # the spline has 95 knot intervals
                t = stamps(P, n, on)
                c["n%d_%s" % (n, "on" if on else "off")] = case(P, t, odometry(P, t))
        t = stamps(P, 65, False)
        q = odometry(P, t)
        t2, q2 = with_tail(P, t)
        c["tail"] = case(P, t2, q2, [3, 20, 67, 68, 69, 70, 71])
        c["sign_scale"] = case(P, t, q * rng.choice([-1.0, 1.0], (65, 1)) * rng.uniform(0.5, 2.0, (65, 1)))
        c["huber"] = case(P, t, with_planted_step(q, 30, 3.0))
        c["huber_half"] = case(P, t, with_planted_step(q, 30, 3.0), opt=options(huber_deg=0.5))
        c["prefixes_short"] = case(P, t, q, [1, 2, 15, 16, 33, 65, 65])
        tl = PL["t0"] + np.arange(60) * 5 * PL["dt"]   # 10 Hz, on the knots
        c["prefixes"] = case(PL, tl, odometry(PL, tl), LONG_PREFIXES)
        c["shifts"] = case(PL, tl[1:42], odometry(PL, tl[1:42], late=SHIFT_TRUE), [20, 41], SHIFTS)
        _CASES = c
    return _CASES
