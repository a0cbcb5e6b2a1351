"""Shared by tests/test_traj_host.py and tests/test_gpu_traj.py: the problem every trajectory-query test uses, the query times of the validity cases, the oracle's
spline and sensor poses, a numpy float64 restatement of the pose-error pass written from include/lvx.h (it never calls the header), reference poses with planted errors,
and the g++ build of lvi-exc_amd/csrc/lvx_traj.h (tests/native/traj_host_check.cpp) behind ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import lvx
import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = O.LOCK_LIDAR_TAU | O.LOCK_CAM_TAU
# bars (absolute): position / quaternion are the project's own for poses (tests/test_gpu_upstream.py); velocity, acceleration, angular velocity and the predicted readings
# are the quantities inside the gyro / accel residual rows the GPU suite holds at 1e-11 after a weight of 18 - 28; pose errors and their summaries 1e-11 (m, rad)
BAR_P, BAR_Q, BAR_D, BAR_E = 1e-12, 1e-13, 1e-11, 1e-11
BARS = {"position": BAR_P, "orientation": BAR_Q, "velocity": BAR_D, "acceleration": BAR_D, "angular_velocity": BAR_D}
ORACLE_KEY = {"position": "pos", "orientation": "quat", "velocity": "vel", "acceleration": "acc", "angular_velocity": "angvel"}
_P = None
_LIB = None
_LIP = {}   # lipschitz() of a reference, computed once per state


def problem():
    """98 knots, valid range [99.8, 101.7), 600 IMU samples inside it.  Read-only."""
    global _P
    if _P is None:
        _P = synth.make_problem(seed=41, duration=1.5, n_surfel=0, n_planes=1, n_landmarks=0)
        assert _P["n_knots"] == 98 and len(_P["t_imu"]) == 600
    return _P


def make_oracle(P):
    o = O.Oracle()
    lvx.load_problem(o, P, TAU)
    o.P = P
    return o


def spline_oracle(P, n_knots):
    """The problem's spline cut to its first n_knots control points."""
    o = O.Oracle()
    o.set_spline(P["t0"], P["dt"], n_knots)
    o.P = P
    return o


def time_range(P, n_knots=None):
    N = P["n_knots"] if n_knots is None else n_knots
    return P["t0"], P["t0"] + (N - 3) * P["dt"]


def is_valid(P, tt, n_knots=None):
    tmin, tmax = time_range(P, n_knots)
    tt = np.asarray(tt, np.float64)
    with np.errstate(invalid="ignore"):
        return (tt >= tmin) & (tt < tmax)


INVALID_TAIL = 6


def query_times(P, n, seed, n_knots=None):
    """n times uniform in the valid range, NOT sorted; then t0, the last double below MaxTime and every knot t0 + k dt with its two neighbouring doubles; then the six
    invalid ones: MaxTime, MaxTime + 5e-6, t0 - 1e-9, NaN, +inf, -inf.  Returns (t, expected valid)."""
    N = P["n_knots"] if n_knots is None else n_knots
    tmin, tmax = time_range(P, N)
    rng = np.random.default_rng(seed)
    knots = P["t0"] + np.arange(N - 2) * P["dt"]
    t = np.concatenate([rng.uniform(tmin, tmax, n), [tmin, np.nextafter(tmax, -np.inf)], knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf),
                        [tmax, tmax + 5e-6, tmin - 1e-9, np.nan, np.inf, -np.inf]])
    ok = is_valid(P, t, N)
    assert not ok[-INVALID_TAIL:].any() and ok[:n + 2].all()
    return t, ok


def oracle_retries(P, tt):
    """True where the ORACLE does not evaluate at tt itself.  Oracle.eval_pose and the IMU rows of Oracle.evaluate build Kontiki's minimal view for the single-time span
    {tt, tt}: a four-knot segment starting at knot i1 = floor((tt - t0) / dt) that accepts [t0 + dt i1, t0 + dt i1 + dt) and otherwise retries at tt - 1e-5
    (spline_base.h:196-222, 387-401).  At a stamp within an ulp of a knot the two roundings can disagree (the quotient says interval i1, the sum says tt is past its end),
    and the oracle then returns the spline at tt - 1e-5: 1e-5 s of motion away.  A query has no span and no retry (lvx_traj.h), so there the oracle is no reference."""
    tt = np.asarray(tt, np.float64)
    i1 = np.floor((tt - P["t0"]) / P["dt"])
    t0_seg = P["t0"] + P["dt"] * i1
    return ~((tt >= t0_seg) & (tt < t0_seg + 1.0 * P["dt"]))


def oracle_times(P, tt, n_knots=None):
    """The stamps the oracle is asked at: tt itself, or — where oracle_retries(tt) — the nearest double that is still inside the range and that the oracle evaluates as
    given: one or two doubles above, else below (the last double below MaxTime has nothing above it), at most 2 ulp (2.9e-14 s at t = 100 s) away.  What that costs
    against the bars: |f'| * 2.9e-14 — 1e-13 m at 3 m/s, 3e-14 of a quaternion at 2 rad/s, 3e-12 m/s^2 at a jerk of 100 m/s^3: below a third of every bar, so the bars
    stay as they are."""
    tt = np.array(tt, np.float64)
    out = tt.copy()
    todo = oracle_retries(P, tt)
    for step in (1, 2, -1, -2):
        cand = tt.copy()
        for _ in range(abs(step)):
            cand = np.nextafter(cand, np.inf if step > 0 else -np.inf)
        take = todo & ~oracle_retries(P, cand) & is_valid(P, cand, n_knots)
        out[take] = cand[take]
        todo &= ~take
    assert not todo.any() and not oracle_retries(P, out).any() and is_valid(P, out, n_knots).all() and np.abs(out - tt).max() <= 2 * np.spacing(np.abs(tt).max())
    return out


def sensor_slots(state, n_knots, frame):
    """(q_S x y z w, p_S, tau_S) of the LiDAR (frame 1) or the camera (frame 2) in the state."""
    o = 7 * n_knots + (16 if frame == lvx.FRAME_LIDAR else 24)
    return state[o:o + 4], state[o + 4:o + 7], state[o + 7]


def oracle_spline(o, state):
    """t -> Oracle.eval_pose(state, t) under the field names of lvx.TRAJ_FIELDS; every stamp must be one the oracle evaluates as given."""
    def fn(t):
        assert not oracle_retries_any(o, t)
        e = o.eval_pose(state, t)
        return {f: e[k] for f, k in ORACLE_KEY.items()}
    fn.key = ("spline", np.asarray(state).tobytes())
    return fn


def oracle_retries_any(o, t):
    return bool(oracle_retries(o.P, t).any())


def oracle_sensor(o, P, state, frame):
    """t -> the sensor frame at the stamps t composed in numpy from Oracle.eval_pose at t + tau_S: pose, velocity of the sensor origin v + w x (R p_S), w."""
    qS, pS, tau = sensor_slots(state, P["n_knots"], frame)

    def fn(t):
        e = oracle_spline(o, state)(np.asarray(t) + tau)
        arm = synth.qrot(e["orientation"], np.broadcast_to(pS, e["position"].shape))
        return {"orientation": synth.qmul(e["orientation"], np.broadcast_to(qS, e["orientation"].shape)), "position": arm + e["position"],
                "velocity": e["velocity"] + np.cross(e["angular_velocity"], arm), "angular_velocity": e["angular_velocity"]}
    return fn


def oracle_imu(P, state):
    """t -> (gyro, acc) the oracle's IMU model predicts at the stamps t with the state's tau_imu: meas - r / w from the gyro and accel rows of Oracle.evaluate (rows: gyro
    [3 n], accel [3 n], ...; measurements zero).  The oracle's IMU offset is locked, so a row's span is the single time {t, t} and its four-knot segment rejects t + tau
    once that leaves the knot interval of t — Oracle.evaluate raises for tau_imu = +-0.3 dt, as Kontiki would.  A query has no span: the oracle gets the offset applied
    to the STAMPS (t + tau, tau_imu = 0 in the state it sees), which is the evaluation time the query forms."""
    N = P["n_knots"]
    tau = state[7 * N + 7]
    s0 = np.array(state, np.float64)
    s0[7 * N + 7] = 0.0

    def fn(t):
        tt = np.asarray(t, np.float64) + tau
        assert not oracle_retries(P, tt).any()
        Q = dict(P)
        Q["t_imu"], Q["gyro"], Q["acc"] = tt, np.zeros((len(tt), 3)), np.zeros((len(tt), 3))
        r = make_oracle(Q).evaluate(s0)["residuals"]
        n = len(tt)
        return {"gyro": -r[:3 * n].reshape(n, 3) / P["w_gyro"], "acc": -r[3 * n:6 * n].reshape(n, 3) / P["w_acc"]}
    return fn


def with_oracle_stamps(P, t, ok, n_knots=None):
    """The query list with, appended, the oracle's stamp (oracle_times) of every valid stamp at which the oracle answers for t - 1e-5 (oracle_retries).
    Returns (t_all, indices of those stamps, len(t))."""
    idx = np.flatnonzero(ok)
    to = oracle_times(P, t[idx], n_knots)
    moved = to != t[idx]
    return np.concatenate([t, to[moved]]), idx[moved], len(t)


def lipschitz(ref_fn, P, fields, n_knots=None, grid_ok=None):
    """A bound on |df/dt| of every field from the REFERENCE: twice the largest difference quotient over a 0.5 ms grid of the valid range (40 points per knot interval;
    the fastest-changing field, the acceleration, is piecewise linear in t, so the quotient is its slope except across a knot)."""
    key = (getattr(ref_fn, "key", None), tuple(fields), n_knots)
    if key[0] is not None and key in _LIP:
        return _LIP[key]
    tmin, tmax = time_range(P, n_knots)
    g = oracle_times(P, np.arange(tmin + 1e-4, tmax - 1e-4, 5e-4), n_knots)
    keep = np.ones(len(g), bool) if grid_ok is None else grid_ok(g)   # (stamps the reference cannot evaluate: the non-unit case)
    e = ref_fn(g[keep])
    pair = keep[1:] & keep[:-1]
    dg = np.diff(g)[pair]
    out = {}
    for f in fields:
        full = np.zeros((len(g),) + e[f].shape[1:])
        full[keep] = e[f]
        out[f] = 2.0 * float((np.abs(np.diff(full, axis=0))[pair].max(axis=1) / dg).max())
    if key[0] is not None:
        _LIP[key] = out
    return out


def check_fields(got, ref_fn, P, t_all, ok, retried, n0, bars, tag, n_knots=None, grid_ok=None):
    """got: the fields at t_all (with_oracle_stamps).  (1) Every valid stamp the oracle evaluates as given, the appended ones included: |got - oracle| <= bar.
    (2) A stamp at which the oracle answers for t - 1e-5 instead: the oracle offers no value f(t) there, so the sample is held against the sample at the appended stamp
    t' (itself under (1)), at most 2 ulp away.  |got(t) - f(t)| <= bar is what (1) asks of a sample; with it, |got(t) - got(t')| <= |got(t) - f(t)| + |f(t) - f(t')| +
    |f(t') - got(t')| <= 2 bar + L |t - t'|, L the reference's own bound on |df/dt| (lipschitz) — 1.4e-14 s of a jerk of 1.5e4 m/s^3 are 2e-10 m/s^2 that no float64
    evaluation can resolve.  That inequality is asserted.  Returns the maxima of (1)."""
    plain = np.array(ok[:n0], bool)
    plain[retried] = False
    sel = np.concatenate([plain, np.ones(len(t_all) - n0, bool)])
    ref = ref_fn(t_all[sel])
    worst = {}
    for f, bar in bars.items():
        worst[f] = float(np.abs(got[f][sel] - ref[f]).max())
        print("%s %s: max |got - oracle| = %.3e (bar %.1e)" % (tag, f, worst[f], bar))
    for f, bar in bars.items():
        assert worst[f] <= bar, (f, worst[f])
    if len(retried):
        L = lipschitz(ref_fn, P, list(bars), n_knots, grid_ok)
        gap = np.abs(t_all[n0:] - t_all[retried])
        assert gap.max() <= 2 * np.spacing(np.abs(t_all[retried]).max())
        for f, bar in bars.items():
            d = np.abs(got[f][retried] - got[f][n0:]).max(axis=1)
            assert (d <= 2.0 * bar + L[f] * gap).all(), (f, d.max(), L[f])
    return worst


def _summary(e, idx):
    if len(e) == 0:
        return {"rmse": 0.0, "mean": 0.0, "max": 0.0, "argmax": 0, "n": 0}
    return {"rmse": float(np.sqrt(np.mean(e * e))), "mean": float(np.mean(e)), "max": float(e.max()), "argmax": int(idx[int(np.argmax(e))]), "n": len(e)}


def _err(qa, pa, qb, pb):
    d = synth.qmul(synth.qconj(qa), qb)
    return np.linalg.norm(pa - pb, axis=-1), 2.0 * np.arctan2(np.linalg.norm(d[..., :3], axis=-1), np.abs(d[..., 3]))


def np_pose_errors(Tq, Tp, valid, qr, pr, align):
    """include/lvx.h, lvx_compare_poses, in numpy: trajectory poses (Tq x y z w, Tp), reference poses (normalised here), align 0 / 1."""
    Tq, Tp, qr, pr = (np.asarray(a, np.float64) for a in (Tq, Tp, qr, pr))
    n = len(Tq)
    qr = qr / np.linalg.norm(qr, axis=1, keepdims=True)
    idx = np.flatnonzero(valid)
    qa, pa = qr, pr
    if align == lvx.ALIGN_FIRST and len(idx):
        a = idx[0]
        qA = synth.qmul(Tq[a], synth.qconj(qr[a]))
        pA = Tp[a] - synth.qrot(qA, pr[a])
        qa, pa = synth.qmul(np.broadcast_to(qA, qr.shape), qr), synth.qrot(np.broadcast_to(qA, qr.shape), pr) + pA
    at, ar = np.zeros(n), np.zeros(n)
    if len(idx):
        at[idx], ar[idx] = _err(Tq[idx], Tp[idx], qa[idx], pa[idx])
    i, j = idx[:-1], idx[1:]
    if len(i):
        rel = lambda q, p: (synth.qmul(synth.qconj(q[i]), q[j]), synth.qrot(synth.qconj(q[i]), p[j] - p[i]))   # noqa: E731
        rt, rr = _err(*rel(Tq, Tp), *rel(qr, pr))
    else:
        rt, rr = np.zeros(0), np.zeros(0)
    return {"n": n, "n_valid": len(idx), "abs_trans_n": at, "abs_rot_n": ar, "abs_trans": _summary(at[idx], idx), "abs_rot": _summary(ar[idx], idx),
            "rel_trans": _summary(rt, i), "rel_rot": _summary(rr, i)}


def assert_errors_close(got, ref, bar=BAR_E):
    assert got["n"] == ref["n"] and got["n_valid"] == ref["n_valid"]
    worst = max(np.abs(got["abs_trans_n"] - ref["abs_trans_n"]).max(), np.abs(got["abs_rot_n"] - ref["abs_rot_n"]).max())
    for k in ("abs_trans", "abs_rot", "rel_trans", "rel_rot"):
        assert got[k]["n"] == ref[k]["n"] and got[k]["argmax"] == ref[k]["argmax"], (k, got[k], ref[k])
        worst = max([worst] + [abs(got[k][m] - ref[k][m]) for m in ("rmse", "mean", "max")])
    print("pose errors: max |device - numpy| = %.3e" % worst)
    assert worst <= bar, worst
    return worst


def planted_reference(rng, q, p, valid):
    """Reference poses = the given poses moved by planted errors: translations 1 mm .. 0.9 m in random directions with ONE of exactly 1 m, rotations 1 mrad .. 0.9 rad about
    random axes with ONE of exactly 1 rad (each at a valid index, not the same one when there is a choice), then every quaternion scaled by a norm in [0.5, 2]."""
    n = len(q)
    idx = np.flatnonzero(valid)
    mt, mr = 10.0 ** rng.uniform(-3, np.log10(0.9), n), 10.0 ** rng.uniform(-3, np.log10(0.9), n)
    it, ir = idx[len(idx) // 3], idx[(2 * len(idx)) // 3]
    mt[it], mr[ir] = 1.0, 1.0
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = rng.standard_normal((n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    qr = synth.qmul(q, synth.q_from_rotvec(ax * mr[:, None])) * rng.uniform(0.5, 2.0, (n, 1))
    return qr, p + d * mt[:, None], int(it), int(ir)


def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "traj_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "libtraj_host_check.so")
        deps = [src] + [os.path.join(ROOT, "lvi-exc_amd", "csrc", f) for f in ("lvx_math.h", "lvx_resid.h", "lvx_traj.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_sample(P, state, t, frame=0, n_knots=None):
    N = P["n_knots"] if n_knots is None else n_knots
    t = np.ascontiguousarray(t, np.float64)
    n = len(t)
    out = {f: np.zeros((n, 4 if f == "orientation" else 3)) for f in lvx.TRAJ_FIELDS}
    valid = np.zeros(n, np.int32)
    st = host_lib().th_sample(_p(np.ascontiguousarray(state, np.float64)), C.c_int(N), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(frame), C.c_int(n), _p(t), _p(out["position"]),
                              _p(out["velocity"]), _p(out["acceleration"]), _p(out["orientation"]), _p(out["angular_velocity"]), _p(valid))
    out["valid"] = valid.astype(bool)
    return out, st


def host_predict_imu(P, state, t):
    t = np.ascontiguousarray(t, np.float64)
    n = len(t)
    g, a, valid = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
    st = host_lib().th_predict_imu(_p(np.ascontiguousarray(state, np.float64)), C.c_int(P["n_knots"]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(n), _p(t), _p(g), _p(a), _p(valid))
    return g, a, valid.astype(bool), st


def host_pose_errors(Tq, Tp, valid, qr, pr, align):
    n = len(Tq)
    Tq, Tp, qr, pr = (np.ascontiguousarray(a, np.float64) for a in (Tq, Tp, qr, pr))
    v = np.ascontiguousarray(valid, np.int32)
    at, ar, out = np.zeros(n), np.zeros(n), np.zeros(21)
    host_lib().th_pose_errors(C.c_int(n), _p(Tq), _p(Tp), _p(v), _p(qr), _p(pr), C.c_int(align), _p(at), _p(ar), _p(out))
    r = {"n": n, "n_valid": int(out[0]), "abs_trans_n": at, "abs_rot_n": ar}
    for k, name in enumerate(("abs_trans", "abs_rot", "rel_trans", "rel_rot")):
        o = out[1 + 5 * k:6 + 5 * k]
        r[name] = {"rmse": o[0], "mean": o[1], "max": o[2], "argmax": int(o[3]), "n": int(o[4])}
    return r


NONUNIT_KNOT, NONUNIT_SCALE = 40, 1.001


def nonunit_window(P, tt):
    """The evaluation times whose four-knot window [i0, i0 + 3] holds control point NONUNIT_KNOT: i0 in [k - 3, k]."""
    with np.errstate(invalid="ignore"):
        return (tt >= P["t0"] + (NONUNIT_KNOT - 3) * P["dt"]) & (tt < P["t0"] + (NONUNIT_KNOT + 1) * P["dt"])


def nonunit_case(P, state, n=257, seed=13):
    """SO3 control point NONUNIT_KNOT scaled by 1.001 and the query times of query_times without the stamps within 1e-9 of the window's two ends (which side those fall
    on is the knot lookup's rounding, not this case).  Returns (state, t, expected-in-range, in the window)."""
    N = P["n_knots"]
    s = np.array(state, np.float64)
    s[3 * N + 4 * NONUNIT_KNOT:3 * N + 4 * NONUNIT_KNOT + 4] *= NONUNIT_SCALE
    t, ok = query_times(P, n, seed)
    lo, hi = P["t0"] + (NONUNIT_KNOT - 3) * P["dt"], P["t0"] + (NONUNIT_KNOT + 1) * P["dt"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(t - lo) < 1e-9) | (np.abs(t - hi) < 1e-9)
    t, ok = t[~near], ok[~near]
    return s, t, ok, ok & nonunit_window(P, t)


def imu_bars(P):
    return {"gyro": BAR_D / P["w_gyro"], "acc": BAR_D / P["w_acc"]}


def sensor_times(P):
    """300 stamps inside, 20 within 3e-4 of each end, 10 up to 3e-4 before t0."""
    tmin, tmax = time_range(P)
    rng = np.random.default_rng(21)
    return np.concatenate([rng.uniform(tmin + 1e-3, tmax - 1e-3, 300), tmin + rng.uniform(0, 3e-4, 20), tmax - rng.uniform(0, 3e-4, 20), tmin - rng.uniform(1e-6, 3e-4, 10)])


def with_sensor_tau(P, state, frame, tau):
    s = np.array(state, np.float64)
    if tau is not None:
        s[7 * P["n_knots"] + (23 if frame == lvx.FRAME_LIDAR else 31)] = tau
    return s


def assert_sensor_tau_moves_the_ends(ok, tau):
    if tau == 3e-4:
        assert not ok[320:340].all() and ok[340:].any()
    if tau == -3e-4:
        assert not ok[300:320].all() and not ok[340:].any()
