"""Visual tracks placed by hand, for everything behind k_reproj_jac: the cross-term groups of k_reproj_cross (csrc/lvx_eval.hip), the landmark rows of k_reproj_lmrows and the
landmark elimination k_lm_schur_grp / k_lm_schur / k_lm_back (csrc/lvx_solver.hip).  synth.make_problem() only draws 25-30 landmarks of consecutive views whose reference view is
the first one; here every track is DATA: the reference frame time, the reference pixel, a depth and a list of views.

build(name) -> (P, locks, expect): P the dict lvx.load_problem takes (P["state0"] / P["state_true"] carry the inverse depths; for the stray cases the camera time offset is set in both),
`locks` the lock mask the case is meant for, `expect` what the tests assert about the construction.
track_regime(P, locks) restates the host's layout rules (ensure_layout in csrc/lvx_eval.hip, solve_local in csrc/lvx_solver.hip) in numpy; it is used for nothing but asserting that a
case reaches the regime it is named for, and for the plan numbers lvx_layout reports (rep_groups, lm_groups, lm_group_spread, lm_row_width).

Geometry of every case: dt = 0.02 s, the spline starts at t0 = 99.8 s, knot interval k is [t0 + k dt, t0 + (k + 1) dt), a window is four aligned intervals (w = k >> 2).  The camera reads
720 rows in 66.6 ms, so a view of frame time t and row v is evaluated at t + v * 92.5 us: 216 rows per interval.  A view is placed either "at" an evaluation time te (the landmark is
projected through the true camera pose at te, the frame time is te - v * readout / rows: the rolling-shutter fixed point by construction) or in a "frame" of given time (fixed-point
iteration on the row time, as synth.make_problem does); 0.5 px noise from a seed derived from the case name.  The map time 100.05 s lies in interval 12: hub knots 12..16."""
import functools

import numpy as np

import lvx
import synth

DT = 0.02
TAU = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
FREE_CAM_TAU = lvx.LOCK_LIDAR_TAU
LOCKS_CAM_DEAD = TAU | lvx.LOCK_CAM_Q | lvx.LOCK_CAM_P
LOCKS_TRAJ = TAU | lvx.LOCK_TRAJ | lvx.LOCK_LIDAR_Q | lvx.LOCK_LIDAR_P
LOCKS_R3 = TAU | lvx.LOCK_R3
SENSOR_MTO = 1e-3            # the library's default bound of a free sensor time offset (lvx_set_time_offset_bounds)
MARGIN = 1e-3                # the reprojection block's span margin (static_rscamera_measurement.h)
GROUP_CAP, FUSED_CAP = 32, 64
ELIM_CAP, ELIM_REACH = 32, 24
LDS_LIMIT = 160 * 1024

GROUP_SIZES = (1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 65)
FUSED_SIZES = (63, 64)                       # with 65: the 64-lane groups of k_reproj_fused
L_SIZES = (1, 3, 4, 5, 33)
FRAME_SIZES = (1, 31, 32, 33, 64, 65)
STRAYS = ("alone", "two_in_trip", "ref_side", "obs_side")

CROSS_CASES = (["grp_%d" % n for n in GROUP_SIZES] + ["same_interval", "ref_as_block", "twice_in_frame", "adjacent_windows", "panel_offsets", "first_last_interval",
                                                      "ref_last", "ref_middle", "mirrored_pairs"] +
               ["stray_%s_%s" % (s, m) for s in STRAYS for m in ("locked", "free")])
FUSED_CASES = ["grp_%d" % n for n in FUSED_SIZES]
ROW_CASES = (["lm_counts"] + ["L_%d" % n for n in L_SIZES] + ["hub_coupled", "hub_coupled_nosurf", "locks_cam_dead", "locks_tau_free", "locks_traj", "locks_r3"])
ELIM_CASES = (["frame_%d" % n for n in FRAME_SIZES] + ["frames_shifted", "frames_shifted_r3", "nn_30", "nn_48", "nn_49", "nn_traj", "nn_traj_tau", "frame_65x10", "ref_only_frame",
                                                       "reach_ends", "long_track"])
NAMES = CROSS_CASES + FUSED_CASES + ROW_CASES + ELIM_CASES
GROUP_SIZE_CASES = ["grp_%d" % n for n in GROUP_SIZES + FUSED_SIZES]
DETERMINISTIC_CASES = ["grp_33", "mirrored_pairs", "frame_65"]
STEP_CASES = ROW_CASES + ELIM_CASES
STEP_SWEEP_CASES = ["lm_counts", "frames_shifted", "frame_65"]     # radius x scaling
LOOP_CASES = ["ref_last", "frame_65", "hub_coupled", "long_track"]
ORACLE_CASES = ["ref_last", "ref_middle", "same_interval", "twice_in_frame"]   # ground the oracle never walked before: finite differences decide
# cases whose damped system at radius 1e4 the float64 reference itself does not solve to 1e-8 (tests/test_landmark_cases.py: test_step_reference_carries_its_bar holds this table to
# the measurement): they are compared at radius 3.0 only
STEP_SMALL_RADIUS_ONLY = ("nn_30",)       # measured 1.3e-8: one landmark whose two poses share their four knots leaves the depth and the camera nearly unobservable


def hash_name(name):
    """A seed from the case name that does not depend on PYTHONHASHSEED."""
    h = 0
    for c in name.encode():
        h = (h * 131 + c) % (1 << 31)
    return h


# ------------------------------------------------------------------------------------------------------------------
# builder
# ------------------------------------------------------------------------------------------------------------------
def _base(seed, duration=2.0, n_surfel=300, imu=True):
    P = synth.make_problem(seed, duration=duration, dt=DT, imu_rate=100.0, n_surfel=n_surfel, n_planes=8, n_landmarks=0)
    if not imu:
        for k in ("t_imu", "gyro", "acc"):
            P[k] = P[k][:0]
    return P


def row_delta(P):
    return P["camera"]["readout"] / P["camera"]["rows"]


def t_of(P, k, frac=0.5):
    """A time inside knot interval k."""
    return P["t0"] + (k + frac) * P["dt"]


def max_time(P):
    return P["t0"] + (P["n_knots"] - 3) * P["dt"]


def lm_at(P, te_ref, views, v=360.0, u=640.0, z=6.0):
    """A landmark whose reference view is EVALUATED at te_ref (row v, so the reference frame time is te_ref - v * row_delta)."""
    return dict(t_ref=te_ref - v * row_delta(P), uv=(u, v), z=z, views=list(views))


def lm_frame(t_ref, views, v=360.0, u=640.0, z=6.0):
    """A landmark whose reference FRAME time is t_ref."""
    return dict(t_ref=t_ref, uv=(u, v), z=z, views=list(views))


def frame_of_knot(P, k):
    """A frame time whose padded span starts in knot interval k (locked camera time offset): floor((t - 1 ms - t0) / dt) = k."""
    return P["t0"] + (k + 0.3) * P["dt"] + MARGIN


class _Projector:
    """The true camera of P: projects a track's views (rolling-shutter fixed point on the row time)."""

    def __init__(self, P):
        N = P["n_knots"]
        u0 = synth.unpack_state(P["state_true"], N, 0)
        self.sp = synth.Spline(P["t0"], P["dt"], u0["r3"], u0["so3"])
        self.q_CI, self.p_CI = u0["cam"][:4], u0["cam"][4:7]
        self.cam, self.rd = P["camera"], row_delta(P)
        self.lo, self.hi = P["t0"] + MARGIN + SENSOR_MTO, max_time(P) - self.cam["readout"] - MARGIN - SENSOR_MTO   # frame times every lock mask accepts

    def cam_pose(self, t):
        e = self.sp.eval(np.asarray(t, dtype=np.float64))
        return synth.qmul(e["quat"], np.broadcast_to(self.q_CI, e["quat"].shape)), synth.qrot(e["quat"], np.broadcast_to(self.p_CI, e["pos"].shape)) + e["pos"]

    def project(self, Pw, te):
        """Pixels of the points Pw seen at the times te, and which of them lie in front of the camera."""
        te = np.clip(te, self.sp.t_min, self.sp.t_max - 1e-9)   # (a diverging fixed point is rejected by its row, not by the spline)
        qo, po = self.cam_pose(te)
        Xc = synth.qrot(synth.qconj(qo), Pw - po)
        ok = Xc[:, 2] > 0.2
        return synth._project(self.cam, np.where(ok[:, None], Xc, np.array([0.0, 0.0, 1.0]))), ok

    def views(self, tracks, rng=None, noise_px=0.5):
        """Per track [(uv, frame time)] of its views, or None when one of them is not a view a camera can have: behind it, a row outside the sensor (the row decides the time
        inside the frame's read-out), a frame outside the spline.  All tracks at once (the spline is evaluated on arrays).  rng = None: no pixel noise (the generators' test)."""
        n = len(tracks)
        uv = np.array([tr["uv"] for tr in tracks], dtype=np.float64).reshape(n, 2)
        t_ref = np.array([tr["t_ref"] for tr in tracks], dtype=np.float64)
        z = np.array([tr["z"] for tr in tracks], dtype=np.float64)
        good = (t_ref > self.lo) & (t_ref < self.hi)
        qc, pc = self.cam_pose(np.clip(t_ref + uv[:, 1] * self.rd, self.sp.t_min, self.sp.t_max - 1e-9))
        Pw = synth.qrot(qc, synth._unproject(self.cam, uv) * z[:, None]) + pc
        flat = [(l, j, v) for l, tr in enumerate(tracks) for j, v in enumerate(tr["views"])]
        nv = len(flat)
        o, t, ok = np.zeros((nv, 2)), np.zeros(nv), np.ones(nv, dtype=bool)
        lm = np.array([f[0] for f in flat], dtype=np.int64)
        kind = np.array([f[2][0] for f in flat]) if nv else np.zeros(0, dtype="<U5")
        noise = noise_px * rng.standard_normal((nv, 2)) if rng is not None else np.zeros((nv, 2))
        for i in np.flatnonzero(kind == "ref"):
            o[i], t[i] = uv[lm[i]], t_ref[lm[i]]
        at = np.flatnonzero(kind == "at")
        if len(at):
            te = np.array([flat[i][2][1] for i in at], dtype=np.float64)
            px, ok[at] = self.project(Pw[lm[at]], te)
            o[at] = px + noise[at]
            t[at] = te - o[at, 1] * self.rd     # the noisy row decides the frame time: the view is evaluated at te exactly
        fr = np.flatnonzero(kind == "frame")
        if len(fr):
            t[fr] = np.array([flat[i][2][1] for i in fr], dtype=np.float64)
            vv = np.full(len(fr), self.cam["cy"])
            for _ in range(6):                   # rolling-shutter fixed point on the row time
                px, okf = self.project(Pw[lm[fr]], t[fr] + np.clip(vv, -50.0, self.cam["rows"] + 50.0) * self.rd)
                vv = px[:, 1]
            ok[fr] = okf
            o[fr] = px + noise[fr]
        for i in np.flatnonzero(kind == "dup"):  # (the view before it is resolved by now: a duplicate follows a view of another kind, or a duplicate handled earlier in this loop)
            o[i], t[i], ok[i] = o[i - 1] + np.array(flat[i][2][1:3], dtype=np.float64), t[i - 1], ok[i - 1]
        for i in np.flatnonzero(kind == "row"):
            o[i], t[i], ok[i] = np.array([o[i - 1][0], flat[i][2][1]]), t[i - 1], ok[i - 1]
        ok &= (t > self.lo) & (t < self.hi) & (o[:, 1] >= 4.0) & (o[:, 1] <= self.cam["rows"] - 4.0)
        np.logical_and.at(good, lm, ok)
        out = [[] if good[l] else None for l in range(n)]
        for i in range(nv):
            if good[lm[i]]:
                out[lm[i]].append((o[i], t[i]))
        return out


def attach_tracks(P, tracks, seed, shuffle=True):
    """Project every track through the true trajectory of P and return the problem dict with the visual arrays and the inverse depths filled in.
    A view is ("ref",): the reference observation itself as a block; ("at", te): evaluated at te; ("frame", t): in the frame of time t; ("dup", du, dv): a second observation
    in the frame of the view before it, (du, dv) pixels away; ("row", v): a second observation in that frame in row v (wherever the landmark projects: an outlier under the Huber loss)."""
    rng = np.random.default_rng(seed)
    N = P["n_knots"]
    L = len(tracks)
    vs = _Projector(P).views(tracks, rng)
    lm_uv, lm_t0, rho = np.zeros((L, 2)), np.zeros(L), np.zeros(L)
    rep_lm, rep_uv, rep_t0 = [], [], []
    for l, tr in enumerate(tracks):
        assert vs[l] is not None, "landmark %d has a view no camera can have" % l
        lm_uv[l], lm_t0[l], rho[l] = tr["uv"], tr["t_ref"], 1.0 / tr["z"]
        for o, t in vs[l]:
            rep_lm.append(l); rep_uv.append(o); rep_t0.append(t)
    rep_lm = np.array(rep_lm, dtype=np.int32).reshape(-1); rep_uv = np.array(rep_uv, dtype=np.float64).reshape(-1, 2); rep_t0 = np.array(rep_t0, dtype=np.float64).reshape(-1)
    if shuffle and len(rep_lm) > 1:
        p = rng.permutation(len(rep_lm))
        rep_lm, rep_uv, rep_t0 = rep_lm[p], rep_uv[p], rep_t0[p]
    Q = dict(P)
    Q.update(n_landmarks=L, lm_uv=lm_uv, lm_t0=lm_t0, rep_lm=rep_lm, rep_uv=rep_uv, rep_t0=rep_t0)
    Q["state_true"] = np.concatenate([P["state_true"][:7 * N + 32], rho])
    Q["state0"] = np.concatenate([P["state0"][:7 * N + 32], rho * (1.0 + 0.05 * rng.standard_normal(L))])
    return Q


def tau_cam_slot(P):
    return 7 * P["n_knots"] + 31


def _draw(P, n, make):
    """n tracks from the generator make(): candidates with a view no camera can have (the row a few pixels inside the sensor, 0.5 px noise to come) are drawn again."""
    pj = _Projector(P)
    out = []
    for _ in range(40):
        cand = [make() for _ in range(2 * n + 8)]
        out += [tr for tr, v in zip(cand, pj.views(cand)) if v is not None]
        if len(out) >= n:
            return out[:n]
    raise AssertionError("no visible tracks")


def _pair_tracks(P, rng, n, w0, w1):
    """n landmarks of one view each: reference view in window w0, the view in window w1."""
    def make():
        te0 = P["t0"] + (4 * w0 + rng.uniform(0.1, 3.9)) * DT
        te1 = P["t0"] + (4 * w1 + rng.uniform(0.1, 3.9)) * DT
        return lm_at(P, te0, [("at", te1)], v=rng.uniform(100, 620), u=rng.uniform(200, 1080), z=rng.uniform(3.0, 12.0))
    return _draw(P, n, make)


def _ordinary(P, rng, n, k_lo=24, k_hi=100, views=3, step=0.05):
    """n landmarks of `views` consecutive frames `step` apart, the reference view first."""
    def make():
        t = frame_of_knot(P, int(rng.integers(k_lo, k_hi - int(views * step / DT) - 4)))
        return lm_frame(t, [("ref",)] + [("frame", t + step * j) for j in range(1, views)], v=rng.uniform(100, 620), u=rng.uniform(200, 1080), z=rng.uniform(3.0, 12.0))
    return _draw(P, n, make)


def _frame_landmarks(P, rng, n, k, views=3, step=0.05, with_ref=True):
    """n landmarks on ONE reference frame (padded span from knot k): the same first band position and the same co-visible frames."""
    t = frame_of_knot(P, k)

    def make():
        return lm_frame(t, ([("ref",)] if with_ref else []) + [("frame", t + step * j) for j in range(1, views)], v=rng.uniform(60, 660), u=rng.uniform(150, 1130), z=rng.uniform(3.0, 12.0))
    return _draw(P, n, make)


@functools.lru_cache(maxsize=None)
def build(name):
    """(P, locks, expect) of a case; memoised: the arrays are shared between the tests of a session and must not be written to."""
    seed = hash_name(name)
    rng = np.random.default_rng(seed)
    locks = TAU
    expect = {"tau": 0.0}
    P = _base(301)
    if name.startswith("grp_"):
        n = int(name[4:])
        tracks = _pair_tracks(P, rng, n, 8, 11)
        expect.update(pair=(8, 11), n=n)
    elif name == "same_interval":
        # a) reference and view in the same interval (both poses on the same four knots), b) same window, different intervals, c) two more in the interval of a): the
        # group (9, 9) adds J_ref^T J_obs where the same variable sits in both local spaces
        tracks = [lm_at(P, t_of(P, 37, 0.25), [("at", t_of(P, 37, 0.75))], v=200.0),
                  lm_at(P, t_of(P, 36, 0.4), [("at", t_of(P, 39, 0.6))], v=500.0, u=400.0),
                  lm_at(P, t_of(P, 37, 0.6), [("at", t_of(P, 37, 0.1)), ("at", t_of(P, 38, 0.5))], v=300.0, u=900.0, z=4.0)]
        expect.update(window=9, interval=37)
    elif name == "ref_as_block":
        tracks = [lm_at(P, t_of(P, 41, 0.3), [("ref",), ("at", t_of(P, 44, 0.5)), ("at", t_of(P, 47, 0.5))], v=250.0),
                  lm_at(P, t_of(P, 50, 0.3), [("at", t_of(P, 53, 0.5)), ("ref",)], v=450.0, u=300.0)]
    elif name == "twice_in_frame":
        tracks = [lm_at(P, t_of(P, 41, 0.3), [("ref",), ("at", t_of(P, 45, 0.5)), ("dup", 3.0, -2.0), ("at", t_of(P, 49, 0.5))], v=250.0),
                  lm_at(P, t_of(P, 60, 0.3), [("at", t_of(P, 62, 0.5)), ("dup", -4.0, 5.0), ("dup", 2.0, 2.0)], v=450.0, u=300.0)]
    elif name == "adjacent_windows":
        # w1 = w0 + 1: the two 7-knot spaces share knots 4 w0 + 4 .. 4 w0 + 6
        tracks = [lm_at(P, t_of(P, 40 + a, 0.5), [("at", t_of(P, 44 + b, 0.5))], v=150.0 + 60 * a + 20 * b, u=300.0 + 100 * b) for a in range(4) for b in range(4)]
        expect.update(pair=(10, 11))
    elif name == "panel_offsets":
        # views in intervals 4 w and 4 w + 3 on either side: panel offsets 0 and 3
        tracks = [lm_at(P, t_of(P, 32 + a, 0.5), [("at", t_of(P, 44 + b, 0.5))], v=200.0 + 100 * (a > 0), u=400.0 + 200 * (b > 0)) for a in (0, 3) for b in (0, 3)]
        expect.update(pair=(8, 11))
    elif name == "first_last_interval":
        last = P["n_knots"] - 4
        tm = max_time(P)
        one = lambda te, views, v_lo, v_hi: _draw(P, 1, lambda: lm_at(P, te, views, v=rng.uniform(v_lo, v_hi), u=rng.uniform(200, 1080), z=rng.uniform(3.0, 12.0)))[0]   # noqa: E731
        tracks = [one(P["t0"] + 0.012, [("at", t_of(P, 3, 0.5)), ("at", t_of(P, 6, 0.5))], 10.0, 100.0),                  # reference view in interval 0 (a row near the top: the frame starts inside the spline)
                  one(t_of(P, 1, 0.5), [("at", P["t0"] + 0.012), ("at", t_of(P, 5, 0.5))], 10.0, 120.0),                  # a view in interval 0
                  one(tm - 0.006, [("at", t_of(P, last - 4, 0.5)), ("at", t_of(P, last - 8, 0.5))], 680.0, 712.0),        # reference view in the last interval (a row near the bottom: the frame's read-out ends inside the spline)
                  one(t_of(P, last - 1, 0.5), [("at", tm - 0.012), ("at", t_of(P, last - 6, 0.5))], 600.0, 712.0)]        # a view in the last interval
        expect.update(last=last)
    elif name == "ref_last":
        tracks = [_draw(P, 1, lambda: lm_at(P, t_of(P, 70 + 2 * j, 0.4), [("at", t_of(P, 70 + 2 * j - 3 * (i + 1), 0.3 + 0.1 * i)) for i in range(5)] + [("ref",)], v=rng.uniform(100, 620),
                                            u=rng.uniform(200, 1080), z=rng.uniform(3.0, 12.0)))[0] for j in range(6)]
    elif name == "ref_middle":
        tracks = [_draw(P, 1, lambda: lm_at(P, t_of(P, 60 + 2 * j, 0.4), [("at", t_of(P, 60 + 2 * j + 3 * i, 0.3 + 0.05 * (i + 3))) for i in (-3, -2, -1, 1, 2, 3)] + [("ref",)],
                                            v=rng.uniform(100, 620), u=rng.uniform(200, 1080), z=rng.uniform(3.0, 12.0)))[0] for j in range(6)]
    elif name == "mirrored_pairs":
        # (3, 5) and (5, 3) from two landmarks (window 3 holds the hub knots), and (7, 9) / (9, 7) on intervals 31 and 36: their common entries (knots 33, 34 x 36) also
        # take the IMU's blocks, so the ORDER of the two groups' additions shows in the bits
        tracks = [lm_at(P, t_of(P, 13, 0.5), [("at", t_of(P, 21, 0.5)), ("at", t_of(P, 22, 0.3))], v=200.0),
                  lm_at(P, t_of(P, 22, 0.6), [("at", t_of(P, 14, 0.5)), ("at", t_of(P, 12, 0.7))], v=400.0, u=400.0),
                  lm_at(P, t_of(P, 31, 0.5), [("at", t_of(P, 36, 0.5)), ("at", t_of(P, 37, 0.3))], v=300.0, u=800.0),
                  lm_at(P, t_of(P, 36, 0.6), [("at", t_of(P, 31, 0.2)), ("at", t_of(P, 30, 0.7))], v=500.0, u=500.0)]
        expect.update(mirrored=[((3, 5), (5, 3)), ((7, 9), (9, 7))])
    elif name.startswith("stray_"):
        kind, mode = name[6:].rsplit("_", 1)
        locks = TAU if mode == "locked" else FREE_CAM_TAU
        expect["tau"] = 5e-4                                  # moves a view 0.2 ms inside the upper edge of its window into the next window
        edge = lambda w: P["t0"] + (4 * w + 4) * DT - 2e-4    # noqa: E731
        if kind == "alone":
            tracks = [lm_at(P, t_of(P, 33, 0.5), [("at", edge(11))], v=300.0)]
            expect.update(strays=1)
        elif kind == "two_in_trip":
            tracks = _pair_tracks(P, rng, 6, 8, 11) + [lm_at(P, t_of(P, 33, 0.5), [("at", edge(11))], v=300.0), lm_at(P, t_of(P, 34, 0.5), [("at", edge(11))], v=500.0, u=900.0)]
            expect.update(strays=2)
        elif kind == "ref_side":
            tracks = _pair_tracks(P, rng, 3, 8, 11) + [lm_at(P, edge(8), [("at", t_of(P, 45, 0.5)), ("at", t_of(P, 46, 0.5))], v=300.0)]
            expect.update(strays=2)                           # both blocks of the landmark
        elif kind == "obs_side":
            tracks = _pair_tracks(P, rng, 3, 8, 11) + [lm_at(P, t_of(P, 33, 0.5), [("at", edge(11)), ("at", t_of(P, 45, 0.5))], v=300.0)]
            expect.update(strays=1)
        else:
            raise KeyError(name)
    elif name == "lm_counts":
        # blocks per landmark 0 (first id, a middle id, the last id), 1 (the reference view only), 2, 3, 4, 5, 8, 9, 40: the 40-view one sets the row width, the others' rows are mostly zeros
        cnt = [0, 1, 2, 3, 4, 0, 5, 8, 9, 40, 0]
        tracks = []
        for l, c in enumerate(cnt):
            k = 30 + 4 * l
            if c == 0:
                views = []
            elif c == 1:
                views = [("ref",)]
            elif c == 40:
                views = [("at", t_of(P, 40 + 0.5 * i, 0.25)) for i in range(40)]
            else:
                views = [("ref",)] + [("at", t_of(P, k + 2 * i, 0.4)) for i in range(1, c)]
            tracks.append(lm_at(P, t_of(P, 50 if c == 40 else k, 0.5), views, v=120.0 + 45 * l, u=250.0 + 70 * l, z=4.0 + 0.5 * l))
        expect.update(counts=cnt)
    elif name.startswith("L_"):
        n = int(name[2:])
        tracks = _ordinary(P, rng, n)
        expect.update(L=n)
    elif name in ("hub_coupled", "hub_coupled_nosurf"):
        # landmark 0: reference view on knots 11..14 (12..14 are hub knots), views on knots 8..11 and 16..19: border slots and band couplings on both sides of the hub gap
        if name.endswith("nosurf"):
            P = _base(301, n_surfel=0)                        # no hub: the border is the 22 calibration scalars only
        tracks = [lm_at(P, t_of(P, 11, 0.5), [("ref",), ("at", t_of(P, 8, 0.5)), ("at", t_of(P, 16, 0.5)), ("at", t_of(P, 20, 0.5))], v=300.0)] + _ordinary(P, rng, 7, k_lo=6, k_hi=60)
    elif name.startswith("locks_"):
        locks = {"locks_cam_dead": LOCKS_CAM_DEAD, "locks_tau_free": FREE_CAM_TAU, "locks_traj": LOCKS_TRAJ, "locks_r3": LOCKS_R3}[name]
        if name == "locks_r3":
            P = _base(301, imu=False)                         # LOCK_R3 has no accelerometer rows on the device; the oracle drops them only for the SO3-only estimator, which has no camera positions: no IMU family
        tracks = [lm_at(P, t_of(P, 11, 0.5), [("ref",), ("at", t_of(P, 8, 0.5)), ("at", t_of(P, 16, 0.5))], v=300.0)] + _ordinary(P, rng, 8, k_lo=6, k_hi=90, views=4)
    elif name.startswith("frame_") and name[6:].isdigit():
        n = int(name[6:])
        tracks = _frame_landmarks(P, rng, n, 40) + _ordinary(P, rng, 3, k_lo=60)
        expect.update(on_frame=n)
    elif name in ("frames_shifted", "frames_shifted_r3"):
        # reference frames whose first band positions differ by 6, 24 (one group, rows shifted inside it) and 30 (a new group); under LOCK_R3 a knot is 3 scalars: 24 is eight knots
        r3 = name.endswith("_r3")
        if r3:
            P = _base(301, imu=False)
            locks = LOCKS_R3
        ks = [40, 42, 48, 50] if r3 else [40, 41, 44, 45]
        tracks = []
        for k in ks:
            tracks += _frame_landmarks(P, rng, 2, k)
        expect.update(frame_knots=ks, groups=[6, 2], spread=24)
    elif name == "nn_30":
        tracks = [lm_at(P, t_of(P, 37, 0.25), [("at", t_of(P, 37, 0.75))], v=200.0)]      # both poses on knots 37..40: 24 knot columns + 6 camera
        expect.update(nn=[30])
    elif name in ("nn_48", "nn_49"):
        if name == "nn_49":
            locks = FREE_CAM_TAU
        tracks = [lm_at(P, t_of(P, 37, 0.5), [("at", t_of(P, 40, 0.5))], v=200.0)]        # knots 37..43: 42 columns + 6 camera (+ the time offset: one column in a fourth tile)
        expect.update(nn=[48 if name == "nn_48" else 49])
    elif name in ("nn_traj", "nn_traj_tau"):
        locks = LOCKS_TRAJ if name == "nn_traj" else (LOCKS_TRAJ & ~lvx.LOCK_CAM_TAU)
        tracks = _frame_landmarks(P, rng, 3, 40, with_ref=False)
        expect.update(nn=[6 if name == "nn_traj" else 7])
    elif name == "frame_65x10":
        tracks = _frame_landmarks(P, rng, 65, 30, views=10, step=0.07)
        expect.update(on_frame=65)
    elif name == "ref_only_frame":
        t = frame_of_knot(P, 50)
        tracks = [lm_frame(t, [("ref",)], v=100.0 + 200 * j, u=300.0 + 300 * j) for j in range(3)] + _ordinary(P, rng, 4, k_lo=30, k_hi=90)
        expect.update(ref_only=[0, 1, 2])
    elif name == "reach_ends":
        # the widest landmark's row is non-zero at BOTH ends of its padded span, so the elimination writes an entry at distance exactly `bandwidth`: the reference view in the
        # top rows of the first frame (its four knots start where the span starts), and in the last frame a second observation in the bottom rows (its knots end where the span ends)
        # No IMU: the knots at the two ends are held by a few surfel points and this landmark, so the far-corner entry weighs in the step.
        P = _base(301, imu=False)
        t1 = P["t0"] + (40 + 0.02) * DT + MARGIN
        t2 = P["t0"] + (70 + 0.9) * DT - 715.0 * row_delta(P)
        tracks = [lm_frame(t1, [("ref",), ("frame", t1 + 0.2), ("frame", t2), ("row", 715.0)], v=12.0, u=640.0, z=8.0)] + _ordinary(P, rng, 3, k_lo=44, k_hi=66)
    elif name == "long_track":
        # one landmark seen in 41 frames over more than 105 knots (reference view in the middle) next to 20 ordinary ones: the group panel of k_lm_schur_grp does not fit 160 KB
        P = _base(302, duration=3.2)
        te = [t_of(P, 22 + 2.7 * i, 0.3) for i in range(41)]
        tracks = [lm_at(P, te[20], [("at", t) for i, t in enumerate(te) if i != 20] + [("ref",)], v=360.0, u=640.0, z=9.0)] + _ordinary(P, rng, 20, k_lo=20, k_hi=140)
    else:
        raise KeyError(name)
    Q = attach_tracks(P, tracks, seed)
    if expect["tau"] != 0.0:
        for k in ("state0", "state_true"):
            Q[k] = Q[k].copy(); Q[k][tau_cam_slot(Q)] = expect["tau"]
    return Q, locks, expect


# ------------------------------------------------------------------------------------------------------------------
# the host's layout rules, restated
# ------------------------------------------------------------------------------------------------------------------
def _locked(g, N, locks):
    if g < 6 * N:
        return bool(locks & lvx.LOCK_TRAJ) or ((g % 6) < 3 and bool(locks & lvx.LOCK_R3))
    c = g - 6 * N
    bit = (None if c < 2 else lvx.LOCK_ACC_BIAS if c < 5 else lvx.LOCK_GYRO_BIAS if c < 8 else lvx.LOCK_LIDAR_Q if c < 11 else lvx.LOCK_LIDAR_P if c < 14 else lvx.LOCK_LIDAR_TAU if c < 15
           else lvx.LOCK_CAM_Q if c < 18 else lvx.LOCK_CAM_P if c < 21 else lvx.LOCK_CAM_TAU if c < 22 else lvx.LOCK_LANDMARKS)
    return False if bit is None else bool(locks & bit)


def interval(P, t):
    return np.floor((np.asarray(t, dtype=np.float64) - P["t0"]) / P["dt"]).astype(np.int64)


def track_regime(P, locks, tau=0.0):
    """What ensure_layout decides for the visual part of P under `locks` (numpy restatement; see the module docstring).  `tau`: the camera time offset of the state, for the
    intervals the EVALUATION finds (k0_eval / k1_eval: strays are the blocks they move out of their group's windows); the layout itself always works at tau = 0."""
    N, L = P["n_knots"], P["n_landmarks"]
    rd = row_delta(P)
    lm, uv, t_obs = np.asarray(P["rep_lm"], dtype=np.int64), np.asarray(P["rep_uv"]), np.asarray(P["rep_t0"])
    n = len(lm)
    R = {}
    k1 = interval(P, t_obs + uv[:, 1] * rd)
    k0 = interval(P, P["lm_t0"][lm] + P["lm_uv"][lm, 1] * rd)
    R["k0"], R["k1"] = k0, k1
    R["k0_eval"] = interval(P, P["lm_t0"][lm] + P["lm_uv"][lm, 1] * rd + tau)
    R["k1_eval"] = interval(P, t_obs + uv[:, 1] * rd + tau)
    w0, w1 = k0 >> 2, k1 >> 2
    order = np.lexsort((lm, k0, k1, w0, w1))               # (observation window, reference window, observation interval, reference interval, landmark), stable
    R["order"] = order
    s0, s1, sl = k0[order], k1[order], lm[order]

    def runs(cap):
        out = []
        for i in range(n):
            a0, a1 = int(s0[i] >> 2), int(s1[i] >> 2)
            if not out or out[-1][2] != a0 or out[-1][3] != a1 or i - out[-1][0] >= cap:
                out.append([i, 0, a0, a1])
            out[-1][1] += 1
        return [tuple(g) for g in out]
    R["groups"] = runs(GROUP_CAP)                            # (first row, blocks, w0, w1) of k_reproj_cross
    R["fused_groups"] = runs(FUSED_CAP)                      # ... of k_reproj_fused
    R["pair_sizes"] = {}
    for _, c, a0, a1 in R["groups"]:
        R["pair_sizes"][(a0, a1)] = R["pair_sizes"].get((a0, a1), 0) + c
    R["last_trips"] = [((c - 1) % 8) + 1 for _, c, _, _ in R["groups"]]              # blocks of each group's last trip of 8
    R["nks"] = [(2 * r + 3) >> 2 for r in R["last_trips"]]                           # its MFMA k-steps
    strays = (R["k0_eval"] >> 2 != w0) | (R["k1_eval"] >> 2 != w1)
    R["strays"] = strays[order]                              # per device row
    R["stray_side"] = [("ref" if (R["k0_eval"][i] >> 2) != w0[i] else "") + ("obs" if (R["k1_eval"][i] >> 2) != w1[i] else "") for i in order]
    R["lm_blocks"] = [np.flatnonzero(sl == l) for l in range(L)]                     # device rows of every landmark
    # deterministic colouring: a group touches the UNORDERED pairs of 4-knot blocks {w0, w0 + 1} x {w1, w1 + 1}; first colour without a common key
    keys = [frozenset((min(a0 + a, a1 + b), max(a0 + a, a1 + b)) for a in range(2) for b in range(2)) for _, _, a0, a1 in R["groups"]]
    used, colour = [], []
    for ks in keys:
        c = 0
        while c < len(used) and used[c] & ks:
            c += 1
        if c == len(used):
            used.append(set())
        used[c] |= ks
        colour.append(c)
    R["colour_keys"], R["colours"] = keys, colour
    # padded frame spans (build_segments): first and last knot of every block, of every landmark
    free_tau = not (locks & lvx.LOCK_CAM_TAU)
    t1 = np.minimum(P["lm_t0"][lm], t_obs) - (SENSOR_MTO if free_tau else 0.0)
    t2 = np.maximum(P["lm_t0"][lm], t_obs) + (SENSOR_MTO if free_tau else 0.0)
    kmin = interval(P, t1 - MARGIN)
    kmax = interval(P, t2 + P["camera"]["readout"] + MARGIN) + 3
    R["kmin"], R["kmax"] = kmin, kmax
    lm_first, lm_last = np.full(L, N), np.full(L, -1)
    np.minimum.at(lm_first, lm, kmin); np.maximum.at(lm_last, lm, kmax)
    R["lm_first"], R["lm_last"] = lm_first, lm_last
    # hub knots and band positions
    nh = h0 = 0
    if len(P["surf_t"]) > 0 or len(P["cs_lm"]) > 0:
        pad = SENSOR_MTO if (not (locks & lvx.LOCK_LIDAR_TAU) or free_tau) else 0.0
        h0 = int(interval(P, P["t_map"] - pad)); nh = min(N, int(interval(P, P["t_map"] + pad)) + 5) - h0
    R["n_hub"], R["hub0"] = nh, h0
    R["n_border"] = 6 * nh + 22
    nbd_ext = R["n_border"] + 12
    nt = 6 * N + 22 + L
    ordv = np.full(nt, -(1 << 30), dtype=np.int64)          # >= 0 band position, -1 - b border slot, DEAD otherwise; landmarks have rows of their own
    pos = 0
    for k in range(N):
        hub = nh > 0 and h0 <= k < h0 + nh
        for d in range(6):
            if not _locked(6 * k + d, N, locks):
                if hub:
                    ordv[6 * k + d] = -1 - (6 * (k - h0) + d)
                else:
                    ordv[6 * k + d] = pos; pos += 1
    for c in range(22):
        if not _locked(6 * N + c, N, locks):
            ordv[6 * N + c] = -1 - (6 * nh + c)
    R["ord"], R["n_band"] = ordv, pos

    def span_pos(ka, kb):
        o = ordv[6 * ka:6 * min(kb + 1, N)]
        o = o[o >= 0]
        return (int(o.min()), int(o.max())) if len(o) else None
    p0, wl = np.zeros(L, dtype=np.int64), 1
    touches_band = np.zeros(L, dtype=bool)
    for l in range(L):
        if lm_last[l] >= 0:
            s = span_pos(lm_first[l], lm_last[l])
            if s:
                p0[l] = s[0]; wl = max(wl, s[1] - s[0] + 1); touches_band[l] = True
    R["lm_p0"], R["lm_wl"] = p0, wl
    seen = [l for l in range(L) if lm_last[l] >= 0]
    seen.sort(key=lambda l: p0[l])                            # stable
    groups, spread = [], 0
    for l in seen:
        if not groups or len(groups[-1]) >= ELIM_CAP or p0[l] - p0[groups[-1][0]] > ELIM_REACH:
            groups.append([])
        groups[-1].append(l)
        spread = max(spread, int(p0[l] - p0[groups[-1][0]]))
    R["elim_groups"], R["elim_spread"] = groups, spread
    ne_max = wl + spread + nbd_ext
    R["lds_g"] = 32 * (ne_max + 1) * 8 + 32 * 8 + 2 * ne_max * 4 + 16          # solve_local: the group kernel's dynamic LDS
    R["elim_kernel"] = 0 if (L == 0 or n == 0 or (locks & lvx.LOCK_LANDMARKS)) else (1 if groups and R["lds_g"] <= LDS_LIMIT else 2)
    # columns a landmark's row couples to (tangent indices): four knots per pose of every block, the free camera columns, the time offset when free.  `required` leaves out
    # the blocks that ARE the reference observation (both poses equal: the derivatives cancel to zero or to rounding noise), `allowed` keeps them
    cam_cols = [6 * N + 15 + c for c in range(7) if not _locked(6 * N + 15 + c, N, locks)]
    req, alw = [set() for _ in range(L)], [set() for _ in range(L)]
    for i in range(n):
        l = int(lm[i])
        cols = set(cam_cols)
        for k in list(range(k0[i], k0[i] + 4)) + list(range(k1[i], k1[i] + 4)):
            cols |= {6 * k + d for d in range(6) if not _locked(6 * k + d, N, locks)}
        alw[l] |= cols
        if not (t_obs[i] == P["lm_t0"][l] and np.array_equal(uv[i], P["lm_uv"][l])):
            req[l] |= cols
    R["cols_required"], R["cols_allowed"] = req, alw
    R["hub_coupled"] = [any(c < 6 * N and nh > 0 and h0 <= c // 6 < h0 + nh for c in alw[l]) for l in range(L)]
    R["band_sides"] = [(any(c < 6 * h0 for c in alw[l]), any(6 * (h0 + nh) <= c < 6 * N for c in alw[l])) if nh > 0 else (False, False) for l in range(L)]
    R["nn_predicted"] = [len(set().union(*[req[l] for l in g])) for g in groups]
    return R
