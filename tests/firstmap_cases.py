"""The first DataAssociation of a calibration, map from per-scan odometry poses (lvx_data_association_poses): a case table and numpy float64 restatements of its two
device stages and of its host rule that do not rest on the oracle.  tests/test_firstmap_cases.py holds every case to what it claims on the CPU and the oracle
(oracle/pipeline.py::first_data_association) to the restatements; tests/test_gpu_firstmap.py runs the same cases through lvx.set_scans / lvx.data_association_poses.

Restated here:
  presence        a scan is in the map iff its stamp + tau_lidar lies in [t0, t0 + (N - 3) dt) (evaluateLidarPose, trajectory_manager_lvi.cpp:401-402) and it has a pose
                  (loam_poses_map_.find, lvi_initialize_surfel_orb.cpp:1262-1300)
  de-skew         undistortScan(correct_position = false) (scan_undistortion.h:40-57, 132-180): rotation only, into the LiDAR orientation at the scan's stamp, rounded to
                  float; a point whose own stamp lies outside the spline keeps the resize()'d zeros (intensity 0 with them); x = NaN gives a NaN point
  transform       pcl::transformPointCloud with the scan's Matrix4d (scan_undistortion.h:95-116): double arithmetic on the float coordinates, the sum left to right,
                  rounded to float; non-finite points are copied; absent scans are NaN with intensity 0
  key-scan rule   LiDAROdometry::checkKeyScan (lidar_odometry.cpp:107-128) with mathutils::R2ypr (math_utils.h:192-207) and normalize_angle (lidar_odometry.h:95-102)

Sequences: synth.make_sequence(seed=53, duration=1.5, H=16, W=225, n_reproj=200) — 12 scans x 3 600 points — and its small-HW variants; W = 450, duration = 2.0 where one key
scan alone has to carry a surfel map."""
import functools
import math

import numpy as np

import synth

KEY_DIST, KEY_ANGLE = 0.25, 5.0            # the key-rule cases' thresholds (the reference's: 0.2 m, 5 deg)
BASE = (16, 225, 1.5)                      # H, W, duration
DENSE = (16, 450, 2.0)
ROOM = 30.0                                # every coordinate of a scan in the map frame lies inside +- ROOM (the room is 20 x 15 m)
RIGHT = dict(strict=True, last="key", wrap=True, has_pose=True)      # the key-scan and presence rules as the reference has them; wrong variants: tests/test_firstmap_cases.py


@functools.lru_cache(maxsize=None)
def sequence(H, W, duration):
    S = synth.make_sequence(seed=53, duration=duration, H=H, W=W, n_reproj=200)
    rng = np.random.default_rng(H * 10000 + W)
    S["scans"]["intensity"] = rng.uniform(1.0, 100.0, S["scans"].shape).astype(np.float32)      # (make_sequence leaves it 0: nothing would tell it from the zeros of an absent scan)
    S["scans"].setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def loam(H, W, duration):
    """(scan_t [n], T [n, 16]) of the sequence: the LiDAR poses of the ground truth in the frame of the map time, slightly perturbed."""
    scan_t, _, _, _, T = synth.sequence_loam_poses(sequence(H, W, duration), noise_m=2e-3, noise_rad=5e-4, seed=7)
    scan_t.setflags(write=False); T.setflags(write=False)
    return scan_t, T


def pose(yaw=0.0, pitch=0.0, roll=0.0, p=(0.0, 0.0, 0.0)):
    """Row-major 4 x 4 [Rz(yaw) Ry(pitch) Rx(roll) | p], angles in degrees."""
    y, b, r = (math.radians(a) for a in (yaw, pitch, roll))
    Rz = np.array([[math.cos(y), -math.sin(y), 0.0], [math.sin(y), math.cos(y), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[math.cos(b), 0.0, math.sin(b)], [0.0, 1.0, 0.0], [-math.sin(b), 0.0, math.cos(b)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(r), -math.sin(r)], [0.0, math.sin(r), math.cos(r)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = p
    return T.ravel()


# ------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ------------------------------------------------------------------------------------------------------------------------
def ypr_deg(T16):
    """mathutils::R2ypr of the rotation of a row-major 4 x 4, in degrees."""
    R = [[float(T16[4 * i + j]) for j in range(3)] for i in range(3)]
    n, o, a = [R[i][0] for i in range(3)], [R[i][1] for i in range(3)], [R[i][2] for i in range(3)]
    y = math.atan2(n[1], n[0])
    p = math.atan2(-n[2], n[0] * math.cos(y) + n[1] * math.sin(y))
    r = math.atan2(a[0] * math.sin(y) - a[1] * math.cos(y), -o[0] * math.sin(y) + o[1] * math.cos(y))
    return [v / math.pi * 180.0 for v in (y, p, r)]


def np_key_scans(poses, present, key_dist, key_angle_deg, rules=RIGHT):
    """checkKeyScan over the scans that are fed, in order: position_last / ypr_last start at zero and move ONLY when a scan becomes a key scan; the first fed scan is one
    (key_frame_index_ is empty); otherwise dist > key_dist or one of |yaw|, |pitch|, |roll| differences, wrapped once by +-360, > key_angle_deg."""
    over = (lambda v, lim: v > lim) if rules["strict"] else (lambda v, lim: v >= lim)
    pos_last, ypr_last, key = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], []
    for s in range(len(poses)):
        if not present[s]:
            continue
        T = np.asarray(poses[s], np.float64).ravel()
        pos = [float(T[3]), float(T[7]), float(T[11])]
        dist = math.sqrt(sum((pos[a] - pos_last[a]) ** 2 for a in range(3)))
        ypr = ypr_deg(T)
        turned = False
        for a in range(3):
            d = ypr[a] - ypr_last[a]
            if rules["wrap"]:
                if d > 180:
                    d -= 360
                if d < -180:
                    d += 360
            turned = turned or over(abs(d), key_angle_deg)
        is_key = not key or over(dist, key_dist) or turned
        if is_key:
            key.append(s)
        if is_key or rules["last"] == "scan":
            pos_last, ypr_last = pos, ypr
    return key


def _spline(S, state):
    u = synth.unpack_state(state, S["n_knots"], S["n_landmarks"])
    return synth.Spline(S["t0"], S["dt"], u["r3"], u["so3"]), u["lidar"][:4], float(u["lidar"][7])


def np_inside(S, state, t):
    """evaluateLidarPose's range test at t + tau_lidar."""
    tau = float(state[7 * S["n_knots"] + 16 + 7])
    tt = np.asarray(t, np.float64) + tau
    return (S["t0"] <= tt) & (tt < S["t0"] + (S["n_knots"] - 3) * S["dt"])


def np_present(S, state, scan_t, has_pose, rules=RIGHT):
    ok = np_inside(S, state, scan_t)
    if has_pose is not None and rules["has_pose"]:
        ok = ok & (np.asarray(has_pose) != 0)
    return ok


def np_scans_in_map(S, state, scan_t, poses, has_pose):
    """(scans in the map frame [n, H, W, 4] float32, present [n] bool, zeroed [n, H W] bool: points of present scans that took the zero-then-transform branch)."""
    sp, qL, tau = _spline(S, state)
    sc = S["scans"]
    n, HW = sc.shape
    present = np_present(S, state, scan_t, has_pose)
    out = np.full((n, HW, 4), np.nan, np.float32)
    out[:, :, 3] = 0.0
    zeroed = np.zeros((n, HW), bool)
    for s in np.nonzero(present)[0]:
        q_scan = synth.qmul(sp.eval([scan_t[s] + tau])["quat"][0], qL)
        nan = np.isnan(sc["x"][s])
        ok = np_inside(S, state, sc["timestamp"][s]) & ~nan
        zeroed[s] = ~ok & ~nan
        und = np.zeros((HW, 4), np.float32)
        q_pt = synth.qmul(sp.eval(sc["timestamp"][s][ok] + tau)["quat"], qL)
        xyz = np.stack([sc[k][s][ok].astype(np.float64) for k in ("x", "y", "z")], axis=1)
        und[ok, :3] = synth.qrot(synth.qmul(synth.qconj(q_scan), q_pt), xyz).astype(np.float32)
        und[ok, 3] = sc["intensity"][s][ok]
        T = np.asarray(poses[s], np.float64).reshape(4, 4)
        x, y, z = (und[:, a].astype(np.float64) for a in range(3))
        for r in range(3):
            out[s, :, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
        out[s, :, 3] = und[:, 3]
        out[s, nan, :3] = np.nan
    return out.reshape(n, S["H"], S["W"], 4), present, zeroed


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call: the first n scans of a sequence (n = None: all), a state (state_true with tau_lidar set), stamps, poses, has_pose and the key thresholds.
    poses = None: the sequence's own.  scan_t_set {scan: stamp} and point_t_set (scan, point indices, stamp) move stamps.  key: the key scans the case claims (None: whatever
    the rule gives); absent: the scans it claims absent; zeroed: it claims points on the zero-then-transform branch; may_be_empty: no surfel is required of it."""

    def __init__(self, name, group, seq=BASE, n=None, tau=0.0, has_pose=None, scan_t_set=None, point_t_set=None, poses=None, key_dist=0.2, key_angle=5.0, key=None, absent=(),
                 zeroed=False, may_be_empty=False):
        self.name, self.group, self.seq, self.tau, self.key_dist, self.key_angle, self.key, self.absent, self.zeroed, self.may_be_empty = (
            name, group, seq, tau, key_dist, key_angle, key, tuple(absent), zeroed, may_be_empty)
        self.n = len(poses) if poses is not None else (n if n is not None else len(loam(*seq)[0]))
        self._has_pose, self._scan_t_set, self._point_t_set, self._poses = has_pose, dict(scan_t_set or {}), point_t_set, poses

    @property
    def H(self):
        return self.seq[0]

    @property
    def W(self):
        return self.seq[1]

    def S(self):
        return _case_sequence(self.name)

    def state(self):
        S = sequence(*self.seq)
        x = np.array(S["state_true"], np.float64)
        x[7 * S["n_knots"] + 16 + 7] = self.tau
        return x

    def scan_t(self):
        t = np.array(loam(*self.seq)[0][:self.n])
        for s, v in self._scan_t_set.items():
            t[s] = v
        return t

    def poses(self):
        return np.array(loam(*self.seq)[1][:self.n]) if self._poses is None else np.stack([np.asarray(T, np.float64).ravel() for T in self._poses])

    def has_pose(self):
        if self._has_pose is None:
            return None
        h = np.ones(self.n, np.int32)
        h[list(self._has_pose)] = 0
        return h

    def raw(self):
        """[n, H W] PointXYZIT records, as lvx.set_scans takes them."""
        return self.S()["scans"]

    def expected(self):
        return _expected(self.name)

    def __repr__(self):
        return "Case(%s)" % self.name


@functools.lru_cache(maxsize=None)
def _case_sequence(name):
    c = BY_NAME[name]
    S = dict(sequence(*c.seq))
    sc = np.array(S["scans"][:c.n])
    if c._point_t_set is not None:
        s, idx, t = c._point_t_set
        sc["timestamp"][s][np.asarray(idx)] = t
    sc.setflags(write=False)
    S["scans"] = sc
    return S


@functools.lru_cache(maxsize=None)
def _expected(name):
    """dict(scans, present, zeroed, key) by the restatements."""
    c = BY_NAME[name]
    scans, present, zeroed = np_scans_in_map(c.S(), c.state(), c.scan_t(), c.poses(), c.has_pose())
    key = np_key_scans(c.poses(), present, c.key_dist, c.key_angle)
    for a in (scans, present, zeroed):
        a.setflags(write=False)
    return dict(scans=scans, present=present, zeroed=zeroed, key=key)


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """oracle/pipeline.py::first_data_association of the case (plane_lambda = 0.6)."""
    from oracle import pipeline
    c = BY_NAME[name]
    return pipeline.first_data_association(c.S(), c.state(), c.scan_t(), c.poses(), c.has_pose(), key_dist=c.key_dist, key_angle_deg=c.key_angle)


T0 = sequence(*BASE)["t0"]
ZERO_POINTS = np.arange(40) * 89 + 7          # 40 points of scan 3, spread over its rings and columns (never point 0: the scan's stamp is read from it)


def _key_case(name, poses, key, **kw):
    return Case(name, "key_rule", poses=poses, key_dist=KEY_DIST, key_angle=KEY_ANGLE, key=key, **kw)


def _key_rule():
    step = dict(yaw_only="yaw", pitch_only="pitch", roll_only="roll")
    return [
        # 0.25 away from the last key scan is not one; (0.1875, 0.25) is 0.3125 away; scan 3 is 0.25 from scan 2; scan 4 is 0.2500001 above scan 2
        _key_case("dist_strict", [pose(p=p) for p in ((0, 0, 0), (0.25, 0, 0), (0.1875, 0.25, 0), (0.4375, 0.25, 0), (0.1875, 0.25, 0.2500001))], [0, 2, 4]),
        _key_case("last_key", [pose(p=(0.1 * k, 0, 0)) for k in range(10)], [0, 3, 6, 9]),                 # 0.1 m per scan: against the last SCAN nothing after scan 0 is a key scan
    ] + [_key_case(name, [pose(**{a: 2.0 * k}) for k in range(10)], [0, 3, 6, 9]) for name, a in step.items()] + [
        _key_case("yaw_wrap", [pose(yaw=a) for a in (178.0, -179.0, -176.0)], [0, 2]),                     # differences -357 -> 3 and -354 -> 6
        _key_case("angle_margin", [pose(yaw=a) for a in (0.0, 4.999999, 5.000001)], [0, 2]),
        # scan 0 has no pose, scan 1 is stamped before the spline: the first PRESENT scan is the first key scan, whatever the zero start values say (5.1 m from them)
        _key_case("first_absent", [pose(p=(0, 0, 5.0)), pose(p=(0, 0, 5.0)), pose(p=(0, 0, 5.1)), pose(p=(0, 0, 5.4))], [2, 3], has_pose=(0,), scan_t_set={1: T0 - 0.5}, absent=(0, 1)),
        Case("nondefault_all", "key_rule", key_dist=0.05, key_angle=1.0, key=list(range(12))),
        Case("nondefault_one", "key_rule", seq=DENSE, key_dist=1e9, key_angle=1e9, key=[0]),
    ]


def _presence():
    mixed = dict(has_pose=(0, 5), scan_t_set={1: T0 - 0.5}, point_t_set=(3, ZERO_POINTS, T0 - 1.0), tau=0.25)
    return [
        Case("mixed", "presence", key=[2, 3, 6, 7, 9, 10, 11], absent=(0, 1, 5), zeroed=True, **mixed),
        Case("tau_tail", "presence", tau=0.55, zeroed=True),                       # the last scan's stamp is inside the spline, its late columns are not
        Case("tau_drop", "presence", tau=0.65, absent=(11,), zeroed=True),         # the last scan is dropped (and the late columns of the one before it are outside)
        Case("has_pose_null", "presence"),
        Case("all_key", "presence", key_dist=-1.0, key_angle=5.0, key=list(range(12))),      # every scan a key scan: the map cloud is the whole recording
    ]


def _shapes():
    # S = 1 and 2 take the all-pairs association kernel, S = 3 is the first size with the prepared map; one scan of the base sequence alone carries no surfel, the denser one does
    return [Case("s1", "shapes", seq=DENSE, n=1)] + [Case("s%d" % n, "shapes", n=n) for n in (2, 3)] + [
        Case("w15", "shapes", seq=(16, 15, 1.5), may_be_empty=True),               # 240 points a scan: below one workgroup
        Case("w17", "shapes", seq=(16, 17, 1.5), may_be_empty=True),               # 272: one workgroup and a tail
        Case("h3", "shapes", seq=(3, 225, 1.5), may_be_empty=True),                # 675
    ]


def _empty():
    return [
        Case("empty_no_pose", "empty", has_pose=tuple(range(12)), key=[], absent=tuple(range(12)), may_be_empty=True),
        Case("empty_outside", "empty", tau=5.0, key=[], absent=tuple(range(12)), may_be_empty=True),
    ]


def _context():
    # one context, successive calls on the denser sequence: all scans key -> one key scan (nondefault_one) -> a refinement round -> all scans key again
    return [Case("dense_all_key", "context", seq=DENSE, key_dist=-1.0, key=list(range(17)))]


CASES = _key_rule() + _presence() + _shapes() + _empty() + _context()
BY_NAME = {c.name: c for c in CASES}
MAY_BE_EMPTY = [c.name for c in CASES if c.may_be_empty and c.group != "empty"]
WRONG_RULES = dict(ge=dict(RIGHT, strict=False), last_scan=dict(RIGHT, last="scan"), no_wrap=dict(RIGHT, wrap=False), ignore_has_pose=dict(RIGHT, has_pose=False))
