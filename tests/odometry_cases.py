"""Shared by tests/test_odometry_cases.py (CPU) and tests/test_gpu_odometry.py: the scan sequences of the LiDAR odometry tests and a restatement of
LiDAROdometry::feedScan(using_loam = false) (src/lvi_exc/src/core/lidar_odometry.cpp:45-128) composed only of oracle calls — O.voxelgrid_xyzi (downsampleCloud),
NA.NdtAligner at the odometry's settings (:36-41), PL.key_scans (checkKeyScan) and PL.transform_cloud (updateKeyScan).  step() runs ONE scan from a given state (map cloud,
guess), run() the whole loop.

Why one step.  The loop is chaotic: the line search takes steps capped at 0.01 and stops once one falls below 1e-3, nowhere near a fixed point, so a 1e-7 m change of a
guess grows to centimetres within a dozen scans and the iteration counts part.  No test compares two free-running loops.  The GPU loop is held bit for bit to its own
parts (filter, grid build, align) and, step by step from the GPU's own state, to step() — on the steps whose oracle result is itself stable under a 1e-7 m change of
the guess (stability()).

Cases: a room ray-cast from a moving, rolling LiDAR exactly as synth.make_sequence does it (same extrinsics, same _raycast_room), 16 scans of 16 x 225 points at 10 Hz,
range noise 0.01 m, 1 % of the points with x = NaN.  `gentle` moves slowly (two key scans), `lively` fast enough for several more."""
import functools

import numpy as np

import synth
from oracle import ndt_align as NA
from oracle import oracle as O
from oracle import pipeline as PL

H, W, N_SCANS, SCAN_RATE = 16, 225, 16, 10.0
LEAF, RESOLUTION, KEY_DIST, KEY_ANGLE_DEG = 0.5, 0.5, 0.2, 5.0
NDT = dict(resolution=RESOLUTION, search=NA.DIRECT7, step_size=0.01, transformation_epsilon=1e-3, max_iterations=50)
KEY_MARGIN = 1e-3            # every key decision lies at least this far from its threshold (m, degrees)
PERTURB, N_PERTURB = 1e-7, 4  # stability record: the guess translation moved by PERTURB * N(0, 1), N_PERTURB times
UNSTABLE_ABOVE = 1e-4        # a step whose p6 moves by more than this (or whose iteration count changes) is unstable
MAX_UNSTABLE = dict(gentle=0, lively=2)
P6_BAR = 1e-6                # the project's bar for lvx_ndt_align with line-search iterations (tests/test_gpu_ndt_align.py)
CASES = dict(gentle=dict(seed=7, pos_amp=0.3, rot_amp=0.1), lively=dict(seed=7, pos_amp=0.6, rot_amp=0.25))


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Raw scans [N_SCANS][H * W] (lvx.POINT_XYZIT layout) and their header stamps."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    t0, dt = 100.0, 0.02
    n_knots = int(np.ceil((0.2 + (N_SCANS + 1) / SCAN_RATE) / dt)) + 6
    r3, so3 = synth.make_trajectory(n_knots, t0, dt, rng, pos_amp=c["pos_amp"], rot_amp=c["rot_amp"])
    r3[:, 2] *= 0.25                                                     # stay between floor and ceiling
    sp = synth.Spline(t0, dt, r3, so3)
    q_LI = synth.q_from_rpy(np.deg2rad(2.0), np.deg2rad(-3.0), np.deg2rad(91.0)); p_LI = np.array([0.05, -0.10, 0.12])   # make_sequence's LiDAR mounting
    az = np.deg2rad(np.arange(W) * (360.0 / W)); el = np.deg2rad(np.linspace(-15.0, 15.0, H))
    E, A = np.meshgrid(el, az, indexing="ij")
    dirs_L = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    col_dt = np.tile(np.arange(W) / W / SCAN_RATE, H)
    scans = np.zeros((N_SCANS, H * W), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("pad2", "<f4"), ("timestamp", "<f8")]))
    stamps = t0 + 0.2 + np.arange(N_SCANS) / SCAN_RATE
    for s in range(N_SCANS):
        ts = stamps[s] + col_dt
        assert sp.t_min <= ts[0] and ts[-1] < sp.t_max
        ek = sp.eval(ts)
        org = synth.qrot(ek["quat"], np.broadcast_to(p_LI, (len(ts), 3))) + ek["pos"]
        dW = synth.qrot(ek["quat"], synth.qrot(np.broadcast_to(q_LI, (len(ts), 4)), dirs_L))
        rr = synth._raycast_room(dW, org) + 0.01 * rng.standard_normal(len(ts))
        xyz = (dirs_L * rr[:, None]).astype(np.float32)
        scans["x"][s], scans["y"][s], scans["z"][s], scans["timestamp"][s] = xyz[:, 0], xyz[:, 1], xyz[:, 2], ts
        scans["intensity"][s] = (10.0 * rng.random(len(ts))).astype(np.float32)
        scans["x"][s][rng.random(len(ts)) < 0.01] = np.nan
    scans.setflags(write=False)
    return dict(name=name, scans=scans, stamps=stamps, H=H, W=W)


def scan_xyzi(raw):
    """One raw scan as the xyzi cloud the filter, the registration and the map take."""
    return np.stack([raw["x"], raw["y"], raw["z"], raw["intensity"]], axis=-1).astype(np.float32)


def finite(xyzi):
    return xyzi[np.isfinite(xyzi[:, :3]).all(axis=1)]


def source(xyzi):
    """downsampleCloud(cur_scan, filtered, 0.5) (:81): pcl::VoxelGrid leaves non-finite points out"""
    return O.voxelgrid_xyzi(finite(xyzi), LEAF)


def aligner(map_cloud):
    """ndtInit (:32-43) + setInputTarget(map_cloud_) (:102)"""
    return NA.NdtAligner(map_cloud, **NDT)


def guess_of(pose_last, predict=None):
    """T_LtoM_predict = pose[k - 1] * predict (:59) in double, the sum taken left to right, cast to float (:84)"""
    L = np.asarray(pose_last, np.float64).reshape(4, 4)
    if predict is None:
        return L.astype(np.float32)
    P = np.asarray(predict, np.float64).reshape(4, 4)
    G = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            G[i, j] = ((L[i, 0] * P[0, j] + L[i, 1] * P[1, j]) + L[i, 2] * P[2, j]) + L[i, 3] * P[3, j]
    return G.astype(np.float32)


def step(map_cloud, guess16, scan, ndt=None):
    """registration() (:76-87) of one scan against `map_cloud` from the float guess: dict(pose (double 4 x 4), p6, iterations, n_evaluations, n_src).  ndt: an aligner
    already built over this map."""
    a = aligner(map_cloud) if ndt is None else ndt
    src = source(scan)
    final = a.align(src, np.asarray(guess16, np.float32).reshape(4, 4))
    return dict(pose=np.asarray(final, np.float32).astype(np.float64), p6=np.array(a.p), iterations=a.nr_iterations, n_evaluations=a.n_eval, n_src=len(src))


def is_key(poses):
    """checkKeyScan for the last of `poses` given all before it (PL.key_scans replays the rule from the first scan)"""
    return (len(poses) - 1) in PL.key_scans(poses, [True] * len(poses), KEY_DIST, KEY_ANGLE_DEG)


def key_margin(poses):
    """Smallest distance of any quantity checkKeyScan compares from its threshold, over the scans after the first (m, degrees)."""
    pos_last, ypr_last, m = np.zeros(3), np.zeros(3), np.inf
    keys = PL.key_scans(poses, [True] * len(poses), KEY_DIST, KEY_ANGLE_DEG)
    for s in range(len(poses)):
        T = np.asarray(poses[s], np.float64).reshape(4, 4)
        ypr = PL.r2ypr_deg(T[:3, :3])
        if s > 0:
            d = ypr - ypr_last
            d = np.where(d > 180, d - 360, d)
            d = np.where(d < -180, d + 360, d)
            m = min(m, abs(np.linalg.norm(T[:3, 3] - pos_last) - KEY_DIST), np.abs(np.abs(d) - KEY_ANGLE_DEG).min())
        if s in keys:
            pos_last, ypr_last = T[:3, 3].copy(), ypr
    return m


@functools.lru_cache(maxsize=None)
def run(name):
    """The whole oracle loop: poses [n][4][4], key scan list, per-step records (None for the first scan), the map cloud each step started from (its key count)."""
    C = make_case(name)
    poses, keys, steps, maps, n_map = [], [], [], [np.zeros((0, 4), np.float32)], []
    ndt = None
    for k in range(N_SCANS):
        scan = scan_xyzi(C["scans"][k])
        n_map.append(len(keys))
        if not keys:
            poses.append(np.eye(4)); steps.append(None)
        else:
            r = step(maps[-1], guess_of(poses[-1]), scan, ndt)
            poses.append(r["pose"]); steps.append(r)
        if is_key(poses):
            keys.append(k)
            maps.append(np.concatenate([maps[-1], PL.transform_cloud(scan, poses[-1])]))
            ndt = aligner(maps[-1])
    return dict(poses=np.array(poses), keys=keys, steps=steps, maps=maps, n_map=n_map)


@functools.lru_cache(maxsize=None)
def stability(name):
    """Per step k >= 1, from the oracle's own state: s_k = the largest change of p6 over N_PERTURB re-runs of the align with the guess translation moved by
    PERTURB * N(0, 1) (float, same map, fixed seed), and whether the step is unstable (an iteration count changed or s_k > UNSTABLE_ABOVE)."""
    C, R = make_case(name), run(name)
    rng = np.random.default_rng(1234)
    s, unstable = np.zeros(N_SCANS), np.zeros(N_SCANS, bool)
    ndt, built = None, -1
    for k in range(1, N_SCANS):
        if built != R["n_map"][k]:
            ndt, built = aligner(R["maps"][R["n_map"][k]]), R["n_map"][k]
        scan = scan_xyzi(C["scans"][k])
        for _ in range(N_PERTURB):
            g = guess_of(R["poses"][k - 1]).copy()
            g[:3, 3] += (PERTURB * rng.standard_normal(3)).astype(np.float32)
            r = step(None, g, scan, ndt)
            s[k] = max(s[k], np.abs(r["p6"] - R["steps"][k]["p6"]).max())
            unstable[k] |= r["iterations"] != R["steps"][k]["iterations"]
        unstable[k] |= s[k] > UNSTABLE_ABOVE
    return s, unstable
