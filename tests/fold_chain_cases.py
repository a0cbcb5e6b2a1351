"""Shared by tests/test_fold_chain_cases.py (CPU) and tests/test_gpu_fold_chain.py: the cases in which the fold of the pseudo pose rows onto the hub control points
(k_fold_all: dense border block in closed form, border rows) and the hub prepass of k_clear take their different paths.

Base problem: the one of tests/test_gpu_pass_launches.py — both LiDAR sets (surfel, camera-surfel) are evaluated and share the hub rows, the case in which the two
sets' folds interact.  A case is (problem dict, state, second state, locks, extras); extras["poses"] is a lidarpos_cases.Case where LiDAR position blocks are set."""
import functools

import numpy as np

import lidarpos_cases as lc
import lvx
import synth
from oracle import oracle as O

TAU = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
DEAD_LOCKS = TAU | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS   # position columns of every control point dead, the hub's among them (3 of 6 per hub knot)
HUB_KNOT = 12       # t_map of the moved cases sits at / around knot 12, as in test_gpu_pass_launches._problem(True)

LOCK_CASES = {"locks_tau": TAU, "locks_free_offsets": 0, "locks_r3": TAU | lvx.LOCK_R3, "locks_landmarks": TAU | lvx.LOCK_LANDMARKS, "locks_dead_hub_columns": DEAD_LOCKS}
NAMES = (["both_sets", "surfel_only", "camsurf_only"] + list(LOCK_CASES) + ["fallback_lists", "lidar_poses", "tmap_mid_interval", "tmap_behind_knot", "tmap_before_knot"])


def base_problem():
    return synth.make_problem(seed=4, duration=2.0, n_surfel=700, n_planes=12, n_landmarks=30, n_camsurf=10)


def second_state(P, s, seed=7, amp=1e-3):
    """`s` with every control point and extrinsic moved by up to amp (quaternions renormalised); time offsets, gravity and biases as they are."""
    N = P["n_knots"]
    rng = np.random.default_rng(seed)
    t = np.array(s, np.float64)
    t[:7 * N] += amp * rng.uniform(-1.0, 1.0, 7 * N)
    for o in (7 * N + 16, 7 * N + 24):
        t[o:o + 7] += amp * rng.uniform(-1.0, 1.0, 7)
        t[o:o + 4] /= np.linalg.norm(t[o:o + 4])
    q = t[3 * N:7 * N].reshape(N, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return t


def _move_tmap(P, t_map, rows_behind):
    """t_map moved; with rows_behind, 40 surfel points in the interval right behind it (their spans merge with the map-time span)."""
    P = dict(P)
    P["t_map"] = t_map
    assert P["surf_t"].min() > t_map
    if rows_behind:
        P["surf_t"] = np.sort(np.concatenate([t_map + np.linspace(2e-3, 0.03, 40), P["surf_t"][40:]]))
    return P


@functools.lru_cache(maxsize=None)
def build(name):
    P = base_problem()
    s = P["state0"].copy()
    N = P["n_knots"]
    locks, ex = TAU, {"poses": None}
    knot = P["t0"] + HUB_KNOT * P["dt"]
    if name == "surfel_only":
        P = dict(P); P.update(cs_lm=P["cs_lm"][:0], cs_plane=P["cs_plane"][:0])
    elif name == "camsurf_only":
        P = dict(P); P.update(surf_pt=P["surf_pt"][:0], surf_t=P["surf_t"][:0], surf_plane=P["surf_plane"][:0])
    elif name in LOCK_CASES:
        locks = LOCK_CASES[name]
    elif name == "fallback_lists":     # test_gpu_pass_launches._problem(True)
        P = _move_tmap(P, knot - 5e-6, True)
        s[7 * N + 16 + 7] = 8e-6
    elif name == "lidar_poses":
        t_start = P["t_map"]          # one hub time per problem: the position blocks share the surfel / camera-surfel hub
        ex["poses"] = lc.Case(P, lc.pose_times(P, 9, t_start, "spread"), t_start)
    elif name == "tmap_mid_interval":
        P = _move_tmap(P, knot + 0.5 * P["dt"], False)
    elif name == "tmap_behind_knot":
        P = _move_tmap(P, knot + 5e-6, False)
    elif name == "tmap_before_knot":
        P = _move_tmap(P, knot - 5e-6, True)
    elif name != "both_sets":
        raise KeyError(name)
    s2 = second_state(P, s)
    s.setflags(write=False); s2.setflags(write=False)
    return P, s, s2, locks, ex


def oracle_results(name):
    """The oracle's results at both states.  LiDAR position blocks: J^T J, J^T r and the cost are sums over blocks, so the oracle of the problem and the oracle of
    the blocks alone (converted to surfel blocks, lidarpos_cases.converted_problem; every other family emptied) add; the position rows stand behind the others."""
    P, s, s2, locks, ex = build(name)
    o = O.Oracle()
    n_imu = len(P["t_imu"])
    if locks & lvx.LOCK_R3:
        # With the positions locked the library leaves the accelerometer blocks out (the reference's first solve has none).  The oracle keeps them unless it runs on
        # its SO3-only trajectory, which has no positions for the LiDAR families either: here it gets them with weight 0 — nothing in J^T J, J^T r and the cost —
        # and their rows (behind the gyroscope's 3 n) are taken out of its residual vector.
        P = dict(P, w_acc=0.0)
    lvx.load_problem(o, P, locks)
    out = [o.evaluate(x, normal_eq=True) for x in (s, s2)]
    if locks & lvx.LOCK_R3:
        for r in out:
            assert not r["residuals"][3 * n_imu:6 * n_imu].any()
            r["residuals"] = np.delete(r["residuals"], np.s_[3 * n_imu:6 * n_imu])
    if ex["poses"] is not None:
        Q, sign = lc.converted_problem(P, ex["poses"])
        Q.update(t_imu=P["t_imu"][:0], gyro=P["gyro"][:0], acc=P["acc"][:0], rep_lm=P["rep_lm"][:0], rep_uv=P["rep_uv"][:0], rep_t0=P["rep_t0"][:0])
        oq = O.Oracle()
        lvx.load_problem(oq, Q, locks)
        for r, x in zip(out, (s, s2)):
            q = oq.evaluate(x, normal_eq=True)
            assert q["residuals"].shape == (3 * ex["poses"].n,) and q["H"].shape == r["H"].shape
            r["residuals"] = np.concatenate([r["residuals"], sign * q["residuals"]])
            r["H"] = r["H"] + q["H"]; r["g"] = r["g"] + q["g"]; r["cost"] = r["cost"] + q["cost"]
    return out


def nonunit_hub_case():
    """Only the hub evaluates the scaled control point: no IMU samples, views or camera-surfel blocks, surfel points at least 8 intervals behind t_map.
    Returns (problem, state, the scaled knot)."""
    P = dict(base_problem())
    far = P["surf_t"] > P["t_map"] + 8 * P["dt"]
    P.update(t_imu=P["t_imu"][:0], gyro=P["gyro"][:0], acc=P["acc"][:0], rep_lm=P["rep_lm"][:0], rep_uv=P["rep_uv"][:0], rep_t0=P["rep_t0"][:0],
             cs_lm=P["cs_lm"][:0], cs_plane=P["cs_plane"][:0], surf_pt=P["surf_pt"][far], surf_t=P["surf_t"][far], surf_plane=P["surf_plane"][far])
    N = P["n_knots"]
    k = int(np.floor((P["t_map"] - P["t0"]) / P["dt"])) + 1           # inside the hub's four knots [k - 1, k + 2], outside every surfel point's
    s = P["state0"].copy()
    s[3 * N + 4 * k:3 * N + 4 * k + 4] *= 1.01
    return P, s, k
