"""Problems whose measurement TIMES are irregular, for the layout logic of the fused evaluators (ensure_layout in csrc/lvx_eval.hip: IMU batches and workgroup
ranges, the ownership table of k_imu_own, the sliding accumulator window, the equal-row LiDAR chunks, the permutation back to input order).

build(name) -> (P, state, locks, expect): P is a problem dict for lvx.load_problem, `state` the state to evaluate at (P["state0"], for the tau cases with the IMU
time offset set), expect what the tests need to know about the construction (which interval holds the burst, whether the oracle rejects the state, ...).
Every problem starts from synth.make_problem() and then edits the measurement arrays: parity against the oracle needs no physically consistent data, so stamps
are moved and gyro / acc / point values reused freely.  All cases use dt = 0.02 and stay small enough for the oracle's dense H."""
import numpy as np

import lvx
import synth
from oracle import oracle as O

TAU = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
DT = 0.02

# imu_fused_lds_bytes(span) = 8 * (222 * 24 + 8 * 222 + 8 * 8 + 222 + 8 + 64 + 4 * 1728) + 120 * span + 4 * (7 * span + 8) + 64 = 115 088 + 148 * span bytes (IMU_LV = 222 window
# scalars, ACC_BW = 24, IMU_NGA = 8, four panels of 96 x 18 doubles, sizeof(So3Pre) = 120): <= 160 KB = 163 840 bytes up to span = 329 knots, above it from 330 on.
IMU_LDS_SPAN_LIMIT = 329
IMU_WINDOW = 37          # IMU_CR + 5 knots: the accumulator window of one batch; the span of a workgroup range is (its last batch's first interval - its first one) + 37

IMU_COUNTS = (1, 255, 256, 257, 513)
SURF_COUNTS = (1, 63, 64, 65, 511, 512, 513)

NAMES = (["imu_gap_long", "imu_gaps_short", "imu_burst", "imu_sparse", "imu_sparse_nosurf"] + ["imu_counts_%d" % n for n in IMU_COUNTS] +
         ["imu_shuffled_dups", "imu_on_knots", "imu_tau_inside_pos", "imu_tau_inside_neg", "imu_tau_crossing_pos", "imu_tau_crossing_neg", "imu_tau_ge_dt",
          "surf_burst", "surf_ends"] + ["surf_counts_%d" % n for n in SURF_COUNTS] + ["surf_shuffled_dups", "rep_shuffled_unused"])

# Which of the tau cases the oracle rejects with IndexError (std::range_error of the reference): an IMU block's time span is {t, t}, its segment the four knots of t's
# interval (trajectory_estimator.h:102-127 CheckTimeSpans, spline_base.h:194-222), and t + tau outside that interval by more than the 1e-5 s retry finds no segment.
# tests/test_time_layout_cases.py holds the oracle to this table, tests/test_gpu_time_layouts.py the GPU (LVX_E_RANGE).
TAU_ORACLE_RAISES = {"imu_tau_inside_pos": False, "imu_tau_inside_neg": False, "imu_tau_crossing_pos": True, "imu_tau_crossing_neg": True, "imu_tau_ge_dt": True}


def interval(P, t):
    """Knot interval of every stamp: floor((t - t0) / dt)."""
    return np.floor((np.asarray(t, dtype=np.float64) - P["t0"]) / P["dt"]).astype(np.int64)


def max_time(P):
    return P["t0"] + (P["n_knots"] - 3) * P["dt"]


def tau_imu_slot(P):
    return 7 * P["n_knots"] + 7


def _base(seed, duration, n_surfel=300, n_planes=6, n_landmarks=6, views_per_lm=3, n_camsurf=0):
    return synth.make_problem(seed=seed, duration=duration, dt=DT, n_surfel=n_surfel, n_planes=n_planes, n_landmarks=n_landmarks, views_per_lm=views_per_lm, n_camsurf=n_camsurf)


def _keep_imu(P, keep):
    for k in ("t_imu", "gyro", "acc"):
        P[k] = P[k][keep]


def _set_imu_times(P, t):
    """New stamps, gyro / acc values of the generated stream reused cyclically."""
    n = len(t)
    idx = np.arange(n) % len(P["t_imu"])
    P["gyro"], P["acc"] = P["gyro"][idx].copy(), P["acc"][idx].copy()
    P["t_imu"] = np.asarray(t, dtype=np.float64)


def _set_surf_times(P, t):
    n = len(t)
    idx = np.arange(n) % len(P["surf_t"])
    P["surf_pt"], P["surf_plane"] = P["surf_pt"][idx].copy(), P["surf_plane"][idx].copy()
    P["surf_t"] = np.asarray(t, dtype=np.float64)


def _in_interval(P, k, frac):
    return P["t0"] + (k + np.asarray(frac, dtype=np.float64)) * P["dt"]


def _oracle_accepts_imu_rows(P, t):
    """Which stamps the oracle evaluates as a single IMU row of this spline (the others throw the reference's range_error)."""
    o = O.Oracle()
    o.set_spline(P["t0"], P["dt"], P["n_knots"])
    o.set_locks(TAU)
    state = P["state0"][:7 * P["n_knots"] + 32]
    ok = np.zeros(len(t), dtype=bool)
    for i, ti in enumerate(t):
        o.set_imu(np.array([ti]), np.zeros((1, 3)), np.zeros((1, 3)), 1.0, 1.0)
        try:
            o.evaluate(state)
            ok[i] = True
        except IndexError:
            pass
    return ok


def build(name):
    expect = {"tau_imu": False, "oracle_raises": False}
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "imu_gap_long":
        P = _base(201, 3.0, n_surfel=600)
        gap = (50, 115)                     # intervals [50, 115) lose every sample; the surfel rows (uniform over the sequence) continue through them
        k = interval(P, P["t_imu"])
        _keep_imu(P, (k < gap[0]) | (k >= gap[1]))
        expect["gap"] = gap
    elif name == "imu_gaps_short":
        P = _base(202, 2.0)
        holes = [(30, 1), (50, 4), (80, 5)]  # (first empty interval, run length)
        k = interval(P, P["t_imu"])
        keep = np.ones(len(k), dtype=bool)
        for a, n in holes:
            keep &= (k < a) | (k >= a + n)
        _keep_imu(P, keep)
        expect["holes"] = holes
    elif name == "imu_burst":
        P = _base(203, 2.0)
        kb, nb = 60, 800
        k = interval(P, P["t_imu"])
        rest = np.flatnonzero((k < kb - 1) | (k > kb + 1))
        three = np.flatnonzero(k == kb + 1)[:3]
        src = np.concatenate([rest, three, np.resize(np.flatnonzero(k == kb), nb)])       # the burst: the samples of the interval over and over (noise added below), at dense stamps
        t = np.concatenate([P["t_imu"][rest], P["t_imu"][three], _in_interval(P, kb, np.linspace(0.01, 0.99, nb))])
        P["gyro"], P["acc"], P["t_imu"] = P["gyro"][src] + 1e-3 * rng.standard_normal((len(src), 3)), P["acc"][src] + 1e-2 * rng.standard_normal((len(src), 3)), t
        expect["burst"] = kb
    elif name in ("imu_sparse", "imu_sparse_nosurf"):
        surf = name == "imu_sparse"
        P = _base(204, 13.7, n_surfel=1500 if surf else 0, n_planes=8 if surf else 1, n_landmarks=0)
        last = P["n_knots"] - 4             # last valid interval
        ks = 10 + np.cumsum(rng.integers(3, 8, 150))
        ks = ks[ks <= last]
        _set_imu_times(P, _in_interval(P, ks, rng.uniform(0.05, 0.95, len(ks))))
    elif name.startswith("imu_counts_"):
        n = int(name.rsplit("_", 1)[1])
        P = _base(205, 1.5, n_surfel=200)
        _keep_imu(P, slice(0, n))
        expect["n"] = n
    elif name == "imu_shuffled_dups":
        P = _base(206, 1.5)
        n = len(P["t_imu"])
        dup = rng.choice(n, size=n // 20, replace=False)            # 5 % of the rows take the stamp of ANOTHER row and keep their own gyro / acc values
        P["t_imu"] = P["t_imu"].copy()
        P["t_imu"][dup] = P["t_imu"][(dup + 7) % n]
        p = rng.permutation(n)
        _keep_imu(P, p)
    elif name == "imu_on_knots":
        P = _base(207, 1.5)
        ks = np.arange(20, 60)
        on = P["t0"] + P["dt"] * ks                                 # t0 + dt * k in two roundings, as the host forms a segment's origin (madd_2r)
        cand = np.concatenate([on, np.nextafter(on, np.inf), np.nextafter(on, -np.inf), [P["t0"], np.nextafter(max_time(P), -np.inf)]])
        ok = _oracle_accepts_imu_rows(P, cand)
        special = cand[ok]
        n0 = len(P["t_imu"])
        t = np.concatenate([P["t_imu"], special])
        src = np.concatenate([np.arange(n0), rng.integers(0, n0, len(special))])
        p = np.argsort(t, kind="stable")
        P["gyro"], P["acc"], P["t_imu"] = P["gyro"][src][p], P["acc"][src][p], t[p]
        expect["aligned"] = special
        expect["dropped"] = int((~ok).sum())
    elif name.startswith("imu_tau_"):
        P = _base(208, 1.5)
        sign = -1.0 if name.endswith("_neg") else 1.0
        if name.startswith("imu_tau_inside"):
            last = P["n_knots"] - 4
            ks = np.repeat(np.arange(10, last + 1), 6)
            _set_imu_times(P, _in_interval(P, ks, rng.uniform(0.4, 0.6, len(ks))))   # the middle 20 % of every interval: t + tau stays inside it
        expect["tau_imu"] = True
        expect["tau"] = 1.5 * DT if name == "imu_tau_ge_dt" else sign * 0.3 * DT
        expect["oracle_raises"] = TAU_ORACLE_RAISES[name]
    elif name == "surf_burst":
        P = _base(209, 2.0, n_surfel=2200)
        kb, nb = 40, 2050
        k = interval(P, P["surf_t"])
        rest = np.flatnonzero((k < kb - 1) | (k > kb + 1))[::14]     # a sparse remainder
        src = np.concatenate([rest, rng.integers(0, len(k), nb)])
        t = np.concatenate([P["surf_t"][rest], _in_interval(P, kb, rng.uniform(0.0, 1.0, nb) * 0.98 + 0.01)])
        p = np.argsort(t, kind="stable")
        P["surf_pt"], P["surf_plane"], P["surf_t"] = P["surf_pt"][src][p], P["surf_plane"][src][p], t[p]
        expect["burst"] = kb
    elif name == "surf_ends":
        P = _base(210, 1.5, n_surfel=600)
        km, last = int(interval(P, P["t_map"])), P["n_knots"] - 4
        head = np.concatenate([P["t_map"] + rng.uniform(1e-4, (km + 1) * DT + P["t0"] - P["t_map"] - 1e-4, 150), _in_interval(P, km + 1, rng.uniform(0.01, 0.99, 150))])
        tail = _in_interval(P, last, rng.uniform(0.01, 0.99, 300))
        _set_surf_times(P, np.sort(np.concatenate([head, tail])))
        expect["hub"], expect["last"] = km, last
    elif name.startswith("surf_counts_"):
        n = int(name.rsplit("_", 1)[1])
        P = _base(211, 1.5, n_surfel=600)
        _set_surf_times(P, np.sort(rng.uniform(P["t_map"] + 1e-3, max_time(P) - 1e-3, n)))
        expect["n"] = n
    elif name == "surf_shuffled_dups":
        P = _base(212, 1.5, n_surfel=700, n_planes=9)
        n = len(P["surf_t"])
        dup = rng.choice(n, size=n // 20, replace=False)
        P["surf_t"] = P["surf_t"].copy(); P["surf_plane"] = P["surf_plane"].copy()
        P["surf_t"][dup] = P["surf_t"][(dup + 11) % n]
        P["surf_plane"][dup] = (P["surf_plane"][(dup + 11) % n] + 1) % 9     # same stamp, another plane
        p = rng.permutation(n)
        for k_ in ("surf_t", "surf_pt", "surf_plane"):
            P[k_] = P[k_][p]
        expect["dup_rows"] = int(len(dup))
    elif name == "rep_shuffled_unused":
        P = _base(213, 2.0, n_landmarks=30, views_per_lm=4)
        lm, uv, t0 = P["rep_lm"], P["rep_uv"], P["rep_t0"]
        cnt = np.bincount(lm, minlength=30)
        unused, single, twice = [3, 11, 29], 5, 7
        assert cnt[single] >= 2 and cnt[twice] >= 3
        keep = ~np.isin(lm, unused)
        rows5 = np.flatnonzero(lm == single)
        keep[rows5] = False; keep[rows5[1]] = True                   # one view left, and not the reference observation itself
        rows7 = np.flatnonzero(lm == twice)
        lm = np.concatenate([lm[keep], [twice]]).astype(np.int32)      # a second observation in the frame of the landmark's third view, a few pixels away
        uv = np.concatenate([uv[keep], [uv[rows7[2]] + np.array([3.0, -2.0])]])
        t0 = np.concatenate([t0[keep], [t0[rows7[2]]]])
        p = rng.permutation(len(lm))
        P["rep_lm"], P["rep_uv"], P["rep_t0"] = lm[p], uv[p], t0[p]
        expect.update(unused=unused, single=single, twice=twice, twice_frame=float(t0[-1]))
    else:
        raise KeyError(name)
    state = P["state0"].copy()
    if expect["tau_imu"]:
        state[tau_imu_slot(P)] = expect["tau"]
    return P, state, TAU, expect


def hash_name(name):
    """A seed from the case name that does not depend on PYTHONHASHSEED."""
    h = 0
    for c in name.encode():
        h = (h * 131 + c) % (1 << 31)
    return h
