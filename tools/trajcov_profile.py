"""Cost of lvx_trajectory_covariance at bench config 4 against its yardstick, lvx_calibration_covariance on the same sequential factor (SOLVER_SEQ = 1):
python tools/trajcov_profile.py [repetitions]   ->   profiles/trajcov_profile.json

Host clock around each call (both end in a synchronise), `repetitions` (30) alternating repetitions, median (min - max).  Three figures: the yardstick, the new call
for 1 000 LiDAR-frame queries spread over the spline, the new call for 10 queries in the last second of the spline (the back sweep stops at the lowest band position a
query needs).  The yardstick is the same factorisation without the back sweep, so the ratio is the price of the sweep and the queries."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402

import lvx     # noqa: E402
import synth   # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    P = synth.make_bench_problem(seed=4)
    g = lvx.Context(0)
    g.set_switch("SOLVER_SEQ", 1)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    spread = np.linspace(t0, tmax, 1000, endpoint=False)
    tail = np.linspace(tmax - 1.0, tmax, 10, endpoint=False)
    calls = {"calibration_covariance_seq": lambda: g.calibration_covariance(1e8),
             "trajectory_covariance_1000": lambda: g.trajectory_covariance(spread, lvx.FRAME_LIDAR, 1e8),
             "trajectory_covariance_tail10": lambda: g.trajectory_covariance(tail, lvx.FRAME_LIDAR, 1e8)}
    for f in calls.values():   # warm-up: allocations
        f()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            a = time.perf_counter(); f(); times[k].append(time.perf_counter() - a)
    lo = g.layout()
    r = g.trajectory_covariance(spread, lvx.FRAME_LIDAR, 1e8)
    sp = np.linalg.norm(r["sigma"][:, :3], axis=1); sr = np.linalg.norm(r["sigma"][:, 3:], axis=1)
    out = dict(problem="bench config 4 (synth.make_bench_problem(seed=4))", n_knots=int(N), n_band=int(lo["n_band"]), bandwidth=int(lo["bandwidth"]), n_border=int(lo["n_border"]),
               repetitions=reps, **{k: stats(v) for k, v in times.items()})
    out["ratio_1000_to_yardstick"] = out["trajectory_covariance_1000"]["median_ms"] / out["calibration_covariance_seq"]["median_ms"]
    out["ratio_tail10_to_yardstick"] = out["trajectory_covariance_tail10"]["median_ms"] / out["calibration_covariance_seq"]["median_ms"]
    out["sigma_position_m"] = dict(median=float(np.median(sp)), worst=float(sp.max()), worst_t=float(spread[int(sp.argmax())]))
    out["sigma_rotation_rad"] = dict(median=float(np.median(sr)), worst=float(sr.max()), worst_t=float(spread[int(sr.argmax())]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "trajcov_profile.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
