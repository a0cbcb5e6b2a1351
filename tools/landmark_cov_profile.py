"""Cost of lvx_landmark_covariance at bench config 4 against its yardstick, lvx_trajectory_covariance with ONE query at the same lowest band position on the same build:
python tools/landmark_cov_profile.py [repetitions]   ->   profiles/landmark_cov_profile.json

Host clock around each call (all end in a synchronise), `repetitions` (20) alternating repetitions, median (min - max).  Two pairs: every landmark (var_rho, sigma_rho,
point, point_cov; the window arrays, 8 KB per landmark, are left out) against one spline-frame pose query in the first knot interval any landmark's row reaches; the 100
landmarks with the latest reference frames against one query in the first interval THEIR rows reach.  Both sides of a pair run the same factorisation and the same back
sweep down to the same panel — the yardstick's code is the code of the parent commit — so the ratio is the price of the wide band store and of k_landmark_cov.  No
threshold is set here."""
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


def first_knot(P, ids):
    """the first knot interval a row of the landmarks `ids` reaches: the earlier of the reference and the observation stamps, less the 1 ms margin of the spans"""
    first = P["lm_t0"].copy()
    np.minimum.at(first, P["rep_lm"], P["rep_t0"])
    return int(np.floor((first[ids].min() - 1e-3 - P["t0"]) / P["dt"]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    P = synth.make_bench_problem(seed=4)
    g = lvx.Context(0)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    t0, dt, L = P["t0"], P["dt"], P["n_landmarks"]
    every = np.arange(L, dtype=np.int32)
    late = np.argsort(P["lm_t0"], kind="stable")[-100:].astype(np.int32)
    t_all = t0 + (first_knot(P, every) + 0.5) * dt
    t_late = t0 + (first_knot(P, late) + 0.5) * dt
    calls = {"landmark_covariance_all": lambda: g.landmark_covariance(1e8, window=False),
             "trajectory_covariance_1_at_all": lambda: g.trajectory_covariance([t_all], lvx.FRAME_TRAJECTORY, 1e8),
             "landmark_covariance_late100": lambda: g.landmark_covariance(1e8, ids=late, window=False),
             "trajectory_covariance_1_at_late100": lambda: g.trajectory_covariance([t_late], lvx.FRAME_TRAJECTORY, 1e8)}
    for f in calls.values():   # warm-up: allocations
        f()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            a = time.perf_counter(); f(); times[k].append(time.perf_counter() - a)
    lo = g.layout()
    r = g.landmark_covariance(1e8, window=False)
    rho = P["state0"][7 * P["n_knots"] + 32:7 * P["n_knots"] + 32 + L]
    rel = r["sigma_rho"][r["valid"]] / np.abs(rho[r["valid"]])
    out = dict(problem="bench config 4 (synth.make_bench_problem(seed=4))", n_knots=int(P["n_knots"]), n_landmarks=int(L), n_band=int(lo["n_band"]), bandwidth=int(lo["bandwidth"]),
               n_border=int(lo["n_border"]), lm_row_width=int(lo["lm_row_width"]), repetitions=reps, query_t_all=float(t_all), query_t_late100=float(t_late),
               **{k: stats(v) for k, v in times.items()})
    out["ratio_all"] = out["landmark_covariance_all"]["median_ms"] / out["trajectory_covariance_1_at_all"]["median_ms"]
    out["ratio_late100"] = out["landmark_covariance_late100"]["median_ms"] / out["trajectory_covariance_1_at_late100"]["median_ms"]
    out["n_valid"] = int(r["valid"].sum())
    out["relative_depth_sigma"] = dict(median=float(np.median(rel)), worst=float(rel.max()))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "landmark_cov_profile.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
