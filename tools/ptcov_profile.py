"""Kernel time of lvx_map_point_covariance per point against its yardstick, the parent's k_pose_cov per query, in ONE process:
python tools/ptcov_profile.py [repetitions]   ->   profiles/ptcov_profile.json

The project's kernel timers (lvx_set_profiling: a HIP event pair around the launches of one kernel id) around
  LVX_KERNEL_POINT_COV   k_pt_hub + k_point_cov of lvx_map_point_covariance_xyzi_d, at one refinement round's map (57 scans x 7 200 points, each scan's points in time
                         order over its 0.1 s sweep) and at 4 M points (the same sweeps repeated), point / cov / sigma / sigma_max written;
  LVX_KERNEL_POSE_COV    k_pose_cov of lvx_trajectory_covariance_d (LiDAR frame, cov and sigma written) at 65 536 queries spread over the same span.
The point kernel is timed twice: the MFMA tiles (the default) and the plain per-lane product (switch PTCOV_VALU), so that DESIGN.md can state both.
The selected inverse in front of either is the same code and is not part of either record.  One warm-up call per shape, then `repetitions` (5) rounds alternating the
five; median (min - max) of the per-launch kernel time.  The 5.7 s problem (a knot every 0.02 s) stands in for the sequence the scans belong to; the kernels' time
does not depend on the band.  The one condition (asserted by the tool's exit status): time per point below time per k_pose_cov query in this run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402

import lvx     # noqa: E402
import synth   # noqa: E402

SCANS, PER_SCAN, BIG, QUERIES = 57, 7200, 4_000_000, 65536


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    P = synth.make_problem(seed=21, duration=5.7 + 0.2, n_surfel=500, n_planes=8, n_landmarks=20, n_camsurf=5)
    g = lvx.Context(0)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    t_scan = P["t0"] + 0.05 + 0.1 * np.arange(SCANS)[:, None] + (0.1 / PER_SCAN) * np.arange(PER_SCAN)[None, :]
    t_map = t_scan.reshape(-1)
    n_map = len(t_map)
    t_big = np.tile(t_map, BIG // n_map + 1)[:BIG]

    def points(n):
        x = rng.uniform(-30, 30, (n, 4)).astype(np.float32)
        return torch.from_numpy(x).to(dev)

    def outputs(n):
        return dict(point=torch.zeros((n, 3), dtype=torch.float64, device=dev), cov=torch.zeros((n, 9), dtype=torch.float64, device=dev),
                    sigma=torch.zeros((n, 3), dtype=torch.float64, device=dev), sigma_max=torch.zeros((n,), dtype=torch.float64, device=dev)), torch.zeros((n,), dtype=torch.uint8, device=dev)
    shapes = {}
    for key, t in (("map_57x7200", t_map), ("points_4M", t_big)):
        o, valid = outputs(len(t))
        shapes[key] = (points(len(t)), torch.from_numpy(t).to(dev), o, valid, len(t))
    tq = torch.from_numpy(np.sort(rng.uniform(t_map[0], t_map[-1], QUERIES))).to(dev)
    qo = dict(cov=torch.zeros((QUERIES, 36), dtype=torch.float64, device=dev), sigma=torch.zeros((QUERIES, 6), dtype=torch.float64, device=dev))
    qv = torch.zeros((QUERIES,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run_points(key):
        x, t, o, valid, n = shapes[key]
        g.map_point_covariance_d(x.data_ptr(), t.data_ptr(), n, {k: v.data_ptr() for k, v in o.items()}, valid.data_ptr(), xyzi=True)
        g.synchronize()

    def run_queries():
        g.trajectory_covariance_d(tq.data_ptr(), QUERIES, {k: v.data_ptr() for k, v in qo.items()}, qv.data_ptr(), lvx.FRAME_LIDAR)
        g.synchronize()

    def run_points_valu(key):   # the plain per-lane product (switch PTCOV_VALU) in place of the MFMA tiles
        g.set_switch("PTCOV_VALU", 1)
        run_points(key)
        g.set_switch("PTCOV_VALU", 0)
    calls = {"map_57x7200": (lambda: run_points("map_57x7200"), lvx.KERNEL_POINT_COV), "points_4M": (lambda: run_points("points_4M"), lvx.KERNEL_POINT_COV),
             "map_57x7200_valu": (lambda: run_points_valu("map_57x7200"), lvx.KERNEL_POINT_COV), "points_4M_valu": (lambda: run_points_valu("points_4M"), lvx.KERNEL_POINT_COV),
             "pose_cov_65536": (run_queries, lvx.KERNEL_POSE_COV)}
    run_points_valu("map_57x7200")
    cov_valu = shapes["map_57x7200"][2]["cov"].clone()
    run_points("map_57x7200")
    cov_mfma = shapes["map_57x7200"][2]["cov"]
    # the two formulations differ in the order of the sums only.  A point measured within rounding of t_map has cov = 0 + cancellation noise of 1e-19 m^2 in either, so
    # the difference is taken against the trace with a floor of (1 um)^2
    scale = torch.clamp(torch.abs(cov_mfma[:, 0:1]) + torch.abs(cov_mfma[:, 4:5]) + torch.abs(cov_mfma[:, 8:9]), min=1e-12)
    valu_vs_mfma = float((torch.abs(cov_valu - cov_mfma) / scale).max().item())
    for f, _ in calls.values():   # warm-up: code objects, allocations
        f()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, (f, kid) in calls.items():
            g.set_profiling(True, only=kid)
            g.kernel_ms_ext()
            f()
            m, n = g.kernel_ms_ext()
            g.set_profiling(False)
            assert n[kid] == 1
            ms[k].append(m[kid])
    n_valid = {k: int(shapes[k][3].sum().item()) for k in shapes}
    assert n_valid["map_57x7200"] == n_map and n_valid["points_4M"] == BIG and int(qv.sum().item()) == QUERIES
    lo = g.layout()
    out = dict(problem="synth.make_problem(seed=21, duration=5.9, n_surfel=500, n_planes=8, n_landmarks=20, n_camsurf=5)", n_knots=int(P["n_knots"]), n_band=int(lo["n_band"]),
               bandwidth=int(lo["bandwidth"]), n_border=int(lo["n_border"]), repetitions=reps, **{k: stats(v) for k, v in ms.items()})
    sizes = {"map_57x7200": n_map, "points_4M": BIG, "map_57x7200_valu": n_map, "points_4M_valu": BIG, "pose_cov_65536": QUERIES}
    out["valu_vs_mfma_max_cov_difference_of_trace_floor_1um2"] = valu_vs_mfma
    for k, n in sizes.items():
        out[k]["n"] = n
        out[k]["ns_per_item"] = 1e6 * out[k]["median_ms"] / n
        out[k]["items_per_s"] = n / (1e-3 * out[k]["median_ms"])
    out["sigma_max_mm"] = dict(median=float(1e3 * shapes["map_57x7200"][2]["sigma_max"].median().item()), worst=float(1e3 * shapes["map_57x7200"][2]["sigma_max"].max().item()))
    out["point_over_query"] = {k: out[k]["ns_per_item"] / out["pose_cov_65536"]["ns_per_item"] for k in ("map_57x7200", "points_4M")}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ptcov_profile.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    g.close()
    return 0 if max(out["point_over_query"].values()) < 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
