"""Kernel time of lvx_projection_covariance against its yardstick, lvx_render_map_d on the same cloud, in ONE process:
python tools/projcov_profile.py [repetitions]   ->   profiles/projcov_profile.json

The project's kernel timers (lvx_set_profiling: a HIP event pair around the launches of one kernel id) around
  LVX_KERNEL_PROJ_HUB   k_proj_poses + k_proj_hub (a wavefront per image),
  LVX_KERNEL_PROJ_COV   k_proj_cov (a lane per point; uv, cov, sigma, sigma_max, image and status written: 16 B in, 76 B + the status byte = 77 B out per point),
  LVX_KERNEL_UPSTREAM   k_render_poses + k_render_map of lvx_render_map_d on the same cloud, images and times (16 B in, 16 B out per point, one byte gathered),
at one refinement round's map (57 scans x 7 200 points) and at 4 M points, with 1 and with 32 images; beside them the existing queries in the same process:
  LVX_KERNEL_POSE_COV   k_pose_cov of lvx_trajectory_covariance_d at 65 536 queries,   LVX_KERNEL_POINT_COV   lvx_map_point_covariance_xyzi_d at the 57 x 7 200 map,
and the wall time of lvx_landmark_covariance (no timer id of its own).  The selected inverse in front of every query is the same code and is not part of any record.
One warm-up call per shape, then `repetitions` (5) rounds alternating all of them; median (min - max) of the per-launch kernel time and the achieved bytes/s.
The cloud: points spread through the frustum of the image at t_map + 1 s and around it (about half project, the rest are skipped or outside), so the decision chain
takes all its exits.  The 5.7 s problem (a knot every 0.02 s) stands in for the sequence the scans belong to."""
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

SCANS, PER_SCAN, BIG, QUERIES = 57, 7200, 4_000_000, 65536
BYTES_PROJ, BYTES_RENDER = 16 + 77, 16 + 16


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    P = synth.make_problem(seed=21, duration=5.7 + 0.2, n_surfel=500, n_planes=8, n_landmarks=20, n_camsurf=5)
    cam = P["camera"]
    g = lvx.Context(0)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    x = P["state0"]
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n_map = SCANS * PER_SCAN
    # points in the camera frame of the first image, half of them inside its frustum, carried into the LiDAR frame at t_map
    t_img = {1: np.array([P["t_map"] + 1.0]), 32: P["t_map"] + 1.0 + 0.1 * np.arange(32)}
    qc, pc, ok = lvx.eval_camera_pose(g, x, t_img[1])
    ql, pl, okl = lvx.eval_lidar_pose(g, x, [P["t_map"]])
    assert ok[0] and okl[0]

    def cloud(n):
        z = rng.uniform(-3.0, 18.0, n)
        s = rng.uniform(-1.6, 1.6, (n, 2))
        ptc = np.stack([s[:, 0] * z, s[:, 1] * z, z], axis=1)
        ptg = synth.qrot(np.broadcast_to(qc[0], (n, 4)), ptc) + pc[0]
        qli = np.array([-ql[0][0], -ql[0][1], -ql[0][2], ql[0][3]])
        out = np.zeros((n, 4), np.float32)
        out[:, :3] = synth.qrot(np.broadcast_to(qli, (n, 4)), ptg - pl[0])
        return torch.from_numpy(out).to(dev)
    clouds = {"map_57x7200": cloud(n_map), "points_4M": cloud(BIG)}
    images = {k: torch.zeros((k, cam["rows"], cam["cols"]), dtype=torch.uint8, device=dev) for k in (1, 32)}
    times_d = {k: torch.from_numpy(v).to(dev) for k, v in t_img.items()}

    def outputs(n, ni):
        o = dict(uv=torch.zeros((n, 2), dtype=torch.float64, device=dev), cov=torch.zeros((n, 4), dtype=torch.float64, device=dev), sigma=torch.zeros((n, 2), dtype=torch.float64, device=dev),
                 sigma_max=torch.zeros((n,), dtype=torch.float64, device=dev), image=torch.zeros((n,), dtype=torch.int32, device=dev))
        return o, torch.zeros((n,), dtype=torch.uint8, device=dev), dict(pose_cov=torch.zeros((ni, 144), dtype=torch.float64, device=dev)), torch.zeros((ni,), dtype=torch.int32, device=dev)
    bufs = {(k, ni): outputs(len(c), ni) for k, c in clouds.items() for ni in (1, 32)}
    rec = {k: torch.zeros((len(c) * 16,), dtype=torch.uint8, device=dev) for k, c in clouds.items()}
    tq = torch.from_numpy(np.sort(rng.uniform(P["t_map"], P["t_map"] + 5.6, QUERIES))).to(dev)
    qo = dict(cov=torch.zeros((QUERIES, 36), dtype=torch.float64, device=dev), sigma=torch.zeros((QUERIES, 6), dtype=torch.float64, device=dev))
    qv = torch.zeros((QUERIES,), dtype=torch.uint8, device=dev)
    t_pts = torch.from_numpy((P["t_map"] + 0.1 * np.arange(SCANS)[:, None] + (0.1 / PER_SCAN) * np.arange(PER_SCAN)[None, :]).reshape(-1)).to(dev)
    po = dict(cov=torch.zeros((n_map, 9), dtype=torch.float64, device=dev), sigma_max=torch.zeros((n_map,), dtype=torch.float64, device=dev))
    pv = torch.zeros((n_map,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run_proj(k, ni):
        o, st, im, iv = bufs[(k, ni)]
        g.projection_covariance_d(clouds[k].data_ptr(), len(clouds[k]), times_d[ni].data_ptr(), ni, {a: b.data_ptr() for a, b in im.items()}, iv.data_ptr(),
                                  {a: b.data_ptr() for a, b in o.items()}, st.data_ptr())
        g.synchronize()

    def run_render(k, ni):
        lvx.render_map_d(g, x, P["t_map"], images[ni].data_ptr(), ni, cam["cols"], t_img[ni], rec[k].data_ptr(), map_d_ptr=clouds[k].data_ptr(), n=len(clouds[k]))

    def run_queries():
        g.trajectory_covariance_d(tq.data_ptr(), QUERIES, {a: b.data_ptr() for a, b in qo.items()}, qv.data_ptr(), lvx.FRAME_LIDAR)
        g.synchronize()

    def run_points():
        g.map_point_covariance_d(clouds["map_57x7200"].data_ptr(), t_pts.data_ptr(), n_map, {a: b.data_ptr() for a, b in po.items()}, pv.data_ptr(), xyzi=True)
        g.synchronize()
    calls = {}
    for k in clouds:
        for ni in (1, 32):
            calls["proj_hub_%s_%d" % (k, ni)] = (lambda k=k, ni=ni: run_proj(k, ni), lvx.KERNEL_PROJ_HUB, ni, 0)
            calls["proj_cov_%s_%d" % (k, ni)] = (lambda k=k, ni=ni: run_proj(k, ni), lvx.KERNEL_PROJ_COV, len(clouds[k]), BYTES_PROJ)
            calls["render_%s_%d" % (k, ni)] = (lambda k=k, ni=ni: run_render(k, ni), lvx.KERNEL_UPSTREAM, len(clouds[k]), BYTES_RENDER)
    calls["pose_cov_65536"] = (run_queries, lvx.KERNEL_POSE_COV, QUERIES, 0)
    calls["point_cov_57x7200"] = (run_points, lvx.KERNEL_POINT_COV, n_map, 0)
    for f, _, _, _ in calls.values():   # warm-up: code objects, allocations
        f()
    ms = {k: [] for k in calls}
    wall_lm = []
    for _ in range(reps):
        for k, (f, kid, _, _) in calls.items():
            g.set_profiling(True, only=kid)
            g.kernel_ms_ext()
            f()
            m, n = g.kernel_ms_ext()
            g.set_profiling(False)
            assert n[kid] == 1, (k, n[kid])
            ms[k].append(m[kid])
        t0 = time.perf_counter()
        g.landmark_covariance(window=False)
        wall_lm.append(1e3 * (time.perf_counter() - t0))
    lo = g.layout()
    out = dict(problem="synth.make_problem(seed=21, duration=5.9, n_surfel=500, n_planes=8, n_landmarks=20, n_camsurf=5)", n_knots=int(P["n_knots"]), n_band=int(lo["n_band"]),
               bandwidth=int(lo["bandwidth"]), n_border=int(lo["n_border"]), repetitions=reps, landmark_covariance_wall=stats(wall_lm))
    for k, (_, _, n, nbytes) in calls.items():
        out[k] = stats(ms[k])
        out[k]["n"] = n
        out[k]["ns_per_item"] = 1e6 * out[k]["median_ms"] / n
        if nbytes:
            out[k]["bytes_per_s"] = n * nbytes / (1e-3 * out[k]["median_ms"])
    for k in clouds:
        for ni in (1, 32):
            st = bufs[(k, ni)][1]
            out["status_%s_%d" % (k, ni)] = [int((st == s).sum().item()) for s in (0, 1, 2)]
            out["proj_over_render_bytes_per_s_%s_%d" % (k, ni)] = out["proj_cov_%s_%d" % (k, ni)]["bytes_per_s"] / out["render_%s_%d" % (k, ni)]["bytes_per_s"]
    sm = bufs[("map_57x7200", 1)][0]["sigma_max"][bufs[("map_57x7200", 1)][1] == 2]
    out["sigma_max_px"] = dict(median=float(sm.median().item()), worst=float(sm.max().item()))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "projcov_profile.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    g.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
