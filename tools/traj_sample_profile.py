"""Time the trajectory queries on an MI355X: a spline of 25 023 control points (500 s at dt = 0.02: a 1.4 MB state), sorted stamps.

    python tools/traj_sample_profile.py [--steps 30] [--warmup 5] [--out profiles/traj_sample.json] [--small]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o stats -- python tools/traj_sample_profile.py --steps 10 --warmup 2     (a run of its own)

  lvx_sample_trajectory_d, all five fields, n = 200 000 and 4 000 000; lvx_predict_imu_d, n = 200 000: HIP events around the enqueue on the context's stream, median
  of --steps after warm-up, and the bytes moved (8 in + 128 out + 4 flag per sample for the full query; 8 + 48 + 4 for the IMU) over that time, against the ~6.3 TB/s
  achievable HBM figure of DESIGN.md 3.3.  4 M samples are 560 MB: written once, they do not fit the 256 MB Infinity Cache, the 1.4 MB state stays in L2.
  lvx_compare_poses, n = 5 000: wall time of the call (upload, one workgroup, one host stop).
  The pose-only LiDAR-frame query against lvx_evaluate_lidar_pose's kernel on the same 200 000 stamps, alternating the two in one process: both host-array calls, the
  kernel's own time from the context's launch events (lvx_set_profiling)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lvi-exc_amd"))
HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/100 of the sizes (checks the script, not a measurement)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import lvx
    import synth
    div = 100 if a.small else 1
    N, t0, dt = 25023 // div + 4, 100.0, 0.02
    rng = np.random.default_rng(4)
    r3, so3 = synth.make_trajectory(N, t0, dt, rng)
    state = synth.pack_state(r3, so3, synth.imu_block(0.02, -0.015, (0.05, 0.02, -0.03), (0.01, -0.02, 0.005)),
                             synth.sensor_block(synth.q_from_rpy(0.03, -0.05, 1.6), [0.05, -0.10, 0.12]), synth.sensor_block(synth.q_from_rpy(-1.57, 0.0, -1.57), [-0.22, 0.02, 0.22]), ())
    tmin, tmax = t0, t0 + (N - 3) * dt
    g = lvx.Context(0)
    g.set_spline(t0, dt, N)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    s_d = torch.from_numpy(state).to(dev)
    res = dict(n_knots=N, state_bytes=int(state.nbytes), steps=a.steps, hbm_achievable_TBps=HBM_ACHIEVABLE / 1e12)

    def timed(enqueue):
        ev = []
        with torch.cuda.stream(stream):
            for k in range(a.warmup + a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                enqueue()
                e1.record(stream)
                e1.synchronize()
                if k >= a.warmup:
                    ev.append(e0.elapsed_time(e1))
        g.synchronize()
        return ev

    def report(ev, n, bytes_per_sample):
        med = float(np.median(ev))
        return dict(n=n, event_ms=dict(median=med, min=float(np.min(ev)), max=float(np.max(ev))), bytes=int(n * bytes_per_sample), TBps=n * bytes_per_sample / (med * 1e-3) / 1e12,
                    fraction_of_achievable_hbm=n * bytes_per_sample / (med * 1e-3) / HBM_ACHIEVABLE, Msamples_per_s=n / (med * 1e-3) / 1e6)

    for n in (200000 // div, 4000000 // div):
        with torch.cuda.stream(stream):
            t_d = torch.from_numpy(np.sort(rng.uniform(tmin, tmax, n))).to(dev)
            out = {f: torch.empty((n, 4 if f == "orientation" else 3), dtype=torch.float64, device=dev) for f in lvx.TRAJ_FIELDS}
            valid = torch.empty((n,), dtype=torch.int32, device=dev)
        stream.synchronize()
        ptrs = {f: out[f].data_ptr() for f in out}
        res["sample_trajectory_d_all_fields_%d" % n] = report(timed(lambda: lvx.sample_trajectory_d(g, t_d.data_ptr(), n, ptrs, valid.data_ptr(), lvx.FRAME_TRAJECTORY, s_d.data_ptr())), n, 140)
        assert int(valid.sum().item()) == n
        if n == 200000 // div:
            gy, ac = out["velocity"], out["acceleration"]
            res["predict_imu_d_%d" % n] = report(timed(lambda: lvx.predict_imu_d(g, t_d.data_ptr(), n, gy.data_ptr(), ac.data_ptr(), valid.data_ptr(), s_d.data_ptr())), n, 60)
        del out, valid, t_d
    g.set_stream(None)

    # pose errors at 5 000 stamps: wall time of the host-array call
    n = 5000 // div
    t = np.sort(rng.uniform(tmin, tmax, n))
    q, p, ok = lvx.eval_lidar_pose(g, state, t)
    wall = []
    for k in range(a.warmup + a.steps):
        w0 = time.perf_counter()
        c = lvx.compare_poses(g, state, lvx.FRAME_LIDAR, t, q * 1.5, p + 0.01, lvx.ALIGN_FIRST)
        if k >= a.warmup:
            wall.append((time.perf_counter() - w0) * 1e3)
    assert c["n_valid"] == n
    res["compare_poses_%d" % n] = dict(n=n, wall_ms=dict(median=float(np.median(wall)), min=float(np.min(wall)), max=float(np.max(wall))))

    # the pose-only LiDAR-frame query against lvx_evaluate_lidar_pose's kernel: same stamps, alternating, the kernels' own launch events
    n = 200000 // div
    t = np.sort(rng.uniform(tmin, tmax, n))
    new_ms, old_ms = [], []
    g.set_profiling(True)
    for k in range(a.warmup + a.steps):
        for which in (0, 1):
            g.kernel_ms()   # (reads and clears the records)
            if which == 0:
                smp = lvx.sample_trajectory(g, state, t, lvx.FRAME_LIDAR, ("position", "orientation"))
            else:
                q, p, ok = lvx.eval_lidar_pose(g, state, t)
            ms, cnt = g.kernel_ms()
            i = lvx.KERNEL_NAMES.index("upstream")
            assert cnt[i] == 1
            if k >= a.warmup:
                (new_ms if which == 0 else old_ms).append(float(ms[i]))
    g.set_profiling(False)
    assert smp["position"].tobytes() == p.tobytes() and smp["orientation"].tobytes() == q.tobytes() and np.array_equal(smp["valid"], ok)
    st = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))   # noqa: E731
    res["pose_only_lidar_%d" % n] = dict(n=n, k_traj_sample_ms=st(new_ms), k_lidar_pose_ms=st(old_ms), ratio_of_medians=float(np.median(new_ms) / np.median(old_ms)))
    g.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
