"""Time the rotation initialisation on an MI355X: lvx_estimate_rotation_d at 60 and 5 000 odometry poses x 1 and 41 shifts, on the reference's prefix schedule
(30, 40, ... <= n), and the blocking lvx_estimate_rotation beside it.

    python tools/rotinit_profile.py [--steps 30] [--warmup 5] [--out profiles/rotinit.json]

  _d: HIP events around the enqueue (the two kernels k_rot_pairs and k_rot_solve) on the context's stream, median of --steps after warm-up.
  blocking: wall time of the call (five uploads, two kernels, three downloads, one host stop)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lvi-exc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import lvx
    import synth
    N, t0, dt = 25023 + 4, 100.0, 0.02   # 500 s: 5 000 poses at 10 Hz
    rng = np.random.default_rng(4)
    r3, so3 = synth.make_trajectory(N, t0, dt, rng)
    state = synth.pack_state(r3, so3, synth.imu_block(), synth.sensor_block([0, 0, 0, 1.0], [0, 0, 0]), synth.sensor_block([0, 0, 0, 1.0], [0, 0, 0]), ())
    g = lvx.Context(0)
    g.set_spline(t0, dt, N)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    s_d = torch.from_numpy(state).to(dev)
    res = dict(n_knots=N, steps=a.steps)
    for n in (60, 5000):
        t = t0 + 0.05 + 0.1 * np.arange(n)
        q = rng.standard_normal((n, 4))
        pl = np.arange(30, n + 1, 10, dtype=np.int32)
        for n_tau in (1, 41):
            tau = np.linspace(-0.02, 0.02, n_tau) if n_tau > 1 else np.zeros(1)
            with torch.cuda.stream(stream):
                t_d, q_d, pl_d, tau_d = (torch.from_numpy(x).to(dev) for x in (t, q, pl, tau))
                res_d = torch.empty((n_tau * len(pl) * 80,), dtype=torch.uint8, device=dev)
                first_d = torch.empty((n_tau,), dtype=torch.int32, device=dev)
            stream.synchronize()
            ev = []
            with torch.cuda.stream(stream):
                for k in range(a.warmup + a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    lvx.estimate_rotation_d(g, t_d.data_ptr(), q_d.data_ptr(), n, res_d.data_ptr(), first_d.data_ptr(), pl_d.data_ptr(), len(pl), tau_d.data_ptr(), n_tau, None, s_d.data_ptr())
                    e1.record(stream)
                    e1.synchronize()
                    if k >= a.warmup:
                        ev.append(e0.elapsed_time(e1))
            g.synchronize()
            wall = []
            for k in range(a.warmup + a.steps):
                w0 = time.perf_counter()
                lvx.estimate_rotation(g, state, t, q, pl, tau)
                if k >= a.warmup:
                    wall.append((time.perf_counter() - w0) * 1e3)
            key = "poses_%d_shifts_%d" % (n, n_tau)
            res[key] = dict(n_prefix=int(len(pl)), event_ms=dict(median=float(np.median(ev)), min=float(np.min(ev)), max=float(np.max(ev))),
                            blocking_wall_ms=dict(median=float(np.median(wall)), min=float(np.min(wall)), max=float(np.max(wall))))
            print(key, json.dumps(res[key]))
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
