"""Time the device-side error statistics (lvx_error_statistics_d) at config 4 (synth.make_bench_problem) against the route the library offered before it:
lvx_evaluate(COST | RESIDUALS) + the residual copy to the host + the numpy reduction to the same numbers.  Both in one process, after warm-up.

    python tools/error_stats_bench.py [--steps 50] [--warmup 5] [--out profiles/error_stats_config4.json] [--small]

The statistics call is timed with HIP events on the stream it runs on (the device time of its kernels and result copy) and with the wall clock (what a caller waits);
the old route with the wall clock (it is host work for the most part).  tools/error_stats_profile.sh runs this and the kernel trace."""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a 1/50 size problem (checks the script, not a measurement)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import lvx
    import synth
    P = synth.make_bench_problem(seed=4, n_imu=4000, n_surfel=20000, n_reproj=1000, n_planes=100) if a.small else synth.make_bench_problem(seed=4)
    g = lvx.Context(0)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    s = P["state0"]
    g.set_state(s)
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    fr = g.family_rows()
    w = [P["w_gyro"], P["w_acc"], 1.0, P["w_surf"], P["w_rep"], P["w_cs"]]
    nr = [3, 3, 1, 1, 2, 1]

    def old_route():
        r = g.evaluate(s)["residuals"]          # a whole pass with the residual rows, copied to the host
        out = []
        for f in range(6):
            e = r[fr[f]:fr[f + 1]].reshape(-1, nr[f]) / w[f]
            out.append((len(e), np.abs(e).sum(axis=0), e.sum(axis=0), (e * e).sum(axis=0), np.abs(e).max(axis=0) if len(e) else 0.0))
        return out

    def new_route():
        return g.error_statistics(None)

    for _ in range(a.warmup):
        new_route(); old_route()
    ev, wall_new = [], []
    with torch.cuda.stream(stream):
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t = time.perf_counter()
            st = new_route()
            wall_new.append((time.perf_counter() - t) * 1e3)
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
    wall_old = []
    for _ in range(max(3, a.steps // 5)):
        t = time.perf_counter()
        ref = old_route()
        wall_old.append((time.perf_counter() - t) * 1e3)
    # the two routes agree (the fused pass and the value-only pass differ in the last bits of a row)
    for f, name in enumerate(lvx.FAMILY_NAMES):
        if ref[f][0]:
            k = nr[f]
            assert st[name]["n_evaluated"] == ref[f][0]
            assert np.abs(st[name]["sum_abs"][:k] - ref[f][1]).max() <= 1e-9 * np.abs(ref[f][1]).max(), name
    lo = g.layout()
    res = dict(config="synth.make_bench_problem(seed=4)" + (" small" if a.small else ""), n_blocks=lo["n_blocks"], n_residuals=lo["n_residuals"], steps=a.steps,
               error_statistics_d_event_ms=dict(median=float(np.median(ev)), min=float(np.min(ev)), p90=float(np.percentile(ev, 90))),
               error_statistics_d_wall_ms=dict(median=float(np.median(wall_new)), min=float(np.min(wall_new))),
               evaluate_residuals_copy_numpy_wall_ms=dict(median=float(np.median(wall_old)), min=float(np.min(wall_old))),
               bytes_returned=int(8 * (6 * 16 + 2 + 3 * len(P["planes"]) + 3 * P["n_landmarks"])), bytes_old_route=int(8 * lo["n_residuals"]))
    g.set_stream(None)
    g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
