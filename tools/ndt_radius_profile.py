"""Time the NDT neighbour searches on an MI355X: one derivative evaluation (k_ndt_derivatives, score + gradient + Hessian) with each of KDTREE / DIRECT1 / DIRECT7 /
DIRECT26, the radius lookup alone (k_vx_radius), and lvx_ndt_align with the KDTREE search on the reference's demo beside the times its README publishes.

    python tools/ndt_radius_profile.py [--steps 30] [--warmup 5] [--out profiles/ndt_radius.json]

  demo   the two scans of tests/golden reduced at 0.1 m, resolution 1.0 (apps/align.cpp): 15 950 source points against 1 098 leaves
  raw    the raw target scan at the calibration's 0.5 m, every fourth point of the raw source: 17 448 points against 2 683 leaves
  align  lvx_ndt_align(search = 0) on the demo: wall time of the blocking call (upload, six evaluations, host bookkeeping) and the sum of its kernels

Kernel times are the context's own launch events (lvx_set_profiling on the upstream family), median of --steps after warm-up; the blocking calls' wall time stands
beside them.  Every step runs in a child process of its own under a time limit, one after the other; the first that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
STEPS = (("demo", 120), ("raw", 120), ("align", 120))      # (name, time limit in seconds)
SEARCHES = ((0, "KDTREE"), (1, "DIRECT1"), (7, "DIRECT7"), (26, "DIRECT26"))
README_ALIGN_MS = dict(kdtree_1_thread=207.7, kdtree_8_threads=55.0)      # the reference's README, pcl::NDT-style KDTREE rows


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def _clouds(step):
    from oracle import oracle as O
    gold = os.path.join(ROOT, "tests", "golden")
    tgt = np.load(os.path.join(gold, "ndt_data_251370668.npz"))["xyzi"]
    src = np.load(os.path.join(gold, "ndt_data_251371071.npz"))["xyzi"]
    if step == "raw":
        return tgt, np.ascontiguousarray(src[::4]), 0.5
    return O.voxelgrid_xyzi(tgt, 0.1), O.voxelgrid_xyzi(src, 0.1), 1.0


def run_step(step, steps, warmup):
    import lvx
    tgt, src, res = _clouds(step)
    g = lvx.Context(0)
    info = lvx.voxel_build(g, tgt, res, fetch=False)
    out = dict(n_target=int(len(tgt)), n_source=int(len(src)), resolution=res, n_leaves=int(info["n_leaves"]))
    g.set_profiling(True, only=lvx.KERNEL_UPSTREAM)

    def timed(call):
        ker, wall = [], []
        for k in range(warmup + steps):
            g.kernel_ms()                                   # reads and clears the records
            w0 = time.perf_counter()
            call()
            w = (time.perf_counter() - w0) * 1e3
            ms, _n = g.kernel_ms()
            if k >= warmup:
                ker.append(ms[lvx.KERNEL_UPSTREAM]); wall.append(w)
        return dict(kernel_ms=_stats(ker), blocking_wall_ms=_stats(wall))

    if step in ("demo", "raw"):
        p6 = np.zeros(6)
        for search, name in SEARCHES:
            out["derivatives_" + name] = timed(lambda: lvx.ndt_derivatives(g, src, src, p6, search=search))
        out["radius_lookup"] = timed(lambda: lvx.voxel_radius_search(g, src, res))
        _ids, _d2, cnt = lvx.voxel_radius_search(g, src, res)
        out["neighbours"] = dict(mean=float(cnt.mean()), max=int(cnt.max()))
    else:
        r = lvx.ndt_align(g, src, search=0)
        out.update(iterations=int(r["iterations"]), n_evaluations=int(r["n_evaluations"]), fitness=float(lvx.ndt_fitness(g, src, r["final_transformation"], tgt)))
        out["align_KDTREE"] = timed(lambda: lvx.ndt_align(g, src, search=0))
        out["align_DIRECT7"] = timed(lambda: lvx.ndt_align(g, src, search=7))
        out["readme_ms"] = README_ALIGN_MS
    g.set_profiling(False)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(run_step(a.step, a.steps, a.warmup)))
        return 0
    res = dict(steps=a.steps, warmup=a.warmup)
    for name, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit of %d s: stopping" % (name, limit))
            return 1
        if p.returncode != 0:
            print("step %s failed with status %d: stopping\n%s" % (name, p.returncode, p.stderr[-2000:]))
            return 1
        res[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
