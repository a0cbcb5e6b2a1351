"""The Ceres seam at config 4 (synth.make_bench_problem(seed=4)): both routes of lvi-exc_amd/host/lvx_ceres_shim.hpp — the 64-wide debug rows
(LVX_EVAL_JACOBIAN, per-segment kernels, pageable copies) and the per-block records (LVX_EVAL_JACOBIAN_BLOCKS, fused kernels, pinned copies behind
each family's last kernel) — each timed as evaluate / exposed copy / host scatter of every block through LvxRowBlock::Evaluate, plus the pass without
either bit and the pinned device -> host rate of one large hipMemcpyAsync in the same run.  Prints one JSON line.

    python tools/ceres_seam_bench.py [--reps 10] [--warmup 2] [--seed 4]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lvi-exc_amd"))
import lvx  # noqa: E402
import synth  # noqa: E402


def driver():
    import build as lvx_build
    lvx_build.build()
    src, so = os.path.join(ROOT, "tools", "ceres_seam_driver.cpp"), os.path.join(ROOT, "tools", "libceres_seam_driver.so")
    deps = [src, os.path.join(ROOT, "lvi-exc_amd", "host", "lvx_ceres_shim.hpp"), os.path.join(ROOT, "include", "lvx.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests", "native", "mock_ceres"), "-I" + os.path.join(ROOT, "lvi-exc_amd", "host"),
                               "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-o", so, "-L" + os.path.join(ROOT, "lvi-exc_amd"), "-llvx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "lvi-exc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lib = C.CDLL(so)
    lib.seam_create.restype = C.c_void_p
    lib.seam_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.seam_blocks.argtypes = [C.c_void_p, C.c_void_p]
    lib.seam_destroy.argtypes = [C.c_void_p]
    lib.seam_pinned_d2h_gbs.restype = C.c_double
    lib.seam_pinned_d2h_gbs.argtypes = [C.c_size_t]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=4)
    a = ap.parse_args()
    lib = driver()
    P = synth.make_bench_problem(seed=a.seed)
    locks = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
    g = lvx.Context(0)
    lvx.load_problem(g, P, locks)
    lo = g.layout()
    d = lambda x: np.ascontiguousarray(x, np.float64)
    i = lambda x: np.ascontiguousarray(x, np.int32)
    keep = [d(P["t_imu"]), d(P["surf_t"]), i(P["rep_lm"]), d(P["rep_t0"]), d(P["lm_t0"]), i(P["cs_lm"])]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    h = lib.seam_create(C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(P["n_knots"]), C.c_int(P["n_landmarks"]), C.c_double(P["camera"]["readout"]), C.c_uint(locks),
                        C.c_int(len(keep[0])), p(keep[0]), C.c_int(0), C.c_double(0.0), C.c_int(len(keep[1])), p(keep[1]), C.c_double(P["t_map"]),
                        C.c_int(len(keep[2])), p(keep[2]), p(keep[3]), p(keep[4]), C.c_int(len(keep[5])), p(keep[5]))
    skipped = C.c_int(0)
    nblk = lib.seam_blocks(h, C.byref(skipped))
    state = d(P["state0"])
    out = {"config": "make_bench_problem(seed=%d)" % a.seed, "n_blocks": int(lo["n_blocks"]), "n_residuals": int(lo["n_residuals"]), "shim_blocks": nblk, "shim_blocks_skipped": skipped.value,
           "reps": a.reps}
    # the pass without either bit (cost + residuals on the host), same state
    for _ in range(a.warmup):
        g.evaluate(state)
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter(); g.evaluate(state); ts.append((time.perf_counter() - t) * 1e3)
    out["pass_ms_without_bit"] = float(np.median(ts))
    for name, blocks in (("blocks", 1), ("debug_rows", 0)):
        o = (C.c_double * 4)()
        rows = []
        for r in range(a.warmup + a.reps):
            rc = lib.seam_run(h, g._h, p(state), blocks, o)
            if rc != 0:
                raise RuntimeError("seam_run(%s) = %d: %s" % (name, rc, g._l.lvx_last_error(g._h).decode()))
            if r >= a.warmup:
                rows.append(list(o))
        m = np.median(np.array(rows), axis=0)
        # rows_on_host_ms: from the call to the rows on the host (the pass, the residual read-back, the copies); bytes / that time is a LOWER bound on the copy rate
        out[name] = {"evaluate_ms": m[0], "exposed_copy_ms": m[1], "rows_on_host_ms": m[0] + m[1], "scatter_ms": m[2], "end_to_end_ms": m[0] + m[1] + m[2], "d2h_bytes": int(m[3]),
                     "copy_gbs_lower_bound": m[3] / (m[0] + m[1]) / 1e6}
    out["pinned_d2h_gbs"] = lib.seam_pinned_d2h_gbs(1 << 30)
    out["blocks"]["copy_lower_bound_fraction_of_pinned_rate"] = out["blocks"]["copy_gbs_lower_bound"] / out["pinned_d2h_gbs"]
    # kernel time of the pass with and without the bit: the sum of the per-launch event timings (lvx_set_profiling; launches on the side streams overlap, so this
    # is the sum of kernel durations, not the critical path)
    for name, kw in (("without_bit", {}), ("with_bit", {"jac_blocks": True})):
        g.set_profiling(True)
        g.kernel_ms()
        ks = []
        for _ in range(a.reps):
            g.evaluate(state, residuals=False, **kw)
            ms, _n = g.kernel_ms()
            ks.append(float(np.sum(ms)))
        g.set_profiling(False)
        out["kernel_ms_sum_" + name] = float(np.median(ks))
    out["kernel_time_ratio"] = out["kernel_ms_sum_with_bit"] / out["kernel_ms_sum_without_bit"]
    out["speedup_end_to_end"] = out["debug_rows"]["end_to_end_ms"] / out["blocks"]["end_to_end_ms"]
    out["scatter_ratio"] = out["blocks"]["scatter_ms"] / out["debug_rows"]["scatter_ms"]
    lib.seam_destroy(h)
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
