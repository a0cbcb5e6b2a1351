"""Time the hand-off from a DataAssociation round to a laid-out evaluator, both routes in one process on an MI355X.

    python tools/handoff_profile.py [--reps 9] [--warmup 2] [--long 12] [--out profiles/handoff_profile.json] [--small]

  From the end of lvx_data_association to the return of the first lvx_get_layout after the hand-off (wall clock; both ends are host stops):
    host    lvx_get_surfel_map + lvx_get_surfel_points, every step-th point with t >= t_map picked on the host (numpy here, a loop in lvx_host::Calibrator),
            lvx_set_planes + lvx_set_surfel, lvx_get_layout
    device  lvx_set_surfel_from_association, lvx_get_layout
  alternating, a fresh association before every measurement (the fetched planes are cached per association), median of --reps after --warmup.
  Sizes: synth.make_sequence(seed=50) — 6 s, 57 scans, the refinement round of the README — and the same generator at --long seconds (default 12: the map cloud of
  the association stays below the 1 048 576 points up to which the voxel grid sorts with its own kernels — no larger association has been run through to its end).
  Bytes are counted from the shapes: 120 per plane record and 60 per SurfelPoint down, 24 per plane and 36 + 64 per used row up on the host route (the setter's
  arrays, then the layout's sorted copies, row-ordered plane copy and permutation); 16 + 4 (N + 1) down on the device route; the chunk tables go up on both.
  The device route's time is split into the call and the layout, and the layout is timed again with the IMU and reprojection families cleared: the difference is what
  the re-layout of families that did not change costs (layout_dirty is one flag for all of them)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lvi-exc_amd"))


def med(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def profile(lvx, synth, S, step, reps, warmup):
    g = lvx.Context(0)
    g.set_spline(S["t0"], S["dt"], S["n_knots"])
    c = S["camera"]
    g.set_camera(c["rows"], c["cols"], c["readout"], c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"], c["k3"])

    def others(on):
        if on:
            g.set_imu(S["t_imu"], S["gyro"], S["acc"], 28.0, 18.0)
            g.set_reproj(S["rep_lm"], S["rep_uv"], S["rep_t0"], 5.0, 1.0)
        else:
            g.set_imu(np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)), 28.0, 18.0)
            g.set_reproj(np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0), 5.0, 1.0)
    g.set_landmarks(S["lm_uv"], S["lm_t0"])
    others(True)
    g.set_locks(lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    raw = np.zeros(S["scans"].shape, dtype=lvx.POINT_XYZIT)
    for k in ("x", "y", "z", "timestamp"):
        raw[k] = S["scans"][k]
    lvx.set_scans(g, raw, S["H"], S["W"])
    x = np.ascontiguousarray(S["state_true"], np.float64)
    t_map = S["t_map"]
    ms = dict(host=[], device=[], device_call=[], device_layout=[], device_layout_surfel_only=[], association=[])
    n_used = {}
    for k in range(warmup + reps):
        for route in ("host", "device"):
            w = time.perf_counter()
            npl, npt = lvx.data_association(g, x, t_map)
            t_assoc = (time.perf_counter() - w) * 1e3
            w0 = time.perf_counter()
            if route == "host":
                planes, pts = lvx.get_surfel_map(g, npl), lvx.get_surfel_points(g, npt)
                idx = np.arange(0, npt, max(1, step))
                idx = idx[pts["t"][idx] >= t_map]
                g.set_planes(np.ascontiguousarray(planes["Pi"]))
                g.set_surfel(pts["pt"][idx], pts["t"][idx], pts["plane"][idx], t_map, 5.0, 10.0)
                n_used[route] = len(idx)
                w1 = w0
            else:
                n_used[route] = lvx.set_surfel_from_association(g, step, t_map, 5.0, 10.0)
                w1 = time.perf_counter()
            lo = g.layout()
            w2 = time.perf_counter()
            if k >= warmup:
                ms[route].append((w2 - w0) * 1e3); ms["association"].append(t_assoc)
                if route == "device":
                    ms["device_call"].append((w1 - w0) * 1e3); ms["device_layout"].append((w2 - w1) * 1e3)
            if route == "device":   # the same layout without the families that did not change
                others(False)
                w3 = time.perf_counter()
                g.layout()
                if k >= warmup:
                    ms["device_layout_surfel_only"].append((time.perf_counter() - w3) * 1e3)
                others(True)
    assert n_used["host"] == n_used["device"]
    n, N, P = n_used["device"], S["n_knots"], npl
    cost = g.evaluate(x, residuals=False)["cost"]
    g.close()
    n_chunk_ints = 3 * (n // 512 + 2) + 1
    b = dict(host_down=120 * P + 60 * npt, host_up=24 * P + 36 * n + 64 * n + 4 * n_chunk_ints, device_down=16 + 4 * (N + 1), device_up=4 * n_chunk_ints)
    r = dict(scans=len(S["scans"]), n_knots=N, planes=int(P), surfel_points=int(npt), step=step, rows_used=int(n), residual_rows=int(lo["n_residuals"]), cost_after=cost, bytes=b,
             ms={k: med(v) for k, v in ms.items()})
    d = r["ms"]
    r["speedup_of_medians"] = d["host"]["median"] / d["device"]["median"]
    r["unchanged_families_ms"] = d["device_layout"]["median"] - d["device_layout_surfel_only"]["median"]
    r["unchanged_families_share_of_device_route"] = r["unchanged_families_ms"] / d["device"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long", type=float, default=12.0, help="duration [s] of the large sequence (12 s = 117 scans = 842 k map points)")
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1.2 s and 2.4 s sequences (checks the script, not a measurement)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import lvx
    import synth
    res = {}
    for name, dur in (("refinement_round_57_scans", 1.2 if a.small else 6.0), ("long", 2.4 if a.small else a.long)):
        S = synth.make_sequence(seed=50, duration=dur)
        print("%s: %.1f s, %d scans, %d knots" % (name, dur, len(S["scans"]), S["n_knots"]), file=sys.stderr, flush=True)
        res[name] = dict(duration_s=dur, **profile(lvx, synth, S, a.step, a.reps, a.warmup))
        print(json.dumps({name: res[name]}), flush=True)
    print("| sequence | scans | SurfelPoints | rows used | host: MB down / up | host ms | device: bytes down / up | device ms (call + layout) | of which unchanged families |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, r in res.items():
        b, d = r["bytes"], r["ms"]
        print("| %s (%.0f s) | %d | %d | %d | %.2f / %.2f | %.2f | %d / %d | %.2f (%.2f + %.2f) | %.2f ms = %.0f %% |" % (
            name, r["duration_s"], r["scans"], r["surfel_points"], r["rows_used"], b["host_down"] / 1e6, b["host_up"] / 1e6, d["host"]["median"], b["device_down"], b["device_up"],
            d["device"]["median"], d["device_call"]["median"], d["device_layout"]["median"], r["unchanged_families_ms"], 100 * r["unchanged_families_share_of_device_route"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
