"""Time the two ways a recording's LiDAR scans reach the device, on an MI355X:

    python tools/vlp16_profile.py [--scans 600] [--packets 76] [--steps 10] [--warmup 3] [--out profiles/vlp16.json]

  records  lvx_set_scans of host-unpacked records ([scans][16][24 x packets] x 32 bytes): the upload alone — the host's unpacking is NOT counted
  packets  lvx_set_scans_vlp16 of the raw packets ([scans x packets] x 1206 bytes): upload, k_vlp16_unpack (and k_vlp16_pad when a scan is short), the counters' way back

Both are blocking calls; their wall time is a host clock around the call, the kernel time is the context's own launch events (lvx_set_profiling on the upstream
slot).  The two routes alternate inside one loop, --warmup rounds are dropped, and median / min / max of --steps rounds are reported.  The kernel's traffic is
computed from the shapes (32 bytes written per record, 1206 bytes read per 384 records) and set against the 6.2 TB/s the part streams with plain stores
(HBM3E peak 8 TB/s).  The records the two routes leave in the context are compared once, bytes for bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
STREAM_STORE_TBS = 6.2      # plain 16-byte streaming stores, measured on the part


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=600)
    ap.add_argument("--packets", type=int, default=76)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lvx
    import vlp16
    rng = np.random.default_rng(1)
    cols = 24 * a.packets
    packets = b"".join(vlp16.encode_packets(rng.uniform(0.3, 60.0, (16, cols)), rng.integers(0, 256, (16, cols)), int(rng.integers(0, 36000)), 39) for _ in range(a.scans))
    offsets = np.arange(a.scans + 1, dtype=np.int32) * a.packets
    stamps = 1.6e9 + 0.1 * np.arange(a.scans)
    g = lvx.Context(0)      # (raises without a device: nothing here runs on the CPU)
    records, info = lvx.vlp16_unpack(g, packets, offsets, stamps)
    n_records = records.size
    out = dict(scans=a.scans, packets_per_scan=a.packets, W=info["W"], record_bytes=int(records.nbytes), packet_bytes=len(packets), steps=a.steps, warmup=a.warmup, info=info)
    g.set_profiling(True, only=lvx.KERNEL_UPSTREAM)
    wall = dict(records=[], packets=[])
    ker = dict(records=[], packets=[])
    launches = dict(records=0, packets=0)
    for k in range(a.warmup + a.steps):
        for route in ("records", "packets"):
            g.kernel_ms()                                   # reads and clears the launch records
            w0 = time.perf_counter()
            if route == "records":
                lvx.set_scans(g, records, 16, info["W"])
            else:
                g.set_scans_vlp16(packets, offsets, stamps)
            w = (time.perf_counter() - w0) * 1e3
            ms, n = g.kernel_ms()
            if k >= a.warmup:
                wall[route].append(w); ker[route].append(float(ms[lvx.KERNEL_UPSTREAM])); launches[route] = int(n[lvx.KERNEL_UPSTREAM])
    same = lvx.get_scans_raw(g, 0, a.scans, 16, info["W"]).tobytes() == records.tobytes()      # the last call was the packet route
    g.set_profiling(False)
    g.close()
    for route in ("records", "packets"):
        out[route] = dict(blocking_wall_ms=_stats(wall[route]), kernel_ms=_stats(ker[route]), timed_launch_groups=launches[route])
    kbytes = n_records * 32 + len(packets)
    kms = out["packets"]["kernel_ms"]["median"]
    out["kernel_bytes"] = int(kbytes)
    out["kernel_TBps"] = kbytes / (kms * 1e-3) / 1e12 if kms > 0 else None
    out["kernel_share_of_streaming_stores"] = (out["kernel_TBps"] / STREAM_STORE_TBS) if kms > 0 else None
    out["upload_GBps"] = dict(records=records.nbytes / (out["records"]["blocking_wall_ms"]["median"] * 1e-3) / 1e9, packets=len(packets) / (out["packets"]["blocking_wall_ms"]["median"] * 1e-3) / 1e9)
    out["routes_leave_the_same_bytes"] = bool(same)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
