"""Shared by tests/test_vlp16_host.py, tests/test_gpu_vlp16.py and tests/test_gpu_vlp16_demo.py: a numpy restatement of licalib::VelodyneCorrection::unpack_scan written
from the reference's src/lvi_exc/include/utils/vlp_common.h (:51-149 the packet overload, :152-176 the organised one, :179-181 and :244-248 the time table, :184-242 the
constants, :252-255 the range test) that never includes lvi-exc_amd/csrc/lvx_vlp16.h, the packet builders, the cases, and the g++ build of the header
(tests/native/vlp16_host_check.cpp) behind ctypes.

The restatement works in float32 where the reference has `float` and in float64 where it has `double`, one rounding per C operation.  Its rotation and vertical
tables come from the RUNNING machine's libm (cosf / sinf through ctypes), as the reference's setParameters fills them — never from numpy, whose float32 cos differs
from libm's at thousands of the 36000 entries."""
import ctypes as C
import ctypes.util
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("pad2", "<f4"), ("timestamp", "<f8")])
PACKET_BYTES, BLOCKS = 1206, 12
F = np.float32
SCAN_MAPPING_16 = np.array([15, 7, 14, 6, 13, 5, 12, 4, 11, 3, 10, 2, 9, 1, 8, 0])   # :227-242
VERT_CORRECTION = [-0.2617993877991494, 0.017453292519943295, -0.22689280275926285, 0.05235987755982989, -0.19198621771937624, 0.08726646259971647, -0.15707963267948966,
                   0.12217304763960307, -0.12217304763960307, 0.15707963267948966, -0.08726646259971647, 0.19198621771937624, -0.05235987755982989, 0.22689280275926285,
                   -0.017453292519943295, 0.2617993877991494]                       # :205-222
DEFAULTS = dict(min_range=0.6, max_range=150.0, min_angle=0, max_angle=36000)          # :186-189
_TABLES = None
_LIB = None


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------------------------------
def tables():
    """cos_rot, sin_rot [36000], cos_vert, sin_vert [16] as setParameters builds them, from this machine's libm."""
    global _TABLES
    if _TABLES is None:
        libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (libm.cosf, libm.sinf):
            f.restype, f.argtypes = C.c_float, [C.c_float]
        cr, sr, cv, sv = np.zeros(36000, F), np.zeros(36000, F), np.zeros(16, F), np.zeros(16, F)
        for i in range(36000):
            degrees = float(F(0.01) * F(i))                           # ROTATION_RESOLUTION * rot_index in float, then from_degrees' double parameter
            rotation = float(F(degrees * math.pi / 180.0))            # angles::from_degrees in double, narrowed by `float rotation =`
            cr[i], sr[i] = libm.cosf(rotation), libm.sinf(rotation)
        for i, v in enumerate(VERT_CORRECTION):
            cv[i], sv[i] = libm.cosf(float(F(v))), libm.sinf(float(F(v)))   # float vert_correction[]; std::cos(float)
        _TABLES = (cr, sr, cv, sv)
    return _TABLES


def _c_rem(a, b):
    """C's % on ints: the quotient truncates towards zero."""
    return int(math.fmod(a, b))


def restate_scan(pk, stamp, min_range=0.6, max_range=150.0, min_angle=0, max_angle=36000, trace=None):
    """unpack_scan (:51-149) for one scan.  pk: uint8 [n][1206].  Returns (cloud [16][24 n] POINT — value-initialised where the reference does not write —,
    counts [in range, out of range, outside the window, bad headers]).  trace (a list): every corrected azimuth BEFORE the % 36000."""
    cr, sr, cv, sv = tables()
    n = len(pk)
    cloud = np.zeros((16, 24 * n), POINT)
    counts = [0, 0, 0, 0]
    firing, dsr = np.meshgrid(np.arange(2), np.arange(16), indexing="ij")
    t_in_block = dsr.astype(F) * F(2.304) + firing.astype(F) * F(55.296)       # (dsr*DSR_TOFFSET) + (firing*FIRING_TOFFSET), float
    row = SCAN_MAPPING_16[dsr]
    block_counter = 0
    for i in range(n):
        blocks = pk[i, :1200].reshape(BLOCKS, 100).astype(np.int64)
        header = blocks[:, 0] | (blocks[:, 1] << 8)
        rotation = blocks[:, 2] | (blocks[:, 3] << 8)
        last_azimuth_diff = F(0)
        for block in range(BLOCKS):
            counts[3] += int(header[block] != 0xEEFF)
            azimuth = F(rotation[block])
            if block < BLOCKS - 1:
                azimuth_diff = F(_c_rem(36000 + int(rotation[block + 1]) - int(rotation[block]), 36000))
                last_azimuth_diff = azimuth_diff
            else:
                azimuth_diff = last_azimuth_diff
            corrected_f = azimuth + (azimuth_diff * t_in_block) / F(110.592)
            assert corrected_f.dtype == F
            c64 = corrected_f.astype(np.float64)
            rounded = (np.sign(c64) * np.floor(np.abs(c64) + 0.5)).astype(np.int64)          # round(): halves away from zero
            if trace is not None:
                trace.extend(rounded.ravel().tolist())
            corrected = np.fmod(rounded, 36000)                                               # C's %
            inside = ((corrected >= min_angle) & (corrected <= max_angle) & (min_angle < max_angle)) | \
                     ((min_angle > max_angle) & ((corrected <= max_angle) | (corrected >= min_angle)))
            # A NEGATIVE index (block 11 with the negative difference of a raw rotation that fell from above 36000 in block 10): min_angle >= 0 keeps it out of a
            # window with min < max; in a wrapped window the reference would read in front of its tables — the project leaves the record unwritten there too
            inside &= corrected >= 0
            corrected = np.where(corrected >= 0, corrected, 0)
            data = blocks[block, 4:].reshape(2, 16, 3)
            distance = (data[..., 0] | (data[..., 1] << 8)).astype(F) * F(0.002)
            x = distance * cv[dsr] * sr[corrected]
            y = distance * cv[dsr] * cr[corrected]
            z = distance * sv[dsr]
            assert x.dtype == F and y.dtype == F and z.dtype == F
            col = 2 * block_counter + firing
            t = np.float64(stamp) + (row.astype(np.float64) * 2.304 * 1e-6 + col.astype(np.float64) * 55.296 * 1e-6)   # the table of :246 at [column][MAPPED row]
            in_range = (distance.astype(np.float64) >= min_range) & (distance.astype(np.float64) <= max_range)
            p = np.zeros((2, 16), POINT)
            p["timestamp"] = t
            p["x"], p["y"], p["z"] = np.where(in_range, y, F(np.nan)), np.where(in_range, -x, F(np.nan)), np.where(in_range, z, F(np.nan))
            p["intensity"] = np.where(in_range, data[..., 2].astype(F), F(0))
            cloud[row[inside], col[inside]] = p[inside]
            counts[0] += int((inside & in_range).sum()); counts[1] += int((inside & ~in_range).sum()); counts[2] += int((~inside).sum())
            block_counter += 1
    return cloud, counts


def restate(offsets, packets, stamps, W=0, trace=None, **options):
    """Every scan of a call into one array [n_scans][16][W] as lvx_set_scans_vlp16 defines it (include/lvx.h): W = 0 means 24 x the longest scan, the columns beyond a
    shorter scan hold x = y = z = NaN, intensity 0, timestamp 0.  Returns (records, info), or (None, None) where the call must refuse: a scan of more than 76 packets,
    or W too small."""
    pk = np.frombuffer(bytes(packets), np.uint8).reshape(-1, PACKET_BYTES)
    counts_per = np.diff(offsets)
    if (counts_per > 76).any() or (W and W < 24 * counts_per.max()):
        return None, None
    W = W or 24 * int(counts_per.max())
    out = np.zeros((len(stamps), 16, W), POINT)
    out["x"] = out["y"] = out["z"] = np.nan
    total = [0, 0, 0, 0]
    for s in range(len(stamps)):
        cloud, counts = restate_scan(pk[offsets[s]:offsets[s + 1]], stamps[s], trace=trace, **{**DEFAULTS, **options})
        out[s, :, :cloud.shape[1]] = cloud
        total = [a + b for a, b in zip(total, counts)]
    info = dict(n_packets=int(offsets[-1] - offsets[0]), n_in_range=total[0], n_out_of_range=total[1], n_outside_window=total[2], n_bad_headers=total[3], W=W)
    return out, info


def restate_organised(xyzi, stamps):
    """unpack_scan's PointCloud2 overload (:152-176): xyzi [n][H][W][4] -> records whose time is timebase + mVLP16TimeBlock[w][h]."""
    xyzi = np.asarray(xyzi, F)
    n, H, W, _ = xyzi.shape
    out = np.zeros((n, H, W), POINT)
    out["x"], out["y"], out["z"], out["intensity"] = xyzi[..., 0], xyzi[..., 1], xyzi[..., 2], xyzi[..., 3]
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    table = h.astype(np.float64) * 2.304 * 1e-6 + w.astype(np.float64) * 55.296 * 1e-6
    out["timestamp"] = np.asarray(stamps, np.float64)[:, None, None] + table[None]
    return out


# ---- packet builders ---------------------------------------------------------------------------------------------------------------------------------------------------
# 0.6 m through the float -> double promotion, the ends of the field (65535 = 131.07 m: the default 150 m is out of a packet's reach), and 1 m / 100 m for the case
# with narrower bounds
RAW_EDGES = np.array([0, 299, 300, 65535, 1, 301, 499, 500, 501, 49999, 50000, 50001], np.int64)


def packet(rotation, raw, intensity, header=0xEEFF):
    """One packet from rotation [12], raw distances [12][32] (index 16 * firing + dsr), intensity [12][32], header: one value or [12]."""
    b = np.zeros((BLOCKS, 100), np.uint8)
    header, rotation = np.broadcast_to(np.asarray(header, np.int64), (BLOCKS,)), np.asarray(rotation, np.int64)
    raw, intensity = np.broadcast_to(np.asarray(raw, np.int64), (BLOCKS, 32)), np.broadcast_to(np.asarray(intensity, np.int64), (BLOCKS, 32))
    assert 0 <= rotation.min() and rotation.max() <= 65535 and 0 <= raw.min() and raw.max() <= 65535 and 0 <= intensity.min() and intensity.max() <= 255
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = header & 255, header >> 8, rotation & 255, rotation >> 8
    b[:, 4::3], b[:, 5::3], b[:, 6::3] = raw & 255, raw >> 8, intensity
    return np.concatenate([b.ravel(), np.array([1, 2, 3, 4, 0x37, 0x22], np.uint8)])   # 6 trailer bytes nobody reads


def random_packets(rng, n, rotation0=1000, step=40, modulus=36000):
    """n packets: the rotation advances by `step` per block (mod `modulus`), distances drawn from RAW_EDGES and from the whole field, any intensity."""
    out = []
    for i in range(n):
        rot = (rotation0 + step * (BLOCKS * i + np.arange(BLOCKS))) % modulus
        raw = np.where(rng.random((BLOCKS, 32)) < 0.3, rng.choice(RAW_EDGES, (BLOCKS, 32)), rng.integers(0, 65536, (BLOCKS, 32)))
        out.append(packet(rot, raw, rng.integers(0, 256, (BLOCKS, 32))))
    return np.stack(out)


def _case(name, scans, stamps=None, W=0, refused=False, **options):
    """scans: a list of uint8 [n_s][1206] arrays."""
    counts = [len(s) for s in scans]
    pk = np.concatenate([np.asarray(s, np.uint8).reshape(-1, PACKET_BYTES) for s in scans]) if sum(counts) else np.zeros((0, PACKET_BYTES), np.uint8)
    stamps = np.asarray(stamps if stamps is not None else [1.6e9 + 0.1 * s + 1e-3 / 3 for s in range(len(scans))], np.float64)
    return dict(name=name, offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), packets=pk.tobytes(), stamps=stamps, W=W, refused=refused, options=options)


def _cases():
    rng = np.random.default_rng(20241)
    out = [_case("one_packet", [random_packets(rng, 1)]),
           _case("three_packets", [random_packets(rng, 3, rotation0=17000, step=39)]),
           _case("two_scans_2_and_3", [random_packets(rng, 2, rotation0=300), random_packets(rng, 3, rotation0=9000)]),
           _case("wider_than_needed", [random_packets(rng, 2)], W=50)]
    # the rotation wraps 35990 -> 10 between two blocks and between a packet's last block and the next packet; block 10 -> 11 of the first packet advances by 17,
    # the next packet starts 20 further: block 11 must take the 17
    rot_a = np.array([35750, 35770, 35790, 35810, 35990, 10, 30, 50, 70, 90, 35953, 35990])
    rot_b = (10 + 20 * np.arange(BLOCKS)) % 36000
    out.append(_case("wrap", [np.stack([packet(rot_a, rng.integers(300, 60000, (BLOCKS, 32)), 7), packet(rot_b, rng.integers(300, 60000, (BLOCKS, 32)), 9)])]))
    # azimuth 35990 + 20 * 55.296 / 110.592 = 36000 at (firing 1, dsr 0): the index is 36000 % 36000 = 0
    out.append(_case("rounds_to_36000", [packet(np.array([35990 + 20 * b for b in range(BLOCKS)]) % 36000, 5000, 100)[None]]))
    # raw rotations >= 36000 (never reduced by the reference before the % of the corrected azimuth), 65535 -> 5: a NEGATIVE difference
    rot_c = np.array([36000, 36040, 40000, 40040, 65535, 5, 45, 65500, 65535, 35999, 36000, 36001])
    out.append(_case("raw_rotation_past_36000", [packet(rot_c, rng.integers(300, 60000, (BLOCKS, 32)), rng.integers(0, 256, (BLOCKS, 32)))[None],
                                                 random_packets(rng, 2, rotation0=50000, step=700, modulus=65536)]))
    # block 10 at 65535, block 11 at 5: block 11 reuses the difference -29530 on the azimuth 5 — a negative table index, outside every window
    rot_d = np.array([100, 140, 180, 220, 260, 300, 340, 380, 420, 65535, 65535, 5]); rot_d[9] = 65495
    for nm, win in (("negative_index", {}), ("negative_index_wrapped_window", dict(min_angle=35000, max_angle=1000))):
        out.append(_case(nm, [packet(rot_d, rng.integers(300, 60000, (BLOCKS, 32)), 11)[None]], **win))
    raw = np.tile(np.array([0, 299, 300, 65535], np.int64), (BLOCKS, 8))
    inten = np.tile(np.array([0, 255, 255, 0, 255, 0, 0, 255], np.int64), (BLOCKS, 4))
    out.append(_case("range_and_intensity_edges", [packet(2000 + 40 * np.arange(BLOCKS), raw, inten)[None]]))
    out.append(_case("narrow_range_option", [random_packets(rng, 2)], min_range=1.0, max_range=100.0))
    hdr = np.full(BLOCKS, 0xEEFF); hdr[3], hdr[7] = 0xDDFF, 0
    out.append(_case("wrong_headers", [packet(500 + 40 * np.arange(BLOCKS), rng.integers(300, 60000, (BLOCKS, 32)), 50, hdr)[None], random_packets(rng, 1)]))
    out.append(_case("window_min_below_max", [random_packets(rng, 3, rotation0=8700, step=25)], min_angle=9000, max_angle=9400))
    out.append(_case("window_min_above_max", [random_packets(rng, 3, rotation0=35500, step=40)], min_angle=35900, max_angle=300))
    out.append(_case("an_empty_scan_between", [random_packets(rng, 1), np.zeros((0, PACKET_BYTES), np.uint8), random_packets(rng, 2)]))
    # more scans than one round of the kernel's 64-probe search of the offsets, empty ones among them, the last one empty
    out.append(_case("many_scans", [random_packets(rng, k, rotation0=int(rng.integers(0, 36000))) if k else np.zeros((0, PACKET_BYTES), np.uint8) for k in [1, 0, 2, 1, 1, 0] * 23]))
    out.append(_case("seventy_six_packets", [random_packets(rng, 76, rotation0=0, step=39)]))
    out.append(_case("seventy_seven_packets", [random_packets(rng, 1), np.tile(random_packets(rng, 1), (77, 1))], refused=True))
    out.append(_case("W_too_small", [random_packets(rng, 3)], W=48, refused=True))
    return out


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]
ORGANISED = {"16x24": (2, 16, 24), "15x24": (2, 15, 24), "16x1824": (1, 16, 1824)}
_RESTATED = {}


def case(name):
    return CASES[CASE_NAMES.index(name)]


def restated(name, trace=None):
    """(records, info) of a case from the restatement, computed once (read-only), (None, None) for a refused case."""
    if name not in _RESTATED or trace is not None:
        c = case(name)
        res = restate(c["offsets"], c["packets"], c["stamps"], c["W"], trace=trace, **c["options"])
        if res[0] is not None:
            res[0].setflags(write=False)
        _RESTATED[name] = res
    return _RESTATED[name]


def organised_input(name):
    n, H, W = ORGANISED[name]
    rng = np.random.default_rng(H * W)
    xyzi = rng.uniform(-30, 30, (n, H, W, 4)).astype(F)
    xyzi[..., 3] = rng.integers(0, 256, (n, H, W))
    xyzi[0, H // 2, W // 3, :3] = np.nan                       # a "no return" is copied as it is
    return xyzi, np.array([1.6e9 + 0.1 * s for s in range(n)])


def same_bytes(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the g++ build of the header -------------------------------------------------------------------------------------------------------------------------------------
def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "vlp16_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "libvlp16_host_check.so")
        deps = [src, os.path.join(ROOT, "lvi-exc_amd", "csrc", "lvx_vlp16.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_tables():
    t = [np.zeros(36000, F), np.zeros(36000, F), np.zeros(16, F), np.zeros(16, F)]
    host_lib().vlp16_tables(*[_p(a) for a in t])
    return t


def host_unpack(offsets, packets, stamps, W=0, **options):
    """The header's per-record function over every scan (vlp16_unpack_host): (records, info) or (None, error 1 .. 3 of vlp16_width)."""
    o = {**DEFAULTS, **options}
    off, st = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(stamps, np.float64)
    pk = np.frombuffer(bytes(packets), np.uint8)
    cap_w = max(W, 24 * int(np.diff(off).max()), 1)
    out, info = np.zeros((len(st), 16, cap_w), POINT), np.zeros(5, np.int64)
    rc = host_lib().vlp16_unpack_host(C.c_int(len(st)), _p(off), _p(pk), _p(st), C.c_int(W), C.c_double(o["min_range"]), C.c_double(o["max_range"]), C.c_int(o["min_angle"]),
                                      C.c_int(o["max_angle"]), C.c_int(out.size), _p(out), _p(info))
    if rc < 0:
        return None, -rc
    rec = out.reshape(-1)[:len(st) * 16 * rc].reshape(len(st), 16, rc)
    return rec, dict(n_packets=int(info[0]), n_in_range=int(info[1]), n_out_of_range=int(info[2]), n_outside_window=int(info[3]), n_bad_headers=int(info[4]), W=rc)


def host_organised(xyzi, stamps):
    xyzi, st = np.ascontiguousarray(xyzi, F), np.ascontiguousarray(stamps, np.float64)
    n, H, W, _ = xyzi.shape
    out = np.zeros((n, H, W), POINT)
    host_lib().vlp16_organised_host(C.c_int(n), C.c_int(H), C.c_int(W), _p(xyzi), _p(st), _p(out))
    return out
