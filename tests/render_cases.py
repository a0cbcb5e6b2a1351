"""Shared by tests/test_render_host.py and tests/test_gpu_render.py: the g++ build of lvi-exc_amd/csrc/lvx_render.h (tests/native/render_host_check.cpp) behind ctypes,
a numpy float64 restatement of the reference's per-point code written from its lines (it never calls the header), and seeded generators of map points."""
import ctypes as C
import os
import subprocess

import numpy as np

import lvx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, PITCH = 48, 64, 72
MARGIN = 1e-9   # px from an integer / metres from a depth limit: beyond it the last-bit differences of two correct float64 evaluations cannot change a record
_LIB = None


def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "render_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "librender_host_check.so")
        deps = [src, os.path.join(ROOT, "include", "lvx.h")] + [os.path.join(ROOT, "lvi-exc_amd", "csrc", f) for f in ("lvx_math.h", "lvx_render.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
        _LIB.rh_render.restype = C.c_longlong
    return _LIB


def pinhole(cam):
    return lvx.Pinhole(cam["rows"], cam["cols"], cam.get("readout", 0.0), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"])


def make_camera(fx=40.0, fy=38.0, cx=31.5, cy=23.25, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    return dict(rows=ROWS, cols=COLS, readout=0.0, fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3)


RADTAN = dict(k1=-0.05, k2=0.01, p1=0.001, p2=-0.0015, k3=0.002)
UNIT_CAMERA = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)   # with identity poses and z = 1: uv = (x, y) exactly
IDENTITY = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))


def make_images(seed, n_images=1):
    return np.random.default_rng(seed).integers(0, 256, (n_images, ROWS, PITCH), dtype=np.uint8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def host_render(xyzi, pose_L0, cam_poses, valid, cam, images, z_min=0.1, z_max=15.0):
    """lvx_render.h over host arrays: (records, status, n_colored)."""
    pts = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    qc, pc = _d([q for q, _ in cam_poses]), _d([p for _, p in cam_poses])
    v = np.ascontiguousarray(valid, dtype=np.int32)
    images = np.ascontiguousarray(images, dtype=np.uint8)
    out, st = np.zeros(len(pts), dtype=lvx.POINT_XYZRGB), np.zeros(len(pts), np.int32)
    ph = pinhole(cam)
    n = host_lib().rh_render(C.c_int(len(pts)), _p(pts), _p(_d(pose_L0[0])), _p(_d(pose_L0[1])), C.c_int(len(v)), _p(qc), _p(pc), _p(v), C.byref(ph), _p(images), C.c_int(images.shape[-1]),
                             C.c_double(z_min), C.c_double(z_max), _p(out), _p(st))
    assert n >= 0
    return out, st, n


def host_render_uv(xyzi, pose_L0, pose_C, cam):
    pts = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    zuv = np.zeros((len(pts), 3))
    ph = pinhole(cam)
    host_lib().rh_render_uv(C.c_int(len(pts)), _p(pts), _p(_d(pose_L0[0])), _p(_d(pose_L0[1])), _p(_d(pose_C[0])), _p(_d(pose_C[1])), C.byref(ph), _p(zuv))
    return zuv


def host_overlay_chain(pose_L, pose_C):
    q, p = np.zeros(4), np.zeros(3)
    host_lib().rh_overlay_chain(_p(_d(pose_L[0])), _p(_d(pose_L[1])), _p(_d(pose_C[0])), _p(_d(pose_C[1])), _p(q), _p(p))
    return q, p


def host_overlay(xyzi, q_LtoC, p_LinC, cam):
    pts = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    pix, zuv = np.zeros(len(pts), np.int32), np.zeros((len(pts), 3))
    ph = pinhole(cam)
    host_lib().rh_overlay(C.c_int(len(pts)), _p(pts), _p(_d(q_LtoC)), _p(_d(p_LinC)), C.byref(ph), _p(pix), _p(zuv))
    return pix, zuv


# ---- the reference's lines in numpy float64 (lvi_initialize_surfel_orb.cpp) -----------------------------------------------------------------------------------------
def np_rotation(q_xyzw):
    """q.normalize(); q.toRotationMatrix() (:724-726, :744-745)."""
    x, y, z, w = np.asarray(q_xyzw, dtype=np.float64) / np.sqrt(np.sum(np.asarray(q_xyzw, dtype=np.float64) ** 2))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _mat_vec(R, p, x, y, z):   # row by row, left to right: no BLAS (its FMAs would round differently)
    return [R[i, 0] * x + R[i, 1] * y + R[i, 2] * z + p[i] for i in range(3)]


def np_project(cam, X, Y, Z):
    """:766-779."""
    with np.errstate(all="ignore"):
        tx, ty = X / Z, Y / Z
        r2 = tx * tx + ty * ty
        dist = 1 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
        u = tx * dist + 2 * cam["p1"] * tx * ty + cam["p2"] * (r2 + 2 * tx * tx)
        v = ty * dist + cam["p1"] * (r2 + 2 * ty * ty) + 2 * cam["p2"] * tx * ty
        return cam["fx"] * u + cam["cx"], cam["fy"] * v + cam["cy"]


def _int_cast(u):
    """int(u) where it is defined; elsewhere (not finite, beyond +-2^30) the coordinate is outside any image."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(u) & (np.abs(u) < 2.0 ** 30)
        return ok, np.trunc(np.where(ok, u, 0.0)).astype(np.int64)


def np_render_one(xyzi, pose_L0, pose_C, cam, image, z_min=0.1, z_max=15.0, rec=None):
    """:749-793 for one image; rec (records so far, for the several-image extension) is updated for the points not yet coloured.  Returns (records, status, zuv)."""
    pts = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    n = len(pts)
    if rec is None:
        rec = np.zeros(n, dtype=lvx.POINT_XYZRGB)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    nan = np.isnan(pts[:, 0]) | np.isnan(pts[:, 1]) | np.isnan(pts[:, 2])                # :752
    RL, RC = np_rotation(pose_L0[0]), np_rotation(pose_C[0])
    with np.errstate(all="ignore"):
        g = _mat_vec(RL, np.asarray(pose_L0[1], dtype=np.float64), x, y, z)              # :754
        d = [g[i] - float(pose_C[1][i]) for i in range(3)]
        c = [RC[0, i] * d[0] + RC[1, i] * d[1] + RC[2, i] * d[2] for i in range(3)]      # :755, T_CinG.inverse() of a rigid transform
        in_depth = ~nan & ~((c[2] < z_min) | (c[2] > z_max))                             # :757
    u, v = np_project(cam, c[0], c[1], c[2])
    oku, iu = _int_cast(u)
    okv, iv = _int_cast(v)
    inside = in_depth & oku & okv & ~((iu < 0) | (iv < 0) | (iu > cam["cols"] - 1) | (iv > cam["rows"] - 1))   # :781-784
    todo = rec["a"] == 0
    keep = in_depth & todo
    for k, name in enumerate("xyz"):
        rec[name][keep] = pts[keep, k]                                                   # :759-762
    col = inside & todo
    grey = image[iv[col], iu[col]]                                                       # :785
    for name in "bgr":
        rec[name][col] = grey
    rec["a"][col] = 255
    status = np.where(inside, 2, np.where(in_depth, 1, 0)).astype(np.int32)
    return rec, status, np.stack([c[2], u, v], axis=1)


def np_render(xyzi, pose_L0, cam_poses, valid, cam, images, z_min=0.1, z_max=15.0):
    """The lowest-index valid image that colours a point wins; with one image this is RenderMap."""
    rec, status = None, None
    for k, ok in enumerate(valid):
        if not ok:
            continue
        rec, st, _ = np_render_one(xyzi, pose_L0, cam_poses[k], cam, images[k], z_min, z_max, rec)
        status = st if status is None else np.where(rec["a"] == 255, 2, np.maximum(status, st)).astype(np.int32)
    if rec is None:
        n = len(np.asarray(xyzi).reshape(-1, 4))
        return np.zeros(n, dtype=lvx.POINT_XYZRGB), np.zeros(n, np.int32)
    return rec, status


def np_qrot(q_xyzw, X):
    """Eigen's Quaternion * Vector3 (_transformVector): v + w * uv + qv x uv with uv = 2 qv x v."""
    qv, w = np.asarray(q_xyzw[:3], dtype=np.float64), float(q_xyzw[3])
    uv = np.cross(qv, X)
    uv = uv + uv
    return X + w * uv + np.cross(qv, uv)


def np_overlay(xyzi, q_LtoC, p_LinC, cam):
    """:1343-1353: pixel index int(v) * cols + int(u) or -1; (depth, u, v)."""
    pts = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        c = np_qrot(q_LtoC, pts[:, :3].astype(np.float64)) + np.asarray(p_LinC, dtype=np.float64)   # :1345
        u, v = np_project(cam, c[:, 0], c[:, 1], c[:, 2])
        oku, iu = _int_cast(u)
        okv, iv = _int_cast(v)
        out = (c[:, 2] < 0) | ~oku | ~okv | (u < 0) | (v < 0) | (iu > cam["cols"] - 1) | (iv > cam["rows"] - 1)   # :1346, :1350-1351
    return np.where(out, -1, iv * cam["cols"] + iu).astype(np.int32), np.stack([c[:, 2], u, v], axis=1)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------------
def random_pose(rng, scale=1.0):
    q = rng.standard_normal(4)
    return scale * q / np.linalg.norm(q), rng.uniform(-2, 2, 3)


def random_points(rng, n, pose_L0, pose_C, cam, spread=1.4, z_lo=-6.0, z_hi=24.0):
    """n float32 map points (LiDAR frame at the map time) aimed so that about half are in depth range and about half of those inside the image: camera-frame depth uniform
    in [z_lo, z_hi], normalised coordinates uniform over `spread` times the image's field of view."""
    z = rng.uniform(z_lo, z_hi, n)
    un = rng.uniform(-spread, spread, n) * (0.5 * cam["cols"] / cam["fx"]) + (0.5 * cam["cols"] - cam["cx"]) / cam["fx"]
    vn = rng.uniform(-spread, spread, n) * (0.5 * cam["rows"] / cam["fy"]) + (0.5 * cam["rows"] - cam["cy"]) / cam["fy"]
    pc = np.stack([un * z, vn * z, z], axis=1)
    pg = pc @ np_rotation(pose_C[0]).T + pose_C[1]
    pl = (pg - pose_L0[1]) @ np_rotation(pose_L0[0])
    return np.concatenate([pl, rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)


def assert_margin(zuv, z_min=0.1, z_max=15.0, exclude=None):
    """The byte comparison's condition: every finite uv component at least MARGIN from an integer and every depth at least MARGIN from a limit.  A seed that violates it
    FAILS (nothing is filtered); `exclude` marks constructed edge cases, exact by construction."""
    zuv = np.asarray(zuv)
    m = np.ones(len(zuv), bool) if exclude is None else ~np.asarray(exclude)
    z, uv = zuv[m, 0], zuv[m, 1:]
    fz = np.isfinite(z)
    assert (np.abs(z[fz] - z_min) >= MARGIN).all() and (np.abs(z[fz] - z_max) >= MARGIN).all()
    f = np.isfinite(uv) & (np.abs(uv) < 2.0 ** 30)
    assert (np.abs(uv[f] - np.rint(uv[f])) >= MARGIN).all()
