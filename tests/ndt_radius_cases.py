"""Shared by tests/test_ndt_radius_cases.py (CPU) and tests/test_gpu_ndt_radius.py: the cases of the voxel radius search (VoxelGridCovariance::radiusSearch, the
neighbour search of pclomp::KDTREE), a numpy restatement of lvi-exc_amd/csrc/lvx_vxradius.h and the g++ build of that header behind ctypes.

THE RESTATEMENT (`restate`) is brute force over ALL member leaves — it knows nothing of cells, so it also checks the header's claim that the 27 cells around a query
hold every centroid within a radius <= leaf size:
    members    leaves with nr_points >= min_pts or nr_points == -1 (rejected after the tree was filled: voxel_grid_covariance_omp_impl.hpp:301-330 against :341-345)
    distance   float32: d = q - c per axis, d2 = (dx dx + dy dy) + dz dz; hit: d2 < float32(float64(radius) * float64(radius))
    order      stable sort by d2 over the members in leaf order = ascending (d2, leaf)
    output     ids [nq][27] (-1 padded), d2 [nq][27] (+inf padded), count [nq]
Every case is held to two PRECONDITIONS on its inputs (`Built.margin_ulps`, `Built.equal_rows`; tests/test_ndt_radius_cases.py asserts them): no member centroid has
|d2 - r2| within 4 float ulps of r2 for any query — so neither the strict < nor a last-bit difference can decide a comparison — and no query has two hits at equal
distance, except in the tie case, which is built to have them.  No query is left out of any comparison.

Cases.  Scenes of tests/ndt_cases.py where they exist (rooms measured in cells, sources placed a tenth of a cell off the target), constructions below where not:
    room_*        make_room at leaf 0.25, 0.5 and 2.0; the 0.5 room is also cut to 1, 63, 64, 65, 255, 256, 257 and 1000 queries (SIZES)
    min_pts_*     min_points_per_voxel 3 and 12: leaves below the threshold are not members
    box_*         queries in the outermost cells, one cell outside every face, thousands of cells outside, next to the coordinate planes
    full_house    clusters in all 27 cells around one cell, each at the corner nearest that cell's centre (a corner cell's cluster is 0.95 leaf from it): counts reach 27
    rejected      the 0.5 room plus eight coincident points outside it: a leaf with nr_points = -1 that the tree keeps; queries inside and outside its radius
    tie           two clusters mirrored about the plane x = 0.5 on dyadic coordinates (every float sum exact): queries on the plane see both at the same float d2
    nonfinite     NaN and +-inf in every coordinate, between finite queries
    demo          the reference's two scans reduced at 0.1 m, resolution 1.0 (apps/align.cpp)
    raw           the raw target scan at the calibration's 0.5 m with every fourth point of the raw source: its (0, 0, 0) returns form a rejected leaf
"""
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np

import ndt_cases as NC
from oracle import ndt_align as NA
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 27                       # LVX_VOXEL_RADIUS_MAX
SIZES = NC.SIZES             # 1, 63, 64, 65, 255, 256, 257, 1000
MARGIN_ULPS = 4
_LIB = None

RCase = namedtuple("RCase", "name tgt leaf min_pts src trans p6 outlier_ratio rejected tie")
Built = namedtuple("Built", "case vox ids d2 count margin_ulps equal_rows")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
def members(vox, min_pts):
    n = np.asarray(vox["leaf_n"])
    return np.flatnonzero((n >= min_pts) | (n == -1)).astype(np.int32)


def radius2(radius):
    return np.float32(np.float64(radius) * np.float64(radius))


def restate(vox, min_pts, queries, radius, chunk=1024):
    """(ids [nq][27], d2 [nq][27], count [nq], margin_ulps, equal_rows): margin_ulps = min |d2 - r2| / ulp(r2) over every (query, member) pair, equal_rows = the queries
    with two hits at the same d2."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)[:, :3]
    mem = members(vox, min_pts)
    cen = np.ascontiguousarray(vox["centroid"], np.float32)[mem]
    r2 = radius2(radius)
    nq = len(q)
    ids, d2o, count = np.full((nq, K), -1, np.int32), np.full((nq, K), np.inf, np.float32), np.zeros(nq, np.int32)
    margin, equal_rows = np.inf, []
    if len(mem) == 0:
        return ids, d2o, count, margin, np.zeros(0, np.int64)
    for i0 in range(0, nq, chunk):
        qq = q[i0:i0 + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = qq[:, None, 0] - cen[None, :, 0], qq[:, None, 1] - cen[None, :, 1], qq[:, None, 2] - cen[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            hit = d2 < r2
            gap = np.abs(d2.astype(np.float64) - np.float64(r2))
        fin = np.isfinite(gap)
        if fin.any():
            margin = min(margin, float(gap[fin].min() / np.spacing(r2)))
        cnt = hit.sum(axis=1)
        assert cnt.max() <= K
        key = np.where(hit, d2, np.float32(np.inf))
        order = np.argsort(key, axis=1, kind="stable")[:, :K]            # members are in leaf order: a stable sort leaves equal d2 in ascending leaf index
        w = order.shape[1]
        sd = np.take_along_axis(key, order, axis=1)
        ok = np.arange(w)[None, :] < cnt[:, None]
        ids[i0:i0 + len(qq), :w] = np.where(ok, mem[order], -1)
        d2o[i0:i0 + len(qq), :w] = np.where(ok, sd, np.float32(np.inf))
        count[i0:i0 + len(qq)] = cnt
        eq = (ok[:, 1:] & (sd[:, 1:] == sd[:, :-1])).any(axis=1)
        equal_rows.append(i0 + np.flatnonzero(eq))
    return ids, d2o, count, margin, np.concatenate(equal_rows)


# ---- the g++ build of the header ------------------------------------------------------------------------------------------------------------------------------------
def host_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "native", "vxradius_host_check.cpp")
        so = os.path.join(ROOT, "tests", "native", "libvxradius_host_check.so")
        deps = [src] + [os.path.join(ROOT, "lvi-exc_amd", "csrc", f) for f in ("lvx_math.h", "lvx_vxradius.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = C.CDLL(so)
        _LIB.vr_search.restype = C.c_longlong
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_search(vox, leaf, min_pts, queries, radius):
    """The header's vxr_search per query against the oracle's grid: (ids, d2, count)."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)
    ids, d2, count = np.full((len(q), K), -7, np.int32), np.full((len(q), K), -7.0, np.float32), np.full(len(q), -7, np.int32)
    grid, lk, ln = np.ascontiguousarray(vox["grid"], np.int32), np.ascontiguousarray(vox["leaf_key"], np.int32), np.ascontiguousarray(vox["leaf_n"], np.int32)
    cen = np.ascontiguousarray(vox["centroid"], np.float32)
    cells = host_lib().vr_search(C.c_int(len(q)), _p(q), C.c_float(leaf), C.c_double(radius), C.c_int(min_pts), _p(grid), C.c_int(vox["n_leaves"]), _p(lk), _p(ln), _p(cen),
                                 _p(ids), _p(d2), _p(count))
    assert cells >= 0
    return ids, d2, count


# ---- constructions ----------------------------------------------------------------------------------------------------------------------------------------------------
def _xyzi(xyz, intensity=0.0):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = np.asarray(xyz, np.float64)
    out[:, 3] = intensity
    return out


FULL_LEAF, FULL_CELL = 0.5, np.array([2, -1, 0])      # the centre cell of the full house


def _full_house():
    """Eight points per cell of the 27 cells around FULL_CELL, 0.05 leaf inside the corner (edge, face) nearest the centre cell's centre, spread 0.01 leaf; the centre
    cell's own cluster sits at its centre.  Queries: the centre, 40 within 0.015 leaf of it (all 27 within reach: the farthest cluster is 0.953 + 0.03 leaf away),
    and 40 within 0.45 leaf of it (fewer)."""
    rng = np.random.default_rng(5)
    L, c0 = FULL_LEAF, FULL_CELL.astype(np.float64)
    centre = (c0 + 0.5) * L
    pts = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                d = np.array([dx, dy, dz], np.float64)
                at = np.where(d < 0, c0 * L - 0.05 * L, np.where(d > 0, (c0 + 1) * L + 0.05 * L, centre))
                pts.append(at + 0.01 * L * rng.standard_normal((8, 3)))
    tgt = _xyzi(np.concatenate(pts), 1.0)
    q = np.concatenate([centre[None, :], centre + 0.015 * L * rng.uniform(-1, 1, (40, 3)) / np.sqrt(3.0), centre + 0.45 * L * rng.uniform(-1, 1, (40, 3))])
    return tgt, _xyzi(q)


REJECTED_AT = np.array([8.5, 0.5, 0.5])               # cells: outside the room (its far wall is at 6.3), inside the grid once it is there


def _rejected(leaf=0.5):
    """(target, queries, the coincident point): the room plus eight copies of one point; queries 0.2 to 0.95 leaf from it (in its own cell and in the neighbours), 1.05 to
    1.6 leaf from it, and room points."""
    rng = np.random.default_rng(9)
    room = NC.make_room(11, leaf)
    at = (REJECTED_AT * leaf).astype(np.float32)
    tgt = np.concatenate([room[:4000], np.tile(np.array([[at[0], at[1], at[2], 7.0]], np.float32), (8, 1)), room[4000:]])
    u = rng.standard_normal((60, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.concatenate([rng.uniform(0.2, 0.95, 40), rng.uniform(1.05, 1.6, 20)]) * leaf
    q = np.concatenate([at.astype(np.float64) + u * rad[:, None], room[::400, :3].astype(np.float64)])
    return tgt, _xyzi(q), at


def _tie():
    """Leaf 0.5.  Cluster A: the corners of a cube of side 1/4 about (0.3125, 0.25, 0.25), cluster B its mirror image about x = 0.5 (centre 0.6875): every coordinate
    is a multiple of 1/16, so the float sums of the build and the centroids are exact and B's centroid is A's mirrored.  (The cube is wide on purpose: the queries
    lie within two standard deviations of both leaves, where the float arithmetic of the derivatives is as well conditioned as in the rooms.)  Queries with x = 0.5 exactly (dyadic y, z)
    see both at the same float d2; the others see them at different ones.  A lies in cell x = 0, B in cell x = 1: A has the lower leaf index."""
    cube = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64) / 8.0
    a, b = np.array([0.3125, 0.25, 0.25]) + cube, np.array([0.6875, 0.25, 0.25]) + cube
    tgt = _xyzi(np.concatenate([a, b]), 2.0)
    on = np.array([[0.5, 0.25, 0.25], [0.5, 0.375, 0.125], [0.5, 0.0, 0.5], [0.5, 0.125, 0.25], [0.5, 0.25, 0.0625]])
    off = np.array([[0.46875, 0.25, 0.25], [0.53125, 0.3125, 0.25], [0.25, 0.25, 0.25], [1.5, 0.25, 0.25]])
    return tgt, _xyzi(np.concatenate([on, off])), len(on)


def _nonfinite():
    b = NC.build("size_65")
    q = b.trans.copy()
    bad = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(range(0, 63, 7)):
        q[i, j % 3] = bad[j // 3]
    q[64, :3] = np.nan
    return b, q


@functools.lru_cache(maxsize=None)
def real_clouds():
    tgt = np.load(os.path.join(NC.GOLD, "ndt_data_251370668.npz"))["xyzi"]
    src = np.load(os.path.join(NC.GOLD, "ndt_data_251371071.npz"))["xyzi"]
    td, sd = NC.align_clouds(0.1)
    return dict(tgt=tgt, src=src, td=td, sd=sd)


NC_CASES = dict(room_0p25="grid_leaf0.25_out0.55", room_0p5="size_1000", room_2="grid_leaf2_out0.55", min_pts_3="min_pts_3", min_pts_12="min_pts_12", box_mixed="border_mixed",
                box_outside="border_all_outside")
NAMES = list(NC_CASES) + ["full_house", "rejected", "tie", "nonfinite", "demo", "raw"]
SYNTHETIC = [n for n in NAMES if n not in ("demo", "raw")]


@functools.lru_cache(maxsize=None)
def case(name):
    zero = (0.0,) * 6
    if name in NC_CASES:
        b = NC.build(NC_CASES[name])
        c = b.case
        return RCase(name, b.tgt, c.leaf, c.min_pts, b.src, b.trans, c.p6, c.outlier_ratio, False, False)
    if name == "full_house":
        tgt, q = _full_house()
        return RCase(name, tgt, FULL_LEAF, 6, q, q, zero, 0.55, False, False)
    if name == "rejected":
        tgt, q, _ = _rejected()
        return RCase(name, tgt, 0.5, 6, q, q, zero, 0.55, True, False)
    if name == "tie":
        tgt, q, _ = _tie()
        return RCase(name, tgt, 0.5, 6, q, q, zero, 0.55, False, True)
    if name == "nonfinite":
        b, q = _nonfinite()
        return RCase(name, b.tgt, b.case.leaf, b.case.min_pts, b.src, q, b.case.p6, b.case.outlier_ratio, False, False)
    R = real_clouds()
    if name == "demo":
        return RCase(name, R["td"], 1.0, 6, R["sd"], R["sd"], zero, 0.55, False, False)
    if name == "raw":
        q = np.ascontiguousarray(R["src"][::4])
        return RCase(name, R["tgt"], 0.5, 6, q, q, zero, 0.55, True, False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def build(name, radius_in_leaves=1.0):
    """Built(case, vox, ids, d2, count, margin_ulps, equal_rows): the oracle's grid of the target and the restatement at radius = radius_in_leaves * leaf."""
    c = case(name)
    vox = NC.oracle_grid(11, c.leaf, c.min_pts) if name in NC_CASES or name == "nonfinite" else O.voxel_build(c.tgt, np.float32(c.leaf), c.min_pts)
    ids, d2, count, margin, eq = restate(vox, c.min_pts, c.trans, radius_in_leaves * c.leaf)
    for a in (ids, d2, count):
        a.setflags(write=False)
    return Built(c, vox, ids, d2, count, margin, eq)


def rejected_leaves(vox):
    return np.flatnonzero(np.asarray(vox["leaf_n"]) == -1)


def gauss_d1(leaf, outlier_ratio):
    return NC.gauss_constants(float(leaf), float(outlier_ratio))[0]


# ---- derivatives over the radius ids ---------------------------------------------------------------------------------------------------------------------------------
def dist(got, want):
    """(score, g, H) distances in the units of the bars: |ds| / |s|, max |dg| / max |g|, max |dH| / max |H| (0 / 0 = 0)."""
    out = []
    for a, b in zip(got, want):
        d, m = float(np.abs(np.asarray(a) - np.asarray(b)).max()), float(np.abs(np.asarray(b)).max())
        out.append(0.0 if d == 0.0 else (d / m if m > 0 else np.inf))
    return out


def oracle_derivatives(b, compute_hessian=True):
    """orc_ndt_derivatives_n over the restatement's ids (any width)."""
    c = b.case
    score, g, H = C.c_double(0), np.zeros(6), np.zeros((6, 6))
    ids = np.ascontiguousarray(b.ids)
    O.lib().orc_ndt_derivatives_n(C.c_int(len(c.src)), O._p(np.ascontiguousarray(c.src)), O._p(np.ascontiguousarray(c.trans)), C.c_int(ids.shape[1]), O._p(ids),
                                  O._p(np.ascontiguousarray(b.vox["mean"])), O._p(np.ascontiguousarray(b.vox["icov"])), O._p(O._d(c.p6)), C.c_double(c.leaf), C.c_double(c.outlier_ratio),
                                  C.c_int(1 if compute_hessian else 0), C.byref(score), O._p(g), O._p(H))
    return score.value, g, H


DERIV = [n for n in NAMES if n != "nonfinite"]          # the NDT calls require a finite cloud (include/lvx.h)
