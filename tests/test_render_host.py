"""Coloured map / overlay without a GPU: the per-point math the kernels run (lvi-exc_amd/csrc/lvx_render.h, built here with g++ -O2 -ffp-contract=off) against a numpy
float64 restatement of the reference's lines (tests/render_cases.py: lvi_initialize_surfel_orb.cpp:749-793 and :1343-1353), records byte for byte; and the C ABI exports
the five calls.  Every case: a 48 x 64 image with pitch 72 and random grey values, a few hundred points, fixed seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import render_cases as rc

F32 = np.float32


def _bytes_equal(a, b):
    return a.tobytes() == b.tobytes()


def test_library_exports_the_render_calls():
    l = lvx.lib()
    for name in ("lvx_evaluate_camera_pose", "lvx_render_default_options", "lvx_render_map", "lvx_render_map_d", "lvx_overlay_scans"):
        assert hasattr(l, name), name
    assert lvx.POINT_XYZRGB.itemsize == 16 and rc.host_lib().rh_record_size() == 16
    assert [lvx.POINT_XYZRGB.fields[k][1] for k in ("x", "y", "z", "b", "g", "r", "a")] == [0, 4, 8, 12, 13, 14, 15]
    assert l.lvx_evaluate_camera_pose(None, None, C.c_int(0), None, None, None, None) == lvx.E_ARG
    assert l.lvx_render_default_options(None) == lvx.E_ARG
    assert l.lvx_render_map(None, None, C.c_double(0), C.c_int(0), None, C.c_int(1), None, C.c_int(0), None, None, None, None, None) == lvx.E_ARG
    assert l.lvx_render_map_d(None, None, C.c_double(0), C.c_int(0), None, C.c_int(1), None, C.c_int(0), None, None, None, None, None) == lvx.E_ARG
    assert l.lvx_overlay_scans(None, None, C.c_int(0), None, None, None, None, None) == lvx.E_ARG
    o = lvx.RenderOptions()
    assert l.lvx_render_default_options(C.byref(o)) == lvx.OK and (o.z_min, o.z_max) == (0.1, 15.0)


@pytest.mark.parametrize("distortion", [rc.RADTAN, {}], ids=["radtan_k3", "no_distortion"])
@pytest.mark.parametrize("seed", [11, 12])
def test_render_point_matches_the_restatement(seed, distortion):
    """Random poses (the quaternions are NOT unit: both sides normalise, :724,744), points over all three classes, NaN in each coordinate."""
    rng = np.random.default_rng(seed)
    cam = rc.make_camera(**distortion)
    L0, Cp = rc.random_pose(rng, 1.7), rc.random_pose(rng, 0.6)
    img = rc.make_images(seed)
    pts = rc.random_points(rng, 400, L0, Cp, cam)
    for k in range(3):
        pts[5 + 7 * k::41, k] = np.nan
    ref, st_ref, zuv = rc.np_render_one(pts, L0, Cp, cam, img[0])
    rc.assert_margin(zuv)
    got, st, n = rc.host_render(pts, L0, [Cp], [1], cam, img)
    for cls in (0, 1, 2):
        assert (st_ref == cls).sum() > 40
    assert np.array_equal(st, st_ref) and _bytes_equal(got, ref) and n == (ref["a"] == 255).sum()
    nan = np.isnan(pts[:, :3]).any(axis=1)
    assert nan.sum() >= 25 and not got[nan].tobytes().strip(b"\0")
    out = st == 1
    assert np.array_equal(got["x"][out], pts[out, 0]) and not got["a"][out].any() and not got["r"][out].any()
    col = st == 2
    assert (got["a"][col] == 255).all() and np.array_equal(got["r"][col], got["g"][col]) and np.array_equal(got["g"][col], got["b"][col])


def _edge_points(rows):
    return np.array([r + (0.0,) for r in rows], dtype=F32)


def test_depth_limits_are_inclusive():
    """Identity poses, unit focal scale: pt_C.z is the point's z exactly.  :757 drops z < z_min and z > z_max, so a depth ON a limit is kept.  Default limits: 15 is a
    float, 0.1 is not — its float neighbours straddle it; limits 0.125 / 12.5 are floats on both ends."""
    cam = rc.make_camera(**rc.UNIT_CAMERA)
    img = rc.make_images(3)
    up, dn = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))
    for z_min, z_max, lo_in, lo_out in ((0.1, 15.0, F32(0.1), dn(0.1)), (0.125, 12.5, F32(0.125), dn(0.125))):
        assert float(lo_in) >= z_min > float(lo_out)
        zs = [lo_in, lo_out, F32(z_max), up(z_max), dn(z_max)]
        pts = _edge_points([(0.0, 0.0, float(z)) for z in zs])
        pts[:, 0], pts[:, 1] = F32(2.5) * pts[:, 2], F32(3.5) * pts[:, 2]   # uv = (2.5, 3.5) up to a float rounding: pixel (2, 3)
        ref, st_ref, _ = rc.np_render_one(pts, rc.IDENTITY, rc.IDENTITY, cam, img[0], z_min, z_max)
        got, st, _ = rc.host_render(pts, rc.IDENTITY, [rc.IDENTITY], [1], cam, img, z_min, z_max)
        assert list(st_ref) == [2, 0, 2, 0, 2] and np.array_equal(st, st_ref) and _bytes_equal(got, ref)


def test_image_bounds_of_render_and_overlay_differ():
    """uv from exact binary fractions (identity poses, unit focal scale, z = 1 or 2).  RenderMap tests int(uv) (:781): uv in (-1, 0) truncates to 0 and takes row / column 0;
    uv in [cols - 1, cols) is the last column; uv >= cols and uv <= -1 are outside with xyz kept.  The overlay tests uv < 0 on the doubles (:1350): (-1, 0) is OUTSIDE."""
    cam = rc.make_camera(**rc.UNIT_CAMERA)
    img = rc.make_images(4)
    rows = [(-0.5, 5.0, 1.0), (-0.96875, 5.25, 1.0), (7.5, -0.5, 1.0), (7.0, -0.25, 2.0), (-0.5, -0.5, 1.0),   # (-1, 0) on u, on v, on both
            (63.0, 4.5, 1.0), (63.96875, 4.5, 1.0), (127.5, 9.0, 2.0), (3.5, 47.0, 1.0), (3.5, 47.75, 1.0),      # last column / last row
            (64.0, 4.5, 1.0), (64.5, 4.5, 1.0), (3.5, 48.0, 1.0), (129.0, 4.0, 2.0),                              # >= cols, >= rows
            (-1.0, 5.0, 1.0), (5.0, -1.0, 1.0), (-2.5, 5.0, 1.0),                                                  # <= -1
            (0.0, 0.0, 1.0), (10.5, 20.25, 1.0)]
    pts = _edge_points(rows)
    expect_px = [(0, 5), (0, 5), (7, 0), (3, 0), (0, 0), (63, 4), (63, 4), (63, 4), (3, 47), (3, 47), None, None, None, None, None, None, None, (0, 0), (10, 20)]
    ref, st_ref, zuv = rc.np_render_one(pts, rc.IDENTITY, rc.IDENTITY, cam, img[0])
    got, st, _ = rc.host_render(pts, rc.IDENTITY, [rc.IDENTITY], [1], cam, img)
    assert np.array_equal(st, st_ref) and _bytes_equal(got, ref)
    for i, px in enumerate(expect_px):
        assert (got["x"][i], got["y"][i], got["z"][i]) == tuple(pts[i, :3])   # in depth range: xyz kept either way
        if px is None:
            assert st[i] == 1 and got["a"][i] == 0 and got["r"][i] == 0
        else:
            assert st[i] == 2 and got["a"][i] == 255 and got["r"][i] == img[0][px[1], px[0]]
    q, p = rc.IDENTITY
    pix_ref, _ = rc.np_overlay(pts, q, p, cam)
    pix, _ = rc.host_overlay(pts, q, p, cam)
    assert np.array_equal(pix, pix_ref)
    for i, px in enumerate(expect_px):
        negative = rows[i][0] < 0 or rows[i][1] < 0
        assert pix[i] == (-1 if px is None or negative else px[1] * rc.COLS + px[0])
    assert (pix[:5] == -1).all() and (st[:5] == 2).all()   # the two functions differ exactly here


@pytest.mark.parametrize("distortion", [rc.RADTAN, {}], ids=["radtan_k3", "no_distortion"])
def test_projection_overflow_is_outside(distortion):
    """A lowered z_min lets a depth of 1e-38 .. 1e-45 through: x / z reaches 1e38 .. 1e45, its sixth power overflows with k3 != 0 (inf, then NaN through inf - inf or
    0 * inf).  The reference would cast that to int (undefined); both sides call it outside: xyz kept, no colour, no crash."""
    cam = rc.make_camera(**distortion)
    img = rc.make_images(5)
    tiny = [F32(1e-38), F32(1e-42), F32(1e-45), F32(3e-39)]
    pts = _edge_points([(1.0, -2.0, float(z)) for z in tiny] + [(0.0, 0.0, float(tiny[0])), (1e-30, 0.0, float(tiny[0])), (1.0, 1.0, 0.0)])
    ref, st_ref, zuv = rc.np_render_one(pts, rc.IDENTITY, rc.IDENTITY, cam, img[0], 1e-300, 15.0)
    got, st, _ = rc.host_render(pts, rc.IDENTITY, [rc.IDENTITY], [1], cam, img, 1e-300, 15.0)
    assert np.array_equal(st, st_ref) and _bytes_equal(got, ref)
    assert (st[:4] == 1).all() and not got["a"][:4].any() and np.array_equal(got["x"][:4], pts[:4, 0])
    assert st[4] == 2 and st[6] == 0   # x = y = 0 projects to the principal point however small z is; z = 0 is below any positive z_min
    assert not np.isfinite(zuv[:4, 1:]).all() or (np.abs(zuv[:4, 1:]) >= 2.0 ** 30).all()


def test_lowest_valid_image_wins():
    """Three candidate images, the first one invalid (its pose did not evaluate): a point takes the colour of the lowest-index valid image that sees it."""
    rng = np.random.default_rng(21)
    cam = rc.make_camera(**rc.RADTAN)
    L0 = rc.random_pose(rng)
    cams = [rc.random_pose(rng) for _ in range(3)]
    cams[2] = (cams[1][0], cams[1][1] + np.array([3.0, -2.0, 0.5]))   # overlapping views, neither containing the other
    imgs = rc.make_images(6, 3)
    pts = np.concatenate([rc.random_points(rng, 200, L0, cams[k], cam) for k in range(3)])
    valid = [0, 1, 1]
    for k in (1, 2):
        rc.assert_margin(rc.np_render_one(pts, L0, cams[k], cam, imgs[k])[2])
    ref, st_ref = rc.np_render(pts, L0, cams, valid, cam, imgs)
    got, st, n = rc.host_render(pts, L0, cams, valid, cam, imgs)
    assert np.array_equal(st, st_ref) and _bytes_equal(got, ref) and n == (ref["a"] == 255).sum()
    one = [rc.np_render_one(pts, L0, cams[k], cam, imgs[k])[1] for k in range(3)]
    first, second = one[1] == 2, (one[1] != 2) & (one[2] == 2)
    assert first.sum() > 30 and second.sum() > 10 and (first & (one[2] == 2)).sum() > 10
    assert np.array_equal(got["r"][first], rc.np_render_one(pts, L0, cams[1], cam, imgs[1])[0]["r"][first])
    assert np.array_equal(got["r"][second], rc.np_render_one(pts, L0, cams[2], cam, imgs[2])[0]["r"][second])
    assert ((got["a"] == 255) == (first | second)).all()
    none, _, n0 = rc.host_render(pts, L0, cams, [0, 0, 0], cam, imgs)
    assert n0 == 0 and not none.tobytes().strip(b"\0")


@pytest.mark.parametrize("distortion", [rc.RADTAN, {}], ids=["radtan_k3", "no_distortion"])
def test_overlay_point_matches_the_restatement(distortion):
    rng = np.random.default_rng(31)
    cam = rc.make_camera(**distortion)
    pose_L, pose_C = rc.random_pose(rng), rc.random_pose(rng)
    q, p = rc.host_overlay_chain(pose_L, pose_C)
    # q_LtoC = q_CtoG* (x) q_LtoG, p_LinC = q_CtoG* (p_LinG - p_CinG) (:1335-1336) against rotation matrices
    RL, RC = rc.np_rotation(pose_L[0]), rc.np_rotation(pose_C[0])
    assert np.abs(rc.np_rotation(q) - RC.T @ RL).max() < 1e-14 and np.abs(p - RC.T @ (pose_L[1] - pose_C[1])).max() < 1e-14
    # scan points = the camera-frame construction of the map points with the LiDAR pose in the place of T_L0inG
    pts = rc.random_points(rng, 400, pose_L, pose_C, cam)
    pts[3::50, 0] = np.nan
    pix_ref, zuv = rc.np_overlay(pts, q, p, cam)
    rc.assert_margin(zuv, z_min=0.0, z_max=np.inf)
    pix, zuv_h = rc.host_overlay(pts, q, p, cam)
    assert np.array_equal(pix, pix_ref)
    assert (pix >= 0).sum() > 40 and (zuv[:, 0] < 0).sum() > 40 and ((pix < 0) & (zuv[:, 0] > 0)).sum() > 40
    assert pix.max() < rc.ROWS * rc.COLS and (pix[np.isnan(pts[:, 0])] == -1).all()


def test_host_mirror_candidates_matching_and_pcd(tmp_path):
    """lvx_calibrate.hpp: RenderMap's candidates (i = 50, 50 + size / 10, ...; a step of 0 gives one), the first image with img_t > scan_t within 0.05 s
    (lvi_initialize_surfel_orb.cpp:729-733, 1319-1327), and the PCD the reference saves (fields x y z rgb, the packed colour a << 24 | r << 16 | g << 8 | b)."""
    libdir = os.path.join(rc.ROOT, "lvi-exc_amd")
    exe, pcd = str(tmp_path / "render_host_demo"), str(tmp_path / "map.pcd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(rc.ROOT, "tests", "native", "render_host_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, pcd], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["candidates 5:", "candidates 50:", "candidates 55: 50", "candidates 200: 50 70 90 110 130 150 170 190",
                                     "candidates 1000: 50 150 250 350 450 550 650 750 850 950", "match: 2 -1 5"]
    lines = open(pcd).read().splitlines()
    assert lines[1:11] == ["VERSION 0.7", "FIELDS x y z rgb", "SIZE 4 4 4 4", "TYPE F F F U", "COUNT 1 1 1 1", "WIDTH 3", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS 3", "DATA ascii"]
    assert lines[11:] == ["0 0 0 0", "1.5 -2.25 0.100000001 0", "3 4 5 %d" % ((255 << 24) | (200 << 16) | (200 << 8) | 200)]
