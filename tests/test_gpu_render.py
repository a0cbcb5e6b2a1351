"""Coloured map and LiDAR-to-image overlay on the device (lvi-exc_amd/csrc/lvx_render.hip): the batched camera pose against the LiDAR-pose evaluation, the rendering and
overlay kernels byte for byte against the g++ build of the same per-point header (tests/native/render_host_check.cpp; both built without FP contraction), the
device-resident variant against the host-buffer one, and the error codes.  All inputs are generated; images are 48 x 64 with pitch 72."""
import numpy as np
import pytest

import lvx
import render_cases as rc
import synth

pytestmark = pytest.mark.gpu
TAU = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU


@pytest.fixture(scope="module")
def scene():
    """One problem, one context with the small test camera, the poses every test needs (read-only)."""
    P = synth.make_problem(seed=41, duration=1.5, n_surfel=0, n_planes=1, n_landmarks=0)
    g = lvx.Context(0)
    lvx.load_problem(g, P, TAU)
    cam = rc.make_camera(**rc.RADTAN)
    g.set_camera(cam["rows"], cam["cols"], 0.0, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"])
    s = np.ascontiguousarray(P["state_true"], np.float64)
    t_map = P["t_map"]
    image_t = np.array([P["t0"] - 1.0, 0.8 * P["t_start"] + 0.2 * P["t_end"], 0.15 * P["t_start"] + 0.85 * P["t_end"]])   # image 0 lies outside the spline
    qL, pL, okL = lvx.eval_lidar_pose(g, s, [t_map])
    qC, pC, okC = lvx.eval_camera_pose(g, s, image_t)
    assert okL[0] and list(okC) == [False, True, True]
    yield dict(P=P, g=g, cam=cam, state=s, t_map=t_map, image_t=image_t, L0=(qL[0], pL[0]), cams=[(qC[k], pC[k]) for k in range(3)], images=rc.make_images(8, 3))
    g.close()


def test_camera_pose_is_the_lidar_evaluation_with_the_camera_extrinsics(scene):
    """evaluateCameraPose and evaluateLidarPose are one evaluation with two sets of extrinsics (trajectory_manager_lvi.cpp:398-408, 430-440): with the camera's
    (q, p, time offset) in the LiDAR slots of a copied state, lvx_evaluate_lidar_pose gives the camera poses.  500 times plus before t0, exactly t_max, exactly t0."""
    P, g, s = scene["P"], scene["g"], scene["state"]
    N = P["n_knots"]
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.uniform(P["t_start"], P["t_end"], 500), [P["t0"] - 1.0, P["t0"] + (N - 3) * P["dt"], P["t0"]]])
    s2 = s.copy()
    s2[7 * N + 16:7 * N + 24] = s[7 * N + 24:7 * N + 32]
    qo, po, oko = lvx.eval_lidar_pose(g, s2, t)
    qg, pg, okg = lvx.eval_camera_pose(g, s, t)
    assert np.array_equal(oko, okg) and okg[:500].all() and not okg[500] and not okg[501] and okg[502]
    assert np.abs(qo[oko] - qg[okg]).max() < 1e-13 and np.abs(po[oko] - pg[okg]).max() < 1e-12
    # and composed in numpy: the spline pose (identity extrinsics, the camera's time offset) times the camera extrinsics
    s3 = s.copy()
    s3[7 * N + 16:7 * N + 23] = [0, 0, 0, 1, 0, 0, 0]
    s3[7 * N + 23] = s[7 * N + 31]
    qi, pi, oki = lvx.eval_lidar_pose(g, s3, t)
    q_c, p_c = s[7 * N + 24:7 * N + 28], s[7 * N + 28:7 * N + 31]
    assert np.array_equal(oki, okg)
    assert np.abs(synth.qmul(qi[oki], np.broadcast_to(q_c, qi[oki].shape)) - qg[okg]).max() < 1e-13
    assert np.abs(synth.qrot(qi[oki], np.broadcast_to(p_c, pi[oki].shape)) + pi[oki] - pg[okg]).max() < 1e-12


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5003])
def test_render_map_one_image_equals_the_host_header(scene, n):
    """One image = the reference's RenderMap.  Sizes around the wavefront (64) and the workgroup (256) and one of several workgroups with a ragged tail; about half the
    points are skipped, a quarter outside the image, a quarter coloured."""
    g, cam, k = scene["g"], scene["cam"], 1
    rng = np.random.default_rng(100 + n)
    pts = rc.random_points(rng, n, scene["L0"], scene["cams"][k], cam)
    pts[::29, n % 3] = np.nan
    rc.assert_margin(rc.host_render_uv(pts, scene["L0"], scene["cams"][k], cam))
    ref, st, n_ref = rc.host_render(pts, scene["L0"], [scene["cams"][k]], [1], cam, scene["images"][k:k + 1])
    got, valid, n_col = lvx.render_map(g, scene["state"], scene["t_map"], pts, scene["images"][k], scene["image_t"][k])
    if n >= 63:   # (one point is one class)
        for cls in (0, 1, 2):
            assert (st == cls).sum() > 0
    assert list(valid) == [True]
    assert got.tobytes() == ref.tobytes()
    assert n_col == (got["a"] == 255).sum() == n_ref


def test_render_map_beyond_one_grid_pass(scene):
    """The launch is capped at 8 workgroups of 256 per compute unit (2 048 on the 256 CUs of an MI355X); beyond 524 288 points the lanes loop.  One size past that with a
    ragged tail: every record still equals the host's, the counter still adds up."""
    g, cam, k = scene["g"], scene["cam"], 2
    n = 256 * 8 * 256 + 777
    pts = rc.random_points(np.random.default_rng(5), n, scene["L0"], scene["cams"][k], cam)
    rc.assert_margin(rc.host_render_uv(pts, scene["L0"], scene["cams"][k], cam))
    ref, st, n_ref = rc.host_render(pts, scene["L0"], [scene["cams"][k]], [1], cam, scene["images"][k:k + 1])
    got, valid, n_col = lvx.render_map(g, scene["state"], scene["t_map"], pts, scene["images"][k], scene["image_t"][k])
    assert got.tobytes() == ref.tobytes() and n_col == n_ref == (ref["a"] == 255).sum() > n // 8


def test_render_map_three_images_lowest_valid_index(scene):
    g, cam = scene["g"], scene["cam"]
    rng = np.random.default_rng(7)
    pts = np.concatenate([rc.random_points(rng, 1500, scene["L0"], scene["cams"][k], cam) for k in (1, 2)])
    for k in (1, 2):
        rc.assert_margin(rc.host_render_uv(pts, scene["L0"], scene["cams"][k], cam))
    cams = [rc.IDENTITY] + scene["cams"][1:]   # (the pose of an invalid image is never read)
    ref, st, n_ref = rc.host_render(pts, scene["L0"], cams, [0, 1, 1], cam, scene["images"])
    a = lvx.render_map(g, scene["state"], scene["t_map"], pts, scene["images"], scene["image_t"])
    b = lvx.render_map(g, scene["state"], scene["t_map"], pts, scene["images"], scene["image_t"])
    assert list(a[1]) == [False, True, True]
    assert a[0].tobytes() == ref.tobytes() and a[2] == n_ref == (ref["a"] == 255).sum()
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2]
    # the colours really come from both images: image 1 where it sees the point, image 2 only where image 1 does not
    one = [rc.host_render(pts, scene["L0"], [scene["cams"][k]], [1], cam, scene["images"][k:k + 1]) for k in (1, 2)]
    first, second = one[0][1] == 2, (one[0][1] != 2) & (one[1][1] == 2)
    assert first.sum() > 100 and second.sum() > 100
    assert np.array_equal(a[0]["r"][first], one[0][0]["r"][first]) and np.array_equal(a[0]["r"][second], one[1][0]["r"][second])


def test_render_map_errors_and_empty_input(scene):
    g, cam, P = scene["g"], scene["cam"], scene["P"]
    pts = rc.random_points(np.random.default_rng(1), 300, scene["L0"], scene["cams"][1], cam)
    out = np.full(300, 7, dtype=np.uint8).repeat(16).view(lvx.POINT_XYZRGB)
    import ctypes as C
    valid, ncol = np.ones(1, np.int32), C.c_int64(5)
    img, it, s = scene["images"][1], scene["image_t"][1:2].copy(), scene["state"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda t_map, n, n_images=1, pitch=rc.PITCH: g._l.lvx_render_map(g._h, p(s), C.c_double(t_map), C.c_int(n), p(pts), C.c_int(n_images), p(img), C.c_int(pitch), p(it), None, p(out), p(valid),
                                                                            C.byref(ncol))
    # map time outside the spline: the reference's early return (:720-723) — LVX_E_RANGE, zero records
    assert call(P["t0"] - 1.0, 300) == lvx.E_RANGE
    assert not out.tobytes().strip(b"\0") and ncol.value == 0 and valid[0] == 0
    assert call(scene["t_map"], 300, n_images=0) == lvx.E_ARG and call(scene["t_map"], 300, n_images=33) == lvx.E_ARG
    assert call(scene["t_map"], 300, pitch=rc.COLS - 1) == lvx.E_ARG
    out[:] = np.full(16, 7, np.uint8).view(lvx.POINT_XYZRGB)[0]
    assert call(scene["t_map"], 0) == lvx.OK and (out.view(np.uint8) == 7).all()   # zero points: nothing written
    assert call(scene["t_map"], 300) == lvx.OK and valid[0] == 1 and ncol.value == (out["a"] == 255).sum() > 0
    # no camera: LVX_E_STATE
    g2 = lvx.Context(0)
    g2.set_spline(P["t0"], P["dt"], P["n_knots"])
    assert g2._l.lvx_render_map(g2._h, p(s), C.c_double(scene["t_map"]), C.c_int(300), p(pts), C.c_int(1), p(img), C.c_int(rc.PITCH), p(it), None, p(out), p(valid), C.byref(ncol)) == lvx.E_STATE
    g2.close()


@pytest.fixture(scope="module")
def sequence():
    """A short recorded-sequence stand-in with organised scans (synth.make_sequence), the test camera set on its context."""
    import torch   # device buffers of the _d call
    S = synth.make_sequence(seed=50, duration=1.5, n_reproj=300)
    g = lvx.Context(0)
    g.set_spline(S["t0"], S["dt"], S["n_knots"])
    cam = rc.make_camera(**rc.RADTAN)
    g.set_camera(cam["rows"], cam["cols"], 0.0, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"])
    raw = np.zeros(S["scans"].shape, dtype=lvx.POINT_XYZIT)
    for k in ("x", "y", "z", "timestamp"):
        raw[k] = S["scans"][k]
    yield dict(S=S, g=g, cam=cam, raw=raw, state=np.ascontiguousarray(S["state0"], np.float64), torch=torch)
    g.close()


def test_render_map_d_on_the_scans_of_the_last_association(sequence):
    """map_xyzi4_d == NULL: the cloud is what lvx_data_association left on the device; the records equal lvx_render_map fed with lvx_get_scans_in_map.  Before any
    association: LVX_E_STATE."""
    S, g, torch, s = sequence["S"], sequence["g"], sequence["torch"], sequence["state"]
    n = sequence["raw"].size
    images = rc.make_images(9, 2)
    image_t = np.array([S["t_map"] + 0.2, S["t_map"] + 0.5])
    img_d = torch.from_numpy(images).cuda()
    out_d = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (g, s, S["t_map"], img_d.data_ptr(), 2, rc.PITCH, image_t, out_d.data_ptr())
    with pytest.raises(lvx.LvxError) as e:
        lvx.render_map_d(*args)
    assert e.value.code == lvx.E_STATE
    lvx.set_scans(g, sequence["raw"], S["H"], S["W"])
    with pytest.raises(lvx.LvxError) as e:
        lvx.render_map_d(*args)
    assert e.value.code == lvx.E_STATE
    npl, npt = lvx.data_association(g, s, S["t_map"])
    assert npl > 0 and npt > 0
    valid_d, ncol_d = lvx.render_map_d(*args)
    got = out_d.cpu().numpy().view(lvx.POINT_XYZRGB)
    cloud = lvx.get_scans_in_map(g, len(S["scans"]), S["H"], S["W"]).reshape(-1, 4)
    ref, valid, ncol = lvx.render_map(g, s, S["t_map"], cloud, images, image_t)
    assert len(got) == len(ref) == n and list(valid_d) == list(valid) == [True, True]
    assert got.tobytes() == ref.tobytes() and ncol_d == ncol == (ref["a"] == 255).sum()
    assert ncol > 100 and (ref["a"] == 0).sum() > 100
    # the host-buffer call on the resident cloud (what the header-only stage driver uses): nothing uploaded but the images
    res, _, ncol_r = lvx.render_map(g, s, S["t_map"], None, images, image_t, n_resident=n)
    assert res.tobytes() == ref.tobytes() and ncol_r == ncol
    # an explicit device cloud takes the same path
    cloud_d = torch.from_numpy(cloud[:1001].copy()).cuda()
    out2 = torch.zeros(1001 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lvx.render_map_d(g, s, S["t_map"], img_d.data_ptr(), 2, rc.PITCH, image_t, out2.data_ptr(), map_d_ptr=cloud_d.data_ptr(), n=1001)
    assert out2.cpu().numpy().tobytes() == ref[:1001].tobytes()


def test_overlay_scans_equals_the_host_header(sequence):
    """Pairs (scan 3, a valid image time), (scan 4, an image time outside the spline), (scan 3 again).  Host side: the scan de-skewed rotation-only into its own frame by
    lvx_undistort_scan (the reference's scan_data_), the chain q_LtoC / p_LinC from the two evaluated poses, overlay_point per point."""
    S, g, cam, s, raw = sequence["S"], sequence["g"], sequence["cam"], sequence["state"], sequence["raw"]
    lvx.set_scans(g, raw, S["H"], S["W"])
    scan_t = np.array([raw["timestamp"][3].min(), raw["timestamp"][4].min(), raw["timestamp"][3].min()])
    image_t = np.array([scan_t[0] + 0.03, S["t0"] - 5.0, scan_t[0] + 0.03])
    mask, valid = lvx.overlay_scans(g, s, [3, 4, 3], scan_t, image_t, rc.ROWS, rc.COLS)
    assert list(valid) == [True, False, True]
    assert not mask[1].any() and np.array_equal(mask[0], mask[2])
    qL, pL, okL = lvx.eval_lidar_pose(g, s, scan_t[:1])
    qC, pC, okC = lvx.eval_camera_pose(g, s, image_t[:1])
    assert okL[0] and okC[0]
    pts = lvx.undistort(g, s, raw[3], synth.qconj(qL[0]), pL[0], correct_position=False)
    q, p = rc.host_overlay_chain((qL[0], pL[0]), (qC[0], pC[0]))
    pix, zuv = rc.host_overlay(pts, q, p, cam)
    rc.assert_margin(zuv, z_min=0.0, z_max=np.inf)
    ref = np.zeros(rc.ROWS * rc.COLS, np.uint8)
    ref[pix[pix >= 0]] = 1
    assert ref.sum() > 50 and (pix < 0).sum() > 50 and np.isnan(pts[:, 0]).sum() > 0
    assert mask[0].tobytes() == ref.tobytes() and set(np.unique(mask)) == {0, 1}
    with pytest.raises(lvx.LvxError) as e:
        lvx.overlay_scans(g, s, [len(raw)], scan_t[:1], image_t[:1], rc.ROWS, rc.COLS)
    assert e.value.code == lvx.E_ARG
