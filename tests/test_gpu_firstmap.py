"""GPU: the first DataAssociation of a calibration from per-scan odometry poses (lvx_data_association_poses) at the cases of tests/firstmap_cases.py
(tests/test_firstmap_cases.py holds each case to what it claims on the CPU), through lvx.set_scans / lvx.data_association_poses.

Stage by stage, each stage's expectation computed from the GPU's output of the stage before (one float of the de-skew that rounds the other way may move a point into
another voxel, it cannot hide a wrong rule downstream):
  key flags        equal to the numpy restatement of checkKeyScan
  scans in map     NaN pattern equal, intensity bit-equal, every coordinate inside +-30 m and within 4e-6 m (float32 outputs of FP64 poses), < 0.1 % of the floats not
                   bit-equal; points whose own stamp lies outside the spline exactly on float32(T[:3, 3]); absent scans NaN with intensity 0
  surfel map       oracle voxel grid + setSurfelMap on the GPU's KEY scans, plane_lambda = 0.6: leaves, point / inlier counts, plane types, AABBs exact, planes 1e-9
  SurfelPoints     oracle getAssociation of every scan on the GPU's scans and surfels: the list bit for bit

Reached here and by no older test: the Python binding of the call; thresholds other than 0.2 m / 5 deg; a distance exactly on the threshold; yaw, pitch and roll alone;
the +-360 wrap; absent scans in front of the first key scan; tau_lidar != 0; points on the zero-then-transform branch; has_pose = NULL and key_scan = NULL; H W below and
across 256; S = 1, 2, 3; every scan a key scan and exactly one; a refinement round speculating on capacities learned from a key-scan map; a call with no scan present."""
import ctypes as C

import numpy as np
import pytest

import firstmap_cases as FC
import lvx
from oracle import pipeline

pytestmark = pytest.mark.gpu

OPT = dict(pipeline.DEFAULTS, plane_lambda=0.6)          # SurfelAssociation's constructor value (lvi_initialize_surfel_orb.cpp:127, 240), passed explicitly on both sides
RUN = [c.name for c in FC.CASES if c.group in ("key_rule", "presence", "shapes")]


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _load(g, c):
    S = c.S()
    g.set_spline(S["t0"], S["dt"], S["n_knots"])
    lvx.set_scans(g, c.raw(), c.H, c.W)


def _raw_call(g, c, state=True, scan_t=True, poses=True, key=True):
    """lvx_data_association_poses over ctypes: (status, surfels, SurfelPoints, key flags or None).  False: that pointer is NULL."""
    a = dict(state=np.ascontiguousarray(c.state()) if state else None, scan_t=np.ascontiguousarray(c.scan_t()) if scan_t else None, poses=np.ascontiguousarray(c.poses()) if poses else None,
             has=np.ascontiguousarray(c.has_pose(), np.int32) if c.has_pose() is not None else None, key=np.full(c.n, 7, np.int32) if key else None)
    opt = lvx.assoc_default_options(g, plane_lambda=0.6)
    npl, npt = C.c_int32(-1), C.c_int32(-1)
    rc = g._l.lvx_data_association_poses(g._h, _p(a["state"]), _p(a["scan_t"]), _p(a["poses"]), _p(a["has"]), C.c_double(c.key_dist), C.c_double(c.key_angle), C.byref(opt), C.byref(npl),
                                         C.byref(npt), _p(a["key"]))
    return rc, npl.value, npt.value, a["key"]


def _fetch(g, c, npl, npt, key):
    return dict(key=None if key is None else np.array(key), n_planes=npl, n_points=npt, scans=lvx.get_scans_in_map(g, c.n, c.H, c.W), planes=lvx.get_surfel_map(g, npl).copy(),
                points=lvx.get_surfel_points(g, npt))


def _run(g, c, load=True):
    if load:
        _load(g, c)
    npl, npt, key = lvx.data_association_poses(g, c.state(), c.scan_t(), c.poses(), c.has_pose(), c.key_dist, c.key_angle, lvx.assoc_default_options(g, plane_lambda=0.6))
    return _fetch(g, c, npl, npt, key)


def _planes_dict(pl):
    return dict(p4=np.ascontiguousarray(pl["p4"]), Pi=np.ascontiguousarray(pl["Pi"]), box_min=np.ascontiguousarray(pl["box_min"]), box_max=np.ascontiguousarray(pl["box_max"]))


def _check_scans(label, want, got):
    """The project's bars for scans in the map frame (test_gpu_pipeline_oracle.py): NaN pattern, 4e-6 m inside +-30 m, < 1e-3 of the floats not bit-equal."""
    assert got.shape == want.shape and np.array_equal(np.isnan(want), np.isnan(got))
    assert want[..., 3].tobytes() == got[..., 3].tobytes()
    m = ~np.isnan(want)
    assert np.abs(got[..., :3][m[..., :3]]).max() < FC.ROOM
    diff = np.abs(want[m] - got[m])
    frac = np.count_nonzero(want[m].view(np.uint32) != got[m].view(np.uint32)) / m.sum()
    print("%-16s scans in the map frame: max |diff| %.2e m, %.4f %% of %d floats not bit-equal" % (label, diff.max(), 100 * frac, m.sum()))
    assert diff.max() <= 4e-6 and frac < 1e-3


def _check_map(S, scans, map_scans, got, opt, label):
    """Surfel map of `map_scans` and SurfelPoints of `scans`, both the GPU's, against the oracle."""
    po, pg = pipeline.surfel_map(map_scans, opt), got["planes"]
    assert len(pg) == len(po["p4"]) == got["n_planes"]
    if len(pg) == 0:
        assert got["n_points"] == 0
        print("%-16s no surfel" % label)
        return
    for k in ("leaf", "n_points", "n_inliers", "plane_type", "box_min", "box_max"):
        assert np.array_equal(pg[k], po[k]), k
    assert np.abs(pg["p4"] - po["p4"]).max() <= 1e-9 and np.abs(pg["Pi"] - po["Pi"]).max() <= 1e-9 * np.abs(po["Pi"]).max()
    eo = pipeline.associate(S, scans, _planes_dict(pg), opt)
    assert len(eo["t"]) == got["n_points"] == len(got["points"]["t"])
    for k in ("pt", "pt_map", "t", "plane"):
        assert np.ascontiguousarray(eo[k]).tobytes() == np.ascontiguousarray(got["points"][k]).tobytes(), k
    print("%-16s %d surfels, %d SurfelPoints" % (label, len(pg), got["n_points"]))


def _check(c, got):
    e = c.expected()
    # key flags
    assert got["key"].dtype == np.int32 and set(got["key"]) <= {0, 1}
    assert list(np.nonzero(got["key"])[0]) == e["key"]
    # scans in the map frame
    sg = got["scans"]
    _check_scans(c.name, e["scans"], sg)
    absent = ~e["present"]
    assert np.isnan(sg[absent][..., :3]).all() and not sg[absent][..., 3].any()
    s, i = np.nonzero(e["zeroed"])
    assert (len(s) > 0) == c.zeroed
    on_pose = c.poses().reshape(-1, 4, 4)[s, :3, 3].astype(np.float32)
    assert sg.reshape(c.n, -1, 4)[s, i, :3].tobytes() == on_pose.tobytes() and not sg.reshape(c.n, -1, 4)[s, i, 3].any()
    # surfel map of the key scans, SurfelPoints of every scan
    _check_map(c.S(), sg, sg[e["key"]], got, OPT, c.name)
    assert c.may_be_empty or (got["n_planes"] > 0 and got["n_points"] > 0)


def _same(a, b):
    return (a["scans"].tobytes() == b["scans"].tobytes() and a["planes"].tobytes() == b["planes"].tobytes() and a["n_points"] == b["n_points"]
            and all(np.ascontiguousarray(a["points"][k]).tobytes() == np.ascontiguousarray(b["points"][k]).tobytes() for k in ("pt", "pt_map", "t", "plane")))


@pytest.mark.parametrize("name", RUN)
def test_case_matches_stage_by_stage(ctx, name):
    c = FC.BY_NAME[name]
    _check(c, _run(ctx, c))


def test_one_key_scan_map_is_not_the_map_of_all_scans(ctx):
    """The selection, not the whole recording, fed the voxel grid: with one key scan the map of all scans has other surfels."""
    c = FC.BY_NAME["nondefault_one"]
    got = _run(ctx, c)
    assert list(np.nonzero(got["key"])[0]) == [0] and got["n_planes"] > 0
    every = pipeline.surfel_map(got["scans"], OPT)
    assert len(every["p4"]) != got["n_planes"]
    assert len(pipeline.surfel_map(got["scans"][:1], OPT)["p4"]) == got["n_planes"]


def test_key_scan_null_changes_nothing(ctx):
    c = FC.BY_NAME["mixed"]
    a = _run(ctx, c)
    rc, npl, npt, key = _raw_call(ctx, c, key=False)
    assert rc == lvx.OK and key is None and (npl, npt) == (a["n_planes"], a["n_points"])
    assert _same(a, _fetch(ctx, c, npl, npt, None))


def test_successive_calls_on_one_context():
    """All scans key -> one key scan (the key-scan map cloud shrinks) -> lvx_data_association (a refinement round, speculating on the capacities the key-scan maps left) ->
    all scans key again, the same bytes as the first time."""
    every, one = FC.BY_NAME["dense_all_key"], FC.BY_NAME["nondefault_one"]
    S = every.S()
    g = lvx.Context(0)
    try:
        _load(g, every)
        first = _run(g, every, load=False)
        _check(every, first)
        assert int(first["key"].sum()) == every.n
        second = _run(g, one, load=False)
        _check(one, second)
        assert second["n_planes"] < first["n_planes"]
        # the refinement round (plane_lambda 0.7, the map cloud = every scan at the spline's poses)
        before = lvx.data_association_stats(g)
        state = np.array(S["state_true"])
        npl, npt = lvx.data_association(g, state, S["t_map"])
        runs, misses = (a - b for a, b in zip(lvx.data_association_stats(g), before))
        print("refinement round after the key-scan maps: one-stop rounds +%d, repeated +%d" % (runs, misses))
        assert runs == 1 and misses in (0, 1)
        third = _fetch(g, every, npl, npt, None)
        _check_scans("refinement", pipeline.deskew_into_map(S, state), third["scans"])
        _check_map(S, third["scans"], third["scans"], third, pipeline.DEFAULTS, "refinement")
        assert npl > 0 and npt > 0
        fourth = _run(g, every, load=False)
        assert np.array_equal(fourth["key"], first["key"]) and _same(first, fourth)
    finally:
        g.close()


def _assert_empty(g, c, rc, npl, npt, key):
    assert rc == lvx.OK and (npl, npt) == (0, 0) and not key.any()
    planes = np.full(5, 7, np.uint8).repeat(lvx.SURFEL_PLANE.itemsize).view(lvx.SURFEL_PLANE)
    assert g._l.lvx_get_surfel_map(g._h, C.c_int(5), _p(planes)) == lvx.OK and (planes.view(np.uint8) == 7).all()
    pt, pm, t, pl = np.full((5, 3), 7.0), np.full((5, 3), 7.0), np.full(5, 7.0), np.full(5, 7, np.int32)
    assert g._l.lvx_get_surfel_points(g._h, C.c_int(5), _p(pt), _p(pm), _p(t), _p(pl)) == lvx.OK
    assert (pt == 7).all() and (pm == 7).all() and (t == 7).all() and (pl == 7).all()
    sg = lvx.get_scans_in_map(g, c.n, c.H, c.W)         # succeeds; absent scans: NaN (include/lvx.h), intensity 0 as the oracle's
    assert np.isnan(sg[..., :3]).all() and not sg[..., 3].any()
    assert sg.tobytes() == c.expected()["scans"].tobytes()


def test_no_scan_present_after_a_round_leaves_nothing_stale(ctx):
    """has_pose = 0 for every scan on a context whose buffers hold the previous round: LVX_OK, nothing in the map, the scans all NaN — to lvx_get_scans_in_map and to the
    map rendering that reads the same buffer — and the next call is the normal one again."""
    full, empty = FC.BY_NAME["has_pose_null"], FC.BY_NAME["empty_no_pose"]
    S = full.S()
    cam = S["camera"]
    ctx.set_camera(cam["rows"], cam["cols"], cam["readout"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"])
    image = np.full((cam["rows"], cam["cols"]), 90, np.uint8)
    a = _run(ctx, full)
    assert a["n_planes"] > 0 and a["n_points"] > 0
    render = lambda: lvx.render_map(ctx, S["state_true"], S["t_map"], None, image, S["t_map"], n_resident=full.n * full.H * full.W)
    rec, valid, n_col = render()
    assert list(valid) == [True] and n_col == (rec["a"] == 255).sum() > 0
    _assert_empty(ctx, empty, *_raw_call(ctx, empty))          # (the same scans stay set)
    rec, valid, n_col = render()
    assert list(valid) == [True] and n_col == 0 and not (rec["a"] == 255).any()
    b = _run(ctx, full, load=False)
    assert np.array_equal(a["key"], b["key"]) and _same(a, b)


def test_no_scan_present_on_a_fresh_context():
    """Every stamp outside the spline, nothing run before: the same answers, and lvx_get_scans_in_map has a buffer to read."""
    empty, full = FC.BY_NAME["empty_outside"], FC.BY_NAME["has_pose_null"]
    g = lvx.Context(0)
    try:
        _load(g, empty)
        _assert_empty(g, empty, *_raw_call(g, empty))
        _check(full, _run(g, full, load=False))
    finally:
        g.close()


def test_argument_and_state_errors(ctx):
    c = FC.BY_NAME["s2"]
    _load(ctx, c)
    for null in ("state", "scan_t", "poses"):
        assert _raw_call(ctx, c, **{null: False})[0] == lvx.E_ARG, null
    g = lvx.Context(0)
    try:
        msg = lambda: g._l.lvx_last_error(g._h).decode()
        assert _raw_call(g, c)[0] == lvx.E_STATE and msg() == "lvx_set_spline has not been called"
        S = c.S()
        g.set_spline(S["t0"], S["dt"], S["n_knots"])
        assert _raw_call(g, c)[0] == lvx.E_STATE and msg() == "lvx_set_scans has not been called"
        out = np.zeros((c.n, c.H, c.W, 4), np.float32)
        assert g._l.lvx_get_scans_in_map(g._h, _p(out)) == lvx.E_STATE
        _check(c, _run(g, c))                                   # and the context is usable afterwards
    finally:
        g.close()
