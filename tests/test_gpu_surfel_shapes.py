"""GPU: surfel map extraction (lvx_voxel_build + lvx_surfel_extract: k_surfel_extract, then k_surfel_compact_mb or k_surfel_compact) at the shapes of
tests/surfel_cases.py (tests/test_surfel_cases.py holds each case to its regime on the CPU), through the C ABI: against the oracle at the bars of
test_gpu_upstream.py::test_surfel_map_extraction, through check_result, and against the numpy restatement, which does not rest on the oracle.

Reached here and by no older test: leaves of 20 .. 5 200 points (one lane-trip, exactly one and two trips of 512, eleven trips), outliers in the first lanes only and in
the last partial trip only; 1 .. 4 100 leaves and 266 240 (a second trip of the count loop of k_surfel_compact_mb, 261 publishing workgroups, the cell table grown);
nothing / everything / only the first / only the last / both sides of a workgroup seam accepted; every threshold from both sides, a point exactly ON dist_threshold;
leaves below min_points_per_voxel and a leaf the build rejected; normals exactly along the axes, planes through the origin, cells at +-100 m; the Jacobi fallback of the refit; k_surfel_compact at
all (switch TEST_COMPACT_ONE), also behind both chains of lvx_data_association; fewer publishing workgroups after more on one context; max_planes into sentinels."""
import ctypes as C
import functools

import numpy as np
import pytest

import lvx
import surfel_cases as SC
import synth
from surfel_cases import P4_BAR, PI_BAR

pytestmark = pytest.mark.gpu

DEV_P4, DEV_PI = 1e-9, 1e-9           # device against oracle: the bars of test_surfel_map_extraction


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_one():
    """k_surfel_compact (one workgroup) whatever the co-residency bound says."""
    c = lvx.Context(0)
    c.set_switch("TEST_COMPACT_ONE", 1)
    yield c
    c.close()


def _extract(g, name, **kw):
    """voxel_build(fetch=False) + surfel_extract of a case on context g: (records, count)."""
    c = SC.BY_NAME[name]
    p = c.params._replace(**kw)
    vi = lvx.voxel_build(g, c.cloud, SC.LEAF, p.min_pts, p.eig_mult, fetch=False)
    assert vi["n_leaves"] == SC.np_result(name)["n_leaves"]
    return lvx.surfel_extract(g, vi["n_leaves"], p.p_lambda, p.thr, p.min_leaf, p.min_inl)


@functools.lru_cache(maxsize=None)
def _fresh(name):
    """The case on a context of its own that has done nothing else."""
    g = lvx.Context(0)
    try:
        r, n = _extract(g, name)
        return r.copy(), n
    finally:
        g.close()


def _same_bytes(a, b):
    return a[1] == b[1] and a[0].tobytes() == b[0].tobytes()


def _hold(name, r, n):
    """Device against oracle, check_result, device against numpy."""
    c, ref, orc = SC.BY_NAME[name], SC.np_result(name), SC.oracle_result(name)
    assert n == len(r) == len(orc["leaf"]), (name, n, len(orc["leaf"]))
    m = SC.p4_compared(ref)
    dp4, dpi, same = SC.compare(r, orc, m)
    np4, npi, nsame = SC.compare(r, ref, m)
    print("%s: %d planes of %d leaves; device vs oracle p4 %.3e Pi %.3e; device vs numpy p4 %.3e Pi %.3e" % (name, n, ref["n_leaves"], dp4, dpi, np4, npi))
    tm = SC.type_compared(ref)
    assert same and nsame and np.array_equal(r["plane_type"][tm], orc["plane_type"][tm]) and np.array_equal(r["plane_type"][tm], ref["plane_type"][tm]), name
    assert dp4 <= DEV_P4 and dpi <= DEV_PI, (name, dp4, dpi)
    SC.check_result(c.cloud, c.params, r, ref=ref, normal_tol=P4_BAR + DEV_P4)
    assert np4 <= P4_BAR + DEV_P4 and npi <= PI_BAR + DEV_PI, (name, np4, npi)


@pytest.mark.parametrize("name", SC.SMALL)
def test_case_equals_oracle_and_numpy(ctx, name):
    """Every case on ONE context, one after the other (other leaf sizes, parameters and cloud sizes before it)."""
    r, n = _extract(ctx, name)
    _hold(name, r, n)


def test_the_266240_leaf_cloud():
    """A second trip of the count loop of k_surfel_compact_mb (more than 262 144 leaves), 261 publishing workgroups, the cell table grown past its 262 143 cells;
    planes planted at the first and last leaf and on both sides of the seams at 1 024 and 262 144."""
    r, n = _fresh("big")
    _hold("big", r, n)
    assert list(r["leaf"]) == list(SC.BIG_PLANTED)


# ------------------------------------------------------------------------------------------------------------------------
# both compactions
# ------------------------------------------------------------------------------------------------------------------------
def _scan_of(name, H=8, W=32):
    """A small organised scan: ring h holds the points of one accepted leaf (the first, the last and six between; NaN behind them) — all but the few that span the
    leaf's box lie strictly inside it, on the plane: every ring selects for its leaf's plane.  A case without planes: the first H W points of the cloud."""
    cloud, ref = np.asarray(SC.BY_NAME[name].cloud), SC.np_result(name)
    order, offs, keys = SC.cells(name)
    if not len(ref["leaf"]):
        return cloud[:H * W].reshape(H, W, 4).copy()
    scan = np.full((H, W, 4), np.nan, np.float32)
    for h, k in enumerate(np.linspace(0, len(ref["leaf"]) - 1, H).astype(np.int64)):
        li = ref["leaf"][k]
        pts = cloud[order[offs[li]:offs[li + 1]]][:W]
        scan[h, :len(pts)] = pts
    return scan


@pytest.mark.parametrize("name", SC.COMPACTION + ["big"])
def test_single_workgroup_compaction_equals_the_multi_workgroup_one(ctx, ctx_one, name):
    """TEST_COMPACT_ONE: k_surfel_compact with its own rank arithmetic (16 wavefront sums, the running offset, trips of 1 024 leaves) — the path of a partitioned
    or smaller part, which no map takes on a full MI355X.  Records and count byte for byte those of k_surfel_compact_mb, and the association fed with them agrees."""
    a = _fresh("big") if name == "big" else _extract(ctx, name)
    b = _extract(ctx_one, name)
    assert _same_bytes(a, b), name
    assert a[1] == len(SC.np_result(name)["leaf"])
    scan = _scan_of(name)
    fa = lvx.surfel_assoc(ctx, scan, a[0]["p4"], a[0]["box_min"], a[0]["box_max"], 0.05, 2)
    fb = lvx.surfel_assoc(ctx_one, scan, b[0]["p4"], b[0]["box_min"], b[0]["box_max"], 0.05, 2)
    assert np.array_equal(fa, fb) and (fa >= 0).any() == (a[1] > 0)
    if a[1]:
        assert {int(a[0]["leaf"][k]) for k in set(fa[fa >= 0])} >= {int(SC.np_result(name)["leaf"][0]), int(SC.np_result(name)["leaf"][-1])}   # first and last record reach their rings


def _da_context(S, one):
    g = lvx.Context(0)
    if one:
        g.set_switch("TEST_COMPACT_ONE", 1)
    g.set_spline(S["t0"], S["dt"], S["n_knots"])
    raw = np.zeros(S["scans"].shape, dtype=lvx.POINT_XYZIT)
    for k in ("x", "y", "z", "timestamp"):
        raw[k] = S["scans"][k]
    lvx.set_scans(g, raw, S["H"], S["W"])
    return g


def test_data_association_rounds_behind_the_single_workgroup_compaction():
    """The plane TABLE behind the records feeds the association grid of lvx_data_association: two rounds under TEST_COMPACT_ONE (the four-stop chain, then the one-stop
    chain with the leaf count on the device) give the surfel map and the SurfelPoints of the unswitched rounds, bit for bit."""
    S = synth.make_sequence(seed=50)
    x0 = np.ascontiguousarray(S["state0"], np.float64)
    x1 = x0.copy()
    x1[:3 * S["n_knots"]] += 2e-3 * np.random.default_rng(5).standard_normal(3 * S["n_knots"])
    g, h = _da_context(S, False), _da_context(S, True)
    try:
        for x in (x0, x1):
            res = []
            for c in (g, h):
                npl, npt = lvx.data_association(c, x, S["t_map"])
                res.append((npl, npt, lvx.get_surfel_map(c, npl), lvx.get_surfel_points(c, npt)))
            a, b = res
            assert a[:2] == b[:2] and a[0] > 100 and a[1] > 1000
            assert a[2].tobytes() == b[2].tobytes()
            for k in ("pt", "pt_map", "t", "plane"):
                assert np.array_equal(a[3][k], b[3][k]), k
        assert lvx.data_association_stats(g) == (1, 0) and lvx.data_association_stats(h) == (1, 0)      # the second round took the one-stop chain on both
    finally:
        g.close(); h.close()


def test_data_association_options_hold_the_two_definitions():
    """lvx_assoc_options::min_leaf_points: 0 and -3 mean 1, and below min_points_per_voxel it changes nothing (such leaves are never surfels) — with min_inliers = 3,
    so that small leaves are not hidden behind the inlier count.  One context: the first round four-stop, the others one-stop."""
    S = synth.make_sequence(seed=50)
    x = np.ascontiguousarray(S["state0"], np.float64)
    g = _da_context(S, False)
    try:
        def round_(**kw):
            npl, npt = lvx.data_association(g, x, S["t_map"], lvx.assoc_default_options(g, min_inliers=3, **kw))
            return npl, npt, lvx.get_surfel_map(g, npl).tobytes(), lvx.get_surfel_points(g, npt)["plane"].tobytes()
        one = round_(min_leaf_points=1)
        assert round_(min_leaf_points=0) == one and round_(min_leaf_points=-3) == one
        assert round_(min_leaf_points=6) == one                                      # min_points_per_voxel is 6: the leaves of 1 .. 5 points were no surfels anyway
        twelve = round_(min_leaf_points=12, min_points_per_voxel=12)
        assert round_(min_leaf_points=1, min_points_per_voxel=12) == twelve
        assert round_(min_leaf_points=10)[0] < one[0] and one[0] > 100               # and the option does bite where it is defined to
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------------
# one context, a sequence of calls
# ------------------------------------------------------------------------------------------------------------------------
def test_fewer_publishing_workgroups_after_more():
    """261 workgroups publish (epoch | count), then 1, then 3, then 261 again: the words are never cleared, only the epoch tells this launch's counts from the last
    one's.  Every call equals the case on a fresh context."""
    g = lvx.Context(0)
    try:
        for name in ("big", "leaves_5", "leaves_2049", "big"):
            assert _same_bytes(_extract(g, name), _fresh(name)), name
    finally:
        g.close()


def test_parameters_change_between_calls_on_one_build(ctx):
    """One build, p_lambda 0.7, 0.95, 0.7: the first and the third result are the same bytes (repeatability: the wavefront sums have a fixed order), the second a
    proper subset; and a build followed by look-ups and an association before the extraction gives what the build followed by the extraction gives."""
    name = "ppl_out_last"
    c = SC.BY_NAME[name]
    first = _extract(ctx, name)
    nl = SC.np_result(name)["n_leaves"]
    strict = lvx.surfel_extract(ctx, nl, 0.95, c.params.thr, c.params.min_leaf, c.params.min_inl)
    third = lvx.surfel_extract(ctx, nl, c.params.p_lambda, c.params.thr, c.params.min_leaf, c.params.min_inl)
    assert _same_bytes(first, third)
    ref95 = SC.np_surfel_extract(c.cloud, c.params._replace(p_lambda=0.95))
    assert 0 < strict[1] < first[1] and np.array_equal(strict[0]["leaf"], ref95["leaf"])
    lvx.voxel_build(ctx, c.cloud, SC.LEAF, c.params.min_pts, c.params.eig_mult, fetch=False)
    ids = lvx.voxel_lookup7(ctx, c.cloud[:500])
    assert (ids[:, 0] >= 0).any()
    lvx.surfel_assoc(ctx, _scan_of(name), first[0]["p4"], first[0]["box_min"], first[0]["box_max"], 0.05, 2)
    again = lvx.surfel_extract(ctx, nl, c.params.p_lambda, c.params.thr, c.params.min_leaf, c.params.min_inl)
    assert _same_bytes(first, again)


@pytest.mark.parametrize("name", ["ppl_clean", "jacobi", "far"])
def test_two_calls_return_the_same_bytes(ctx, name):
    assert _same_bytes(_extract(ctx, name), _extract(ctx, name))


# ------------------------------------------------------------------------------------------------------------------------
# max_planes, empty inputs
# ------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def _raw_extract(g, p, max_planes, out):
    n = C.c_int32(-7)
    g._ck(g._l.lvx_surfel_extract(g._h, C.c_double(p.p_lambda), C.c_double(p.thr), C.c_int(p.min_leaf), C.c_int(p.min_inl), C.c_int(max_planes),
                                  out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(n)))
    return n.value


def test_max_planes_into_sentinels(ctx):
    """*n_planes is always the number of planes; the first min(n, max_planes) records are those of the full list; nothing beyond them is written."""
    name = "leaves_1025"
    c = SC.BY_NAME[name]
    full, n = _extract(ctx, name)
    assert n == 257
    assert _raw_extract(ctx, c.params, 0, None) == n
    for mp in (1, n - 1, n, n + 10):
        out = np.full((n + 16) * lvx.SURFEL_PLANE.itemsize, SENTINEL, np.uint8)
        assert _raw_extract(ctx, c.params, mp, out) == n, mp
        k = min(n, mp) * lvx.SURFEL_PLANE.itemsize
        assert out[:k].tobytes() == full[:min(n, mp)].tobytes() and (out[k:] == SENTINEL).all(), mp
    with pytest.raises(lvx.LvxError) as e:                                       # a capacity without an array
        _raw_extract(ctx, c.params, 4, None)
    assert e.value.code == lvx.E_ARG


def test_empty_inputs():
    """include/lvx.h: without a voxel build on the context, and after a build that found no leaf, the map is empty — 0 planes, LVX_OK, nothing written."""
    g = lvx.Context(0)
    try:
        out = np.full(4 * lvx.SURFEL_PLANE.itemsize, SENTINEL, np.uint8)
        assert _raw_extract(g, SC.DEFAULT, 4, out) == 0 and (out == SENTINEL).all()        # no voxel build yet
        vi = lvx.voxel_build(g, np.zeros((0, 4), np.float32), SC.LEAF, fetch=False)
        assert vi["n_leaves"] == 0
        assert _raw_extract(g, SC.DEFAULT, 4, out) == 0 and (out == SENTINEL).all()        # an empty cloud
        r, n = _extract(g, "leaves_5")                                                     # and the context works afterwards
        assert n == 5 and _same_bytes((r, n), _fresh("leaves_5"))
    finally:
        g.close()
