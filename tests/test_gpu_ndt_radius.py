"""GPU: the radius search of pclomp::KDTREE through the C ABI — lvx_voxel_radius_search(_d), lvx_ndt_derivatives_search, lvx_ndt_align and lvx_lidar_odometry with
search = 0 — on the cases of tests/ndt_radius_cases.py (tests/test_ndt_radius_cases.py, CPU, holds the cases and the checkers).

Bars.  Lookup: ids, order, counts and the float bits of d2 equal the brute-force restatement exactly (the cases keep every centroid more than 4 ulps from the radius).
Derivatives: against orc_ndt_derivatives_n over the restatement's ids at ndt_cases.BAR_SCORE / BAR_GH, the bars the direct searches are held to; against the float64
reference with ndt_cases.RECORDED x 4 added, as tests/test_gpu_ndt_edges.py does.  Alignment on the reference's demo: the bars of
tests/test_gpu_ndt_align.py::test_align_follows_the_oracle_loop (same iteration and evaluation counts, p to 1e-7, final transformation 2e-7, fitness 1e-5 relative), and
the fitness within 1e-5 relative of the 0.206161 tests/test_ndt_align_oracle.py records for KDTREE.  Odometry: pose[1] equals lvx_ndt_align(search = 0) bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lvx
import ndt_cases as NC
import ndt_radius_cases as RC
import odometry_cases as OC
from oracle import ndt_align as NA
from oracle import pipeline as PL

pytestmark = pytest.mark.gpu
DERIV, _dist, oracle_derivatives = RC.DERIV, RC.dist, RC.oracle_derivatives
KDTREE_FITNESS = 0.206161        # tests/test_ndt_align_oracle.py: the oracle's KDTREE loop on the demo


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(ctx, b):
    c = b.case
    info = lvx.voxel_build(ctx, c.tgt, c.leaf, min_pts=c.min_pts, fetch=False)
    assert info["n_leaves"] == b.vox["n_leaves"] and np.array_equal(info["grid"], b.vox["grid"])


def _search_patterned(ctx, q, radius):
    """lvx_voxel_radius_search into buffers filled with a pattern: every slot must be written."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 4)
    ids, d2, cnt = np.full((len(q), RC.K), -77, np.int32), np.full((len(q), RC.K), -77.0, np.float32), np.full(len(q), -77, np.int32)
    ctx._ck(ctx._l.lvx_voxel_radius_search(ctx._h, C.c_int(len(q)), lvx._p(q), C.c_double(radius), lvx._p(ids), lvx._p(d2), lvx._p(cnt)))
    return ids, d2, cnt


def _search_device(ctx, q, radius, want=(True, True, True)):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    q_d = torch.from_numpy(np.array(q, np.float32).reshape(-1, 4)).to(dev)
    n = q_d.shape[0]
    ids = torch.full((n, RC.K), -77, dtype=torch.int32, device=dev)
    d2 = torch.full((n, RC.K), -77.0, dtype=torch.float32, device=dev)
    cnt = torch.full((n,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lvx.voxel_radius_search_d(ctx, n, q_d.data_ptr(), radius, ids.data_ptr() if want[0] else 0, d2.data_ptr() if want[1] else 0, cnt.data_ptr() if want[2] else 0)
    ctx.synchronize()
    return ids.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def _same(got, b, n=None):
    s = slice(None) if n is None else slice(0, n)
    return np.array_equal(got[2], b.count[s]) and np.array_equal(got[0], b.ids[s]) and np.array_equal(_bits(got[1]), _bits(b.d2[s]))


# ---- lookup --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_radius_search_gives_the_restatement(ctx, name):
    b = RC.build(name)
    c = b.case
    _grid(ctx, b)
    first = _search_patterned(ctx, c.trans, c.leaf)
    assert _same(first, b)
    again = _search_patterned(ctx, c.trans, c.leaf)
    assert all(np.array_equal(x, y) for x, y in zip((first[0], _bits(first[1]), first[2]), (again[0], _bits(again[1]), again[2])))
    assert _same(_search_device(ctx, c.trans, c.leaf), b)
    assert _same(lvx.voxel_radius_search(ctx, c.trans, c.leaf), b)
    for frac in (0.5, 0.1):                                                              # smaller radii through the same entry
        assert _same(_search_patterned(ctx, c.trans, frac * c.leaf), RC.build(name, frac)), frac


@pytest.mark.parametrize("n", RC.SIZES)
def test_radius_search_at_every_query_count(ctx, n):
    b = RC.build("room_0p5")
    c = b.case
    _grid(ctx, b)
    assert _same(_search_patterned(ctx, c.trans[:n], c.leaf), b, n)
    assert _same(_search_device(ctx, c.trans[:n], c.leaf), b, n)


def test_radius_search_returns_the_rejected_leaf_and_the_cell_lookups_do_not(ctx):
    b = RC.build("rejected")
    c = b.case
    _grid(ctx, b)
    r = RC.rejected_leaves(b.vox)[0]
    ids, _, cnt = lvx.voxel_radius_search(ctx, c.trans, c.leaf)
    assert (ids == r).any(axis=1)[:40].all() and not (ids == r).any(axis=1)[40:].any()
    rel27 = np.array([[i, j, k] for k in (-1, 0, 1) for j in (-1, 0, 1) for i in (-1, 0, 1)], np.int32)
    assert not (lvx.voxel_lookup_rel(ctx, c.trans, rel27) == r).any()
    assert not (lvx.voxel_lookup7(ctx, c.trans) == r).any()


def test_radius_search_outputs_may_be_null(ctx):
    b = RC.build("room_0p5")
    c = b.case
    _grid(ctx, b)
    q = np.ascontiguousarray(c.trans[:257])
    cnt = np.full(257, -77, np.int32)
    ctx._ck(ctx._l.lvx_voxel_radius_search(ctx._h, C.c_int(257), lvx._p(q), C.c_double(c.leaf), None, None, lvx._p(cnt)))
    assert np.array_equal(cnt, b.count[:257])
    ids, d2, cn = _search_device(ctx, q, c.leaf, want=(True, False, False))
    assert np.array_equal(ids, b.ids[:257]) and (d2 == -77.0).all() and (cn == -77).all()
    ids, d2, cn = _search_device(ctx, q, c.leaf, want=(False, True, False))
    assert np.array_equal(_bits(d2), _bits(b.d2[:257])) and (ids == -77).all()


def test_radius_search_argument_errors():
    c = lvx.Context(0)
    try:
        q = np.zeros((3, 4), np.float32)
        with pytest.raises(lvx.LvxError) as e:                                         # no grid yet
            lvx.voxel_radius_search(c, q, 0.5)
        assert e.value.code == lvx.E_STATE
        b = RC.build("tie")
        lvx.voxel_build(c, b.case.tgt, 0.5, fetch=False)
        for radius in (0.0, -0.5, 0.5000001, 1.0, np.nan, np.inf):
            with pytest.raises(lvx.LvxError) as e:
                lvx.voxel_radius_search(c, q, radius)
            assert e.value.code == lvx.E_ARG, radius
        assert c._l.lvx_voxel_radius_search(c._h, C.c_int(3), None, C.c_double(0.5), None, None, None) == lvx.E_ARG
        assert c._l.lvx_voxel_radius_search_d(c._h, C.c_int(3), None, C.c_double(0.5), None, None, None) == lvx.E_ARG
        ids, d2, cnt = lvx.voxel_radius_search(c, q[:0], 0.5)                           # nq = 0 is fine
        assert ids.shape == (0, 27) and cnt.shape == (0,)
        assert _same(lvx.voxel_radius_search(c, b.case.trans, 0.5), b)                  # and the context searches on
    finally:
        c.close()


# ---- derivatives ---------------------------------------------------------------------------------------------------------------------------------------------------
def _gpu(ctx, b, compute_hessian=True, search=0):
    c = b.case
    return lvx.ndt_derivatives(ctx, c.src, c.trans, np.array(c.p6), outlier_ratio=c.outlier_ratio, compute_hessian=compute_hessian, search=search)


def _same_bits(r0, r1):
    return r0[0] == r1[0] and np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2], r1[2])


@pytest.mark.parametrize("name", DERIV)
def test_derivatives_with_the_radius_search(ctx, name):
    b = RC.build(name)
    c = b.case
    _grid(ctx, b)
    want = oracle_derivatives(b)
    got = _gpu(ctx, b)
    es, eg, eH = _dist(got, want)
    f64 = NC.ndt_reference_f64(b.vox, b.ids, c.src, c.trans, c.p6, c.leaf, c.outlier_ratio)
    fs, fg, fH = _dist(got, f64)
    print("%s: n %d score %.6g | gpu-oracle score %.2e g %.2e H %.2e | gpu-f64 score %.2e g %.2e H %.2e" % (name, len(c.src), want[0], es, eg, eH, fs, fg, fH))
    assert es <= NC.BAR_SCORE and eg <= NC.BAR_GH and eH <= NC.BAR_GH
    assert fs <= 4 * NC.RECORDED["score"] + NC.BAR_SCORE and fg <= 4 * NC.RECORDED["g"] + NC.BAR_GH and fH <= 4 * NC.RECORDED["H"] + NC.BAR_GH
    if name != "box_outside":
        assert want[0] > 0 and want[2].any()
    s2, g2, H2 = _gpu(ctx, b, compute_hessian=False)
    assert s2 == got[0] and np.array_equal(g2, got[1]) and not H2.any()
    assert _same_bits(_gpu(ctx, b), got)                                                 # fixed-order sums: same bits run to run


@pytest.mark.parametrize("n", RC.SIZES)
def test_derivatives_at_every_launch_size(ctx, n):
    full = RC.build("room_0p5")
    c = full.case._replace(src=full.case.src[:n], trans=full.case.trans[:n])
    b = full._replace(case=c, ids=full.ids[:n], d2=full.d2[:n], count=full.count[:n])
    _grid(ctx, b)
    es, eg, eH = _dist(_gpu(ctx, b), oracle_derivatives(b))
    assert es <= NC.BAR_SCORE and eg <= NC.BAR_GH and eH <= NC.BAR_GH


def test_the_rejected_leaf_adds_minus_d1_to_the_score_and_nothing_else(ctx):
    b = RC.build("rejected")
    c = b.case
    _grid(ctx, b)
    r = RC.rejected_leaves(b.vox)[0]
    only = (b.ids[:, 0] == r) & (b.count == 1)
    src = np.ascontiguousarray(c.src[only])
    s, g, H = lvx.ndt_derivatives(ctx, src, src, np.zeros(6), outlier_ratio=c.outlier_ratio, search=0)
    assert s == pytest.approx(-RC.gauss_d1(c.leaf, c.outlier_ratio) * only.sum(), rel=NC.BAR_SCORE) and not g.any() and not H.any()
    s7, g7, H7 = lvx.ndt_derivatives(ctx, src, src, np.zeros(6), outlier_ratio=c.outlier_ratio, search=7)
    assert s7 == 0.0 and not g7.any() and not H7.any()                                   # the direct searches never see it


def test_search_7_through_the_new_entry_is_lvx_ndt_derivatives(ctx):
    b = RC.build("room_0p5")
    c = b.case
    _grid(ctx, b)
    for hess in (True, False):
        score, g, H = C.c_double(0), np.zeros(6), np.zeros((6, 6))
        ctx._ck(ctx._l.lvx_ndt_derivatives(ctx._h, C.c_int(len(c.src)), lvx._p(np.ascontiguousarray(c.src)), lvx._p(np.ascontiguousarray(c.trans)), lvx._p(lvx._d(c.p6)),
                                           C.c_double(c.outlier_ratio), C.c_int(int(hess)), C.byref(score), lvx._p(g), lvx._p(H)))
        assert _same_bits(_gpu(ctx, b, hess, search=7), (score.value, g, H))
    assert not _same_bits(_gpu(ctx, b, search=0), _gpu(ctx, b, search=7))
    with pytest.raises(lvx.LvxError) as e:
        _gpu(ctx, b, search=5)
    assert e.value.code == lvx.E_ARG


# ---- the registration loop on the demo ---------------------------------------------------------------------------------------------------------------------------------
def _align_and_compare(ctx, p_bar, **opts):
    R = RC.real_clouds()
    td, sd = R["td"], R["sd"]
    a = NA.NdtAligner(td, 1.0, NA.KDTREE, **opts)
    a.align(sd)
    lvx.voxel_build(ctx, td, 1.0, fetch=False)
    r = lvx.ndt_align(ctx, sd, search=0, **opts)
    fo, fg = a.fitness(), lvx.ndt_fitness(ctx, sd, r["final_transformation"], td)
    dp, dT = np.abs(r["p"] - a.p).max(), np.abs(r["final_transformation"] - a.final_transformation).max()
    print("KDTREE %s: oracle iterations %d evaluations %d line-search iterations %s | gpu iterations %d evaluations %d | dp %.2e dT %.2e fitness oracle %.6f gpu %.6f"
          % (opts, a.nr_iterations, a.n_eval, [t["mt"] for t in a.trace], r["iterations"], r["n_evaluations"], dp, dT, fo, fg))
    assert r["iterations"] == a.nr_iterations and r["n_evaluations"] == a.n_eval and r["converged"]
    assert dp <= p_bar and dT <= 2e-7
    assert abs(r["trans_probability"] - a.trans_probability) <= 1e-6 * abs(a.trans_probability)
    assert abs(fg - fo) <= 1e-5 * fo
    return a, r, fg


def test_align_on_the_demo_follows_the_oracles_kdtree_loop(ctx):
    a, r, fg = _align_and_compare(ctx, 1e-7)
    assert (a.nr_iterations, a.n_eval) == (4, 6)
    assert abs(fg - KDTREE_FITNESS) <= 1e-5 * KDTREE_FITNESS
    again = lvx.ndt_align(ctx, RC.real_clouds()["sd"], search=0)
    assert np.array_equal(again["p"], r["p"]) and again["score"] == r["score"]


def test_align_on_the_demo_through_line_search_and_hessian_pass(ctx):
    """transformation_epsilon = 0.01: More-Thuente iterations, then k_ndt_hessian with the radius search (1e-6: the bar of
    tests/test_gpu_ndt_align.py::test_align_with_line_search_iterations_and_a_guess for this option)."""
    a, r, _ = _align_and_compare(ctx, 1e-6, transformation_epsilon=0.01)
    assert any(t["mt"] > 0 for t in a.trace)


# ---- odometry ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_odometry_with_the_radius_search_equals_its_parts(ctx):
    case = OC.make_case("gentle")
    scans = case["scans"][:2]
    lvx.set_scans(ctx, scans, OC.H, OC.W)
    opt = lvx.odom_default_options(ctx)
    opt.ndt.search = 0
    poses, steps, n_key = lvx.lidar_odometry(ctx, None, opt)
    assert np.array_equal(poses[0], np.eye(4)) and steps["iterations"][1] >= 1
    lvx.voxel_build(ctx, PL.transform_cloud(OC.scan_xyzi(scans[0]), poses[0]), opt.ndt_resolution, opt.min_points_per_voxel, opt.min_covar_eigvalue_mult, fetch=False)
    src = lvx.voxelgrid_downsample(ctx, OC.scan_xyzi(scans[1]), opt.downsample_leaf)
    kw = dict(step_size=opt.ndt.step_size, transformation_epsilon=opt.ndt.transformation_epsilon, max_iterations=opt.ndt.max_iterations, outlier_ratio=opt.ndt.outlier_ratio)
    r = lvx.ndt_align(ctx, src, np.eye(4, dtype=np.float32), search=0, **kw)
    s = steps[1]
    assert s["n_src"] == len(src)
    assert np.array_equal(r["final_transformation"].astype(np.float64), poses[1])
    assert np.array_equal(r["p"], s["p6"]) and r["score"] == s["score"] and (r["iterations"], r["n_evaluations"]) == (s["iterations"], s["n_evaluations"])
    r7 = lvx.ndt_align(ctx, src, np.eye(4, dtype=np.float32), search=7, **kw)
    assert not np.array_equal(r7["p"], r["p"])                                           # the search is what was asked for
    opt.ndt.search = 5
    with pytest.raises(lvx.LvxError) as e:
        lvx.lidar_odometry(ctx, None, opt)
    assert e.value.code == lvx.E_ARG
