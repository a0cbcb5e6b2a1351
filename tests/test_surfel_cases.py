"""CPU: holds the surfel extraction cases of tests/surfel_cases.py to the regime each one claims — derived from the numpy restatement alone — asserts the conditions
on the inputs (a) to (d) and the 5 % cap on exemptions, and holds the oracle (oracle/orc_upstream.cpp) to np_surfel_extract, which does not rest on it, and to
check_result.  Nine wrong variants of the rule must each be noticed by check_result or by the comparison on some case: a variant no case catches means a case is
missing.  tests/test_gpu_surfel_shapes.py then runs the same cases through the C ABI.

surfel_cases.ORACLE_VS_NUMPY_*: the largest difference between the oracle and the numpy restatement over all cases, measured on the CPU; the bars are four
times that (headroom for another libm or BLAS)."""
import numpy as np
import pytest

import surfel_cases as SC

from surfel_cases import ORACLE_VS_NUMPY_P4, ORACLE_VS_NUMPY_PI, P4_BAR, PI_BAR

NAMES = [c.name for c in SC.CASES]


def _types_equal(a, ref):
    m = SC.type_compared(ref)
    return np.array_equal(SC.as_dict(a)["plane_type"][m], ref["plane_type"][m])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_numpy_restatement(name):
    c, ref, orc = SC.BY_NAME[name], SC.np_result(name), SC.oracle_result(name)
    assert orc["n_leaves"] == ref["n_leaves"]
    SC.check_result(c.cloud, c.params, orc, ref=ref, normal_tol=P4_BAR)
    dp4, dpi, same = SC.compare(orc, ref, SC.p4_compared(ref))
    print("%s: oracle vs numpy p4 %.3e Pi %.3e" % (name, dp4, dpi))
    assert same and _types_equal(orc, ref)
    assert dp4 <= P4_BAR and dpi <= PI_BAR


def test_the_recorded_maxima_are_what_is_measured():
    """The bars are four times the recorded figures; the figures must not drift away from what the oracle and the restatement do: the measured maxima lie between a
    quarter of the record and the bar."""
    worst = np.array([SC.compare(SC.oracle_result(n), SC.np_result(n), SC.p4_compared(SC.np_result(n)))[:2] for n in NAMES]).max(axis=0)
    print("oracle vs numpy maxima: p4 %.3e  Pi %.3e  (recorded %.1e, %.1e)" % (worst[0], worst[1], ORACLE_VS_NUMPY_P4, ORACLE_VS_NUMPY_PI))
    assert ORACLE_VS_NUMPY_P4 / 4 <= worst[0] <= P4_BAR and ORACLE_VS_NUMPY_PI / 4 <= worst[1] <= PI_BAR


@pytest.mark.parametrize("name", NAMES)
def test_conditions_on_the_inputs(name):
    """(a) - (d) and the cap, on the numpy restatement's and the oracle's numbers alone."""
    c, ref, orc = SC.BY_NAME[name], SC.np_result(name), SC.oracle_result(name)
    exact = {i for i, l in enumerate(c.leaves) if l.exact}
    leaf_of = _leaf_index_of(c)
    exact_leaves = {leaf_of[i] for i in exact}
    # (a) every point of a fitted leaf at least 1e-6 from dist_threshold, against the first and the refitted plane; a leaf of dyadic coordinates may have points ON the
    #     threshold: its planes are exact in every implementation (normal along an axis, dyadic d), which is asserted instead
    #     (a leaf exempt through (c) has no refitted plane to speak of — its normal is not determined: the first plane alone)
    for li, margin, nin0, nin, margin0, gap in ref["fitted"]:
        if gap < SC.GAP_MIN:
            assert margin0 >= 1e-6, (li, margin0)
        elif li in exact_leaves:
            k = list(ref["leaf"]).index(li)
            for r in (ref, orc):
                n, d = r["p4"][k, :3], r["p4"][k, 3]
                assert sorted(np.abs(n)) == [0.0, 0.0, 1.0] and d * 1024 == round(d * 1024), (li, n, d)
        else:
            assert margin >= 1e-6, (li, margin)
    for k, li in enumerate(orc["leaf"]):              # the same margins against the ORACLE's final planes
        if li not in exact_leaves and SC.p4_compared(ref)[k]:
            x = _points(c, li)
            assert np.abs(np.abs(x @ orc["p4"][k, :3] + orc["p4"][k, 3]) - c.params.thr).min() >= 1e-6, li
    # (b) every planarity at least 1e-9 from p_lambda; the threshold leaves 1e-6 from it
    for li, pl in ref["offered"]:
        assert abs(pl - c.params.p_lambda) >= 1e-9, (li, pl)
    for i, l in enumerate(c.leaves):
        if l.tag.startswith("planarity"):
            pl = dict(ref["offered"])[leaf_of[i]] - c.params.p_lambda
            assert 5e-7 <= abs(pl) <= 1.5e-6 and (pl > 0) == l.tag.endswith("+1"), (l.tag, pl)
            assert (leaf_of[i] in set(ref["leaf"])) == (pl > 0)
    # (c) the only exemption from the p4 comparison, at most 5 % of the accepted leaves
    exempt = ~SC.p4_compared(ref)
    assert exempt.sum() <= SC.EXEMPT_CAP * max(len(exempt), 1), (exempt.sum(), len(exempt))
    # (d) a normal exactly along an axis: both other components exactly zero in the numpy result AND in the oracle's, plane_type the stated one
    for i, l in enumerate(c.leaves):
        if l.axis is not None and leaf_of[i] in set(ref["leaf"]):
            k = list(ref["leaf"]).index(leaf_of[i])
            for r in (ref, orc):
                assert np.abs(r["p4"][k, l.axis]) == 1.0 and np.count_nonzero(r["p4"][k, :3]) == 1
                assert r["plane_type"][k] == SC.PTYPE_OF_AXIS[l.axis]
            assert ref["type_gap"][k] == 0.0


def _leaf_index_of(c):
    """leaf index (rank of the voxel key) of every Leaf of the case, from the numpy cell assignment."""
    order, offs, keys = SC.cells(c.name)
    xyz = np.asarray(c.cloud)[:, :3]
    first = {tuple(np.floor(xyz[order[o]]).astype(int)): li for li, o in enumerate(offs[:-1])}
    return [first[l.cell] for l in c.leaves]


def _points(c, li):
    order, offs, keys = SC.cells(c.name)
    return np.asarray(c.cloud)[order[offs[li]:offs[li + 1]], :3].astype(np.float64)


def test_cells_do_not_depend_on_rounding():
    """Every point MARGIN inside its cell or on a dyadic coordinate; every Leaf alone in its cell with all its points, in the order it was given."""
    for c in SC.CASES:
        order, offs, keys = SC.cells(c.name)
        assert len(offs) - 1 == len(c.leaves) + len(c.singles)
        assert np.isfinite(c.cloud[:, :3]).all(axis=1).sum() == len(c.cloud) - SC.N_BAD
        for l, li in zip(c.leaves, _leaf_index_of(c)):
            assert np.array_equal(np.asarray(c.cloud)[order[offs[li]:offs[li + 1]], :3], l.points()), (c.name, l.tag)


# ------------------------------------------------------------------------------------------------------------------------
# regimes, from numpy alone
# ------------------------------------------------------------------------------------------------------------------------
def _ppl_class(n):
    for name, ok in (("<64", n < 64), ("64", n == 64), ("65..511", n < 512), ("512", n == 512), ("513..1023", n < 1024), ("1024", n == 1024), ("1025..5120", n <= 5120)):
        if ok:
            return name
    return ">5120"


def _leaves_class(n):
    for name, ok in (("<4", n < 4), ("4", n == 4), ("5..1023", n < 1024), ("1024", n == 1024), ("1025..262144", n <= 262144)):
        if ok:
            return name
    return ">262144"


def test_points_per_leaf_regimes():
    """Accepted leaves on either side of and exactly on 64, 512 and 1 024 points and past ten trips of 512, clean and with outliers; the outliers where they were meant
    to be: in the first 64 list positions / only behind the last full trip (k_surfel_extract: lane = position mod 64, trip = position div 512)."""
    for name in ("ppl_clean", "ppl_out_first", "ppl_out_last", "ppl_tilt"):
        c, ref = SC.BY_NAME[name], SC.np_result(name)
        sizes = set(int(n) for n in ref["n_points"])
        want = set(n for n in SC.PPL if n >= (20 if name == "ppl_clean" else 64))
        assert want <= sizes, (name, sorted(want - sizes))
        assert {_ppl_class(n) for n in sizes} >= {"64", "65..511", "512", "513..1023", "1024", "1025..5120", ">5120"}
        if name == "ppl_clean":
            assert set(SC.PPL) <= set(int(n) for n in ref["counts"]) and _ppl_class(20) == "<64"
            assert not {9, 10, 19} & sizes                     # below min_leaf_points / min_inliers
            continue
        for k, li in enumerate(ref["leaf"]):
            x = _points(c, li)
            out = np.nonzero(~(np.abs(x @ ref["p4"][k, :3] + ref["p4"][k, 3]) < c.params.thr))[0]
            assert len(out) >= 1, (name, li)
            n = len(x)
            if name == "ppl_out_first":
                assert out.max() < 64 and len(set(out % 64)) == len(out) < 64          # some lanes hold an outlier as their first point, the others none
            if name == "ppl_out_last":
                last_trip = (n - 1) // SC.EX_TRIP
                assert (out // SC.EX_TRIP == last_trip).all() and out.min() >= n - 40


def test_leaf_count_regimes():
    """1, 3, 4, 5, 1 023, 1 024, 1 025, 2 049, 4 100 leaves and the cloud past 262 144; there the planted leaves at the seams of both compactions, first and last index
    included, and nothing else accepted; the acceptance patterns at 2 049 leaves."""
    counts = [SC.np_result("leaves_%d" % L)["n_leaves"] for L in SC.LEAF_COUNTS]
    assert counts == list(SC.LEAF_COUNTS)
    big = SC.np_result("big")
    assert big["n_leaves"] == SC.BIG_LEAVES >= 263000 and list(big["leaf"]) == list(SC.BIG_PLANTED)
    assert {_leaves_class(n) for n in counts + [big["n_leaves"]]} == {"<4", "4", "5..1023", "1024", "1025..262144", ">262144"}
    assert set(SC.BIG_PLANTED) >= {0, 1023, 1024, 262143, 262144, 262145, big["n_leaves"] - 1}
    assert len(SC.BY_NAME["big"].cloud) < 300000 and all(len(c.cloud) <= 45000 for c in SC.CASES if not c.big)
    for L in SC.LEAF_COUNTS:
        acc = SC.np_result("leaves_%d" % L)["leaf"]
        assert acc[0] == 0 and acc[-1] == L - 1                 # first and last leaf index carry a plane
    pat = {n: list(SC.np_result("accept_" + n)["leaf"]) for n in ("none", "all", "first", "last", "mid", "second")}
    assert all(SC.np_result("accept_" + n)["n_leaves"] == 2049 for n in pat)
    assert pat["none"] == [] and pat["all"] == list(range(2049)) and pat["first"] == [0] and pat["last"] == [2048] and pat["mid"] == [1023, 1024]
    assert pat["second"] == list(range(0, 2049, 2))


def test_threshold_regimes():
    ml = SC.np_result("thr_min_leaf")
    assert sorted(int(n) for n in ml["counts"]) == [23, 24, 25] and sorted(ml["n_points"]) == [24, 25]                 # n = min_leaf_points - 1 / min_leaf_points
    mi = SC.np_result("thr_min_inliers")
    assert [f[3] for f in mi["fitted"]] == [26, 27, 28] and list(mi["n_inliers"]) == [27, 28]                          # inliers = min_inliers - 1 / min_inliers
    for m in (1, 2, 3):                                                                                               # 0, 1, 2 inliers: no refit
        r = SC.np_result("thr_few_inliers_%d" % m)
        assert [f[2] for f in r["fitted"]] == [0, 1, 2, 3, 4] and list(r["n_inliers"]) == list(range(m, 5))
        assert [b for b, n in zip(r["branch"], r["nin0"])] == ["none" if n < 3 else "rq" for n in r["nin0"]]
    assert {SC.BY_NAME[n].params.thr for n in SC.BY_NAME} >= {0.02, 0.05, 0.2}
    assert {SC.BY_NAME[n].params.p_lambda for n in SC.BY_NAME} >= {0.0, 0.6, 0.7, 0.95}
    wide = SC.np_result("thr_wide")
    assert (wide["n_inliers"] == wide["n_points"]).all() and len(wide["leaf"]) == 4                                    # the 0.12 m outliers are inliers at 0.2
    tie = SC.np_result("thr_exact_tie")
    assert [f[1] for f in tie["fitted"]] == [0.0, 0.0, 0.0] and list(tie["n_inliers"]) == [22, 22, 22] and list(tie["n_points"]) == [28, 28, 28]
    # min_leaf_points against min_points_per_voxel: leaves below min_points_per_voxel are never surfels, min_leaf_points <= 0 is 1
    rejected = len(SC.MINPTS_COUNTS)                                # leaf index of the 14 coincident points
    for mp in (6, 12):
        res = {m: SC.np_result("thr_leafpts_%d_%d" % (m, mp)) for m in (1, 6, 10, 50, 0, -3)}
        for m, r in res.items():
            orc = SC.oracle_result("thr_leafpts_%d_%d" % (m, mp))
            assert r["counts"][rejected] == SC.MINPTS_COINCIDENT >= mp and orc["leaf_n"][rejected] == -1            # the build rejects it: nr_points = -1
            assert rejected not in set(r["leaf"]) and rejected not in set(orc["leaf"]), (m, mp)                     # and it never reaches the fit
            assert np.array_equal(orc["leaf_n"][:rejected], SC.MINPTS_COUNTS)                                       # (leaves below min_points_per_voxel keep their count)
            assert r["n_points"].min() >= max(m, mp, 1) and (r["counts"] < mp).sum() >= 3
            enough = r["counts"] >= max(m, mp, 1)
            enough[rejected] = False
            assert np.array_equal(r["leaf"], np.nonzero(enough)[0]), (m, mp)     # every other leaf with enough points is a surfel: the count alone decides
        assert all(np.array_equal(res[m]["leaf"], res[1]["leaf"]) for m in (0, -3))


def test_a_rejected_leaf_with_eigen_data_is_not_fitted_by_the_oracle():
    """min_leaf_points <= 0 means 1.  The coincident leaf of the minpts cases is stopped twice (its count is -1 and its planarity 0 / 0); a leaf marked -1 that HAS
    eigenvalues (the build's other rejection, an inverse covariance that overflows, is out of a float cloud's reach) is stopped by the count alone: mark a good leaf by
    hand and ask with min_leaf_points = -3."""
    from oracle import oracle as O
    c = SC.BY_NAME["thr_min_leaf"]
    vo = O.voxel_build(c.cloud, SC.LEAF, 6, 0.01)
    args = (0.7, 0.05, -3, 1)
    assert list(O.surfel_extract(c.cloud, vo, *args)["leaf"]) == [0, 1, 2]
    vo["leaf_n"] = vo["leaf_n"].copy()
    vo["leaf_n"][1] = -1
    assert list(O.surfel_extract(c.cloud, vo, *args)["leaf"]) == [0, 2]


def test_geometry_and_refit_regimes():
    geo, leaves = SC.np_result("geometry"), SC.BY_NAME["geometry"].leaves
    n, d = geo["p4"][:, :3], geo["p4"][:, 3]
    assert len(geo["leaf"]) == len(leaves)
    axes = [int(np.argmax(np.abs(v))) for v in n if np.count_nonzero(v) == 1]
    assert sorted(set(axes)) == [0, 1, 2] and len(axes) == 9
    assert (d == 0).sum() == 3 and (d < 0).any()                                         # planes through the origin: x = 0, y = 0, z = 0
    assert {tuple(np.sign(v).astype(int)) for v in n[d == 0]} == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
    assert (geo["d_raw"] > 0).any() and (geo["d_raw"] < 0).any()                         # d of both signs before the flip (numpy's own eigenvector signs) ...
    for a in range(3):                                                                   # ... and, whatever sign a solver gives its vectors, planes on both sides
        assert (n[:, a] > 0.2).any() and (n[:, a] < -0.2).any()                          #     of the origin along every axis: final normals of both signs
    cells = np.array([l.cell for l in leaves])
    assert all((cells[:, a] < 0).any() and (cells[:, a] >= 0).any() for a in range(3))
    assert any(np.allclose(np.abs(v), [2 ** -0.5, 2 ** -0.5, 0], atol=0.02) for v in n)   # (1, 1, 0) / sqrt 2
    far = np.array([l.cell for l in SC.BY_NAME["far"].leaves])
    assert all((far[:, a] >= 100).any() and (far[:, a] <= -100).any() for a in range(3)) and len(SC.np_result("far")["leaf"]) == len(far)
    # the refit: no refit, the Rayleigh-quotient iteration, the Jacobi fallback (predicted by the restatement of the acceptance test)
    jac, tags = SC.np_result("jacobi"), [l.tag for l in SC.BY_NAME["jacobi"].leaves]
    by_tag = {tags[i]: k for k, i in enumerate(np.argsort(_leaf_index_of(SC.BY_NAME["jacobi"])))}
    assert len(jac["leaf"]) == len(tags)
    for t in ("rod", "collinear", "turned_plane"):
        assert jac["branch"][by_tag[t]] == "jacobi", t
    assert jac["gap"][by_tag["rod"]] == 0.0 and jac["gap"][by_tag["collinear"]] < 1e-9          # the normal is not determined: exempt through (c)
    assert jac["gap"][by_tag["turned_plane"]] >= SC.GAP_MIN                                       # a determined normal behind the fallback: compared
    assert jac["nin0"][by_tag["turned_plane"]] == 30 and jac["n_inliers"][by_tag["turned_plane"]] != 30
    assert sum(b == "jacobi" for b in jac["branch"]) == 3
    branches = set()
    for name in NAMES:
        branches |= set(SC.np_result(name)["branch"])
    assert branches == {"none", "rq", "jacobi"}


# ------------------------------------------------------------------------------------------------------------------------
# wrong rules
# ------------------------------------------------------------------------------------------------------------------------
def _noticed(name, rule):
    c, ref = SC.BY_NAME[name], SC.np_result(name)
    bad = SC.np_surfel_extract(c.cloud, c.params, wrong=rule)
    try:
        SC.check_result(c.cloud, c.params, bad, ref=ref, normal_tol=P4_BAR)
    except AssertionError as e:
        return "check_result: " + str(e).split("\n")[0]
    dp4, dpi, same = SC.compare(bad, SC.oracle_result(name), SC.p4_compared(ref))
    if not same or dp4 > P4_BAR or dpi > PI_BAR or not _types_equal(bad, ref):
        return "comparison"
    return None


@pytest.mark.parametrize("rule", SC.WRONG_RULES)
def test_a_wrong_rule_is_noticed(rule):
    where = {"le_threshold": ["thr_exact_tie"], "planarity_two_largest": ["geometry"], "n_gt_min_leaf": ["thr_min_leaf"], "count_first_selection": ["jacobi", "ppl_tilt"],
             "box_of_inliers": ["ppl_out_first"], "no_sign_flip": ["geometry"], "refit_skipped": ["ppl_tilt"], "type_ascending": ["geometry"],
             "rejected_leaf_fitted": ["thr_leafpts_-3_6", "thr_leafpts_1_12"]}[rule]
    found = [(n, _noticed(n, rule)) for n in where]
    print(rule, found)
    assert any(f for _, f in found)
    assert _noticed(where[0], None) is None          # and the right rule passes the same checks
