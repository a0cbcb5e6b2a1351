"""GPU: every case of tests/voxel_cases.py through lvx.voxel_build / voxel_lookup1 / voxel_lookup7 / voxel_lookup_rel (k_vx_extent, k_vx_keys, every instance of
k_vx_sort_pass and k_vx_leaf, k_vx_lookup<1 | 7>, k_vx_lookup_rel), held to
  * the numpy restatement by check_build at the bars recorded on the CPU (tests/test_voxel_cases.py): an eigen-solver that shares nothing with the kernel's Jacobi;
  * the oracle at the project's bars (cov 1e-12 of the leaf's scale, evals 1e-10, icov 1e-8, the rest exact) on the determined and exact leaves;
  * check_build's either-outcome rule on the undetermined leaves a case names;
  * np_lookup on the leaves the device built: a rejected leaf is absent, a non-finite query has no neighbour.
The sort cases run on a fresh context each (the digit width follows the context's cell table, which only grows); the sequence tests run several builds on one."""
import numpy as np
import pytest

import lvx
import voxel_cases as VC

pytestmark = pytest.mark.gpu
FIELDS = ("grid", "leaf_key", "leaf_n", "mean", "cov", "icov", "evecs", "evals", "centroid", "offsets", "point_ids")


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _against_oracle(got, orc, ref, cls):
    """the project's bars (tests/upstream_checks.check_voxels), on the determined and exact leaves"""
    assert got["n_leaves"] == orc["n_leaves"] and np.array_equal(got["grid"], orc["grid"])
    m = orc["offsets"][-1]
    assert np.array_equal(got["leaf_key"], orc["leaf_key"]) and np.array_equal(got["offsets"], orc["offsets"]) and np.array_equal(got["point_ids"][:m], orc["point_ids"][:m])
    assert np.array_equal(got["centroid"].view(np.uint32), orc["centroid"].view(np.uint32))
    assert np.allclose(got["mean"], orc["mean"], rtol=1e-12, atol=1e-12)
    de = (cls == "D") | (cls == "E") | (cls == "P")
    assert np.array_equal(got["leaf_n"][de], orc["leaf_n"][de])
    sc = np.abs(orc["cov"][de]).max(axis=1, keepdims=True)
    assert (np.abs(got["cov"][de] - orc["cov"][de]) <= 1e-12 * sc + 1e-18).all()
    ok = de & (cls != "P") & (orc["leaf_n"] >= 0)
    assert np.allclose(got["evals"][ok], orc["evals"][ok], rtol=1e-10, atol=1e-16)
    si = np.abs(orc["icov"][ok]).max(axis=1, keepdims=True)
    assert (np.abs(got["icov"][ok] - orc["icov"][ok]) <= 1e-8 * si).all()
    ev = orc["evals"][ok]
    sep = np.diff(ev, axis=1).min(axis=1) > 1e-6 * ev[:, 2]
    dots = np.abs(np.einsum("nij,nij->nj", got["evecs"][ok].reshape(-1, 3, 3)[sep], orc["evecs"][ok].reshape(-1, 3, 3)[sep]))
    assert (dots > 1 - 1e-8).all()


def _run(case, c):
    got = lvx.voxel_build(c, case.cloud, case.leaf, case.min_pts, case.eig_mult)
    ref, cls = VC.np_result(case.name), VC.classes(case.name)
    fig = VC.check_build(got, ref, case.min_pts, case.eig_mult, cls)
    print(case.name, "device vs numpy:", " ".join("%s %.2e" % kv for kv in fig.items()),
          "| undetermined leaves kept / rejected: %d / %d" % ((got["leaf_n"][cls == "U"] >= 0).sum(), (got["leaf_n"][cls == "U"] < 0).sum()))
    _against_oracle(got, VC.oracle_result(case.name), ref, cls)
    VC.check_lookups(case, got, lambda q: lvx.voxel_lookup1(c, q), lambda q: lvx.voxel_lookup7(c, q), lambda q, rel: lvx.voxel_lookup_rel(c, q, rel))
    gone = np.nonzero(got["leaf_n"] == -1)[0]
    if len(gone):                                       # a rejected leaf is absent: a query at its mean finds nothing in its own cell
        q = np.zeros((len(gone), 4), np.float32)
        q[:, :3] = got["mean"][gone]
        assert (lvx.voxel_lookup1(c, q) == -1).all() and (lvx.voxel_lookup_rel(c, q, VC.REL1) == -1).all()
    return got


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group == "sort"])
def test_sort_instance_on_a_fresh_context(name):
    case = VC.BY_NAME[name]
    c = lvx.Context(0)
    try:
        got = _run(case, c)
    finally:
        c.close()
    assert VC.sort_instance(int(np.prod(got["grid"][6:9].astype(np.int64))))[1:] == case.expect["instance"]      # the host's rule, from the extents the device returned


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group != "sort"])
def test_case(ctx, name):
    case = VC.BY_NAME[name]
    got = _run(case, ctx)
    if case.group == "leaves" and case.undetermined == 0:
        assert (got["leaf_n"][np.diff(got["offsets"]) >= case.min_pts] >= 0).all()


def _same_bytes(a, b):
    assert a["n_leaves"] == b["n_leaves"]
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if k == "point_ids":
            x, y = x[:a["offsets"][-1]], y[:b["offsets"][-1]]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _fresh(cloud, leaf, switches=()):
    c = lvx.Context(0)
    try:
        for s in switches:
            c.set_switch(s, 1)
        return lvx.voxel_build(c, cloud, leaf)
    finally:
        c.close()


def test_a_replayed_graph_builds_what_a_fresh_context_builds():
    """the same point count, buffer and parameters with other content: the captured chain is replayed"""
    a = VC.BY_NAME["tiles_end_at_n"].cloud
    b = VC._profile_case(256, 0, 99)["cloud"]
    assert len(a) == len(b) and not np.array_equal(a, b)
    c = lvx.Context(0)
    try:
        lvx.voxel_build(c, a, 0.5)
        again = lvx.voxel_build(c, b, 0.5)
    finally:
        c.close()
    _same_bytes(again, _fresh(b, 0.5))
    _same_bytes(again, _fresh(b, 0.5, ("NO_GRAPH",)))


def test_a_grown_cell_table_sorts_a_small_grid_at_the_grown_width():
    """small -> wide (the table grows) -> small again, now sorted in three 8-bit passes instead of two 9-bit ones: nothing the build returns depends on the width"""
    small, wide = VC.BY_NAME["sort_9x2"], VC.BY_NAME["sort_8x3"]
    cap = VC.sort_instance(int(np.prod(wide.data["dims"])))[0]
    assert VC.sort_instance(32 ** 3)[2:] == (9, 2) and VC.sort_instance(32 ** 3, cap)[2:] == (8, 3)
    c = lvx.Context(0)
    try:
        first = lvx.voxel_build(c, small.cloud, small.leaf)
        mid = lvx.voxel_build(c, wide.cloud, wide.leaf)
        last = lvx.voxel_build(c, small.cloud, small.leaf)
    finally:
        c.close()
    _same_bytes(first, last)
    _same_bytes(last, _fresh(small.cloud, small.leaf))
    _same_bytes(mid, _fresh(wide.cloud, wide.leaf))


def test_too_many_cells_is_an_error_and_the_context_builds_again():
    """two points 1 301 cells apart on every axis: 1 302^3 cells, more than 2^31 - 1 and far from that boundary"""
    far = np.zeros((2, 4), np.float32)
    far[1, :3] = 1301.5
    far[0, :3] = 0.5
    case = VC.BY_NAME["n_1025"]
    c = lvx.Context(0)
    try:
        with pytest.raises(lvx.LvxError, match="Leaf size is too small"):
            lvx.voxel_build(c, far, 1.0)
        got = lvx.voxel_build(c, case.cloud, case.leaf)
    finally:
        c.close()
    _same_bytes(got, _fresh(case.cloud, case.leaf))
    VC.check_build(got, VC.np_result(case.name), case.min_pts, case.eig_mult, VC.classes(case.name))


def test_a_cloud_without_a_finite_point_and_an_empty_cloud(ctx):
    bad = np.zeros((300, 4), np.float32)
    bad[:, :3] = VC.BAD[np.arange(300) % len(VC.BAD)]
    q = VC.BY_NAME["n_1025"].queries
    for cloud in (bad, bad[:0]):
        got = lvx.voxel_build(ctx, cloud, 1.0)
        assert got["n_leaves"] == 0 and got["offsets"][0] == 0
        assert (lvx.voxel_lookup7(ctx, q) == -1).all() and (lvx.voxel_lookup1(ctx, q) == -1).all() and (lvx.voxel_lookup_rel(ctx, q, VC.REL27) == -1).all()
    VC.check_build(lvx.voxel_build(ctx, bad, 1.0), VC.np_voxel_build(bad, 1.0), 6, 0.01, np.zeros(0, "U1"))
    case = VC.BY_NAME["n_257"]                      # and the context builds on
    VC.check_build(lvx.voxel_build(ctx, case.cloud, case.leaf), VC.np_result(case.name), case.min_pts, case.eig_mult, VC.classes(case.name))
