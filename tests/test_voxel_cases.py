"""CPU: holds the voxel grid cases of tests/voxel_cases.py to what each one claims — the sort instance selected, the sorted positions of its leaf heads, the classes
of its leaves, the points whose build cell is not their lookup cell — derived from the numpy restatements alone, and holds the oracle (oracle/orc_upstream.cpp,
oracle/orc_ndt.cpp) to np_voxel_build and np_lookup, which do not rest on it.  No leaf of min_pts points or more is undetermined unless its case says so.  Eight
wrong variants of the restatements must each be noticed by some case: a variant no case catches means a case is missing.
tests/test_gpu_voxel_cases.py then runs the same cases through the C ABI.

voxel_cases.ORACLE_VS_NUMPY: the largest difference between the oracle and the restatement per quantity over all cases, measured here; the bars are four times that."""
import numpy as np
import pytest

import voxel_cases as VC
from oracle import ndt_align as NA
from oracle import oracle as O

NAMES = [c.name for c in VC.CASES]


def _keys_of_points(ref, n):
    """build key per input point (-1 for the non-finite ones)"""
    k = np.full(n, -1, np.int64)
    m = ref["offsets"][-1]
    k[ref["point_ids"][:m]] = np.repeat(ref["leaf_key"], np.diff(ref["offsets"]))
    return k


def _oracle_lookups(case, orc):
    return (lambda q: O.voxel_lookup7(orc, q, case.leaf, case.min_pts)[:, 0], lambda q: O.voxel_lookup7(orc, q, case.leaf, case.min_pts),
            lambda q, rel: NA.voxel_lookup_rel(orc, q, np.float32(case.leaf), rel, case.min_pts))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_numpy_restatements(name):
    c, ref, orc, cls = VC.BY_NAME[name], VC.np_result(name), VC.oracle_result(name), VC.classes(name)
    fig = VC.check_build(orc, ref, c.min_pts, c.eig_mult, cls)
    print(name, " ".join("%s %.2e" % kv for kv in fig.items()))
    if not c.big:
        VC.check_lookups(c, orc, *_oracle_lookups(c, orc))


def test_the_recorded_maxima_are_what_is_measured():
    """The bars are four times the recorded figures; the figures must not drift away from what the oracle and the restatement do: the measured maxima lie between a
    quarter of the record and the bar."""
    worst = dict.fromkeys(VC.BARS, 0.0)
    for n in NAMES:
        for k, v in VC.compare(VC.oracle_result(n), VC.np_result(n), VC.classes(n)).items():
            worst[k] = max(worst[k], v)
    print("oracle vs numpy maxima:", " ".join("%s %.3e (recorded %.1e)" % (k, v, VC.ORACLE_VS_NUMPY[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert VC.ORACLE_VS_NUMPY[k] / 4 <= v <= VC.BARS[k], (k, v)


@pytest.mark.parametrize("name", NAMES)
def test_no_leaf_is_undetermined_unless_the_case_names_it(name):
    """A condition, not a share; and no determined leaf sits on the inflation threshold, where lambda_min < eig_mult lambda_max would be rounding's choice again."""
    c, ref, cls = VC.BY_NAME[name], VC.np_result(name), VC.classes(name)
    assert int((cls == "U").sum()) == c.undetermined
    live = (cls == "D") & (ref["leaf_n"] >= 0)
    C = ref["cov_raw"][live].reshape(-1, 3, 3)
    if len(C) and c.eig_mult > 0:
        w = np.linalg.eigvalsh(0.5 * (C + C.transpose(0, 2, 1)))
        for k in (0, 1):
            assert (np.abs(w[:, k] / w[:, 2] - c.eig_mult) >= 1e-9).all()


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group == "sort"])
def test_sort_case_selects_its_instance(name):
    c, ref = VC.BY_NAME[name], VC.np_result(name)
    d, n = c.data, len(c.cloud)
    assert tuple(ref["grid"][6:9]) == d["dims"] and 3000 <= n <= 5000 and n > 2 * 1024
    cells = int(np.prod(d["dims"]))
    assert VC.sort_instance(cells)[1:] == c.expect["instance"]
    key = _keys_of_points(ref, n)
    assert (key[:1024] >= 0).all() and len(np.unique(key[:1024] & 1023)) == 1 and len(np.unique(key[:1024])) > 1      # one bin of every digit width takes the first sort tile
    assert ref["leaf_key"][-1] == cells - 1 and (key < 0).sum() == 9                                                  # the largest valid key, then the invalid ones
    l = int(np.argmax(np.diff(ref["offsets"])))
    ids = ref["point_ids"][ref["offsets"][l]:ref["offsets"][l + 1]]
    assert len(ids) == 3000 and len(np.unique(ids // 1024)) >= 3 and (np.diff(ids) > 0).all()


def test_every_instance_but_the_31_bit_one_is_placed():
    assert {c.expect["instance"][1:] for c in VC.CASES if c.group == "sort"} == {(9, 2), (10, 2), (8, 3), (9, 3), (10, 3)}
    assert VC.sort_instance(2 ** 31 - 1)[1:] == (31, 8, 4)
    for bits, want in ((18, (9, 2)), (19, (10, 2)), (20, (10, 2)), (21, (8, 3)), (24, (8, 3)), (25, (9, 3)), (27, (9, 3)), (28, (10, 3)), (30, (10, 3)), (31, (8, 4))):
        assert VC.sort_instance(1, cap=(1 << bits) - 1)[2:] == want


def _profile_claims(heads, off, T, n_valid):
    assert np.array_equal(off[:len(heads)], heads)
    h = set(int(x) for x in heads[:-1])
    assert {255, 256, 257} <= h and {5120 + 3 * T + T - 1, 5120 + 4 * T, 5120 + 4 * T + 1} <= h
    sizes = np.diff(heads)
    assert {256, 257, 512, 513, 2300} <= set(int(s) for s in sizes)
    at = int(heads[list(sizes).index(2300)])
    assert at % T not in (0, T - 1) and at % 256 not in (0, 255)
    per_tile = np.bincount(np.asarray(heads[:-1]) // T)
    assert (per_tile[at // T + 1:(at + 2300) // T] == 0).all() and (at + 2300) // T - at // T >= 2          # tiles the long leaf covers: no head
    assert [int(per_tile[5120 // T + i]) for i in range(3)] == [127, 128, 129]
    run = np.nonzero(sizes == 1)[0]
    assert max(len(r) for r in np.split(run, np.nonzero(np.diff(run) > 1)[0] + 1)) >= 512


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group in ("tiles", "sizes")])
def test_tile_and_size_cases_put_the_heads_where_they_claim(name):
    c, ref = VC.BY_NAME[name], VC.np_result(name)
    d, n = c.data, len(c.cloud)
    n_valid = int(ref["offsets"][-1])
    if c.group == "sizes":
        assert n == int(name[2:])
    if "heads" not in d:
        return
    assert d["T"] == VC.leaf_tile(n)
    _profile_claims(d["heads"], ref["offsets"], d["T"], n_valid)
    if "tail" in d:                                                       # the short profile at the highest keys: the last leaves
        assert np.array_equal(n_valid - ref["offsets"][-len(d["tail"]) - 1:-1], d["tail"])
        assert (n > VC.OWN_SORT_MAX) == (name == "n_1048577")
    if n_valid == n:
        assert name in ("tiles_end_at_n", "n_262144", "n_524288", "n_1048576")            # the last leaf ends at n exactly
    else:
        assert n_valid % d["T"] != 0 and n - n_valid >= 30                                 # the non-finite run begins inside the last leaf's tile


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group == "leaves"])
def test_leaf_cases_hold_both_sides_of_min_pts_and_the_exact_leaves(name):
    c, ref, cls = VC.BY_NAME[name], VC.np_result(name), VC.classes(name)
    cnt = np.diff(ref["offsets"])
    assert {c.min_pts - 1, c.min_pts, c.min_pts + 1} <= set(int(x) for x in cnt)
    far = int(np.argmax(ref["mean"][:, 0]))
    assert ref["mean"][far, 0] > 100 and cls[far] == ("D" if cnt[far] >= c.min_pts else "P")
    if c.eig_mult == 0:
        assert not ref["inflated"].any() and (cls != "E").all()
        return
    ex = np.nonzero(cls == "E")[0]
    assert len(ex) == (3 if c.min_pts <= 8 else 1)
    if c.min_pts <= 8:
        out = sorted((int(ref["leaf_n"][l]), tuple(ref["evals"][l] / max(ref["evals"][l][2], 1e-300))) for l in ex)
        assert out[0][0] == -1                                                            # coincident points: rejected, exactly
        assert out[1] == (8, (c.eig_mult, c.eig_mult, 1.0))                               # the rod: two exact zeros, both inflated
        assert out[2][0] == 16 and out[2][1][0] == c.eig_mult and out[2][1][1] > c.eig_mult   # the plate: one
        for l in ex:
            assert sorted(np.abs(ref["evecs"][l]).round(12)).count(1.0) >= 1 or ref["leaf_n"][l] == -1


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.group == "edges"])
def test_edge_cases_hold_points_whose_build_cell_is_not_their_lookup_cell(name):
    c, ref = VC.BY_NAME[name], VC.np_result(name)
    x = c.data["face"][:, 0]
    differ = VC.build_cells(x, c.leaf) != VC.build_cells(x, c.leaf, divide=True)
    print(name, "build cell != lookup cell:", int(differ.sum()), "of", len(x))
    assert differ.sum() >= 20
    assert np.signbit(x).any() and (x == 0).sum() >= 2                                    # -0.0 and +0.0
    q = c.queries
    ids = VC.np_lookup(ref["grid"], ref["leaf_key"], ref["leaf_n"], q, c.leaf, c.min_pts, VC.DIRECT7)
    out = slice(len(x), len(x) + 8)
    assert (ids[out, 0] == -1).all() and (ids[out][:6, 1:] >= 0).sum(axis=1).min() >= 1   # one cell outside each face: a displacement brings the query back in
    if "thin" in name:
        assert tuple(ref["grid"][7:9]) == (1, 1)


VARIANTS = [("divide_in_build", "edges_0.3"), ("unstable_order", "n_65"), ("le_min_pts", "leaves_min6_mult0.01"), ("inflate_ev0_only", "leaves_min6_mult0.01"),
            ("no_bessel", "n_257"), ("strict_range", "edges_thin_0.3"), ("rejected_visible", "leaves_min6_mult0.01"), ("multiply_in_lookup", "edges_0.7")]


@pytest.mark.parametrize("variant,name", VARIANTS)
def test_a_wrong_variant_is_noticed(variant, name):
    c, ref, cls = VC.BY_NAME[name], VC.np_result(name), VC.classes(name)
    if variant in ("strict_range", "rejected_visible", "multiply_in_lookup"):
        bad = lambda q, rel: VC.np_lookup(ref["grid"], ref["leaf_key"], ref["leaf_n"], q, c.leaf, c.min_pts, rel, variant=variant)
        with pytest.raises(AssertionError):
            VC.check_lookups(c, ref, lambda q: bad(q, VC.REL1)[:, 0], lambda q: bad(q, VC.DIRECT7), bad)
    else:
        with pytest.raises(AssertionError):
            VC.check_build(VC.np_voxel_build(c.cloud, c.leaf, c.min_pts, c.eig_mult, variant=variant), ref, c.min_pts, c.eig_mult, cls)


def test_check_build_accepts_either_outcome_of_an_undetermined_leaf_but_not_a_mixture():
    name = "leaves_min3_mult0.01"
    c, ref, cls = VC.BY_NAME[name], VC.np_result(name), VC.classes(name)
    for l in np.nonzero(cls == "U")[0]:
        got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        if ref["leaf_n"][l] == -1:                      # the other outcome: kept and inflated
            w, V = np.linalg.eigh(0.5 * (ref["cov_raw"][l].reshape(3, 3) + ref["cov_raw"][l].reshape(3, 3).T))
            w = np.maximum(w, c.eig_mult * w[2])
            Cn = (V * w) @ V.T
            got["leaf_n"][l], got["evals"][l], got["cov"][l], got["icov"][l] = np.diff(ref["offsets"])[l], w, Cn.reshape(9), np.linalg.inv(Cn).reshape(9)
        else:                                           # rejected
            got["leaf_n"][l], got["evals"][l], got["icov"][l], got["cov"][l] = -1, 0, 0, ref["cov_raw"][l]
        VC.check_build(got, ref, c.min_pts, c.eig_mult, cls)
        got["icov"][l] = 1.0                            # neither
        with pytest.raises(AssertionError):
            VC.check_build(got, ref, c.min_pts, c.eig_mult, cls)
