"""CPU: holds the scan-registration cases of tests/scanreg_cases.py to the regime each one claims (from the oracle's scan_start / scan_end / less_flat), and the oracle's
own results to checks that do not rest on it (curvature recomputed in numpy float32, `picked` recomputed from the lists, what the reference's pick loop can produce).
tests/test_gpu_scanreg_shapes.py then runs the same cases through the C ABI."""
import numpy as np
import pytest

import scanreg_cases as SC
from oracle import oracle as O
from upstream_checks import tie_sectors as _tie_sectors


def test_case_table_is_the_one_asked_for():
    assert [(c.name, c.n_rings) for c in SC.CASES] == [("r32x2048", 32), ("r64x1024", 64), ("r128x512", 128), ("r130x300", 130), ("r1024x24", 1024), ("ring4096", 1), ("ring4097", 1),
                                                       ("long4", 4), ("long16", 16), ("long_ties", 3), ("sec2048", 1), ("sec2049", 1), ("stray_rings", 16)]
    assert SC.MIN_RANGE == 0.3
    for name, shape in (("r32x2048", 32 * 2048), ("r64x1024", 64 * 1024), ("r128x512", 128 * 512), ("r130x300", 130 * 300), ("r1024x24", 1024 * 24), ("ring4096", 4096),
                        ("ring4097", 4097), ("long4", 4 * 4200), ("long16", 16 * 4500), ("long_ties", 3 * 4500), ("sec2048", 12299), ("sec2049", 12305), ("stray_rings", 16 * 1800)):
        assert len(SC.points(name)) == shape
    assert max(len(SC.points(c.name)) for c in SC.CASES) == 72000


def test_one_ring_has_exactly_the_kept_points_asked_for():
    for m in (4096, 4097, 12299, 12305):
        pts = SC.one_ring(20, m)
        assert len(pts) == m and (pts["ring"] == 0).all() and O.scan_register(pts, 1, SC.MIN_RANGE)["n"] == m


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_case_is_in_its_regime(name):
    case, ro = SC.BY_NAME[name], SC.oracle_result(name)
    npts, sec = SC.ring_points(ro), SC.sector_lengths(ro)
    lf = SC.less_flat_per_ring(ro)
    print("%s: path %s, rings of %d-%d points, longest sector %d, less-flat per ring at most %d, tie sectors %d" % (name, SC.path_of(ro), npts.min(), npts.max(), sec.max(), lf.max(), _tie_sectors(ro)))
    assert npts.sum() == ro["n"] == int((SC.kept_mask(SC.points(name)) & (SC.points(name)["ring"] < case.n_rings)).sum())
    assert SC.path_of(ro) == case.path
    assert (npts <= SC.SR_RING_MAX).all() if case.path == "lds" else (npts[npts > 0] > SC.SR_RING_MAX).all()
    if name in SC.MULTI_RING:
        assert (npts > 0).all() and len(sec) == case.n_rings        # every ring non-empty, and long enough to be classified
    if name == "sec2049":
        assert sec.max() == SC.SR_SEC_MAX + 1
    else:
        assert sec.max() <= SC.SR_SEC_MAX
    if name == "sec2048":
        assert (sec == SC.SR_SEC_MAX).all()
    if name in ("ring4096", "ring4097"):
        assert npts[0] == int(name[4:]) and sec.max() <= 1024       # the LDS path's sector capacity (SR_SEC_LDS) on both sides of the seam
    if name == "long4":
        assert (lf <= SC.SRV_CAP).all() and lf.max() > SC.SRV_CAP - 200      # classified on the global path, downsampled in LDS, close to its capacity
    if name == "long16":
        assert (lf > SC.SRV_CAP).any()
    if name == "long_ties":
        assert _tie_sectors(ro) >= 5
    if name == "r128x512":
        assert npts[SC.SR_HIST_RINGS - 1] > 0 and case.n_rings == SC.SR_HIST_RINGS
    if name == "r130x300":
        assert (SC.points(name)["ring"][SC.kept_mask(SC.points(name))] >= SC.SR_HIST_RINGS).any() and (npts[SC.SR_HIST_RINGS:] > 0).all()
    if name == "r1024x24":
        assert case.n_rings == SC.MAX_RINGS and npts.min() >= 17 and npts.max() <= 24 and sec.min() >= 1 and sec.max() <= 3
    if name == "stray_rings":
        ring = SC.points(name)["ring"]
        assert set(np.unique(ring[ring >= 16])) == set(SC.STRAY_IDS) and (ring >= 16).sum() == len(range(50, len(ring), 50)) and ring[0] == 0
        assert (SC.kept_mask(SC.points(name)) & (ring >= 16)).sum() > 500      # the strays are not the points that the range filter removes anyway


def test_batch_sweeps_mix_both_paths():
    sw = SC.batch_sweeps()
    assert [len(p) for p in sw] == [28800, 4097, 0, 4096, 4500, 640]
    paths = []
    for p in sw:
        ro = O.scan_register(p, 16, SC.MIN_RANGE)
        paths.append(SC.path_of(ro) if len(SC.sector_lengths(ro)) else None)
    assert paths == ["lds", "global", None, "lds", "global", "lds"]
    assert (sw[1]["ring"] == 3).all() and (sw[3]["ring"] == 15).all() and (sw[4]["ring"] == 0).all()
    assert _tie_sectors(O.scan_register(sw[4], 16, SC.MIN_RANGE)) >= 1
    assert sorted(SC.BATCH_LONG_AND_EMPTY) == [1, 2, 4]


@pytest.mark.parametrize("name", SC.CHECKED)
def test_oracle_result_passes_the_oracle_independent_checks(name):
    SC.check_result(SC.oracle_result(name), SC.BY_NAME[name].n_rings)


def test_checks_notice_a_wrong_result():
    """check_result is the judge of the device's output too: it must see a swapped pick, a missed neighbour mark, a marked fourth flat point, one ulp of curvature."""
    ro = SC.oracle_result("long4")

    def broken(**kw):
        r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ro.items()}
        for k, f in kw.items():
            f(r[k])
        with pytest.raises(AssertionError):
            SC.check_result(r, 4)

    SC.check_result({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ro.items()}, 4)
    fourth = ro["flat"][3]
    assert ro["picked"][fourth] == 0        # sector 0 of ring 0 has four flat points and nothing after them reaches the fourth

    def one_ulp(c): c.view(np.uint32)[100] += 1
    def swap(a): a[[0, 1]] = a[[1, 0]]
    def mark_fourth(p): p[fourth] = 1
    def unmark(p): p[ro["less_sharp"][0] + 1] ^= 1
    def drop_label(l): l[ro["flat"][0]] = 0
    def unsorted(s): s[[ro["scan_start"][0], ro["scan_start"][0] + 1]] = s[[ro["scan_start"][0] + 1, ro["scan_start"][0]]]
    broken(curvature=one_ulp)
    broken(less_sharp=swap)
    broken(flat=swap)
    broken(picked=mark_fourth)
    broken(picked=unmark)
    broken(label=drop_label)
    broken(sort_ind=unsorted)
    broken(less_flat=swap)


def test_oracle_drops_ring_ids_outside_the_ring_count():
    """Ring ids >= n_rings: the reference indexes its per-ring vector with them unchecked (undefined); the oracle drops them, as the library does — the result is the
    one of the sweep without those points, in every field."""
    pts, n_rings = SC.points("stray_rings"), 16
    assert (pts["ring"] >= n_rings).sum() > 500
    r_all, r_filtered = O.scan_register(pts, n_rings, SC.MIN_RANGE), SC.oracle_result("stray_rings")
    assert r_all["n"] == r_filtered["n"] < int(SC.kept_mask(pts).sum())
    for k in ("scan_start", "scan_end", "label", "picked", "sort_ind", "sharp", "less_sharp", "flat", "less_flat"):
        assert np.array_equal(r_all[k], r_filtered[k]), k
    for k in ("cloud", "curvature"):
        assert np.array_equal(r_all[k].view(np.uint32), r_filtered[k].view(np.uint32)), k
    only = pts.copy(); only["ring"][:] = 16
    r = O.scan_register(only, n_rings, SC.MIN_RANGE)
    assert r["n"] == 0 and all(len(r[k]) == 0 for k in ("sharp", "less_sharp", "flat", "less_flat"))
