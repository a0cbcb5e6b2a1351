"""GPU: scan registration past the 16 x 1 800 sweep — the cases of tests/scanreg_cases.py (tests/test_scanreg_cases.py holds each to its regime on the CPU) through the
C ABI, bit-exact against the oracle as in tests/test_gpu_upstream.py, and the device's own result through the oracle-independent checks of scanreg_cases.check_result.

Reached here and by no older test: sr_classify_ring<false> (rings > 4 096 points: ring in global memory, workgroup-wide sector sort, serial pick, libstdc++'s order for
tied curvatures in that layout), the seam at 4 096 / 4 097, sectors of exactly 2 048 points and the handled error one point beyond, ring counts of 1 / 3 / 4 / 32 / 64 /
128 / 130 / 1 024 (k_sr_count's global-atomic branch from ring 128 on, the per-ring list strides, k_sr_bucket's prefix over rings), ring ids >= n_rings, the less-flat
down-sampling after the global path and its capacity error."""
import numpy as np
import pytest

import lvx
import scanreg_cases as SC
import synth
from oracle import oracle as O
from upstream_checks import compare_scanreg

pytestmark = pytest.mark.gpu

KEYS = ("cloud", "curvature", "label", "picked", "sort_ind", "scan_start", "scan_end", "sharp", "less_sharp", "flat", "less_flat")


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _register(ctx, name):
    """lvx.scan_register of a case, compared with the oracle in every field and held to the oracle-independent checks."""
    case = SC.BY_NAME[name]
    rg = lvx.scan_register(ctx, SC.points(name), case.n_rings, SC.MIN_RANGE)
    compare_scanreg(rg, SC.oracle_result(name), strict=True)
    SC.check_result(rg, case.n_rings)
    return rg


def _downsample_expected(ro, n_rings, leaf=0.2):
    lf = ro["less_flat"]
    return [O.voxelgrid_xyzi(ro["cloud"][lf[(lf >= ro["scan_start"][r] - 5) & (lf <= ro["scan_end"][r] + 5)]], leaf) for r in range(n_rings)]


def _check_downsample(ctx, ro, n_rings):
    want = _downsample_expected(ro, n_rings)
    got, ring_counts, n = lvx.scan_less_flat_downsample(ctx, n_rings, max_out=len(ro["less_flat"]))
    assert list(ring_counts) == [len(w) for w in want]
    want = np.concatenate(want)
    assert n == len(want) and 0 < n < len(ro["less_flat"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", SC.PARITY)
def test_case_is_bit_exact_and_passes_the_independent_checks(ctx, name):
    rg = _register(ctx, name)
    assert len(rg["sharp"]) > 0 and len(rg["less_sharp"]) >= len(rg["sharp"])


@pytest.mark.parametrize("order", [("ring4096", "ring4097"), ("ring4097", "ring4096")])
def test_both_sides_of_the_ring_seam_on_one_context(ctx, order):
    """4 096 points: the ring lives in LDS; 4 097: in global memory.  Either order on one context: the second call reuses the first one's work buffers."""
    for name in order + order[:1]:
        _register(ctx, name)


def test_downsample_after_the_global_path(ctx):
    """long4: rings of ~4 130 points are classified on the global path; their ~4 010 less-flat points still fit the down-sampling's LDS sort (4 096)."""
    _register(ctx, "long4")
    _check_downsample(ctx, SC.oracle_result("long4"), 4)


def test_downsample_capacity_error_leaves_the_context_usable(ctx):
    """long16: ~4 320 less-flat points in a ring are more than the down-sampling sorts in LDS: E_ARG, and the context goes on."""
    _register(ctx, "long16")
    with pytest.raises(lvx.LvxError) as e:
        lvx.scan_less_flat_downsample(ctx, 16, max_out=len(SC.oracle_result("long16")["less_flat"]))
    assert e.value.code == lvx.E_ARG and "LDS sort capacity (4096)" in str(e.value)
    pts = synth.make_vlp16_sweep(seed=1)
    ro = O.scan_register(pts, 16, SC.MIN_RANGE)
    compare_scanreg(lvx.scan_register(ctx, pts, 16, SC.MIN_RANGE), ro, strict=True)
    _check_downsample(ctx, ro, 16)


def test_sector_capacity_error_leaves_the_context_usable(ctx):
    """A ring of 12 305 points has sectors of 2 049: one more than the sector sort holds.  The kernel reports it through its error word (a handled argument error);
    the same context then registers the ring of 12 299 points, whose sectors are exactly 2 048 — the full power-of-two sort, no padding keys."""
    with pytest.raises(lvx.LvxError) as e:
        lvx.scan_register(ctx, SC.points("sec2049"), 1, SC.MIN_RANGE)
    assert e.value.code == lvx.E_ARG and "scan sector longer than the LDS sort capacity" in str(e.value)
    _register(ctx, "sec2048")


def test_ring_ids_outside_the_ring_count_are_dropped(ctx):
    """Every 50th point carries ring 16, 17, 300 or 65535 at n_rings = 16: the result is the one of the sweep without those points, in all fields."""
    pts = SC.points("stray_rings")
    assert (pts["ring"] >= 16).sum() > 500
    rg = _register(ctx, "stray_rings")
    assert rg["n"] == len(SC.oracle_input("stray_rings")[SC.kept_mask(SC.oracle_input("stray_rings"))])
    compare_scanreg(rg, O.scan_register(pts, 16, SC.MIN_RANGE), strict=True)      # the oracle drops them too
    only = pts.copy(); only["ring"][:] = 16
    r = lvx.scan_register(ctx, only, 16, SC.MIN_RANGE)
    assert r["n"] == 0 and all(len(r[k]) == 0 for k in ("sharp", "less_sharp", "flat", "less_flat"))


@pytest.mark.parametrize("n_rings", [1025, 0])
def test_ring_count_outside_the_abi_is_an_argument_error(ctx, n_rings):
    with pytest.raises(lvx.LvxError) as e:
        lvx.scan_register(ctx, synth.make_vlp16_sweep(seed=4, n_az=40), n_rings, SC.MIN_RANGE)
    assert e.value.code == lvx.E_ARG
    with pytest.raises(lvx.LvxError) as e:
        lvx.scan_register_batch(ctx, [synth.make_vlp16_sweep(seed=4, n_az=40)], n_rings, SC.MIN_RANGE)
    assert e.value.code == lvx.E_ARG
    _register(ctx, "r64x1024")


def test_batch_with_long_and_short_rings_in_one_launch(ctx):
    """One lvx_scan_register_batch call, n_rings = 16: the default sweep, a ring of 4 097 points on ring 3, an empty sweep, a ring of 4 096 on ring 15, a ring of 4 500
    points with tied curvatures on ring 0, a sweep of 40-point rings.  blockIdx.y selects the sweep and the path is chosen per ring; every sweep is bit-exact against
    the oracle run on it alone."""
    sweeps = SC.batch_sweeps()
    want = [O.scan_register(p, 16, SC.MIN_RANGE) for p in sweeps]
    res = lvx.scan_register_batch(ctx, sweeps, 16, SC.MIN_RANGE)
    assert len(res) == len(sweeps)
    for k, (rg, ro) in enumerate(zip(res, want)):
        assert rg["n"] == ro["n"], k
        if len(sweeps[k]):
            assert np.array_equal(rg["scan_start"], ro["scan_start"]) and np.array_equal(rg["scan_end"], ro["scan_end"]), k
        assert np.array_equal(rg["cloud"].view(np.uint32), ro["cloud"].view(np.uint32)) and np.array_equal(rg["curvature"].view(np.uint32), ro["curvature"].view(np.uint32)), k
        for key in ("label", "picked", "sort_ind", "sharp", "less_sharp", "flat", "less_flat"):
            assert np.array_equal(rg[key], ro[key]), (k, key)
        if len(sweeps[k]):
            SC.check_result(rg, 16)
    # device-resident variant: points uploaded once by the caller, results stay in the context, one sweep fetched on demand
    import torch
    allp = np.concatenate(sweeps)
    off = np.concatenate([[0], np.cumsum([len(p) for p in sweeps])]).astype(np.int32)
    pd = torch.from_numpy(allp.view(np.uint8).reshape(-1)).to("cuda")
    nk, cnt = lvx.scan_register_batch_d(ctx, pd.data_ptr(), off, 16, SC.MIN_RANGE)
    assert list(nk) == [r_["n"] for r_ in want] and [list(c_) for c_ in cnt] == [[len(r_[k]) for k in ("sharp", "less_sharp", "flat", "less_flat")] for r_ in want]
    for k in SC.BATCH_LONG_AND_EMPTY:
        rg = lvx.scan_register_get(ctx, k, len(sweeps[k]), 16)
        for key in ("label", "picked", "sort_ind", "sharp", "less_sharp", "flat", "less_flat"):
            assert np.array_equal(rg[key], want[k][key]), (k, key)
        for key in ("cloud", "curvature"):
            assert np.array_equal(rg[key].view(np.uint32), want[k][key].view(np.uint32)), (k, key)


def test_global_path_with_ties_is_repeatable():
    """long_ties on a fresh context, twice: identical bytes in every output (the tie order is one lane's restatement of libstdc++'s sort, not a race)."""
    out = []
    for _ in range(2):
        c = lvx.Context(0)
        try:
            out.append(lvx.scan_register(c, SC.points("long_ties"), 3, SC.MIN_RANGE))
        finally:
            c.close()
    assert out[0]["n"] == out[1]["n"]
    for key in KEYS:
        assert out[0][key].tobytes() == out[1][key].tobytes(), key
    compare_scanreg(out[0], SC.oracle_result("long_ties"), strict=True)
