"""Comparison helpers shared by the upstream-kernel parity tests (GPU result dict vs oracle result dict)."""
import numpy as np


def check_voxels(vg, vo, min_pts=6):
    """voxel grid: leaf keys / counts / point lists exact; mean, cov 1e-12 rel; eigenvalues 1e-10 rel; eigenvectors up to sign; inverse covariance 1e-8 rel"""
    assert vg["n_leaves"] == vo["n_leaves"] and np.array_equal(vg["grid"], vo["grid"])
    assert np.array_equal(vg["leaf_key"], vo["leaf_key"]) and np.array_equal(vg["leaf_n"], vo["leaf_n"])
    assert np.array_equal(vg["offsets"], vo["offsets"]) and np.array_equal(vg["point_ids"][:vo["offsets"][-1]], vo["point_ids"][:vo["offsets"][-1]])
    assert np.allclose(vg["mean"], vo["mean"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(vg["centroid"].view(np.uint32), vo["centroid"].view(np.uint32))
    ok = vo["leaf_n"] >= min_pts     # (the value the grids were built with: leaves below it carry placeholders, rejected ones -1)
    sc = np.abs(vo["cov"][ok]).max(axis=1, keepdims=True)
    assert (np.abs(vg["cov"][ok] - vo["cov"][ok]) <= 1e-12 * sc + 1e-18).all()
    assert np.allclose(vg["evals"][ok], vo["evals"][ok], rtol=1e-10, atol=1e-16)
    si = np.abs(vo["icov"][ok]).max(axis=1, keepdims=True)
    assert (np.abs(vg["icov"][ok] - vo["icov"][ok]) <= 1e-8 * si).all()
    Vg, Vo = vg["evecs"][ok].reshape(-1, 3, 3), vo["evecs"][ok].reshape(-1, 3, 3)
    ev = vo["evals"][ok]
    sep = (np.diff(ev, axis=1).min(axis=1) > 1e-6 * ev[:, 2])       # eigenvectors only comparable for separated eigenvalues
    dots = np.abs(np.einsum("nij,nij->nj", Vg[sep], Vo[sep]))
    assert (dots > 1 - 1e-8).all()


def compare_scanreg(rg, ro, strict=True):
    """One result dict of lvx.scan_register (or of one sweep of a batch) against the oracle's: counts, ring bounds, cloud and curvature bits, labels, picks and lists."""
    assert rg["n"] == ro["n"]
    assert np.array_equal(rg["scan_start"], ro["scan_start"]) and np.array_equal(rg["scan_end"], ro["scan_end"])
    assert np.array_equal(rg["cloud"].view(np.uint32), ro["cloud"].view(np.uint32))
    assert np.array_equal(rg["curvature"].view(np.uint32), ro["curvature"].view(np.uint32))
    if strict:
        for k in ("label", "picked", "sort_ind", "sharp", "less_sharp", "flat", "less_flat"):
            assert np.array_equal(rg[k], ro[k]), k
    else:   # equal curvatures inside a sector: std::sort (unstable) may order them differently -> compare modulo tie permutation
        c = ro["curvature"]
        assert np.array_equal(c[rg["sort_ind"]].view(np.uint32), c[ro["sort_ind"]].view(np.uint32))
        assert np.array_equal(np.sort(rg["sort_ind"]), np.sort(ro["sort_ind"]))


def check_scanreg(ctx, pts, n_rings, min_range, strict=True):
    """lvx.scan_register against the oracle on the same sweep; returns the oracle's result."""
    import lvx
    from oracle import oracle as O
    ro = O.scan_register(pts, n_rings, min_range)
    compare_scanreg(lvx.scan_register(ctx, pts, n_rings, min_range), ro, strict)
    return ro


def tie_sectors(ro):
    """Sectors (scanRegistration.cpp:321-322) that hold two equal curvatures."""
    c, n = ro["curvature"], 0
    for i in range(len(ro["scan_start"])):
        s, e = ro["scan_start"][i], ro["scan_end"][i]
        for j in range(6):
            sp, ep = s + (e - s) * j // 6, s + (e - s) * (j + 1) // 6 - 1
            n += len(np.unique(c[sp:ep + 1])) < ep - sp + 1
    return n
