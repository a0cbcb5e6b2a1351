"""Shared by tests/test_scanreg_cases.py (CPU) and tests/test_gpu_scanreg_shapes.py: scan-registration sweeps PAST the 16 x 1 800 sweep of the older tests, one per
branch of csrc/lvx_upstream.hip that ring count and ring length select, and checks of a result dict that do not rest on the oracle.

    k_sr_classify   a ring of <= SR_RING_MAX = 4 096 kept points lives in LDS (ballot pick); a longer one takes sr_classify_ring<false>: ring in global memory, one
                    sector at a time sorted by the whole workgroup, serial pick on one lane.  A sector holds at most SR_SEC_MAX = 2 048 points (a ring of 12 299).
    k_sr_count      LDS histogram for rings 0-127, global atomics for rings >= 128; the ABI takes up to 1 024 rings.
    k_sr_voxelgrid  at most SRV_CAP = 4 096 less-flat points per ring.
    ring ids >= n_rings are dropped (library and oracle; the reference indexes its per-ring vector with them unchecked).

tests/test_scanreg_cases.py holds every case to its regime from the oracle's scan_start / scan_end / less_flat alone (ring_points, sector_lengths, less_flat_per_ring).

check_result(r, n_rings) takes the dict of oracle.scan_register or lvx.scan_register.  The oracle is a restatement by the same hands as the kernel, so: the curvature is
recomputed in numpy float32 in the reference's order of additions (scanRegistration.cpp:295-305), `picked` is recomputed from the four lists and the cloud (:374-391,
:407-423), and the lists are held to what the reference's loop can produce at all (:316-447)."""
import functools
from collections import namedtuple

import numpy as np

import synth

MIN_RANGE = 0.3
SR_RING_MAX, SR_SEC_MAX, SRV_CAP, SR_HIST_RINGS, MAX_RINGS = 4096, 2048, 4096, 128, 1024
STRAY_IDS = (16, 17, 300, 65535)


def kept_mask(pts, min_range=MIN_RANGE):
    """What removeClosedPointCloud keeps (scanRegistration.cpp:101-131): float range^2 >= min_range^2, no NaN coordinate."""
    x, y, z = pts["x"], pts["y"], pts["z"]
    thr = np.float32(min_range)
    with np.errstate(invalid="ignore"):
        far = ~(x * x + y * y + z * z < thr * thr)
    return far & ~(np.isnan(x) | np.isnan(y) | np.isnan(z))


def one_ring(seed, m, **kw):
    """A sweep of ONE ring with exactly m kept points: the first m survivors of a sweep of m + 400."""
    pts = synth.make_vlp16_sweep(seed=seed, n_rings=1, n_az=m + 400, **kw)
    pts = pts[kept_mask(pts)][:m].copy()
    assert len(pts) == m and kept_mask(pts).all()
    return pts


def _stray_rings():
    pts = synth.make_vlp16_sweep(seed=1)
    idx = np.arange(50, len(pts), 50)
    pts["ring"][idx] = np.array(STRAY_IDS, np.uint16)[np.arange(len(idx)) % len(STRAY_IDS)]
    assert pts["ring"][0] == 0
    return pts


Case = namedtuple("Case", "name make n_rings path")      # path: the branch of k_sr_classify every non-empty ring must take
_sweep = synth.make_vlp16_sweep

CASES = [
    Case("r32x2048", lambda: _sweep(seed=6, n_rings=32, n_az=2048), 32, "lds"),
    Case("r64x1024", lambda: _sweep(seed=5, n_rings=64, n_az=1024), 64, "lds"),
    Case("r128x512", lambda: _sweep(seed=22, n_rings=128, n_az=512), 128, "lds"),
    Case("r130x300", lambda: _sweep(seed=4, n_rings=130, n_az=300), 130, "lds"),
    Case("r1024x24", lambda: _sweep(seed=21, n_rings=1024, n_az=24), 1024, "lds"),
    Case("ring4096", lambda: one_ring(20, 4096), 1, "lds"),
    Case("ring4097", lambda: one_ring(20, 4097), 1, "global"),
    Case("long4", lambda: _sweep(seed=3, n_rings=4, n_az=4200), 4, "global"),
    Case("long16", lambda: _sweep(seed=1, n_rings=16, n_az=4500), 16, "global"),
    Case("long_ties", lambda: _sweep(seed=8, n_rings=3, n_az=4500, xyz_quantum=0.01, noise=0.0), 3, "global"),
    Case("sec2048", lambda: one_ring(20, 12299), 1, "global"),
    Case("sec2049", lambda: one_ring(20, 12305), 1, "global"),
    Case("stray_rings", _stray_rings, 16, "lds"),
]
BY_NAME = {c.name: c for c in CASES}
MULTI_RING = ("r32x2048", "r64x1024", "r128x512", "r130x300", "r1024x24", "long4", "long16", "long_ties", "stray_rings")
CHECKED = [c.name for c in CASES if c.name != "sec2049"]                                   # sec2049: only the library has the capacity, its result is an error
PARITY = [c.name for c in CASES if c.name not in ("sec2049", "stray_rings")]


@functools.lru_cache(maxsize=None)
def points(name):
    pts = BY_NAME[name].make()
    pts.setflags(write=False)
    return pts


def oracle_input(name):
    """What the oracle is given: the sweep itself; for stray_rings the sweep without the points whose ring id is outside [0, n_rings)."""
    pts = points(name)
    return pts[pts["ring"] < BY_NAME[name].n_rings] if name == "stray_rings" else pts


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    from oracle import oracle as O
    r = O.scan_register(oracle_input(name), BY_NAME[name].n_rings, MIN_RANGE)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def batch_sweeps():
    """The sweeps of the batch test (n_rings = 16): long and short rings in one launch, the path chosen per ring."""
    a = one_ring(20, 4097); a["ring"][:] = 3
    b = one_ring(20, 4096); b["ring"][:] = 15
    t = one_ring(8, 4500, xyz_quantum=0.01, noise=0.0)
    return [_sweep(seed=1), a, _sweep(seed=3)[:0], b, t, _sweep(seed=4, n_az=40)]


BATCH_LONG_AND_EMPTY = (1, 4, 2)      # fetched again through scan_register_batch_d + scan_register_get


# ---- regimes: from scan_start / scan_end / less_flat only --------------------------------------------------------------------------------------------------
def ring_points(r):
    return r["scan_end"].astype(np.int64) - r["scan_start"] + 11


def sector_bounds(r):
    """(sp, ep) [rings with scan_end - scan_start >= 6][6], as scanRegistration.cpp:321-322 divides a ring."""
    s, e = r["scan_start"].astype(np.int64), r["scan_end"].astype(np.int64)
    ok = e - s >= 6
    s, e = s[ok, None], e[ok, None]
    j = np.arange(6)[None, :]
    return s + (e - s) * j // 6, s + (e - s) * (j + 1) // 6 - 1


def sector_lengths(r):
    sp, ep = sector_bounds(r)
    return ep - sp + 1


def less_flat_per_ring(r):
    lf = r["less_flat"]
    return np.array([int(((lf >= s - 5) & (lf <= e + 5)).sum()) for s, e in zip(r["scan_start"], r["scan_end"])])


def path_of(r):
    """'lds' / 'global' / 'mixed' over the rings that are classified at all (scan_end - scan_start >= 6)."""
    n = ring_points(r)[r["scan_end"].astype(np.int64) - r["scan_start"] >= 6]
    return "lds" if (n <= SR_RING_MAX).all() else "global" if (n > SR_RING_MAX).all() else "mixed"


# ---- checks that do not rest on the oracle -----------------------------------------------------------------------------------------------------------------
def curvature_f32(cloud):
    """scanRegistration.cpp:295-305 in float32, the eleven taps added in the reference's order, over the ring-major cloud (ring borders are not special there)."""
    m = len(cloud)
    out = np.zeros(m, np.float32)
    if m < 11:
        return out
    d = []
    for a in range(3):
        v = np.ascontiguousarray(cloud[:, a], np.float32)
        t = lambda k: v[5 + k:m - 5 + k]
        s = t(-5) + t(-4)
        s = s + t(-3); s = s + t(-2); s = s + t(-1)
        s = s - np.float32(10) * t(0)
        s = s + t(1); s = s + t(2); s = s + t(3); s = s + t(4); s = s + t(5)
        assert s.dtype == np.float32
        d.append(s)
    c = d[0] * d[0] + d[1] * d[1]
    out[5:m - 5] = c + d[2] * d[2]
    return out


def _position_in_group(g):
    """For a non-decreasing array: index of every element inside its run of equal values."""
    return np.arange(len(g)) - np.searchsorted(g, g, side="left")


def check_result(r, n_rings):
    """Asserts on one result dict; see the module docstring."""
    m = r["n"]
    cloud, c, label, sort_ind, picked = r["cloud"], r["curvature"], r["label"], r["sort_ind"], r["picked"]
    assert len(cloud) == len(c) == len(label) == len(sort_ind) == len(picked) == m and len(r["scan_start"]) == len(r["scan_end"]) == n_rings
    # rings tile the cloud
    npts = ring_points(r)
    assert (npts >= 0).all() and npts.sum() == m and np.array_equal(r["scan_start"] - 5, np.concatenate([[0], np.cumsum(npts)[:-1]]))
    # curvature
    assert np.array_equal(c.view(np.uint32), curvature_f32(cloud).view(np.uint32))
    # sectors
    sp, ep = sector_bounds(r)
    sec = np.full(m, -1, np.int64)
    for k, (a, b) in enumerate(zip(sp.ravel(), ep.ravel())):
        sec[a:b + 1] = k
    # sort_ind: the identity outside the sectors, inside a sector a permutation of it with non-decreasing curvature
    assert np.array_equal(np.sort(sort_ind), np.arange(m)) and np.array_equal(sec[sort_ind], sec) and np.array_equal(sort_ind[sec < 0], np.flatnonzero(sec < 0))
    cs = c[sort_ind]
    inside = (sec[1:] == sec[:-1]) & (sec[1:] >= 0)
    assert (cs[1:][inside] >= cs[:-1][inside]).all()
    # the lists: pushed sector after sector; at most 2 / 20 / 4 per sector; sharp = the first two less-sharp picks of its sector; thresholds as the reference compares
    # them (float against the double 0.1)
    c64 = c.astype(np.float64)
    grp = {}
    for key, cap in (("sharp", 2), ("less_sharp", 20), ("flat", 4)):
        L = r[key]
        assert len(np.unique(L)) == len(L) and ((L >= 0) & (L < m)).all()
        g = sec[L]
        assert (g >= 0).all() and (np.diff(g) >= 0).all(), key
        pos = _position_in_group(g)
        assert (pos < cap).all(), key
        assert (c64[L] < 0.1).all() if key == "flat" else (c64[L] > 0.1).all(), key
        grp[key] = pos
    sharp, lsharp, flat = r["sharp"], r["less_sharp"], r["flat"]
    assert np.array_equal(sharp, lsharp[grp["less_sharp"] < 2])
    # picks in a sector go by curvature: descending for the less-sharp list, ascending for the flat one
    for L, sign in ((lsharp, -1), (flat, 1)):
        same = sec[L][1:] == sec[L][:-1]
        assert (sign * (c[L][1:] - c[L][:-1])[same] >= 0).all()
    # labels are set by the picks and by nothing else
    want = np.zeros(m, np.int32)
    want[lsharp] = 1; want[sharp] = 2; want[flat] = -1
    assert len(np.intersect1d(lsharp, flat)) == 0 and np.array_equal(label, want)
    # less_flat: every sector point with label <= 0, sectors in order, increasing inside each
    assert np.array_equal(r["less_flat"], np.flatnonzero((sec >= 0) & (label <= 0)))
    # picked, from the lists: every pick marks itself and up to five neighbours on each side, a side ending at its first gap^2 > 0.05 — except the FOURTH flat point of
    # a sector, where the reference breaks before marking (:394-403); such a point is picked only where a neighbouring pick of a later sector reached it
    marking = np.concatenate([lsharp, flat[grp["flat"] < 3]]).astype(np.int64)
    d = cloud[1:, :3] - cloud[:-1, :3]
    brk = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float64) > 0.05       # between i and i + 1, float as gap2; symmetric in its two points
    assert d.dtype == np.float32
    exp = np.zeros(m, np.int32)
    exp[marking] = 1
    fwd, bwd = np.ones(len(marking), bool), np.ones(len(marking), bool)
    for l in range(1, 6):
        fwd &= ~brk[marking + l - 1]
        bwd &= ~brk[marking - l]
        exp[marking[fwd] + l] = 1
        exp[marking[bwd] - l] = 1
    assert np.array_equal(picked, exp)
    for key in ("sharp", "less_sharp"):
        assert picked[r[key]].all()
    assert picked[flat[grp["flat"] < 3]].all()
    fourth = flat[grp["flat"] == 3]
    reached = np.zeros(m, bool)
    for l in range(-5, 6):
        reached[np.clip(marking + l, 0, m - 1)] = True
    assert not picked[fourth[~reached[fourth]]].any()
