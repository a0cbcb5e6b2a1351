"""Voxel covariance grid (lvx_voxel_build: k_vx_extent, k_vx_keys, k_vx_sort_pass<FIRST, DB>, k_vx_leaf<PT>; lvx_voxel_lookup1 / 7 / _rel: k_vx_lookup<1 | 7>,
k_vx_lookup_rel): a case table that places every sort instance, every tile width and the leaf and cell edges directly, numpy restatements of the build
(voxel_grid_covariance_omp_impl.hpp:49-374) and of the lookups (:378-446), and check_build — what a result has to be whoever computed it.  Nothing here rests on the
oracle or on the kernels.  tests/test_voxel_cases.py holds every case to what it claims on the CPU and the oracle to the restatements; tests/test_gpu_voxel_cases.py
runs the same cases through the C ABI.

A leaf is one of four classes (classify):
  placeholder    fewer than min_pts points: identity cov and evecs, zero icov and evals, the count kept.
  determined     n >= 4 and lambda_min / lambda_max >= 1e-6 of the centred covariance (taken in long double): every solver agrees on it to the bars below.
  exact          dyadic coordinates and a power-of-two count: every sum, mean and product is exact in double, rows of the covariance that are zero are exactly zero and
                 stay zero through any Jacobi rotation, and what is left of it is well conditioned: rank deficiency is decided without rounding.
  undetermined   everything else — every leaf of <= 3 points, every coplanar or collinear leaf that is not exact.  Its smallest eigenvalue is +-1e-17 of the largest and
                 the rule "negative -> rejected, else inflated" follows the sign of rounding noise (the reference, with Eigen's solver, flips the same coin): either
                 outcome is accepted, but whichever is taken must be self-consistent (check_build).  A case states how many such leaves it holds.

Not placed: eig_mult = 0 on a leaf whose covariance is singular.  Nothing is inflated, the cofactor inverse is 0 * inf = NaN next to +-inf, and whether the
"icov holds an infinity" rejection sees the infinity behind a leading NaN depends on how max() treats NaN (fmax, std::max and Eigen's maxCoeff differ): undefined in the
reference too."""
import functools

import numpy as np

import surfel_cases as SC

DIRECT7 = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int32)
REL1 = DIRECT7[:1]
REL27 = np.array([[i, j, k] for k in (-1, 0, 1) for j in (-1, 0, 1) for i in (-1, 0, 1)], np.int32)
REL26 = REL27[np.abs(REL27).sum(axis=1) > 0]
CELLS_CAP0 = (1 << 18) - 1       # the cell table of a fresh context
OWN_SORT_MAX = 1048576           # points up to which the build sorts with k_vx_sort_pass (rocPRIM above)
DETERMINED_RATIO = 1e-6

# Largest oracle-vs-restatement differences over all cases, measured on the CPU (tests/test_voxel_cases.py prints them).  The bars are four times
# the record: headroom for another LAPACK or libm.  cov / icov relative to the leaf's largest entry, evals relative to lambda_max, evec = 1 - |cos| of separated
# eigenvectors.  Plain (not inflated) covariances are the same sums in the same order: bit-equal, the bar is zero.  The inflated covariance and its inverse carry the
# asymmetry of :333 (sum_a mu_b and sum_b mu_a round apart by 1e-16 mu^2, 80 m from the origin 1e-10 of a thin leaf's covariance): LAPACK reads the symmetrised matrix,
# a Jacobi sweep its upper triangle.
ORACLE_VS_NUMPY = dict(cov_plain=0.0, cov_inflated=1.5e-10, evals=2.1e-15, icov=6.6e-10, evec=1.3e-15)
BARS = {k: 4 * v for k, v in ORACLE_VS_NUMPY.items()}
# The project's bars between kernel and oracle (tests/upstream_checks.py): two copies of one Jacobi
ORACLE_BARS = dict(cov_plain=1e-12, cov_inflated=1e-12, evals=1e-10, icov=1e-8, evec=1e-8)


def sort_instance(cells, cap=CELLS_CAP0):
    """(cells_cap, sort_bits, digit width, passes) the host selects for a grid of `cells` cells on a context whose cell table holds `cap`: the table grows to
    cells + cells / 4 when the grid does not fit, and never shrinks (voxel_build_device, vox_info, voxel_enqueue)."""
    if cells > cap:
        cap = min(cells + cells // 4, 2 ** 31 - 1)
    bits = 1
    while (1 << bits) - 1 < cap and bits < 31:
        bits += 1
    db, passes = 8, (bits + 7) // 8
    for d in (9, 10):
        if (bits + d - 1) // d < passes:
            db, passes = d, (bits + d - 1) // d
    return cap, bits, db, passes


def leaf_tile(n):
    """sorted positions per workgroup of k_vx_leaf"""
    return 1024 if n > 524288 else (512 if n > 262144 else 256)


# ------------------------------------------------------------------------------------------------------------------------
# the numpy restatements
# ------------------------------------------------------------------------------------------------------------------------
def _eigh3(C):
    """Ascending eigenvalues and eigenvectors (columns) of a symmetric 3 x 3 by LAPACK.  An axis the matrix does not couple to the others (exact zeros off its diagonal)
    is an eigenvector exactly and is split off by hand, as any rotation-based solver leaves it: the exact leaves are about exact zeros."""
    S = 0.5 * (C + C.T)
    free = [a for a in range(3) if not S[a, [b for b in range(3) if b != a]].any()]
    if len(free) == 3 or not free:
        if free:
            w, V = np.diag(S).copy(), np.eye(3)
        else:
            w, V = np.linalg.eigh(S)
    else:
        a = free[0]
        rest = [b for b in range(3) if b != a]
        w2, V2 = np.linalg.eigh(S[np.ix_(rest, rest)])
        w, V = np.append(w2, S[a, a]), np.zeros((3, 3))
        V[np.ix_(rest, [0, 1])] = V2
        V[a, 2] = 1.0
    k = np.argsort(w, kind="stable")
    return w[k], V[:, k]


def build_cells(xyz, leaf, divide=False):
    """float32 cells of the BUILD: floor(x * (1 / leaf)) (:86-95, 220-222); divide: floor(x / leaf), what the lookups use"""
    leaf = np.float32(leaf)
    xyz = np.asarray(xyz, np.float32)
    return np.floor(xyz / leaf) if divide else np.floor(xyz * (np.float32(1.0) / leaf))


def np_voxel_build(cloud, leaf, min_pts=6, eig_mult=0.01, variant=None):
    """The filter of voxel_grid_covariance_omp_impl.hpp:49-374 in numpy; the same fields as oracle.voxel_build, and cov_raw (the covariance before inflation), inflated.
    variant: one of the wrong rules the cases must notice."""
    xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    n = len(xyz)
    ok = np.isfinite(xyz).all(axis=1)
    ids = np.nonzero(ok)[0]
    out = dict(point_ids=np.zeros(max(n, 1), np.int32))
    if not len(ids):      # (the extents of an empty cloud are not defined by the reference: an empty grid)
        out.update(n_leaves=0, grid=np.array([0, 0, 0, -1, -1, -1, 0, 0, 0, 1, 0, 0], np.int32), offsets=np.zeros(1, np.int32))
        for k, w, t in (("leaf_key", 0, np.int32), ("leaf_n", 0, np.int32), ("mean", 3, float), ("cov", 9, float), ("cov_raw", 9, float), ("icov", 9, float),
                        ("evecs", 9, float), ("evals", 3, float), ("centroid", 3, np.float32), ("inflated", 0, bool)):
            out[k] = np.zeros((0, w) if w else 0, t)
        return out
    f = build_cells(xyz[ids], leaf, divide=variant == "divide_in_build")          # float32
    min_b, max_b = f.min(axis=0).astype(np.int64), f.max(axis=0).astype(np.int64)
    div = max_b - min_b + 1
    mul = np.array([1, div[0], div[0] * div[1]], np.int64)
    assert int(div[0]) * int(div[1]) * int(div[2]) <= 2 ** 31 - 1, "Leaf size is too small for the input dataset. Integer indices would overflow."
    ijk = (f - min_b.astype(np.float32)).astype(np.int64)                          # floor(x * inv) - float(min_b), in float (:220-222)
    key = ijk @ mul
    srt = np.argsort(key, kind="stable")
    if variant == "unstable_order":
        srt = np.lexsort((-np.arange(len(key)), key))
    keys, first = np.unique(key[srt], return_index=True)
    off = np.append(first, len(srt))
    nl = len(keys)
    order = ids[srt]
    out["point_ids"][:len(order)] = order
    pts = xyz[order]
    x = pts.astype(np.float64)
    terms = np.concatenate([x, x[:, [0, 0, 0, 1, 1, 2]] * x[:, [0, 1, 2, 1, 2, 2]]], axis=1)
    sums, cen = np.zeros((nl, 9)), np.zeros((nl, 3), np.float32)
    for l in range(nl):                                                            # strictly in input order: cumsum is sequential
        a, b = off[l], off[l + 1]
        if b - a == 1:
            sums[l], cen[l] = terms[a], pts[a]
        else:
            sums[l], cen[l] = np.cumsum(terms[a:b], axis=0)[-1], np.cumsum(pts[a:b], axis=0)[-1]
    cnt = np.diff(off)
    mean = sums[:, :3] / cnt[:, None]
    centroid = cen / cnt[:, None].astype(np.float32)
    sq = sums[:, [3, 4, 5, 4, 6, 7, 5, 7, 8]].reshape(nl, 3, 3)
    C = (sq - 2 * (sums[:, :3, None] * mean[:, None, :])) / cnt[:, None, None] + mean[:, :, None] * mean[:, None, :]      # :333
    if variant != "no_bessel":
        C = C * ((cnt - 1.0) / cnt)[:, None, None]                                                                            # :334
    eye = np.eye(3).reshape(9)
    leaf_n = cnt.astype(np.int32)
    cov, icov, evecs, evals = np.tile(eye, (nl, 1)), np.zeros((nl, 9)), np.tile(eye, (nl, 1)), np.zeros((nl, 3))
    cov_raw, inflated = np.tile(eye, (nl, 1)), np.zeros(nl, bool)
    live = cnt > min_pts if variant == "le_min_pts" else cnt >= min_pts
    for l in np.nonzero(live)[0]:
        ev, V = _eigh3(C[l])
        evecs[l], cov_raw[l] = V.reshape(9), C[l].reshape(9)
        if ev[0] < 0 or ev[1] < 0 or ev[2] <= 0:                                                                              # :343-347
            leaf_n[l], cov[l] = -1, C[l].reshape(9)
            continue
        Cl, m = C[l], eig_mult * ev[2]
        if ev[0] < m:                                                                                                         # :349-358
            ev = ev.copy()
            ev[0] = m
            if ev[1] < m and variant != "inflate_ev0_only":
                ev[1] = m
            Cl = (V * ev) @ V.T
            inflated[l] = True
        evals[l], cov[l] = ev, Cl.reshape(9)
        with np.errstate(all="ignore"):
            try:
                ic = np.linalg.inv(Cl)
            except np.linalg.LinAlgError:
                ic = np.full((3, 3), np.inf)
        icov[l] = ic.reshape(9)
        if np.isinf(ic).any():                                                                                                # :364-367
            leaf_n[l] = -1
    out.update(n_leaves=nl, grid=np.concatenate([min_b, max_b, div, mul]).astype(np.int32), leaf_key=keys.astype(np.int32), leaf_n=leaf_n, mean=mean, cov=cov,
               cov_raw=cov_raw, icov=icov, evecs=evecs, evals=evals, centroid=centroid, offsets=off.astype(np.int32), inflated=inflated)
    return out


def np_lookup(grid, leaf_key, leaf_n, queries, leaf, min_pts, rel, variant=None):
    """getNeighborhoodAtPoint (:378-408) for the displacement table rel [n_rel, 3]: ids [nq, n_rel], -1 = outside the grid, no leaf, fewer than min_pts points
    (a rejected leaf carries -1 points) or a query with a non-finite coordinate (include/lvx.h)."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)[:, :3]
    rel = np.asarray(rel, np.int64).reshape(-1, 3)
    grid = np.asarray(grid, np.int64)
    min_b, max_b, mul = grid[0:3], grid[3:6], grid[9:12]
    fin = np.isfinite(q).all(axis=1)
    with np.errstate(all="ignore"):
        f = build_cells(np.where(fin[:, None], q, 0), leaf, divide=variant != "multiply_in_lookup")
    ijk = f.astype(np.int64)[:, None, :]                                           # [nq, 1, 3]
    d = rel[None, :, :]
    if variant == "strict_range":
        ok = ((min_b - ijk < d) & (max_b - ijk > d)).all(axis=2)
    else:
        ok = ((min_b - ijk <= d) & (max_b - ijk >= d)).all(axis=2)                 # :386-387, 396
    ok &= fin[:, None]
    key = ((ijk + d - min_b) * mul).sum(axis=2)
    ids = np.full(ok.shape, -1, np.int32)
    if len(leaf_key):
        lk = np.asarray(leaf_key, np.int64)
        at = np.clip(np.searchsorted(lk, key), 0, len(lk) - 1)
        cnt = np.asarray(leaf_n)[at]
        hit = ok & (lk[at] == key) & ((cnt >= min_pts) | ((cnt == -1) if variant == "rejected_visible" else False))
        ids[hit] = at[hit]
    return ids


def exact_spectrum(points):
    """Ascending eigenvalues of the centred covariance sum (x - mu)(x - mu)^T / n of float points, accumulated in long double (no cancellation to speak of: the sums are
    of centred coordinates), and the covariance itself."""
    x = np.asarray(points, np.longdouble)
    c = x - x.mean(axis=0)
    C = np.asarray((c.T @ c) / len(x), np.float64)
    return np.linalg.eigvalsh(C), C


def _is_dyadic_small(points):
    """multiples of 2^-8 below 16 in at most 16 points, a power of two: 12-bit coordinates, 16-bit sums and means, 32-bit products — every step of :286-334 is exact"""
    x = np.asarray(points, np.float64)
    return len(x) in (2, 4, 8, 16) and np.abs(x).max() < 16 and np.array_equal(x * 256, np.round(x * 256))


def classify(cloud, ref, min_pts):
    """One letter per leaf of ref: P placeholder, D determined, E exact, U undetermined."""
    xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    off, cls = ref["offsets"], np.full(ref["n_leaves"], "P", "U1")
    for l in range(ref["n_leaves"]):
        n = off[l + 1] - off[l]
        if n < min_pts:
            continue
        p = xyz[ref["point_ids"][off[l]:off[l + 1]]]
        w, C = exact_spectrum(p)
        if n >= 4 and w[2] > 0 and w[0] / w[2] >= DETERMINED_RATIO:
            cls[l] = "D"
        elif _is_dyadic_small(p):
            nz = [a for a in range(3) if C[a].any()]
            wb = np.linalg.eigvalsh(C[np.ix_(nz, nz)]) if nz else np.ones(1)
            cls[l] = "E" if wb[0] / wb[-1] >= DETERMINED_RATIO else "U"
        else:
            cls[l] = "U"
    return cls


def _rel_err(a, b):
    """largest |a - b| per leaf relative to the leaf's largest |b| (0 where both are zero)"""
    a, b = np.asarray(a, float).reshape(len(a), -1), np.asarray(b, float).reshape(len(b), -1)
    if not len(a):
        return np.zeros(0)
    sc = np.abs(b).max(axis=1)
    d = np.abs(a - b).max(axis=1)
    return np.where(d == 0, 0.0, d / np.where(sc > 0, sc, 1.0))


def compare(got, ref, cls):
    """The largest difference per quantity over the determined and exact leaves: dict like ORACLE_VS_NUMPY."""
    de = (cls == "D") | (cls == "E")
    kept = de & (ref["leaf_n"] >= 0)
    out = dict(cov_plain=0.0, cov_inflated=0.0, evals=0.0, icov=0.0, evec=0.0)
    pl, inf = de & ~ref["inflated"], kept & ref["inflated"]
    if pl.any():
        out["cov_plain"] = float(_rel_err(got["cov"][pl], ref["cov"][pl]).max())
    if inf.any():
        out["cov_inflated"] = float(_rel_err(got["cov"][inf], ref["cov"][inf]).max())
    if kept.any():
        ev = ref["evals"][kept]
        out["evals"] = float((np.abs(got["evals"][kept] - ev).max(axis=1) / ev[:, 2]).max())
        out["icov"] = float(_rel_err(got["icov"][kept], ref["icov"][kept]).max())
        Vg, Vr = got["evecs"][kept].reshape(-1, 3, 3), ref["evecs"][kept].reshape(-1, 3, 3)
        Cr = ref["cov_raw"][kept].reshape(-1, 3, 3)
        raw = np.linalg.eigvalsh(0.5 * (Cr + Cr.transpose(0, 2, 1)))
        sep = np.diff(raw, axis=1).min(axis=1) > 1e-3 * raw[:, 2]                 # eigenvectors are comparable only for separated eigenvalues (of the raw covariance)
        if sep.any():
            out["evec"] = float((1 - np.abs(np.einsum("nij,nij->nj", Vg[sep], Vr[sep]))).max())
    return out


def check_build(got, ref, min_pts, eig_mult, cls, bars=BARS):
    """What a build's result has to be, against the restatement `ref` and the classes of its leaves; returns compare()'s figures (asserted against bars)."""
    assert got["n_leaves"] == ref["n_leaves"] and np.array_equal(got["grid"], ref["grid"]), (got["n_leaves"], ref["n_leaves"], got["grid"], ref["grid"])
    nl = ref["n_leaves"]
    assert np.array_equal(got["leaf_key"], ref["leaf_key"]) and np.array_equal(got["offsets"], ref["offsets"])
    m = ref["offsets"][-1]
    assert np.array_equal(got["point_ids"][:m], ref["point_ids"][:m])              # input order inside a leaf
    if not nl:
        return dict.fromkeys(BARS, 0.0)
    assert np.array_equal(np.asarray(got["centroid"]).view(np.uint32), ref["centroid"].view(np.uint32))
    assert np.allclose(got["mean"], ref["mean"], rtol=1e-12, atol=1e-12)
    cnt = np.diff(ref["offsets"])
    eye = np.eye(3).reshape(9)
    ph = cls == "P"
    assert np.array_equal(ph, cnt < min_pts)
    assert np.array_equal(got["leaf_n"][ph], cnt[ph])
    for k, want in (("cov", eye), ("evecs", eye), ("icov", 0 * eye), ("evals", np.zeros(3))):
        assert (got[k][ph] == want).all(), k
    de = (cls == "D") | (cls == "E")
    assert np.array_equal(got["leaf_n"][de], ref["leaf_n"][de])
    rej = de & (ref["leaf_n"] < 0)
    assert (got["evals"][rej] == 0).all() and (got["icov"][rej] == 0).all()
    fig = compare(got, ref, cls)
    for k, v in fig.items():
        assert v <= bars[k], (k, v, bars[k])
    for l in np.nonzero(cls == "U")[0]:                                            # either outcome, self-consistent
        raw = ref["cov_raw"][l]
        if got["leaf_n"][l] == -1:
            assert (got["evals"][l] == 0).all() and (got["icov"][l] == 0).all(), l
            assert _rel_err(got["cov"][l:l + 1], raw[None])[0] <= max(bars["cov_plain"], 1e-12), l
        else:
            assert got["leaf_n"][l] == cnt[l], l
            ev, Cg = got["evals"][l], got["cov"][l].reshape(3, 3)
            lam = np.linalg.eigvalsh(0.5 * (raw.reshape(3, 3) + raw.reshape(3, 3).T))
            mm = eig_mult * ev[2]
            assert abs(ev[2] - lam[2]) <= 1e-10 * lam[2], l
            assert abs(ev[0] - mm) <= 1e-14 * ev[2] and abs(ev[1] - max(lam[1], mm)) <= 1e-10 * ev[2], (l, ev, lam, mm)
            assert np.abs(np.linalg.eigvalsh(0.5 * (Cg + Cg.T)) - ev).max() <= 1e-10 * ev[2], l
            assert np.abs(got["icov"][l].reshape(3, 3) @ Cg - np.eye(3)).max() <= 1e-8, l
    return fig


# ------------------------------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------------------------------
BAD = np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [np.nan, np.nan, np.nan]], np.float32)


def _assemble(parts, n_bad, rng, head=None):
    """[N, 4] float32: the parts' points under a seeded permutation with n_bad non-finite points sprinkled in; `head` (points) stays in front, in its order."""
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in parts] + [BAD[np.arange(n_bad) % len(BAD)]])
    pts = pts[rng.permutation(len(pts))]
    if head is not None:
        pts = np.concatenate([np.asarray(head, np.float32).reshape(-1, 3), pts])
    cloud = np.zeros((len(pts), 4), np.float32)
    cloud[:, :3] = pts
    cloud[:, 3] = rng.uniform(0, 100, len(pts)).astype(np.float32)
    return cloud


def cell_points(cells, sizes, leaf, rng):
    """sizes[k] points uniform in the interior of cells[k] (0.1 leaf from every face: the cell of a point does not depend on rounding)"""
    cells = np.repeat(np.asarray(cells, np.float64).reshape(-1, 3), sizes, axis=0)
    return ((cells + rng.uniform(0.1, 0.9, cells.shape)) * leaf).astype(np.float32)


def profile_sizes(T):
    """Leaf sizes laid along consecutive keys from sorted position 0, for a leaf kernel tile of T = 256 PT positions (stage = 256, finalize chunk = 128 leaves)."""
    s = [255, 1, 1, 256, 257, 512, 513, 125]      # heads at 0, 255, 256, 257, 513, 770, 1282, 1795: leaves of exactly 256, 257, 512 and 513 points
    s += [2300]                                   # 1920 .. 4220: begins mid-tile for T = 256, 512 and 1024; the tiles it covers have no head
    s += [900]                                    # .. 5120, a boundary of every tile width
    for h in (127, 128, 129):                     # a tile with exactly h heads: either side of the 128-leaf finalize chunk
        s += [1] * (h - 1) + [T - (h - 1)]
    s += [T - 1, 1, 1, 300]                       # heads at T - 1, T and T + 1
    s += [1] * 512 + [700]                        # 256 k single-point leaves, then a long one
    return s


PROFILE_TAIL = [300, 1, 1, 257, 600]


def raster(first_key, count, W, z):
    k = first_key + np.arange(count)
    return np.stack([k % W, k // W, np.full(count, z)], axis=1)


def _profile_case(T, n_bad, seed):
    rng = np.random.default_rng(seed)
    sizes = profile_sizes(T)
    cloud = _assemble([cell_points(raster(0, len(sizes), len(sizes), 0), sizes, 0.5, rng)], n_bad, rng)
    return dict(cloud=cloud, leaf=0.5, heads=np.cumsum([0] + sizes), T=T)


def _filler(n, seed):
    import synth
    tiles = max(1, -(-n // 100_000))
    c = synth.tile_voxel_cloud(synth.make_voxel_cloud(seed=seed, n=100_000), tiles)[:n, :3].astype(np.float64)
    return c


def _sized_case(n, n_bad, seed, leaf=2.0):
    """n points in all: the profile for this size's tile at the lowest keys, a tiled generic cloud, a short profile at the highest keys; n_bad non-finite points."""
    rng = np.random.default_rng(seed)
    T = leaf_tile(n)
    lo, hi = profile_sizes(T), PROFILE_TAIL
    fill = _filler(n - sum(lo) - sum(hi) - n_bad, seed)
    fill = fill - np.floor(fill.min(axis=0)) + np.array([0.0, 0.0, 2 * leaf]) + 0.25            # lowest cell (0, 0, 2)
    fill = fill.astype(np.float32)
    cf = build_cells(fill, leaf)
    W, D, top = int(cf[:, 0].max()) + 1, int(cf[:, 1].max()) + 1, int(cf[:, 2].max())
    assert len(lo) < W * D and len(hi) < W * D
    parts = [cell_points(raster(0, len(lo), W, 0), lo, leaf, rng), fill, cell_points(raster(W * D - len(hi), len(hi), W, top + 2), hi, leaf, rng)]
    return dict(cloud=_assemble(parts, n_bad, rng), leaf=leaf, heads=np.cumsum([0] + lo), T=T, tail=np.cumsum(hi[::-1])[::-1])


def _small_case(n, seed):
    """n points in all, two of them non-finite where n > 2, in 3 x 3 x 2 cells about the origin"""
    rng = np.random.default_rng(seed)
    n_bad = 2 if n > 2 else 0
    pts = rng.uniform([-1.4, -1.4, -0.9], [1.4, 1.4, 0.9], (n - n_bad, 3))
    return dict(cloud=_assemble([pts], n_bad, rng), leaf=1.0)


def _sort_case(dims, seed):
    """A grid of dims cells placed by its two corner points.  In front, in input order, 1 100 points whose keys share their low 10 bits (one bin of every digit width
    takes the whole first sort tile); 3 000 points of one cell spread over the rest of the input (three sort tiles: the point list keeps input order); clusters;
    the largest valid key (the far corner) sorts next to the invalid keys of the non-finite points."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    o = np.array([-7, -3, -2], np.int64)        # (cell 0 inside the grid: where a NaN query would land on the device without the guard)
    cells = int(dims.prod())
    step = 1024
    nk = min(1100, (cells - 5) // step)
    keys = 5 + step * (rng.permutation(1100) % nk)
    same = np.stack([keys % dims[0], (keys // dims[0]) % dims[1], keys // (dims[0] * dims[1])], axis=1)
    head = cell_points(same + o, np.ones(len(same), int), 1.0, rng)
    corners = np.array([[0, 0, 0], dims - 1]) + o
    mid = (dims // 2) + o
    near = rng.integers(0, np.minimum(dims, 12), (40, 3)) + o
    parts = [cell_points(corners, [1, 7], 1.0, rng), cell_points([mid], [3000], 1.0, rng), cell_points(near, rng.integers(1, 30, 40), 1.0, rng)]
    return dict(cloud=_assemble(parts, 9, rng, head=head), leaf=1.0, dims=tuple(int(d) for d in dims), long_cell=tuple(int(c) for c in mid))


def _blob(cell, n, rng):
    return (np.asarray(cell, np.float64) + rng.uniform(0.15, 0.85, (n, 3)))


def _leaves_case(seed, degenerate):
    """Leaves of 1 .. 13 generic points in a row of 1.0 m cells; a thin plate (1 mm) 100 m from the origin.  degenerate: and the exact leaves (8 coincident points:
    rejected; an 8-point rod along x and a 16-point plate z = const: inflated, exact zeros), and the placed undetermined ones (three points; 12 points of a tilted
    plane, exactly coplanar)."""
    rng = np.random.default_rng(seed)
    parts = [_blob((k - 1, 0, 0), k, rng) for k in range(1, 14)]
    n, u, v = SC._basis((0.2, -0.3, 0.93))
    ab = rng.uniform(-0.3, 0.3, (40, 2))
    parts.append(np.array([100.5, 0.5, 0.5]) + ab[:, :1] * u + ab[:, 1:] * v + rng.uniform(-1e-3, 1e-3, (40, 1)) * n)
    if degenerate:
        parts.append(np.tile([0.5, 2.25, 0.5], (8, 1)))
        parts.append(np.stack([2 + np.arange(1, 9) / 16.0, np.full(8, 2.5), np.full(8, 0.5)], axis=1))
        parts.append(SC.axis_patch((4, 2, 0), 16, axis=2, seed=seed).points())
        g = np.array([[i, j] for i in range(4) for j in range(3)]) / 8.0
        parts.append(np.stack([6.25 + g[:, 0], 2.25 + g[:, 1], 0.25 + g[:, 0] / 2 + g[:, 1] / 4], axis=1))
    return dict(cloud=_assemble(parts, 3, rng), leaf=1.0)


def face_floats(leaf, k_range=399):
    """the float product k * leaf for k in -k_range .. k_range, and the floats next to it: 3 (2 k_range + 1) values at and next to cell faces"""
    f = np.arange(-k_range, k_range + 1).astype(np.float32) * np.float32(leaf)
    return np.concatenate([np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))])


def _edges_case(leaf, seed, thin=False):
    """A row of 801 cells along x (iy = iz = 0), every one a determined 6-point leaf, sparse neighbour rows about it (thin: none, a one-cell-thick grid in y and z);
    the face floats (faces -399 .. 399) as points (x on a face, y and z mid-cell) and as queries; -0.0 and +0.0; queries one cell outside each face of the grid."""
    rng = np.random.default_rng(seed)
    ix = np.arange(-400, 401)
    row = np.stack([ix, 0 * ix, 0 * ix], axis=1)
    parts = [cell_points(row, np.full(len(row), 6), leaf, rng)]
    if not thin:
        for dy, dz in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1)):
            r = row[::10] + np.array([0, dy, dz])
            parts.append(cell_points(r, np.full(len(r), 6), leaf, rng))
    fx = np.concatenate([face_floats(leaf), np.array([-0.0, 0.0], np.float32)])
    face = np.stack([fx, np.full(len(fx), 0.5 * leaf, np.float32), np.full(len(fx), 0.5 * leaf, np.float32)], axis=1)
    parts.append(face)
    cloud = _assemble(parts, 4, rng)
    cx = build_cells(cloud[np.isfinite(cloud[:, 0]), 0], leaf)                      # (-400 .. 400: the faces stop one cell short of the row's ends, whose leaves stay full)
    lo, hi = (float(cx.min()) - 0.5) * leaf, (float(cx.max()) + 1.5) * leaf
    m = 0.5 * leaf
    t = 0.0 if thin else leaf
    outside = np.array([[lo, m, m], [hi, m, m], [m, -t - leaf + m, m], [m, t + leaf + m, m], [m, m, -t - leaf + m], [m, m, t + leaf + m],
                        [lo, -t - leaf + m, m], [hi, m, t + leaf + m]], np.float32)
    q = np.zeros((len(face) + len(outside), 4), np.float32)
    q[:, :3] = np.concatenate([face, outside])
    return dict(cloud=cloud, leaf=leaf, queries=q, face=face)


NONFINITE_QUERIES = np.array([[np.nan, 0.04, 0.04, 0], [0.04, np.nan, 0.04, 0], [0.04, 0.04, np.nan, 0], [np.inf, 0.04, 0.04, 0], [0.04, -np.inf, 0.04, 0], [0.04, 0.04, np.inf, 0],
                              [-np.inf, 0.04, 0.04, 0], [np.nan, np.nan, np.nan, 0], [np.inf, np.nan, -np.inf, 0]], np.float32)


class Case:
    """make() -> dict(cloud, leaf, ...), made on first use.  undetermined: how many leaves of >= min_pts points are undetermined (named by the case)."""

    def __init__(self, name, group, make, min_pts=6, eig_mult=0.01, undetermined=0, big=False, **expect):
        self.name, self.group, self._make, self.min_pts, self.eig_mult, self.undetermined, self.big, self.expect = name, group, make, min_pts, eig_mult, undetermined, big, expect

    @property
    def data(self):
        return _data(self.name)

    @property
    def cloud(self):
        return self.data["cloud"]

    @property
    def leaf(self):
        return self.data["leaf"]

    @property
    def queries(self):
        """the case's own queries, a sample of its points moved by a third of a cell, and the non-finite ones (the other two coordinates inside the grid about cell 0)"""
        d = self.data
        c = d["cloud"]
        rng = np.random.default_rng(len(c))
        samp = c[rng.permutation(len(c))[:300]].copy()
        samp = samp[np.isfinite(samp).all(axis=1)]
        moved = samp.copy()
        moved[:, :3] += np.float32(0.37 * d["leaf"])
        return np.concatenate([d.get("queries", samp[:0]), samp, moved, NONFINITE_QUERIES])

    def __repr__(self):
        return "Case(%s)" % self.name


CASES = []
# sort: one case per instance, each on a fresh context
for _dims, _inst in (((32, 32, 32), (18, 9, 2)), ((64, 64, 64), (19, 10, 2)), ((128, 128, 100), (21, 8, 3)), ((300, 300, 250), (25, 9, 3)), ((480, 480, 470), (28, 10, 3))):
    CASES.append(Case("sort_%dx%d" % (_inst[1], _inst[2]), "sort", functools.partial(_sort_case, _dims, 11 + _inst[0]), instance=_inst))
# sizes
for _n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
    CASES.append(Case("n_%d" % _n, "sizes", functools.partial(_small_case, _n, _n)))
for _n in (262144, 262145, 524288, 524289, 1048576, 1048577):
    CASES.append(Case("n_%d" % _n, "sizes", functools.partial(_sized_case, _n, 37 * (_n % 2), 3 + _n % 7), big=True))
# tiles (PT = 1; the PT = 2 and PT = 4 profiles are the prefixes of the big clouds above)
CASES.append(Case("tiles_end_at_n", "tiles", functools.partial(_profile_case, 256, 0, 5)))
CASES.append(Case("tiles_nonfinite_run", "tiles", functools.partial(_profile_case, 256, 40, 6)))
# leaves: both sides of min_pts 3, 6 and 12; eig_mult 0.01, 0.1 and (on full-rank leaves only) 0
for _mp in (3, 6, 12):
    for _em in (0.01, 0.1):
        CASES.append(Case("leaves_min%d_mult%g" % (_mp, _em), "leaves", functools.partial(_leaves_case, 21, True), min_pts=_mp, eig_mult=_em, undetermined=2 if _mp == 3 else 1))
    # (eig_mult = 0 inflates nothing: a three-point leaf that rounding keeps has an inverse of 1e17 that means nothing — the cut there is 4, below the first full-rank count)
    CASES.append(Case("leaves_min%d_mult0" % max(_mp, 4), "leaves", functools.partial(_leaves_case, 22, False), min_pts=max(_mp, 4), eig_mult=0.0))
# edges
for _leaf in (0.3, 0.1, 0.7):
    CASES.append(Case("edges_%g" % _leaf, "edges", functools.partial(_edges_case, _leaf, int(_leaf * 100))))
CASES.append(Case("edges_thin_0.3", "edges", functools.partial(_edges_case, 0.3, 77, True)))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
REL_TABLES = {"rel1": (REL1, 257), "rel7": (DIRECT7, 37), "rel26": (REL26, 10), "rel27": (REL27, 10)}     # (table, queries): nq n_rel just above one workgroup of 256


@functools.lru_cache(maxsize=None)
def _data(name):
    d = BY_NAME[name]._make()
    d["cloud"].setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def np_result(name):
    c = BY_NAME[name]
    return np_voxel_build(c.cloud, c.leaf, c.min_pts, c.eig_mult)


@functools.lru_cache(maxsize=None)
def classes(name):
    c = BY_NAME[name]
    return classify(c.cloud, np_result(name), c.min_pts)


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    from oracle import oracle as O
    c = BY_NAME[name]
    return O.voxel_build(c.cloud, c.leaf, c.min_pts, c.eig_mult)


def check_lookups(case, res, lookup1, lookup7, lookup_rel):
    """The three lookups (callables on queries / queries, rel) against np_lookup on the leaves of `res` — a rejected leaf (-1 points) is absent."""
    q = case.queries
    args = (res["grid"], res["leaf_key"], res["leaf_n"])
    want7 = np_lookup(*args, q, case.leaf, case.min_pts, DIRECT7)
    assert np.array_equal(np.asarray(lookup7(q)).reshape(-1, 7), want7)
    assert np.array_equal(np.asarray(lookup1(q)).reshape(-1), want7[:, 0])
    assert (want7[-len(NONFINITE_QUERIES):] == -1).all()
    for tag, (rel, nq) in REL_TABLES.items():
        qq = q[:: max(1, len(q) // nq)][:nq]
        assert np.array_equal(lookup_rel(qq, rel), np_lookup(*args, qq, case.leaf, case.min_pts, rel)), tag
    assert np.array_equal(lookup_rel(q, REL27), np_lookup(*args, q, case.leaf, case.min_pts, REL27))
    return want7
