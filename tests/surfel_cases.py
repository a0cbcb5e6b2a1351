"""Surfel map extraction (lvx_surfel_extract: k_surfel_extract, then k_surfel_compact_mb or k_surfel_compact): a case table that chooses every leaf directly, a
numpy restatement of setSurfelMap + checkPlaneType (surfel_association.cpp:50-86,246-266) with the deterministic plane fit that oracle/orc_upstream.cpp documents
as its deviation, and check_result — the properties a result has to have whoever computed it.  Nothing here rests on the oracle or on the kernels.
tests/test_surfel_cases.py holds every case to the regime it claims on the CPU; tests/test_gpu_surfel_shapes.py runs the same cases through the C ABI.

The cloud: a lattice of 1.0 m cells.  A leaf is a cell and the points put into it — a planar patch of n points about the cell's centre with a chosen normal, in-plane
extent, noise and outliers — in the ORDER the leaf's point list will have (the cloud is the leaves shuffled into one another, every leaf keeping its own order, plus a
few NaN / inf points).  Every point stays MARGIN inside its cell, so the cell of a point does not depend on rounding; the exceptions are coordinates that are exact
dyadic numbers (a plane z = 0, x = 0.5 ...), whose cell is exact as well.

Definitions held here (include/lvx.h): a leaf below min_points_per_voxel has no eigen data and is never a surfel; min_leaf_points <= 0 means 1."""
import functools
from collections import namedtuple

import numpy as np

LEAF = 1.0
MARGIN = 0.05
EX_TRIP = 512            # points a wavefront of k_surfel_extract walks per trip (64 lanes x EX_U = 8)
SC_LEAVES = 1024         # leaves per workgroup of k_surfel_compact_mb / per trip of k_surfel_compact
SC_SECOND_TRIP = 262144  # leaves above which the count loop of k_surfel_compact_mb (256 threads over the workgroups) takes a second trip
PTYPE_OF_AXIS = {0: 2, 1: 2, 2: 1}   # (d) plane_type of a normal exactly along x / y / z: the two zero components tie and the reference's descending sort (stable
#                                      on three elements) leaves the LAST of them at the end

Params = namedtuple("Params", "p_lambda thr min_leaf min_inl min_pts eig_mult")
Params.__new__.__defaults__ = (0.7, 0.05, 10, 20, 6, 0.01)
DEFAULT = Params()

GENERIC = (0.31, -0.52, 0.79)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _basis(n):
    n = _unit(n)
    a = np.eye(3)[np.argmin(np.abs(n))]
    u = _unit(np.cross(n, a))
    return n, u, np.cross(n, u)


def _iso(ab, extent):
    """In-plane places with EXACTLY equal sample variances and no correlation, inside [-extent, extent]^2: the planarity 2 (l_mid - l_min) / sum punishes an uneven
    patch (a quarter of all random 24-point patches fall below 0.7), and whether a leaf is accepted is this table's choice, not the sample's."""
    if len(ab) < 3:
        return ab
    ab = ab - ab.mean(axis=0)
    w, V = np.linalg.eigh(ab.T @ ab / len(ab))
    ab = ab @ V / np.sqrt(w)
    return ab * (extent / np.abs(ab).max())


def _grid(n, rng):
    """n distinct places of a centred m x m lattice with a dyadic step (m = ceil(sqrt(n))), shuffled: dyadic numbers in [0.18, 0.82]."""
    m = int(np.ceil(np.sqrt(n)))
    step = 2.0 ** -(int(np.floor(np.log2(max(m, 2)))) + 1)
    g = 0.5 + (np.arange(m) - (m - 1) / 2.0) * step
    q = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    return q[rng.permutation(len(q))[:n]]


class Leaf:
    """One cell's points.  local: [n, 3] offsets from the cell's lower corner, in point-list order.  exempt: the normal is not determined (Jacobi cases);
    exact: distances to the plane are computed without rounding (dyadic coordinates), so a point may sit exactly on dist_threshold; axis: normal exactly along it."""

    def __init__(self, cell, local, tag="", exact=False, axis=None):
        self.cell, self.local, self.tag, self.exact, self.axis = tuple(int(c) for c in cell), np.asarray(local, np.float64).reshape(-1, 3), tag, exact, axis
        self.n = len(self.local)
        assert exact or self.n == 0 or (self.local.min() >= MARGIN and self.local.max() <= 1.0 - MARGIN), (cell, tag, self.local.min(), self.local.max())

    def points(self):
        return (np.asarray(self.cell, np.float64) * LEAF + self.local).astype(np.float32)


def patch(cell, n, normal=GENERIC, extent=0.3, sigma=0.004, n_out=0, out_off=0.12, out_side="sym", where="spread", seed=0, tag="", thick=None):
    """A planar patch of n points about the centre of `cell`: in-plane uniform in [-extent, extent]^2, Gaussian noise sigma along the normal (thick: uniform in
    [-thick, thick] instead).  n_out of the points are outliers at out_off along the normal ('pos': all on one side, 'sym': alternating sides), drawn from the inner
    half of the patch; where: their places in the leaf's point list — 'first' (from position 0: the first lanes of the first trip hold them all), 'last' (the end:
    only the last, partial trip), 'spread' (every n // n_out-th)."""
    rng = np.random.default_rng([seed, n, n_out, abs(hash(tuple(cell))) % 100003])
    nn, u, v = _basis(normal)
    ab = rng.uniform(-extent, extent, (n, 2))
    off = rng.uniform(-thick, thick, n) if thick is not None else np.clip(sigma * rng.standard_normal(n), -3 * sigma, 3 * sigma)
    if n_out:
        at = {"first": np.arange(n_out), "last": np.arange(n - n_out, n), "spread": (np.arange(n_out) * (n // n_out))}[where]
    ab = _iso(ab, extent)
    if n_out:
        ab[at] *= 0.5 * extent / max(np.abs(ab[at]).max(), 0.5 * extent)      # (outliers in the inner half: they stay inside the cell)
        sgn = np.ones(n_out) if out_side == "pos" else np.where(np.arange(n_out) % 2 == 0, 1.0, -1.0)
        off[at] = sgn * out_off + np.clip(sigma * rng.standard_normal(n_out), -3 * sigma, 3 * sigma)
    return Leaf(cell, 0.5 + ab[:, :1] * u + ab[:, 1:] * v + off[:, None] * nn, tag or "n%d_o%d%s" % (n, n_out, where if n_out else ""))


def axis_patch(cell, n, axis, const=0.5, n_pairs=0, off=0.125, seed=0, tag=""):
    """n points with coordinate `axis` EXACTLY const (a dyadic number), the other two on a dyadic lattice: every sum of the covariance is exact, its row
    `axis` is exactly zero and the normal is exactly the axis.  n_pairs pairs of extra points at const +- off over the same in-plane place keep the mean on the plane and
    the row's off-diagonal entries zero: with dist_threshold = off they sit EXACTLY on the threshold."""
    rng = np.random.default_rng([seed, n, axis, n_pairs])
    q = _grid(n + n_pairs, rng)
    others = [a for a in range(3) if a != axis]
    loc = np.zeros((n + 2 * n_pairs, 3))
    loc[:n, others] = q[:n]; loc[:n, axis] = const
    for s, sl in ((1.0, slice(n, n + n_pairs)), (-1.0, slice(n + n_pairs, n + 2 * n_pairs))):
        loc[sl, others] = q[n:]; loc[sl, axis] = const + s * off
    return Leaf(cell, loc, tag or "axis%d_n%d" % (axis, n), exact=True, axis=axis)


def sheets(cell, n_side, k_mid, normal=GENERIC, gap=0.03, extent=0.28, seed=0, tag="", mid_line=False):
    """Two sheets of n_side points each at +-gap from the patch plane over the SAME in-plane places (the mean stays on the plane and the plane is not tilted), then
    k_mid points on it (mid_line: on one straight line in it): under a dist_threshold below gap the inliers are the k_mid points alone."""
    rng = np.random.default_rng([seed, n_side, k_mid])
    nn, u, v = _basis(normal)
    ab = _iso(rng.uniform(-extent, extent, (n_side, 2)), extent)
    ab = np.concatenate([ab, ab])
    off = np.concatenate([np.full(n_side, gap), np.full(n_side, -gap)])
    if mid_line:
        mid = rng.uniform(-extent, extent, (k_mid, 2))
        mid[:, 1] = 0.4 * mid[:, 0]
    else:                                                # on a circle: three of them are no line
        ang = 0.3 + 2 * np.pi * np.arange(k_mid) / max(k_mid, 1)
        mid = 0.2 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    ab, off = np.concatenate([ab, mid]), np.concatenate([off, np.zeros(k_mid)])
    return Leaf(cell, 0.5 + ab[:, :1] * u + ab[:, 1:] * v + off[:, None] * nn, tag or "sheets%d_mid%d" % (n_side, k_mid))


def rod(cell, n, side=2.0 ** -7, seed=0, tag="rod"):
    """A rod along x with a square cross-section, all coordinates dyadic: n // 4 stations, at each the four corners (0.5 +- side, 0.5 +- side); and, 1 / 16 above and
    below it, two sheets of 16 points over a 4 x 4 lattice, which make the leaf planar with the normal exactly along z.  Under a dist_threshold between side and 1 / 16
    the inliers are the rod alone: their covariance is exactly diagonal with two EQUAL smallest entries — the normal of the fit is not determined."""
    rng = np.random.default_rng([seed, n])
    xs = rng.integers(32, 225, n // 4) / 256.0
    loc = [np.stack([xs, np.full(len(xs), 0.5 + su * side), np.full(len(xs), 0.5 + sv * side)], axis=1) for su in (-1, 1) for sv in (-1, 1)]
    g = 0.5 + (np.arange(4) - 1.5) * 0.125
    q = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    loc += [np.concatenate([q, np.full((16, 1), 0.5 + s / 16.0)], axis=1) for s in (-1, 1)]
    return Leaf(cell, np.concatenate(loc), tag, exact=True)


def sym_blob(cell, s, a, b, normal=GENERIC, m=5, seed=0, tag="blob"):
    """8 m points (+-A_i, +-B_i, +-s O_i) about the centre in the basis (u, v, normal), every combination of signs: all cross-covariances vanish and the eigenvalues
    are the three variances.  A in [0.3 a, a]; B the same numbers in another order where b == a (equal in-plane variances), else in [0.3 b, b]; O = B in another
    order: the planarity 2 (var B - s^2 var O) / sum falls as s grows and is zero at s = 1."""
    rng = np.random.default_rng([seed, m])
    A = rng.uniform(0.3 * a, a, m)
    B = np.roll(A, 2) if a == b else rng.uniform(0.3 * b, b, m)
    O = np.roll(B, 1)
    nn, u, v = _basis(normal)
    sg = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64)
    loc = np.concatenate([sg * np.array([A[i], B[i], s * O[i]]) for i in range(m)])
    return Leaf(cell, 0.5 + loc[:, :1] * u + loc[:, 1:2] * v + loc[:, 2:] * nn, tag)


def single(cell, seed=0):
    rng = np.random.default_rng([seed, abs(hash(tuple(cell))) % 100003])
    return Leaf(cell, rng.uniform(0.1, 0.9, (1, 3)), "single")


class Case:
    """build() -> leaves, or (leaves, singles): a list of Leaf and [m, 3] further cells that get one point each (vectorised: the 266 k-leaf cloud), made on first
    use — importing the table builds nothing; params: the extraction's parameters."""

    def __init__(self, name, build, params=DEFAULT, seed=0, group=None, big=False):
        self.name, self._build, self.params, self.seed, self.group, self.big = name, build, params, seed, group or name, big
        self._made = None

    def _make(self):
        if self._made is None:
            made = self._build()
            leaves, singles = made if isinstance(made, tuple) else (made, None)
            singles = np.zeros((0, 3), np.int64) if singles is None or not len(singles) else np.asarray(singles, np.int64).reshape(-1, 3)
            cells = [l.cell for l in leaves]
            assert len(set(cells)) == len(cells), self.name
            self._made = (list(leaves), singles)
        return self._made

    @property
    def leaves(self):
        return self._make()[0]

    @property
    def singles(self):
        return self._make()[1]

    @property
    def cloud(self):
        return _cloud(self.name)

    def __repr__(self):
        return "Case(%s)" % self.name


N_BAD = 6


def build_cloud(case):
    """[N, 4] float32: the leaves' points shuffled into one another — a leaf's points keep their order — and N_BAD points with a NaN or an inf coordinate."""
    rng = np.random.default_rng(7919 * (1 + case.seed) + sum(map(ord, case.name)))
    pts = [l.points() for l in case.leaves]
    owner = [np.full(l.n, i) for i, l in enumerate(case.leaves)]
    if len(case.singles):
        pts.append((case.singles + rng.uniform(0.1, 0.9, (len(case.singles), 3))).astype(np.float32))
        owner.append(len(case.leaves) + np.arange(len(case.singles)))
    pts = np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)
    owner = np.concatenate(owner) if owner else np.zeros(0, np.int64)
    M, N = len(pts), len(pts) + N_BAD
    slots = rng.permutation(N)
    mine = slots[:M]
    mine = mine[np.lexsort((mine, owner))]          # per owner, ascending: points were concatenated owner by owner in list order
    cloud = np.zeros((N, 4), np.float32)
    cloud[:, 3] = rng.uniform(0, 100, N).astype(np.float32)
    cloud[mine, :3] = pts
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [np.nan, np.nan, np.nan]], np.float32)
    cloud[slots[M:], :3] = bad
    return cloud


@functools.lru_cache(maxsize=None)
def _cloud(name):
    c = build_cloud(BY_NAME[name])
    c.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ------------------------------------------------------------------------------------------------------------------------
def cells_of(cloud, leaf=LEAF):
    """The reference's own float cell assignment (voxel_grid_covariance_omp_impl.hpp:211-267): floorf(x * (1 / leaf)) in float, key = (ijk - min_b) . divb_mul, the
    leaves in ascending key order, every leaf's points in input order.  Returns (order, offsets, keys): cloud[order[offsets[l]:offsets[l + 1]]] are the points of leaf l."""
    xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    ok = np.isfinite(xyz).all(axis=1)
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(xyz[ok] * inv).astype(np.int64)
    if not len(ijk):
        return np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    min_b, max_b = ijk.min(axis=0), ijk.max(axis=0)
    div = max_b - min_b + 1
    key = (ijk - min_b) @ np.array([1, div[0], div[0] * div[1]])
    srt = np.argsort(key, kind="stable")
    keys, first = np.unique(key[srt], return_index=True)
    return np.nonzero(ok)[0][srt], np.append(first, len(srt)), keys


def _smallest_vec(C):
    """(ascending eigenvalues, eigenvector of the smallest) by eigh.  An axis that the covariance does not couple to the other two (exact zeros off its diagonal) is an
    eigenvector EXACTLY and is split off by hand: LAPACK leaves 1e-17 in the zero components, and the tie rule of plane_type (d) and the points that sit exactly on
    dist_threshold are about exact zeros."""
    for a in range(3):
        rest = [b for b in range(3) if b != a]
        if not C[a, rest].any():
            w2, V2 = np.linalg.eigh(C[np.ix_(rest, rest)])
            w, V = np.append(w2, C[a, a]), np.zeros((3, 3))
            V[np.ix_(rest, [0, 1])] = V2
            V[a, 2] = 1.0
            if not C[rest[0], rest[1]]:
                V[np.ix_(rest, [0, 1])] = np.eye(2)
                w[:2] = C[rest[0], rest[0]], C[rest[1], rest[1]]
            k = np.argsort(w, kind="stable")
            return np.maximum(w[k], 0.0), V[:, k[0]].copy()
    w, V = np.linalg.eigh(C)
    return np.maximum(w, 0.0), V[:, 0].copy()            # (a centred covariance is positive semi-definite: a negative eigenvalue is rounding)


def _centred_cov(x):
    mu = x.mean(axis=0)
    d = x - mu
    return mu, d.T @ d / len(x)


def plane_type_of(n):
    """checkPlaneType (:262-265): index of the smallest |n| component, the LAST one of a tie (descending stable sort of three)."""
    a = np.abs(n)
    return int(max(i for i in range(3) if a[i] == a.min()))


def rq_accepts(C, n0):
    """Restatement of the kernel's acceptance of its Rayleigh-quotient refit — used ONLY to choose inputs and to name the regime a leaf is predicted to take:
    four rounds of nv <- adj(C - lam I) nv from the leaf normal, then |nv|^2 within 1e-12 of 1 and lam below the smaller of the other two roots by 1e-9 |tr C|."""
    nv, lam = np.asarray(n0, np.float64).copy(), 0.0
    for _ in range(4):
        lam = nv @ C @ nv
        R = C - lam * np.eye(3)
        y = np.array([np.cross(R[1], R[2]), np.cross(R[2], R[0]), np.cross(R[0], R[1])]).T @ nv
        yy = y @ y
        if not yy > 1e-290:
            break
        nv = y / np.sqrt(yy) * (-1.0 if y @ nv < 0 else 1.0)
    tr = np.trace(C)
    s2 = tr - lam
    mn = (C[0, 0] * C[1, 1] - C[0, 1] ** 2) + (C[0, 0] * C[2, 2] - C[0, 2] ** 2) + (C[1, 1] * C[2, 2] - C[1, 2] ** 2)
    disc = s2 * s2 - 4.0 * (mn - lam * s2)
    small_other = 0.5 * (s2 - np.sqrt(max(disc, 0.0)))
    return bool(abs(nv @ nv - 1.0) < 1e-12 and lam < small_other - 1e-9 * abs(tr))


WRONG_RULES = ("le_threshold", "planarity_two_largest", "n_gt_min_leaf", "count_first_selection", "box_of_inliers", "no_sign_flip", "refit_skipped", "type_ascending",
               "rejected_leaf_fitted")


def np_surfel_extract(cloud, params=DEFAULT, leaf=LEAF, wrong=None):
    """setSurfelMap over the NDT leaves of `cloud`, float64 throughout: leaf mean and centred two-pass covariance (scaled (n - 1) / n as :333-334 leave it), eigh,
    the eigenvalue inflation (:349-357), planarity 2 (l_mid - l_min) / sum >= p_lambda, then the deterministic fit: points closer than thr to the leaf's PCA plane,
    PCA of those (centred, eigh) if there are three, reselect, at least min_inl; d <= 0 (lexicographic at d == 0); box = float min / max of ALL the leaf's points.
    wrong: one of WRONG_RULES — the same with one rule broken (tests/test_surfel_cases.py: every one must be noticed).
    Returns the oracle's dict plus, per accepted leaf, what the conditions on the inputs need: margin (distance of the nearest point to thr, over both planes),
    gap ((c): two smallest eigenvalues of the fitted covariance, relative to the largest), type_gap ((d)), branch ('none' / 'rq' / 'jacobi' predicted), nin0, d_raw;
    offered = [(leaf, planarity)] of every leaf with enough points ((b)); fitted = [(leaf, margin, first inlier count, final inlier count, margin against the first plane alone, gap)] of every
    leaf that reached the fit ((a), also those that min_inl then rejects); counts = points of every leaf."""
    order, offs, keys = cells_of(cloud, leaf)
    xyz32 = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    cnt = np.diff(offs)
    min_leaf = max(params.min_leaf, 1)
    out = {k: [] for k in ("p4", "Pi", "box_min", "box_max", "leaf", "n_points", "n_inliers", "plane_type", "margin", "gap", "type_gap", "branch", "nin0", "d_raw")}
    offered, fitted = [], []
    inside = (lambda dist: dist <= params.thr) if wrong == "le_threshold" else (lambda dist: dist < params.thr)
    enough = (cnt > min_leaf) if wrong == "n_gt_min_leaf" else (cnt >= min_leaf)
    for li in np.nonzero(enough & (cnt >= params.min_pts))[0]:
        p32 = xyz32[order[offs[li]:offs[li + 1]]]
        x = p32.astype(np.float64)
        n = len(x)
        mean, C = _centred_cov(x)
        w, nrm = _smallest_vec(C * ((n - 1.0) / n))
        if w[2] <= 0:                                           # nr_points = -1 (:341-345): never fitted
            if wrong != "rejected_leaf_fitted":
                continue
            nrm = np.array([0.0, 0.0, 1.0])                     # (the wrong rule: the build's placeholder eigen data taken at their word, 0 / 0 passing as planar)
        else:
            m = params.eig_mult * w[2]
            if w[0] < m:
                w[0] = m
                w[1] = max(w[1], m)
            pl = 2.0 * (w[2] - w[1]) / w.sum() if wrong == "planarity_two_largest" else 2.0 * (w[1] - w[0]) / w.sum()
            offered.append((int(li), pl))
            if not pl >= params.p_lambda:
                continue
        ptype = plane_type_of(nrm)
        if wrong == "type_ascending":
            ptype = int(np.argsort(np.abs(nrm), kind="stable")[0])
        a = np.sort(np.abs(nrm))
        type_gap = 0.0 if (a[0] == 0 and a[1] == 0) else a[1] - a[0]
        d = -(nrm @ mean)
        dist0 = np.abs(x @ nrm + d)
        in0 = inside(dist0)
        nin = nin0 = int(in0.sum())
        margin, gap, branch = np.abs(dist0 - params.thr).min(), (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0, "none"
        margin0 = margin
        if nin0 >= 3 and wrong != "refit_skipped":
            mu, Ci = _centred_cov(x[in0])
            wi, n2 = _smallest_vec(Ci)
            branch = "rq" if rq_accepts(Ci, nrm) else "jacobi"
            gap = (wi[1] - wi[0]) / wi[2] if wi[2] > 0 else 0.0
            nrm, d = n2, -(n2 @ mu)
            dist1 = np.abs(x @ nrm + d)
            in1 = inside(dist1)
            margin = min(margin, np.abs(dist1 - params.thr).min())
            if wrong != "count_first_selection":
                nin = int(in1.sum())
        else:
            in1 = in0
        fitted.append((int(li), float(margin), nin0, nin, float(margin0), float(gap)))
        if nin < params.min_inl:
            continue
        d_raw = d
        if wrong != "no_sign_flip" and (d > 0 or (d == 0 and tuple(nrm) < (0.0, 0.0, 0.0))):
            nrm, d = -nrm, -d
        nrm = nrm + 0.0                                         # (-0.0 -> 0.0 compares equal anyway)
        bx = p32[in1] if wrong == "box_of_inliers" else p32
        for k, v in zip(out, (np.append(nrm, d), -d * nrm, bx.min(axis=0).astype(np.float64), bx.max(axis=0).astype(np.float64), li, n, nin, ptype, margin, gap, type_gap,
                              branch, nin0, d_raw)):
            out[k].append(v)
    r = dict(p4=np.array(out["p4"]).reshape(-1, 4), Pi=np.array(out["Pi"]).reshape(-1, 3), box_min=np.array(out["box_min"]).reshape(-1, 3),
             box_max=np.array(out["box_max"]).reshape(-1, 3))
    for k in ("leaf", "n_points", "n_inliers", "plane_type", "nin0"):
        r[k] = np.array(out[k], np.int32)
    for k in ("margin", "gap", "type_gap", "d_raw"):
        r[k] = np.array(out[k], np.float64)
    r["branch"], r["offered"], r["fitted"], r["n_leaves"], r["counts"] = out["branch"], offered, fitted, len(cnt), cnt
    return r


ORACLE_VS_NUMPY_P4 = 3.9e-14         # max |p4 difference| between the oracle and np_surfel_extract over all cases, measured on the CPU (case ppl_clean)
ORACLE_VS_NUMPY_PI = 9.7e-15         # max |Pi difference| / max |Pi| of the case  (cases thr_few_inliers_*)
P4_BAR, PI_BAR = 4 * ORACLE_VS_NUMPY_P4, 4 * ORACLE_VS_NUMPY_PI      # (the factor leaves headroom for another libm or BLAS)
GAP_MIN = 1e-3          # (c)
TYPE_GAP_MIN = 1e-9     # (d)
EXEMPT_CAP = 0.05


def p4_compared(ref):
    """(c): the accepted leaves of the numpy result whose normal is determined — the only exemption from the p4 / Pi / inlier-count comparisons."""
    return ref["gap"] >= GAP_MIN


def type_compared(ref):
    """(d): plane_type is compared where the two smallest |n| components differ by more than 1e-9 or are both exactly zero."""
    return p4_compared(ref) & ((ref["type_gap"] > TYPE_GAP_MIN) | (ref["type_gap"] == 0.0))


def as_dict(r):
    """A result as the oracle's dict (lvx.surfel_extract returns a structured array)."""
    return {k: np.array(r[k]) for k in ("p4", "Pi", "box_min", "box_max", "leaf", "n_points", "n_inliers", "plane_type")}


def compare(a, b, mask=None):
    """max |p4 difference|, max |Pi difference| / max |Pi| over the leaves of mask; the leaves, counts and boxes have to be identical everywhere, the inlier counts and
    plane types on the mask (type_mask for the types).  Returns (dp4, dPi_rel, discrete_equal)."""
    a, b = as_dict(a), as_dict(b)
    if len(a["leaf"]) != len(b["leaf"]) or not np.array_equal(a["leaf"], b["leaf"]):
        return np.inf, np.inf, False
    m = np.ones(len(a["leaf"]), bool) if mask is None else mask
    same = (np.array_equal(a["n_points"], b["n_points"]) and np.array_equal(a["box_min"], b["box_min"]) and np.array_equal(a["box_max"], b["box_max"])
            and np.array_equal(a["n_inliers"][m], b["n_inliers"][m]))
    if not m.any():
        return 0.0, 0.0, same
    scale = max(np.abs(b["Pi"][m]).max(), 1e-300)
    return np.abs(a["p4"][m] - b["p4"][m]).max(), np.abs(a["Pi"][m] - b["Pi"][m]).max() / scale, same


def check_result(cloud, params, result, ref=None, leaf=LEAF, normal_tol=1e-6, stated_types=None):
    """What a result of setSurfelMap has to be, whoever computed it (applied to the oracle's and the device's): planes in ascending voxel-key order; n_points the
    numpy count of the cell; the box the float min / max of ALL the cell's points, bit for bit; |n| = 1 and Pi = -d n to 1e-12; d <= 0, the first non-zero component of
    n positive at d == 0; n_inliers recounted in float64 from the returned plane (between the counts at thr -+ 1e-9: equal under condition (a)); the normal along the
    smallest eigenvector (eigh) of the centred covariance of the points the leaf's own plane selects, where (c) says it is determined; plane_type the argmin of |n|
    where (d) says it is decided, the stated value at an exact-zero tie; exactly the leaves the numpy restatement accepts.  Raises AssertionError naming the rule.
    The recount is a window, so it cannot tell <= from < for a point that sits exactly ON dist_threshold (the exact-tie leaves, which condition (a) lets through on
    purpose): there only the comparison of n_inliers with the numpy result and the oracle decides.  Nor does it bind a leaf exempt through (c) to one inlier count."""
    r = as_dict(result)
    ref = np_surfel_extract(cloud, params, leaf) if ref is None else ref
    order, offs, keys = cells_of(cloud, leaf)
    xyz32 = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    P = len(r["leaf"])
    assert all(len(r[k]) == P for k in r), "ragged result"
    assert np.array_equal(r["leaf"], ref["leaf"]), "accepted leaves: got %d, numpy %d" % (P, len(ref["leaf"]))
    if P == 0:
        return
    lf = r["leaf"].astype(np.int64)
    assert (np.diff(lf) > 0).all() and lf[0] >= 0 and lf[-1] < len(keys), "voxel-key order"
    assert np.array_equal(r["n_points"], np.diff(offs)[lf]), "n_points"
    srt = xyz32[order]
    bmin, bmax = np.minimum.reduceat(srt, offs[:-1], axis=0), np.maximum.reduceat(srt, offs[:-1], axis=0)
    assert np.array_equal(r["box_min"], bmin[lf].astype(np.float64)) and np.array_equal(r["box_max"], bmax[lf].astype(np.float64)), "box"
    n, d = r["p4"][:, :3], r["p4"][:, 3]
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12, "|n| = 1"
    assert np.abs(r["Pi"] + d[:, None] * n).max() <= 1e-12 * max(1.0, np.abs(d).max()), "Pi = -d n"
    assert (d <= 0).all(), "d <= 0"
    for k in np.nonzero(d == 0)[0]:
        nz = n[k][n[k] != 0]
        assert len(nz) and nz[0] > 0, "lexicographic sign at d == 0"
    cmp4, cmpt = p4_compared(ref), type_compared(ref)
    for k in range(P):
        x = xyz32[order[offs[lf[k]]:offs[lf[k] + 1]]].astype(np.float64)
        dist = np.abs(x @ n[k] + d[k])
        lo, hi = int((dist < params.thr - 1e-9).sum()), int((dist < params.thr + 1e-9).sum())
        assert lo <= r["n_inliers"][k] <= hi and r["n_inliers"][k] >= params.min_inl, "n_inliers recount (leaf %d: %d not in [%d, %d])" % (lf[k], r["n_inliers"][k], lo, hi)
        if cmp4[k]:
            mean, C = _centred_cov(x)
            _, n0 = _smallest_vec(C)
            in0 = np.abs(x @ n0 - n0 @ mean) < params.thr
            nfit = _smallest_vec(_centred_cov(x[in0])[1])[1] if in0.sum() >= 3 else n0
            assert np.linalg.norm(np.cross(nfit, n[k])) <= normal_tol, "normal is not the smallest eigenvector of the inlier covariance (leaf %d)" % lf[k]
        if cmpt[k]:
            a = np.abs(n[k])
            two = np.sort(a)[:2]
            if ref["type_gap"][k] > TYPE_GAP_MIN:
                assert two[1] - two[0] > 0 and r["plane_type"][k] == int(np.argmin(a)), "plane_type = argmin |n| (leaf %d)" % lf[k]
            else:
                want = plane_type_of(ref["p4"][k, :3]) if stated_types is None else stated_types.get(int(lf[k]), plane_type_of(ref["p4"][k, :3]))
                assert r["plane_type"][k] == want, "plane_type at an exact tie (leaf %d: %d, stated %d)" % (lf[k], r["plane_type"][k], want)


# ------------------------------------------------------------------------------------------------------------------------
# tuning: planarity a chosen distance from p_lambda
# ------------------------------------------------------------------------------------------------------------------------
def leaf_planarity(leaf_obj, params=DEFAULT):
    x = leaf_obj.points().astype(np.float64)
    n = len(x)
    w, _ = _smallest_vec(_centred_cov(x)[1] * ((n - 1.0) / n))
    m = params.eig_mult * w[2]
    if w[0] < m:
        w[0] = m
        w[1] = max(w[1], m)
    return 2.0 * (w[1] - w[0]) / w.sum()


def tuned(make, target, lo, hi, tol=2.5e-7):
    """make(s) -> Leaf whose planarity falls as s grows (s = thickness): bisect s until the planarity (numpy, of the float32 points) is within tol of target."""
    flo, fhi = leaf_planarity(make(lo)), leaf_planarity(make(hi))
    assert flo > target > fhi, (flo, target, fhi)
    for _ in range(200):
        s = 0.5 * (lo + hi)
        l = make(s)
        f = leaf_planarity(l)
        if abs(f - target) <= tol:
            return l
        lo, hi = (s, hi) if f > target else (lo, s)
    raise AssertionError("planarity %g not reached (%g)" % (target, f))


# ------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------
PPL = (9, 10, 19, 20, 21, 63, 64, 65, 127, 128, 511, 512, 513, 1023, 1024, 1025, 2298, 5200)      # points per leaf; 5200 = eleven trips of 512
LEAF_COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 4100)
BIG_W, BIG_LAYERS = 64, 65                                                                      # the 266 240-leaf cloud: every cell of a 64 x 64 x 65 block
BIG_LEAVES = BIG_W * BIG_W * BIG_LAYERS
BIG_PLANTED = (0, 1023, 1024, 262143, 262144, 262145, BIG_LEAVES - 1)
NORMALS = [GENERIC, (0.8, 0.1, -0.55), (-0.2, 0.9, 0.3), (1, 1, 0), (0.05, 0.02, 1.0), (0.6, -0.6, 0.5)]


def cell_of_index(i, W=16):
    """Cell of leaf index i in a block of W x W x ... cells about the origin, filled in voxel-key order (x fastest, then y, then z): with the first row (W > L) or
    the first layer complete, leaf index = i.  The block keeps every coordinate within a few metres of the origin (the covariance is summed in a single pass)."""
    i = np.asarray(i)
    return np.stack([i % W - W // 2, (i // W) % W - W // 2, i // (W * W) - W // 2], axis=-1)


def _block(L, accepted, n=20, seed=0):
    """L leaves, leaf index i in cell_of_index(i).  accepted(i) -> planar patch of n points (sigma = 4 mm: accepted), else a single point."""
    leaves, singles = [], []
    for i in range(L):
        if accepted(i):
            leaves.append(patch(cell_of_index(i), n, NORMALS[i % len(NORMALS)], seed=seed + i))
        else:
            singles.append(cell_of_index(i))
    return leaves, singles


def coincident(cell, n, tag="coincident"):
    """n copies of one dyadic point: at least min_points_per_voxel of them have a zero covariance, which the voxel build rejects (nr_points = -1, zero eigenvalues,
    identity eigenvectors).  Such a leaf must never reach the fit: fitted with the identity's e_z through its mean, all n points would be inliers."""
    return Leaf(cell, np.tile([0.5, 0.25, 0.75], (n, 1)), tag, exact=True)


MINPTS_COUNTS = (1, 2, 5, 6, 7, 9, 10, 11, 12, 13, 49, 50, 51, 60)
MINPTS_COINCIDENT = 14          # points of the rejected leaf of the minpts cases (above both min_points_per_voxel, 6 and 12)


@functools.lru_cache(maxsize=None)
def _few_inliers():
    return [sheets((i, 0, 0), 12, k, NORMALS[i % 3], seed=42) for i, k in enumerate((0, 1, 2, 3, 4))]


@functools.lru_cache(maxsize=None)
def _minpts_leaves():
    return [patch((i, 0, 0), n, NORMALS[i % len(NORMALS)], seed=49) for i, n in enumerate(MINPTS_COUNTS)] + [coincident((len(MINPTS_COUNTS), 0, 0), MINPTS_COINCIDENT)]


def _lambda_leaves(lam):
    lv = [tuned(lambda s, i=i, sg=sg: sym_blob((i, 0, 0), s, 0.25, 0.25, NORMALS[i % 3], seed=44, tag="planarity%+d" % sg), lam + sg * 1e-6, 0.02, 0.9)
          for i, sg in enumerate((-1, 1))]
    return lv + [patch((2 + i, 0, 0), 24, NORMALS[i], seed=45) for i in range(4)]


def _big():
    planted = [patch(cell_of_index(i, BIG_W), 24, NORMALS[j % len(NORMALS)], seed=30) for j, i in enumerate(BIG_PLANTED)]
    taken = np.zeros(BIG_LEAVES, bool); taken[list(BIG_PLANTED)] = True
    return planted, cell_of_index(np.nonzero(~taken)[0], BIG_W)


def _geometry():
    # normals exactly along the axes (dyadic constants: the covariance row is exactly zero, the inflation decides the planarity), (1, 1, 0) / sqrt 2, generic
    geo = [axis_patch((i, 0, 0), 24 + i, ax, seed=50) for i, ax in enumerate((0, 1, 2))]
    geo += [axis_patch((3, 0, 0), 64, 0, const=0.25, seed=51), axis_patch((-1, 0, 0), 32, 1, const=0.75, seed=51), axis_patch((0, 0, -1), 30, 2, const=0.5, seed=51)]
    geo += [patch((5 + i, 0, 0), 30, nrm, seed=52) for i, nrm in enumerate(NORMALS)]
    # the plane z = 0 through the origin: d == 0, lexicographic sign; x = 0 and y = 0 as well (z = 0.0 is the lower face of its cell: exact)
    geo += [axis_patch((0, 1, 0), 26, 2, const=0.0, seed=53), axis_patch((0, 2, 1), 26, 0, const=0.0, seed=53), axis_patch((1, 0, 2), 26, 1, const=0.0, seed=53)]
    # cells on both sides of every coordinate plane, d of both signs before the flip (the same normal on either side of the origin)
    geo += [patch(c, 28, nrm, seed=54) for k, nrm in enumerate((GENERIC, (-0.31, 0.52, -0.79)))
            for c in ((3 + k, 3, 3), (-4 - k, 3, 3), (3, -4 - k, 3), (3, 3, -4 - k), (-4 - k, -4, -4))]
    return geo


def _far():
    far = [patch(tuple(int(s * 100 * (a == k)) for a in range(3)), 30 + 3 * k, NORMALS[(k + (s > 0)) % len(NORMALS)], seed=55) for k in range(3) for s in (-1, 1)]
    return far + [patch((100, -100, 99), 40, NORMALS[1], seed=56), patch((-101, 100, -100), 40, NORMALS[2], seed=56)]


def _jacobi():
    jac = [rod((0, 0, 0), 64, seed=59), sheets((1, 0, 0), 20, 12, NORMALS[1], seed=60, mid_line=True, tag="collinear"), turned_plane((2, 0, 0), seed=61)]
    return jac + [patch((3 + i, 0, 0), 24, NORMALS[i % len(NORMALS)], seed=62) for i in range(40)]


def _cases():
    """The table: names, parameters and builders only — a case's leaves are made when somebody asks for them."""
    C = []
    # points per leaf: once clean ...
    C.append(Case("ppl_clean", lambda: [patch((i, 0, 0), n, NORMALS[i % len(NORMALS)], seed=1) for i, n in enumerate(PPL)], group="ppl"))
    # ... and, from 64 points on, with outliers (set per leaf: an eighth of the points, 40 at the most — more would pull the planarity of the 64-point leaves under 0.7)
    # placed so that some lanes hold none and others hold all of them: in the first 64 list positions (the first lanes' first points), and only in the last partial
    # trip (at 512 / 1 024: the last positions of the last full trip)
    last_trip = lambda n: n - EX_TRIP * ((n - 1) // EX_TRIP)       # (513 and 1 025 points: one point, one outlier)
    for where in ("first", "last"):
        C.append(Case("ppl_out_" + where, lambda where=where: [patch((i, 1, 0), n, NORMALS[(i + 2) % len(NORMALS)], out_off=0.12, where=where, seed=2,
                                                                     n_out=min(40, max(4, n // 8), last_trip(n) if where == "last" else n))
                                                               for i, n in enumerate(PPL) if n >= 64], group="ppl"))
    # one-sided outliers at 0.2 m, set per leaf: they pull the leaf's own plane over (first and second selection differ, the refit matters), few enough to stay planar
    C.append(Case("ppl_tilt", lambda: [patch((i, 2, 0), n, NORMALS[(i + 1) % len(NORMALS)], n_out=max(2, n // 25), out_off=0.2, out_side="pos", where="spread", seed=3)
                                       for i, n in enumerate(PPL) if n >= 64], group="ppl"))
    # leaves per cloud
    for L in LEAF_COUNTS:
        C.append(Case("leaves_%d" % L, lambda L=L: _block(L, (lambda i: True) if L <= 5 else (lambda i: i % 4 == 0 or i == L - 1), n=24, seed=10), group="leaves"))
    # acceptance patterns at 2 049 leaves
    L = 2049
    for name, acc in (("none", lambda i: False), ("all", lambda i: True), ("first", lambda i: i == 0), ("last", lambda i: i == L - 1), ("mid", lambda i: i in (1023, 1024)),
                      ("second", lambda i: i % 2 == 0)):
        C.append(Case("accept_" + name, lambda acc=acc: _block(L, acc, n=20, seed=20), group="accept"))
    # the 266 240-leaf cloud: surfel leaves planted at the seams of both compactions, single points everywhere else
    C.append(Case("big", _big, group="big", big=True))
    # thresholds: min_leaf_points
    C.append(Case("thr_min_leaf", lambda: [patch((0, 0, 0), 23, seed=40), patch((1, 0, 0), 24, seed=40), patch((2, 0, 0), 25, seed=40)], DEFAULT._replace(min_leaf=24), group="thresholds"))
    # ... min_inliers = 27: 30 points of which 4 / 3 / 2 are (two-sided) outliers (ten of them would pull the planarity under 0.7)
    C.append(Case("thr_min_inliers", lambda: [patch((i, 0, 0), 30, n_out=k, out_off=0.12, seed=41) for i, k in enumerate((4, 3, 2))], DEFAULT._replace(min_inl=27), group="thresholds"))
    # ... 0, 1, 2, 3 and 4 inliers under a tight threshold: no refit below three; accepted with the leaf's own plane at min_inliers 1 and 2
    for mi in (1, 2, 3):
        C.append(Case("thr_few_inliers_%d" % mi, _few_inliers, DEFAULT._replace(thr=0.02, min_inl=mi), group="thresholds"))
    # ... dist_threshold 0.2: the 0.12 m outliers are inliers
    C.append(Case("thr_wide", lambda: [patch((i, 0, 0), 40 + i, NORMALS[i], n_out=4, out_off=0.12, seed=43) for i in range(4)], DEFAULT._replace(thr=0.2), group="thresholds"))
    # ... planarity 1e-6 below and above p_lambda (the thickness of a 40-point slab with equal in-plane variances is bisected until the numpy planarity is there)
    for lam in (0.6, 0.7, 0.95):
        C.append(Case("thr_lambda_%g" % lam, lambda lam=lam: _lambda_leaves(lam), DEFAULT._replace(p_lambda=lam, thr=0.2), group="thresholds"))
    # ... p_lambda = 0: nothing lies below it (a planarity is never negative); a blob whose two smallest variances nearly meet sits 1e-6 above (its normal is not
    # determined: exempt through (c)), among 24 ordinary leaves (the 5 % cap)
    C.append(Case("thr_lambda_0", lambda: [tuned(lambda s: sym_blob((0, 0, 0), s, 0.3, 0.1, seed=46, tag="planarity+1"), 1e-6, 0.2, 1.0, tol=4e-7)]
                  + [patch((1 + i, 0, 0), 24, NORMALS[i % len(NORMALS)], seed=47) for i in range(24)], DEFAULT._replace(p_lambda=0.0, thr=0.2), group="thresholds"))
    # ... a point exactly ON dist_threshold (dyadic coordinates: no rounding anywhere): strict <
    C.append(Case("thr_exact_tie", lambda: [axis_patch((i, 0, 0), 22, ax, n_pairs=3, off=0.125, seed=48) for i, ax in enumerate((0, 1, 2))], DEFAULT._replace(thr=0.125), group="thresholds"))
    # ... min_leaf_points against min_points_per_voxel: leaves of 1 .. 60 points — those below min_points_per_voxel carry identity eigen data and are never surfels — and
    # a leaf of 14 coincident points, which the build rejects (nr_points = -1): with min_leaf_points 1, 0 or -3 it must not reach the fit
    for mp in (6, 12):
        for ml in (1, 6, 10, 50, 0, -3):
            C.append(Case("thr_leafpts_%d_%d" % (ml, mp), _minpts_leaves, DEFAULT._replace(min_leaf=ml, min_pts=mp, min_inl=1), group="minpts"))
    C.append(Case("geometry", _geometry, group="geometry"))
    # cells at +-100 m on every axis: a covariance summed over the raw coordinates cancels about six digits there
    C.append(Case("far", _far, group="geometry"))
    # the Jacobi fallback: a rod with a square cross-section (two equal smallest eigenvalues), collinear inliers (min_inliers = 3), and turned_plane — a leaf whose
    # own plane selects a strip with ANOTHER normal: the iteration starts at the strip's middle eigenvector and stays there, the full solve finds a determined normal
    C.append(Case("jacobi", _jacobi, DEFAULT._replace(p_lambda=0.1, thr=0.02, min_inl=3), group="jacobi"))
    return C


def turned_plane(cell, seed=0, normal=(0.12, -0.07, 1.0), tag="turned_plane"):
    """Two wide sheets at +-0.1 m from the patch plane over the same places (the leaf's PCA normal is the patch normal) and a strip of 30 points between them that is
    1 mm thin ACROSS the patch, 0.012 m high and long: the leaf's plane selects the strip alone, whose smallest direction lies in the patch plane."""
    rng = np.random.default_rng([seed, 1])
    nn, u, v = _basis(normal)
    ab = _iso(rng.uniform(-0.22, 0.22, (60, 2)), 0.22)
    ab = np.concatenate([ab, ab])
    off = np.concatenate([np.full(60, 0.1), np.full(60, -0.1)])
    strip = np.stack([0.001 * rng.standard_normal(30), rng.uniform(-0.22, 0.22, 30)], axis=1)
    ab, off = np.concatenate([ab, strip]), np.concatenate([off, rng.uniform(-0.012, 0.012, 30)])
    return Leaf(cell, 0.5 + ab[:, :1] * u + ab[:, 1:] * v + off[:, None] * nn, tag)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALL = [c.name for c in CASES if not c.big]
COMPACTION = [c.name for c in CASES if c.group in ("leaves", "accept")]


@functools.lru_cache(maxsize=None)
def cells(name):
    """cells_of the case's cloud, computed once."""
    return cells_of(BY_NAME[name].cloud)


@functools.lru_cache(maxsize=None)
def np_result(name):
    c = BY_NAME[name]
    return np_surfel_extract(c.cloud, c.params)


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """The oracle's voxel build (its own leaves) and extraction."""
    from oracle import oracle as O
    c = BY_NAME[name]
    vo = O.voxel_build(c.cloud, LEAF, c.params.min_pts, c.params.eig_mult)
    r = O.surfel_extract(c.cloud, vo, c.params.p_lambda, c.params.thr, c.params.min_leaf, c.params.min_inl)
    r["n_leaves"], r["leaf_n"] = vo["n_leaves"], vo["leaf_n"]
    return r
