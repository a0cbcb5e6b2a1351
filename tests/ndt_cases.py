"""Shared by tests/test_ndt_cases.py (CPU) and tests/test_gpu_ndt_edges.py: seeded NDT scenes OFF the 1.0 m grid of the older tests, and a float64 restatement of
the NDT objective's derivatives that shares nothing with the hand-typed angular tables of csrc/lvx_upstream.hip::ndt_tables and oracle/orc_*.cpp.

ndt_reference_f64 builds R = Rx Ry Rz from the 6-vector, takes dR/dp and d2R/dp2 as the same product with one or two axis GENERATORS inserted
(dRx/da = Rx Gx = Gx Rx, so dR/drx = Rx Gx Ry Rz, d2R/drx dry = Rx Gx Ry Gy Rz, ...) and applies Magnusson 2009 eq. 6.9 / 6.12 / 6.13 per (point, neighbour leaf).
The neighbour ids are an INPUT (the oracle's voxel_lookup7 of the float-transformed cloud): which leaf a point sees is not what is compared here.  It does not hold
the |angle| < 10e-5 branch of computeAngleDerivatives: use it at angles that are exactly 0 or well above that.

Scenes are rooms measured in CELLS (scaled by the leaf size), so that every resolution sees the same occupancy: ~8 000 points, walls 0.08 cells thick with a density gradient (leaves
from 1 to 40 points: both sides of min_points_per_voxel = 3, 6 and 12), two pillars, 10 % clutter; the room straddles all three coordinate planes.  The source is a
1 000-point sub-sample of the target moved by the INVERSE of a pose next to the case's p6, so that the transformed cloud lies on the target a tenth of a
cell off — also at rotations of a radian, where a plain sub-sample would leave the room.

ORACLE AGAINST THE FLOAT64 REFERENCE — max |oracle - f64| / max |f64| over the cases of `grid`, `big_angles`, `min_pts` and `border` (their angles are 0 or large),
measured by tests/test_ndt_cases.py::test_oracle_against_the_float64_reference on the CPU (it prints the figures); the oracle's per-point arithmetic is float by
design (computePointDerivatives / updateDerivatives are float in the reference), its sums over cells and points double:

    quantity    measured      asserted (4 x, other seeds of the same size)
    score       4.22e-08      1.69e-07
    gradient    1.13e-07      4.52e-07
    Hessian     2.05e-07      8.20e-07

Against the PLAIN derivation (d1_row_as_reference=False, see REFERENCE_D1_ROW) the Hessian figure is 4.18e-02, all of it in H[ry][ry] at a pitch of 0.9 rad.
"""
import functools
import os
from collections import namedtuple

import numpy as np

from oracle import ndt_align as NA
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# measured oracle-vs-float64 discrepancies (the table above)
RECORDED = dict(score=4.22e-08, g=1.13e-07, H=2.05e-07)
# the project's GPU-vs-oracle bars (tests/test_gpu_upstream.py::test_ndt_derivatives)
BAR_SCORE, BAR_GH = 1e-6, 1e-5

N_TARGET, N_SOURCE = 8000, 1000
ROOM_LO, ROOM_HI = np.array([-5.3, -4.2, -2.6]), np.array([6.3, 4.6, 3.2])   # cells; 11.6 x 8.8 x 5.8, every wall at least 5 sigma inside its outermost cell layer
MISALIGN = np.array([0.15, -0.10, 0.08, 0.010, -0.008, 0.012])              # cells / rad: the source is placed this far from where p6 would put it on the target
WALL_SIGMA = 0.08                                                              # cells
MODERATE = np.array([0.24, -0.14, 0.06, 0.05, -0.04, 0.06])                   # cells / rad

# The ONE place where the reference's tables are not the derivative of R = Rx Ry Rz: row d1 of the second-derivative table (d2 x_0 / d ry^2) reads
# (-cy cz, cy sz, +sy) in ndt_omp_impl.hpp:360 and :382 (as in PCL's ndt.hpp); differentiating (-sy cz, sy sz, cy) gives (-cy cz, cy sz, -sy).  The library and the
# oracle restate the reference, sign included, so ndt_reference_f64 adds 2 sin(ry) x_2 to that one component by default; with d1_row_as_reference=False it is the
# plain derivation, and tests/test_ndt_cases.py::test_the_references_d1_row_is_the_only_departure_from_the_derivation holds the difference to H[ry][ry] alone.
REFERENCE_D1_ROW = "(-cy cz, cy sz, +sy)"

GEN = (np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0.0, 0, 1], [0, 0, 0], [-1, 0, 0]]), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 0]]))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------------------------
def axis_rotation(axis, angle):
    """exp(angle * G_axis) by Rodrigues' formula for a unit axis: I + sin G + (1 - cos) G^2."""
    G = GEN[axis]
    return np.eye(3) + np.sin(angle) * G + (1.0 - np.cos(angle)) * (G @ G)


def rotation_with_generators(angles, inserted=()):
    """Rx Ry Rz with the generator of every axis listed in `inserted` placed after that axis' factor: () = R, (i,) = dR/da_i, (i, j) = d2R/da_i da_j."""
    M = np.eye(3)
    for a in range(3):
        M = M @ axis_rotation(a, angles[a])
        for k in inserted:
            if k == a:
                M = M @ GEN[a]
    return M


def gauss_constants(res, outlier_ratio):
    """Magnusson 2009 eq. 6.8: d1, d2 of the Gaussian fitted to the mixture 'normal + uniform outliers over a cell of volume res^3'."""
    c1, c2 = 10.0 * (1.0 - outlier_ratio), outlier_ratio / (res * res * res)
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def ndt_reference_f64(vox, ids, src, trans, p6, res, outlier_ratio, parts=False, d1_row_as_reference=True):
    """(score, g[6], H[6][6]) in float64.  vox: the oracle's voxel grid (mean, icov per leaf); ids [n][k]: leaf per point and neighbour slot, -1 = none; src, trans:
    the source cloud and its transformed copy as the kernels get them (float32 values, used as they are).  parts=True adds the x'C^-1 d2x term of H alone.
    d1_row_as_reference: see REFERENCE_D1_ROW; False gives the plain derivation."""
    p6 = np.asarray(p6, np.float64)
    d1, d2 = gauss_constants(float(res), float(outlier_ratio))
    x, xt = np.asarray(src)[:, :3].astype(np.float64), np.asarray(trans)[:, :3].astype(np.float64)
    n = len(x)
    J = np.zeros((n, 3, 6))
    J[:, :, :3] = np.eye(3)
    D2 = np.zeros((n, 3, 6, 6))
    for i in range(3):
        J[:, :, 3 + i] = x @ rotation_with_generators(p6[3:], (i,)).T
        for j in range(3):
            D2[:, :, 3 + i, 3 + j] = x @ rotation_with_generators(p6[3:], (i, j)).T
    if d1_row_as_reference:
        D2[:, 0, 4, 4] += 2.0 * np.sin(p6[4]) * x[:, 2]
    pt, slot = np.nonzero(np.asarray(ids) >= 0)
    leaf = np.asarray(ids)[pt, slot]
    xd = xt[pt] - np.asarray(vox["mean"])[leaf]
    Ci = np.asarray(vox["icov"])[leaf].reshape(-1, 3, 3)
    xC = np.einsum("pa,pab->pb", xd, Ci)
    e = np.exp(-0.5 * d2 * np.einsum("pa,pa->p", xC, xd))
    ok = ~((d2 * e > 1) | (d2 * e < 0) | np.isnan(e))          # updateDerivatives drops such a term, score included (ndt_omp_impl.hpp:503-506)
    pt, xC, Ci, e = pt[ok], xC[ok], Ci[ok], e[ok]
    w = d1 * d2 * e
    a = np.einsum("pa,pak->pk", xC, J[pt])                     # x' C^-1 dx/dp_k
    score = float(np.sum(-d1 * e))
    g = np.einsum("p,pk->k", w, a)
    H2 = np.einsum("p,pa,paij->ij", w, xC, D2[pt])
    H = np.einsum("p,pi,pj->ij", -d2 * w, a, a) + H2 + np.einsum("p,pai,pab,pbj->ij", w, J[pt], Ci, J[pt])
    return (score, g, H, H2) if parts else (score, g, H)


def pose_matrix(p6):
    """float64 [R | t] of a 6-vector (Translation * Rx * Ry * Rz), from the generator form."""
    p6 = np.asarray(p6, np.float64)
    return rotation_with_generators(p6[3:]), p6[:3].copy()


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_room(seed, leaf, n=N_TARGET):
    """The target cloud (float32 xyzi), `leaf` metres per cell."""
    rng = np.random.default_rng(seed)
    lo, hi = ROOM_LO, ROOM_HI
    ext = hi - lo
    n_wall, n_pil = int(0.7 * n), int(0.2 * n)
    n_un = n - n_wall - n_pil
    area = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, n_wall, p=area / area.sum())
    uv = np.stack([rng.random(n_wall) ** 1.7, rng.random(n_wall)], axis=1)      # density falls along the first in-plane axis: leaves of a few to a few dozen points
    walls = np.zeros((n_wall, 3))
    for f in range(6):
        m = face == f
        ax, side = f // 2, f % 2
        u, v = [k for k in range(3) if k != ax]
        walls[m, ax] = (hi if side else lo)[ax] + WALL_SIGMA * rng.standard_normal(m.sum())
        walls[m, u] = lo[u] + ext[u] * uv[m, 0]
        walls[m, v] = lo[v] + ext[v] * uv[m, 1]
    pid = rng.integers(0, 2, n_pil)
    pc, pr = np.array([[-2.1, 1.7], [3.4, -1.9]]), np.array([0.45, 0.8])
    th = rng.uniform(0, 2 * np.pi, n_pil)
    pil = np.stack([pc[pid, 0] + pr[pid] * np.cos(th), pc[pid, 1] + pr[pid] * np.sin(th), rng.uniform(lo[2], hi[2], n_pil)], axis=1) + 0.02 * rng.standard_normal((n_pil, 3))
    xyz = np.concatenate([walls, pil, rng.uniform(lo, hi, (n_un, 3))])[rng.permutation(n)] * leaf
    return np.concatenate([xyz, rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_grid(seed, leaf, min_pts):
    return O.voxel_build(make_room(seed, leaf), np.float32(leaf), min_pts)


def place_source(positions, p6, leaf, misalign=True):
    """Source points (float32 xyzi, intensity 0) that the pose next to p6 (p6 + MISALIGN, translation in cells) carries onto `positions`; misalign=False: p6 itself."""
    q = np.asarray(p6, np.float64) + (MISALIGN * np.array([leaf, leaf, leaf, 1, 1, 1]) if misalign else 0.0)
    R, t = pose_matrix(q)
    src = np.zeros((len(positions), 4), np.float32)
    src[:, :3] = ((np.asarray(positions, np.float64)[:, :3] - t) @ R).astype(np.float32)      # R^T (y - t), row form
    return src


def cell_of(trans, leaf):
    """floor(x / leaf) per axis in float, as getNeighborhoodAtPoint computes it."""
    return np.floor(np.asarray(trans, np.float32)[:, :3] / np.float32(leaf)).astype(np.int64)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name group seed leaf min_pts outlier_ratio p6 n variant")
Built = namedtuple("Built", "case tgt vox src trans ids")


def _case(name, group, leaf=0.5, min_pts=6, outlier_ratio=0.55, p6=None, n=N_SOURCE, seed=11, variant=None):
    p = (MODERATE * np.array([leaf, leaf, leaf, 1, 1, 1])) if p6 is None else np.asarray(p6, np.float64)
    return Case(name, group, seed, leaf, min_pts, outlier_ratio, tuple(float(v) for v in p), n, variant)


def _rot_only(rx, ry, rz, leaf=0.5):
    return np.array([0.24 * leaf, -0.14 * leaf, 0.06 * leaf, rx, ry, rz])


BELOW, ABOVE = 9.9e-5, 1.01e-4          # the two sides of computeAngleDerivatives' |angle| < 10e-5
THRESHOLD_ANGLES = ((BELOW, ABOVE, -ABOVE), (ABOVE, ABOVE, ABOVE), (-BELOW, BELOW, ABOVE), (0.0, -ABOVE, BELOW), (-ABOVE, 0.0, -BELOW), (BELOW, -BELOW, BELOW))
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)

CASES = dict(
    grid=[_case("grid_leaf%g_out%g" % (l, o), "grid", leaf=l, outlier_ratio=o) for l in (0.5, 0.25, 2.0) for o in (0.55, 0.1, 0.9)],
    # seeds: the ones at which every angular pair's second-derivative term is visible (tests/test_ndt_cases.py::test_big_angles_can_see_a_wrong_table_row)
    big_angles=[_case("big_%d" % k, "big_angles", p6=_rot_only(*a), seed=sd)
                for k, (a, sd) in enumerate((((0.7, -0.5, 1.1), 22), ((-1.2, 0.4, -0.6), 33), ((0.9, 0.0, 0.0), 22), ((0.0, 0.9, 0.0), 27), ((0.0, 0.0, 0.9), 27)))],
    threshold=[_case("thr_%d" % k, "threshold", p6=_rot_only(*a)) for k, a in enumerate(THRESHOLD_ANGLES)],
    border=[_case("border_mixed", "border", variant="mixed"), _case("border_all_outside", "border", variant="outside")],
    min_pts=[_case("min_pts_%d" % m, "min_pts", min_pts=m) for m in (3, 12)],
    sizes=[_case("size_%d" % n, "sizes", n=n) for n in SIZES],
)
ALL = [c for group in CASES.values() for c in group]
BY_NAME = {c.name: c for c in ALL}
F64_GROUPS = ("grid", "big_angles", "min_pts", "border")      # compared with ndt_reference_f64: every angle is 0 or large


def border_positions(case):
    """Transformed positions for the `border` group and the kind of place of each: 'a' a target point in an outermost cell layer of the box (all six faces), 'b' the
    same points one cell outside their face, 'c' thousands of cells outside (both signs, one and several axes), 'd' target points within a tenth of a cell of a
    coordinate plane (both sides), 'o' two cells outside a face.  mixed = a + b + c + d; outside = c + o."""
    tgt, vox, leaf = make_room(case.seed, case.leaf), oracle_grid(case.seed, case.leaf, case.min_pts), case.leaf
    cell = cell_of(tgt, leaf)
    lo, hi = vox["grid"][0:3].astype(np.int64), vox["grid"][3:6].astype(np.int64)
    pos, kind = [], []
    far = np.array([[3000, 0, 0], [-4000, 0, 0], [0, 5000, 0], [0, -3500, 0], [0, 0, 4500], [0, 0, -2500], [4000, -2500, 3000], [-3000, 5000, -4000]], np.float64) * leaf
    centre = np.tile(tgt[:8, :3].astype(np.float64), (1, 1))
    for a in range(3):
        for bound, sign in ((lo, -1), (hi, 1)):
            layer = tgt[cell[:, a] == bound[a]][:12, :3].astype(np.float64)
            step = np.zeros(3); step[a] = sign * leaf
            pos += [layer, layer + step, layer + 2 * step]
            kind += ["a"] * len(layer) + ["b"] * len(layer) + ["o"] * len(layer)
    pos.append(centre + far); kind += ["c"] * len(far)
    for a in range(3):
        for sign in (-1, 1):
            c = tgt[:, a] / np.float32(leaf)
            near = tgt[(np.sign(c) == sign) & (np.abs(c) < 0.1)][:6, :3].astype(np.float64)
            pos.append(near); kind += ["d"] * len(near)
    pos, kind = np.concatenate(pos), np.array(kind)
    keep = np.isin(kind, list("abcd")) if case.variant == "mixed" else np.isin(kind, list("co"))
    return pos[keep], kind[keep]


@functools.lru_cache(maxsize=None)
def build(name):
    """Built(case, tgt, vox, src, trans, ids): the clouds as the C ABI takes them, the oracle's grid of the target and its 7-cell ids of the transformed source."""
    c = BY_NAME[name]
    tgt, vox = make_room(c.seed, c.leaf), oracle_grid(c.seed, c.leaf, c.min_pts)
    p6 = np.array(c.p6)
    if c.group == "border":
        positions, _ = border_positions(c)
    else:
        positions = tgt[::N_TARGET // N_SOURCE][:c.n, :3]
    src = place_source(positions, p6, c.leaf, misalign=c.group != "border")      # border: the places are the point
    trans = NA.transform_cloud(src, NA.ndt_matrix(p6))
    ids = O.voxel_lookup7(vox, trans, np.float32(c.leaf), c.min_pts)
    for a in (tgt, src, trans, ids):
        a.setflags(write=False)
    return Built(c, tgt, vox, src, trans, ids)


def oracle_derivatives(b, p6=None, compute_hessian=True):
    c = b.case
    return O.ndt_derivatives(b.vox, c.leaf, b.src, b.trans, np.array(c.p6) if p6 is None else p6, c.outlier_ratio, compute_hessian, c.min_pts)


def zeroed_below(p6):
    """p6 with every angle below the 10e-5 threshold replaced by exactly 0."""
    q = np.array(p6, np.float64)
    q[3:][np.abs(q[3:]) < 10e-5] = 0.0
    return q


# ---- the two real scans at the calibration's resolution ----------------------------------------------------------------------------------------------------
ALIGN_RESOLUTION = 0.5
ALIGN_REDUCE = 0.1          # VoxelGrid leaf the two scans are reduced with before the alignment


@functools.lru_cache(maxsize=None)
def align_clouds(reduce=ALIGN_REDUCE):
    tgt = np.load(os.path.join(GOLD, "ndt_data_251370668.npz"))["xyzi"]
    src = np.load(os.path.join(GOLD, "ndt_data_251371071.npz"))["xyzi"]
    td, sd = O.voxelgrid_xyzi(tgt, reduce), O.voxelgrid_xyzi(src, reduce)
    td.setflags(write=False); sd.setflags(write=False)
    return td, sd


def yaw_guess(sd, yaw=0.5):
    """(guess, source'): the source turned back by `yaw` about z and the guess that turns it forward again — the identity start of the plain case, at a large angle."""
    guess = NA.ndt_matrix(np.array([0.0, 0.0, 0.0, 0.0, 0.0, yaw]))
    back = NA.ndt_matrix(np.array([0.0, 0.0, 0.0, 0.0, 0.0, -yaw]))
    return guess, NA.transform_cloud(sd, back)
