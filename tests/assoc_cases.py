"""Scan-to-surfel association and SurfelPoint emission: a case table whose hit sets are chosen directly, and numpy restatements of the reference
(surfel_association.cpp:111-158,296-331) that do not rest on the oracle.  tests/test_assoc_cases.py holds every case to the regime it claims on the CPU;
tests/test_gpu_assoc_shapes.py runs the same cases through the C ABI and compares bit for bit.

The scan: ring h on the line y = h, column w at x = w * DX, z = small noise, ~2 % of the points with x = NaN.  Every plane is z = 0.  The box
[(w0 - 1/2) DX, (w0 + n - 1/2) DX] x [h - 1/2, h + nh - 1/2] x [-1, 1] holds exactly the columns w0 .. w0 + n - 1 of rings h .. h + nh - 1, so a plane's hits on a
ring are those columns minus the NaN ones (minus the ones farther than `radius` from z = 0 where a case moves z)."""
import functools
from collections import namedtuple

import numpy as np

DX = 0.01
NOISE = 0.04
NAN_FRACTION = 0.02
SA_WMAX = 4096          # widest scan of the C ABI
SA_PC = 256             # planes per LDS chunk of k_assoc_hits_allpairs
ASSOC_CHUNK = 64        # scans per launch of lvx_surfel_assoc_batch_d
SE_HMAX = 128           # k_assoc_emit_fused: rings per column thread
SE_COLS = 128           # ... columns per workgroup
SE_MAXWG = 2048         # ... publication words
FUSED_SAFE_WG = 64      # workgroups every part holds at once (64 CUs x 2 resident workgroups, less the margin of one per CU)

POINT_XYZIT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("pad2", "<f4"), ("timestamp", "<f8")])


def x_of(w):
    """float32 x coordinate of column w, as a double."""
    return float(np.float32(w * DX))


def box(h, w0, n, nh=1):
    """(lo, hi) of the box that holds columns w0 .. w0 + n - 1 of rings h .. h + nh - 1."""
    return [(w0 - 0.5) * DX, h - 0.5, -1.0], [(w0 + n - 0.5) * DX, h + nh - 0.5, 1.0]


def table(boxes):
    """p4, bmin, bmax of a list of (lo, hi) boxes; every plane is z = 0."""
    P = len(boxes)
    p4 = np.tile(np.array([0.0, 0.0, 1.0, 0.0]), (P, 1))
    bmin = np.array([b[0] for b in boxes], np.float64).reshape(P, 3)
    bmax = np.array([b[1] for b in boxes], np.float64).reshape(P, 3)
    return p4, bmin, bmax


def filler(k):
    """A box on a row no scan has (y = 1000 + k): reaches the grid and the plane chunks, holds no point."""
    return [(k % 50 - 0.5) * DX, 1000.0 + k - 0.5, -1.0], [(k % 50 + 7.5) * DX, 1000.0 + k + 0.5, 1.0]


def base_scan(H, W, seed, clean=()):
    """[H, W, 4] float32.  clean: (h, w0, n) spans that keep all their points (no NaN)."""
    rng = np.random.default_rng(seed)
    scan = np.zeros((H, W, 4), np.float32)
    scan[..., 0] = (np.arange(W) * DX).astype(np.float32)[None, :]
    scan[..., 1] = np.arange(H, dtype=np.float32)[:, None]
    scan[..., 2] = rng.uniform(-NOISE, NOISE, (H, W)).astype(np.float32)
    scan[..., 3] = rng.uniform(0, 100, (H, W)).astype(np.float32)
    nan = rng.random((H, W)) < NAN_FRACTION
    for h, w0, n in clean:
        nan[h, w0:w0 + n] = False
    scan[nan, 0] = np.nan
    return scan


class Case:
    """One flag case: a plane table, a scan shape, and scan(i) — the i-th scan of a batch (another seed each)."""

    def __init__(self, name, H, W, boxes, sel=2, radius=0.05, clean=(), tweak=None, seed=0, none=False, group=None):
        self.name, self.H, self.W, self.sel, self.radius, self.clean, self.tweak, self.seed, self.none = name, H, W, sel, radius, tuple(clean), tweak, seed, none
        self.group = group or name
        self.p4, self.bmin, self.bmax = table(boxes)
        self.P = len(boxes)

    def scan(self, i):
        return _scan(self.name, i)

    def scans(self, S, first=0):
        return np.stack([self.scan(first + i) for i in range(S)])

    def __repr__(self):
        return "Case(%s)" % self.name


@functools.lru_cache(maxsize=None)
def _scan(name, i):
    c = BY_NAME[name]
    s = base_scan(c.H, c.W, 1000 * (1 + c.seed) + 17 * i + sum(map(ord, name)), c.clean)
    if c.tweak:
        c.tweak(s, i)
    s.setflags(write=False)
    return s


# ------------------------------------------------------------------------------------------------------------------------
# numpy restatements of the reference
# ------------------------------------------------------------------------------------------------------------------------
RIGHT = dict(step=lambda c, sel: max(c // (sel + 1), 1), enough=lambda c, sel: c >= 2 * sel, near=lambda d, r: d <= r, inside=lambda v, lo, hi: (v > lo) & (v < hi), ascending=True)


def np_hits(scan, p4, bmin, bmax, radius, rules=RIGHT):
    """[P, H, W] bool: associateScanToSurfel (:305-331) — x not NaN, strictly inside the box (the float coordinates against the double bounds), |n.p + d| <= radius."""
    s = np.asarray(scan, np.float32)
    x, y, z = (s[..., a].astype(np.float64) for a in range(3))
    ok = ~np.isnan(s[..., 0])
    p4, bmin, bmax = (np.asarray(a, np.float64).reshape(-1, n) for a, n in ((p4, 4), (bmin, 3), (bmax, 3)))
    hits = np.zeros((len(p4),) + x.shape, bool)
    with np.errstate(invalid="ignore"):
        for k in range(len(p4)):
            ins = rules["inside"](x, bmin[k, 0], bmax[k, 0]) & rules["inside"](y, bmin[k, 1], bmax[k, 1]) & rules["inside"](z, bmin[k, 2], bmax[k, 2])
            if not ins.any():
                continue
            dist = x * p4[k, 0] + y * p4[k, 1] + z * p4[k, 2] + p4[k, 3]
            dist = np.where(dist > 0, dist, -dist)
            hits[k] = ok & ins & rules["near"](dist, radius)
    return hits


def np_select(hits, sel, rules=RIGHT):
    """getAssociation's flag pass (:117-137) over the hit sets, planes in ascending id (the serial loop: a later plane overwrites)."""
    P, H, W = hits.shape
    flag = np.full((H, W), -1, np.int32)
    for k in (range(P) if rules["ascending"] else range(P - 1, -1, -1)):
        for h in np.nonzero(hits[k].any(axis=1))[0]:
            m = np.nonzero(hits[k, h])[0]
            if not rules["enough"](len(m), sel):
                continue
            step = rules["step"](len(m), sel)
            for s in range(sel):
                at = step * (s + 1) - 1
                if at < len(m):         # (always, under the right rule; a wrong step rule may point past the list, where the reference would throw)
                    flag[h, m[at]] = k
    return flag


def np_assoc(scan, p4, bmin, bmax, radius, sel, rules=RIGHT):
    return np_select(np_hits(scan, p4, bmin, bmax, radius, rules), sel, rules)


def np_emit(flags, scan_map, raw, column_major=True, skip_zero=True):
    """The chronological emission (:141-158) of one scan: w outer, h inner; a point needs a flag and 0 != timestamp."""
    flags = np.asarray(flags, np.int32)
    H, W = flags.shape
    keep = flags != -1
    if skip_zero:
        keep = keep & ~(raw["timestamp"] == 0)          # (0 == NaN is false: a NaN stamp stays; -0.0 == 0 goes)
    if column_major:
        w, h = np.nonzero(keep.T)
    else:
        h, w = np.nonzero(keep)
    r, q = raw[h, w], np.asarray(scan_map, np.float32)[h, w]
    return dict(pt=np.stack([r["x"], r["y"], r["z"]], axis=1).astype(np.float64).reshape(-1, 3), pt_map=q[:, :3].astype(np.float64).reshape(-1, 3),
                t=r["timestamp"].astype(np.float64), plane=flags[h, w].astype(np.int32))


def same_list(a, b):
    """Bit equality of two SurfelPoint lists (NaN stamps compare by their bytes)."""
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ("pt", "pt_map", "t", "plane"))


def wpr_of(W):
    return (W + 31) // 32


def oshift_of(W):
    return 1 if wpr_of(W) > 64 else 0


def ring_counts(hits):
    """Hit counts of the (plane, ring) pairs that have any."""
    c = hits.sum(axis=2)
    return c[c > 0]


def word_occupancy(hits):
    """[P, H, wpr] bool: which 32-column mask words of a (plane, ring) hold a hit."""
    P, H, W = hits.shape
    pad = np.zeros((P, H, wpr_of(W) * 32), bool)
    pad[..., :W] = hits
    return pad.reshape(P, H, -1, 32).any(axis=3)


# ------------------------------------------------------------------------------------------------------------------------
# flag cases
# ------------------------------------------------------------------------------------------------------------------------
SEL_SLOTS = (32, 63, 95, 127)      # starts of the four short boxes of a ring: selected columns on bit 0 and on bit 31 of a mask word
SEL_LONG = (160, 150)              # the long box: columns 160 .. 309, five mask words


def _sel_case(sel):
    short = (2 * sel - 1, 2 * sel, 2 * sel + 1, 3 * sel + 2)
    boxes, clean = [], []
    for h in range(4):
        for j, w0 in enumerate(SEL_SLOTS):
            n = short[(j + h) % 4]
            boxes.append(box(h, w0, n)); clean.append((h, w0, n))
        boxes.append(box(h, *SEL_LONG))
    return Case("sel%d" % sel, 4, 320, boxes, sel=sel, clean=clean, group="sel")


def _nan_gaps(s, i):
    s[2, 204:210, 0] = np.nan          # a gap in the middle of the run 200 .. 215
    s[2, 233:250:2, 0] = np.nan        # every other column of the run 232 .. 250


def _word_edges():
    runs = [(0, 0, 4), (0, 30, 5), (0, 316, 4), (0, 250, 6),          # from column 0; columns 30-34 across a word boundary; to column W - 1
            (1, 60, 9), (1, 93, 6), (1, 126, 6), (1, 314, 6),          # step > 1: selected 62 65 | 94 96 (bit 0) | 127 (bit 31) 129 | 315 317
            (2, 200, 16), (2, 232, 19), (2, 0, 6),                     # NaN gaps inside (see _nan_gaps)
            (3, 0, 320)]                                               # a whole ring, random NaN points in it
    return Case("word_edges", 4, 320, [box(*r) for r in runs], clean=[r for r in runs if r[2] < 100], tweak=_nan_gaps)


def _width_case(H, W, runs, **kw):
    return Case("w%d" % W if H == 3 else "w%dx%d" % (H, W), H, W, [box(*r) for r in runs], clean=[r[:3] for r in runs if r[2] <= 12], group="widths", **kw)


def _widths():
    return [
        _width_case(3, 1, [(0, 0, 1), (1, 0, 1)], none=True),                                        # one column: never 2 sel hits
        _width_case(3, 31, [(0, 0, 31), (1, 27, 4), (2, 0, 4), (2, 10, 9)]),
        _width_case(3, 33, [(0, 0, 33), (1, 29, 4), (2, 28, 5), (2, 0, 6)]),
        _width_case(5, 100, [(0, 90, 10), (1, 0, 10), (1, 0, 100, 2), (3, 95, 5), (4, 0, 5), (4, 60, 40), (3, 30, 40)]),   # 500 points: two workgroups, wavefronts across two rings
        _width_case(3, 2048, [(0, 2040, 8), (1, 0, 6), (1, 2010, 11), (2, 1000, 100), (2, 2016, 32)]),
        _width_case(3, 2049, [(0, 2040, 9), (1, 20, 31), (2, 40, 11), (2, 2045, 4), (1, 2048, 1), (0, 0, 5)]),
        _width_case(3, 2080, [(0, 2070, 10), (1, 1990, 41), (2, 2020, 12), (2, 2048, 32), (1, 0, 8), (0, 33, 8)]),
        _width_case(3, 4095, [(0, 4085, 10), (1, 4040, 31), (2, 4064, 31), (2, 40, 11), (1, 20, 31), (0, 2040, 12)]),
    ]


def _h130():
    rings = (0, 1, 63, 64, 65, 127, 128, 129)
    runs = [(h, (7 * j) % 30, 4 + j % 5) for j, h in enumerate(rings)] + [(h, 20, 20) for h in rings[::2]] + [(60, 0, 40, 10), (126, 5, 8, 4)]
    return Case("h130", 130, 40, [box(*r) for r in runs], clean=[r[:3] for r in runs if len(r) == 3 and r[2] <= 8])


def _planes_case(P):
    """P planes on a 2 x 128 scan: every eighth plane has a box in columns 0 .. 99 (later ones lie over earlier ones), the others hold nothing; plane 255, plane 256 and
    the last plane have columns of their own."""
    boxes = [filler(k) for k in range(P)]
    for k in range(0, P, 8):
        j = k // 8
        boxes[k] = box(j % 2, (4 * j) % 96, 4 + j % 3)
    clean = [(0, 0, 100), (1, 0, 100)]
    if P > 256:
        boxes[255] = box(0, 100, 4); boxes[256] = box(0, 102, 6)        # share columns 102, 103: 255 keeps 100 101, 256 takes 103 105
        clean += [(0, 100, 8)]
    boxes[P - 1] = box(1, 120, 8)                                       # the last plane, to column W - 1
    clean += [(1, 120, 8)]
    return Case("planes%d" % P, 2, 128, boxes, clean=clean, group="planes")


def _overlap():
    boxes = [filler(k) for k in range(320)]
    for k in (3, 200, 300):
        boxes[k] = box(0, 10, 10)                                       # the same box three times, in both plane chunks: 300 wins
    boxes[5] = box(1, 20, 8); boxes[150] = box(1, 22, 8)                # 5 selects 21 23, 150 selects 23 25: column 23 goes to 150
    boxes[310] = box(2, 0, 64); boxes[7] = box(2, 16, 6)                # a short box under a long later one
    return Case("overlap", 3, 64, boxes, clean=[(0, 10, 10), (1, 20, 10), (2, 16, 6)])


def _bounds_tweak(s, i):
    s[2, 50, 1] = 2.5; s[2, 51, 1] = 1.5           # on the y bounds of ring 2's boxes (2.5 is the largest y of the table)
    s[0, 43, 1] = -0.5                             # on the smallest y of the table


def _outside_tweak(s, i):
    s[0, 10, 0] = -3.0; s[0, 11, 0] = 1.0e6; s[0, 12, 1] = -7.0; s[0, 13, 1] = 400.0; s[0, 14, 2] = 5.0; s[0, 15, 2] = -5.0      # outside the bounds of all boxes
    s[1, 30:40, 2] = 0.5                            # inside a box, farther than the radius from the plane
    s[2, 5, 0] = np.float32(0.75)                   # between the boxes of its ring
    s[2, 6, 0] = np.float32(0.95)                   # column 6 carries an x inside the box of columns 90 .. 95: a ring's hits are ordered by column, not by x


def _nonfinite_tweak(s, i):
    s[0, 10, 1] = np.nan; s[0, 12, 2] = np.nan
    s[1, 30, 0] = np.inf; s[1, 32, 0] = -np.inf; s[1, 34, 1] = np.inf; s[1, 36, 2] = -np.inf
    s[2, 61, 1] = np.nan; s[2, 62, 2] = np.nan; s[2, 63, 0] = np.inf


def _grid_edges():
    three = [(0, 8, 10), (1, 28, 12), (2, 56, 10), (2, 90, 6), (0, 40, 5)]
    clean = [r for r in three]
    # the box of ring 0 reaches from column 0's x to column 5's x, the last box of ring 2 from column 94's to column 99's: points exactly on the smallest lo and the
    # largest hi of the table, which are the bounds of the grid as well — strictly inside are columns 1 .. 4 and 95 .. 98
    on_lo = ([x_of(0), -0.5, -1.0], [x_of(5), 0.5, 1.0])
    on_hi = ([x_of(94), 1.5, -1.0], [x_of(99), 2.5, 1.0])
    return [
        Case("grid_p1", 3, 100, [box(1, 28, 12)], clean=[(1, 28, 12)], group="grid_edges"),
        Case("grid_empty", 3, 100, [box(0, 8, 10), ([0.3, 0.5, -1.0], [0.3, 1.5, 1.0]), box(1, 28, 12), ([0.2, 2.5, -1.0], [0.6, 1.5, 1.0]), box(2, 56, 10),
                                    ([0.0, -0.5, 1.0], [1.0, 2.5, -1.0])], clean=clean, group="grid_edges"),
        Case("grid_far", 3, 100, [box(*r) for r in three] + [([1000.0, 1000.0, 1000.0], [1001.0, 1001.0, 1001.0])], clean=clean, group="grid_edges"),
        Case("grid_bounds", 3, 100, [on_lo, box(1, 16, 10), on_hi, box(2, 46, 10), box(0, 40, 10)], clean=[(0, 0, 6), (1, 16, 10), (2, 94, 6), (2, 46, 10), (0, 40, 10)], tweak=_bounds_tweak, group="grid_edges"),
        Case("grid_outside", 3, 100, [box(*r) for r in three], clean=clean, tweak=_outside_tweak, group="grid_edges"),
        Case("grid_nonfinite", 3, 100, [box(*r) for r in three], clean=clean, tweak=_nonfinite_tweak, group="grid_edges"),
    ]


RADIUS_Z = np.array([0.25, -0.25, np.nextafter(np.float32(0.25), np.float32(1)), 0.1, 0.25, -0.25], np.float32)


def _radius_le_tweak(s, i):
    s[0, 10:16, 2] = RADIUS_Z                       # hits: 10 11 13 14 15; with < only 13, with column 12 as well the step becomes 2
    s[1, 40:46, 2] = RADIUS_Z[::-1]


def _radius_zero_tweak(s, i):
    s[0, 10:14, 2] = [0.0, -0.0, 0.0, 0.0]          # the only points on the plane
    s[1, 40:48, 2] = [0.0, 1e-30, 0.0, 0.0, -1e-30, 0.0, 0.0, 0.0]


def _radius_edges():
    return [Case("radius_le", 2, 64, [box(0, 10, 6), box(1, 40, 6), box(1, 0, 8)], radius=0.25, clean=[(0, 10, 6), (1, 40, 6), (1, 0, 8)], tweak=_radius_le_tweak, group="radius_edges"),
            Case("radius_zero", 2, 64, [box(0, 4, 16), box(1, 36, 16)], radius=0.0, clean=[(0, 4, 16), (1, 36, 16)], tweak=_radius_zero_tweak, group="radius_edges")]


def _chunks_tweak(s, i):
    s[np.random.default_rng(i).random(s.shape[:2]) < 0.15, 0] = np.nan          # every scan of a batch selects other columns: one written to another's place shows


def _chunks():
    runs = [(0, 0, 8), (0, 10, 9), (0, 30, 10), (0, 52, 12), (1, 2, 9), (1, 20, 20), (1, 40, 24), (0, 16, 12)]
    return Case("chunks", 2, 64, [box(*r) for r in runs], tweak=_chunks_tweak)


CHUNK_BATCHES = (66, 67, 130)


def chunk_sizes(S):
    """(scans, path) of the launches lvx_surfel_assoc_batch_d makes for S scans."""
    out = []
    for s0 in range(0, S, ASSOC_CHUNK):
        ns = min(ASSOC_CHUNK, S - s0)
        out.append((ns, "allpairs" if ns <= 2 else "grid"))
    return out


HYGIENE_RUNS = [(h, w0, 8) for h in range(4) for w0 in (0, 24, 40, 70, 88)]


def _hygiene_a(s, i):
    for h, w0, n in HYGIENE_RUNS[:-2]:
        s[h, w0 + 3:w0 + n, 0] = np.nan             # three hits: under 2 sel, cleared without being selected


def _hygiene_b(s, i):
    for h, w0, n in HYGIENE_RUNS:
        s[h, w0:w0 + 3, 0] = np.nan                 # the other five columns: bits left behind by the first call would make eight, and another step


def _hygiene():
    boxes, clean = [box(*r) for r in HYGIENE_RUNS], HYGIENE_RUNS
    return [Case("hygiene_a", 4, 96, boxes, clean=clean, tweak=_hygiene_a, group="hygiene"), Case("hygiene_b", 4, 96, boxes, clean=clean, tweak=_hygiene_b, group="hygiene")]


CASES = ([_sel_case(s) for s in (1, 2, 3, 5)] + [_word_edges()] + _widths() + [Case("h1", 1, 300, [box(0, 0, 5), box(0, 31, 4), box(0, 100, 130), box(0, 290, 10)], clean=[(0, 0, 5), (0, 31, 4), (0, 290, 10)]), _h130()]
         + [_planes_case(P) for P in (255, 256, 257, 513)] + [_overlap()] + _grid_edges() + _radius_edges() + [_chunks()] + _hygiene())
BY_NAME = {c.name: c for c in CASES}
WIDE = {"w2048": (64, 0), "w2049": (65, 1), "w2080": (65, 1), "w4095": (128, 1)}      # name -> (wpr, oshift)
BATCHES = (1, 2, 3)                                                                      # all pairs; all pairs with blockIdx.z = 1; the grid
PARITY = [c.name for c in CASES if c.name != "chunks"]                                   # run at every size of BATCHES; `chunks` has batches of its own


@functools.lru_cache(maxsize=None)
def hits_of(name, i=0):
    c = BY_NAME[name]
    return np_hits(c.scan(i), c.p4, c.bmin, c.bmax, c.radius)


@functools.lru_cache(maxsize=None)
def oracle_flags(name, i=0):
    from oracle import oracle as O
    c = BY_NAME[name]
    f = O.surfel_assoc(c.scan(i), c.p4, c.bmin, c.bmax, c.radius, c.sel)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------------------------------
# emission cases
# ------------------------------------------------------------------------------------------------------------------------
EmitCase = namedtuple("EmitCase", "name S H W density empty path")

EMIT_CASES = [
    EmitCase("two_130x40", 3, 130, 40, 0.3, (), "two_launch"),            # H > 128; 5 200 points: several trips of the 1 024-position loop
    EmitCase("two_200x9", 2, 200, 9, 0.5, (), "two_launch"),
    EmitCase("two_s2049", 2049, 1, 8, 0.4, (), "two_launch"),             # more scans than publication words, and than one trip of the prefix loop
    EmitCase("two_s1100", 1100, 2, 130, 0.1, (), "two_launch"),           # 2 200 workgroups of 128 columns
    EmitCase("fused_1x1", 5, 1, 1, 1.0, (1, 3), "fused"),
    EmitCase("fused_15x127", 5, 15, 127, 0.3, (1, 3), "fused"),
    EmitCase("fused_17x128", 5, 17, 128, 0.3, (1, 3), "fused"),
    EmitCase("fused_64x129", 5, 64, 129, 0.2, (1, 3), "fused"),
    EmitCase("fused_65x300", 5, 65, 300, 0.2, (1, 3), "fused"),
    EmitCase("fused_100x40", 5, 100, 40, 0.3, (1, 3), "fused"),
    EmitCase("fused_128x129", 5, 128, 129, 0.2, (1, 3), "fused"),
    EmitCase("fused_full", 2, 128, 129, 1.0, (), "fused"),                # every point emitted
    EmitCase("pub_16x300", 16, 16, 300, 0.3, (), "fused"),                # 48 publication words; run before and after fused_1x1 on one context
]
EMIT_BY_NAME = {c.name: c for c in EMIT_CASES}
PUB_SEQUENCE = ("pub_16x300", "fused_1x1", "pub_16x300", "two_130x40", "fused_17x128")
MAX_OUT_CASES = ("two_130x40", "fused_17x128")


def emit_path(S, H, W):
    """The host rule of lvx_surfel_emit_d, as far as it does not depend on the device: `fused` / `two_launch` where every part takes that path, None where the
    device decides."""
    wg = S * ((W + SE_COLS - 1) // SE_COLS)
    if H > SE_HMAX or wg > SE_MAXWG:
        return "two_launch"
    return "fused" if wg <= FUSED_SAFE_WG else None


@functools.lru_cache(maxsize=None)
def emit_inputs(name):
    """flags [S, H, W], scans_map [S, H, W, 4], raws [S, H, W] of an emission case.  Stamps: mostly non-zero; 0.0 and -0.0 (skipped); NaN (kept: 0 == NaN is false)."""
    c = EMIT_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = (c.S, c.H, c.W)
    flags = np.where(rng.random(shape) < c.density, rng.integers(0, 3000, shape), -1).astype(np.int32)
    for s in c.empty:
        flags[s] = -1
    sm = rng.standard_normal(shape + (4,)).astype(np.float32)
    raw = np.zeros(shape, POINT_XYZIT)
    for k in ("x", "y", "z", "intensity"):
        raw[k] = rng.standard_normal(shape).astype(np.float32)
    raw["pad"] = 7.0; raw["pad2"] = -7.0
    raw["timestamp"] = 100.0 + rng.random(shape)
    if c.density < 1.0:
        u = rng.random(shape)
        raw["timestamp"][u < 0.06] = 0.0
        raw["timestamp"][u < 0.03] = -0.0
        raw["timestamp"][u > 0.98] = np.nan
    for a in (flags, sm, raw):
        a.setflags(write=False)
    return flags, sm, raw


def concat_lists(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in ("pt", "pt_map", "t", "plane")}


@functools.lru_cache(maxsize=None)
def emit_expected(name):
    """(list, per-scan counts) by np_emit."""
    flags, sm, raw = emit_inputs(name)
    parts = [np_emit(flags[s], sm[s], raw[s]) for s in range(len(flags))]
    return concat_lists(parts), np.array([len(p["t"]) for p in parts], np.int32)


# ------------------------------------------------------------------------------------------------------------------------
# landmark <-> plane association past one trip of the 256-plane table (the construction of test_gpu_upstream.test_landmark_plane_association, extended)
# ------------------------------------------------------------------------------------------------------------------------
LM_PLANES = (256, 257, 600)
LM_L = 300
LM_ONLY_255, LM_ONLY_256, LM_TWO_CHUNKS, LM_FAR, LM_OUTSIDE = 5, 261, 7, 9, 11      # landmarks with a role (one of them in the second workgroup)


@functools.lru_cache(maxsize=None)
def landmark_problem():
    import synth
    P = synth.make_problem(seed=33, duration=1.5, n_surfel=50, n_planes=4, n_landmarks=LM_L, views_per_lm=1, n_camsurf=0)
    return P


def landmark_case(n_planes):
    """(P, state, q_LtoC, t_LinC, p4, bmin, bmax, want): the problem (one landmark's reference view moved outside the spline), the state (one landmark beyond 20 m), the
    plane table, and what the roles must come out as (landmark -> plane id or -1)."""
    import synth
    P = dict(landmark_problem())
    P["lm_t0"] = P["lm_t0"].copy()
    N, L = P["n_knots"], P["n_landmarks"]
    assert L == LM_L
    state = P["state_true"].copy()
    sp = synth.Spline(P["t0"], P["dt"], state[:3 * N].reshape(N, 3), state[3 * N:7 * N].reshape(N, 4))
    qC, pC = state[7 * N + 24:7 * N + 28], state[7 * N + 28:7 * N + 31]
    qL, pL = state[7 * N + 16:7 * N + 20], state[7 * N + 20:7 * N + 23]
    q_LtoC = synth.qmul(synth.qconj(qC), qL); t_LinC = synth.qrot(synth.qconj(qC), pL - pC)
    e0 = sp.eval([P["t_map"]])
    qCG0, pCG0 = synth.qmul(e0["quat"][0], qC), synth.qrot(e0["quat"][0], pC) + e0["pos"][0]
    qL0, tL0 = synth.qmul(qCG0, q_LtoC), synth.qrot(qCG0, t_LinC) + pCG0

    def in_map(l):
        ek = sp.eval([P["lm_t0"][l]])
        pc = synth._unproject(P["camera"], P["lm_uv"][l]) / state[7 * N + 32 + l]
        pG = synth.qrot(synth.qmul(ek["quat"][0], qC), pc) + synth.qrot(ek["quat"][0], pC) + ek["pos"][0]
        return synth.qrot(synth.qconj(qL0), pG - tL0)

    pM = np.array([in_map(l) for l in range(L)])
    rng = np.random.default_rng(n_planes)
    nrm = rng.standard_normal((n_planes, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    centre = np.stack([500.0 + 3.0 * np.arange(n_planes), np.full(n_planes, 500.0), np.full(n_planes, -500.0)], axis=1)      # fillers: far from every landmark
    p4 = np.concatenate([nrm, -(nrm * centre).sum(axis=1, keepdims=True)], axis=1)
    bmin, bmax = centre - 0.3, centre + 0.3

    def put(k, l, off=0.0, half=0.3):
        p4[k, 3] = -nrm[k] @ pM[l] + off; bmin[k] = pM[l] - half; bmax[k] = pM[l] + half

    roles = {LM_ONLY_255, LM_ONLY_256, LM_TWO_CHUNKS, LM_FAR, LM_OUTSIDE}
    reserved = {255, 256, 10, 200, 520, 20, 30}
    free = [k for k in range(n_planes) if k not in reserved]
    for j, l in enumerate(l_ for l_ in range(0, L, 3) if l_ not in roles):          # a surfel through every third landmark, ids spread over the whole table
        put(free[(j * 37) % len(free)], l, off=rng.uniform(-0.12, 0.12))            # some inside 2 radius = 0.1, some outside
    want = {}
    put(255, LM_ONLY_255); want[LM_ONLY_255] = 255
    if n_planes > 256:
        put(256, LM_ONLY_256); want[LM_ONLY_256] = 256
    hi = 520 if n_planes > 520 else 200
    put(10, LM_TWO_CHUNKS); put(hi, LM_TWO_CHUNKS, half=0.4); want[LM_TWO_CHUNKS] = hi      # the first and the third table chunk at 600 planes: the highest id stays
    put(20, LM_FAR); put(30, LM_OUTSIDE)
    state[7 * N + 32 + LM_FAR] = 0.04                                                # beyond 20 m: skipped
    P["lm_t0"][LM_OUTSIDE] = P["t0"] - 1.0                                          # its reference view lies outside the spline: skipped
    keep = P["rep_lm"] != LM_OUTSIDE                                                # (no reprojection factor hangs on that view: the layout would refuse the problem)
    P["rep_lm"], P["rep_uv"], P["rep_t0"] = P["rep_lm"][keep], P["rep_uv"][keep], P["rep_t0"][keep]
    want[LM_FAR] = -1; want[LM_OUTSIDE] = -1
    return P, state, q_LtoC, t_LinC, p4, bmin, bmax, want
