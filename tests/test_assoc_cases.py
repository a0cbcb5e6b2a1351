"""CPU: holds the association and emission cases of tests/assoc_cases.py to the regime each one claims — computed from the numpy hit sets alone — and the oracle
(oracle/orc_upstream.cpp) to the numpy restatements np_assoc / np_emit, which do not rest on it.  Wrong variants of the rule (another step, another threshold, < radius,
lowest id wins, closed boxes, row-major emission, a zero timestamp kept) must each differ from the oracle on some case: a variant no case catches means a case is
missing.  tests/test_gpu_assoc_shapes.py then runs the same cases through the C ABI."""
import numpy as np
import pytest

import assoc_cases as AC
from oracle import oracle as O

FLAG_NAMES = [c.name for c in AC.CASES]


def test_case_table_is_the_one_asked_for():
    shapes = {c.name: (c.H, c.W, c.P, c.sel, c.radius) for c in AC.CASES}
    for sel in (1, 2, 3, 5):
        assert shapes["sel%d" % sel] == (4, 320, 20, sel, 0.05)
    assert shapes["word_edges"][:2] == (4, 320)
    assert [(c.H, c.W) for c in AC.CASES if c.group == "widths"] == [(3, 1), (3, 31), (3, 33), (5, 100), (3, 2048), (3, 2049), (3, 2080), (3, 4095)]
    assert shapes["h1"][:2] == (1, 300) and shapes["h130"][:2] == (130, 40)
    assert [(c.H, c.W, c.P) for c in AC.CASES if c.group == "planes"] == [(2, 128, P) for P in (255, 256, 257, 513)]
    assert shapes["overlap"][2] == 320
    assert [c.name for c in AC.CASES if c.group == "grid_edges"] == ["grid_p1", "grid_empty", "grid_far", "grid_bounds", "grid_outside", "grid_nonfinite"]
    assert shapes["radius_le"][4] == 0.25 and shapes["radius_zero"][4] == 0.0
    assert shapes["chunks"][:3] == (2, 64, 8) and AC.CHUNK_BATCHES == (66, 67, 130)
    assert shapes["hygiene_a"] == shapes["hygiene_b"] and np.array_equal(AC.BY_NAME["hygiene_a"].bmin, AC.BY_NAME["hygiene_b"].bmin)
    for c in AC.CASES:      # small: the smallest shapes at which each branch is still taken
        assert c.W <= AC.SA_WMAX and (c.H <= 5 or c.name == "h130") and (c.P <= 48 or c.group in ("planes", "overlap")), c
    assert AC.BATCHES == (1, 2, 3) and "chunks" not in AC.PARITY and len(AC.PARITY) == len(AC.CASES) - 1


@pytest.mark.parametrize("name", FLAG_NAMES)
def test_numpy_restatement_equals_the_oracle(name):
    c = AC.BY_NAME[name]
    for i in range(3):          # the three scans of the largest batch (another seed each)
        want = AC.np_assoc(c.scan(i), c.p4, c.bmin, c.bmax, c.radius, c.sel)
        assert np.array_equal(AC.oracle_flags(name, i), want), i
        assert (want >= 0).any() != c.none, i                       # at least one flag, unless the case exists to have none
        assert i == 0 or not np.array_equal(c.scan(i), c.scan(0), equal_nan=True)


def test_chunk_batches_equal_the_oracle_scan_by_scan():
    c = AC.BY_NAME["chunks"]
    seen = set()
    for i in range(max(AC.CHUNK_BATCHES)):
        want = AC.np_assoc(c.scan(i), c.p4, c.bmin, c.bmax, c.radius, c.sel)
        assert np.array_equal(AC.oracle_flags("chunks", i), want) and (want >= 0).any()
        seen.add(want.tobytes())
    assert len(seen) == max(AC.CHUNK_BATCHES)      # every scan of a batch selects other columns: a scan written to another scan's place shows


def test_scans_of_a_batch_select_differently():
    """S = 2 and S = 3 index the scans through blockIdx.z / blockIdx.y: in these cases a result taken from or written to the wrong scan cannot pass."""
    for name in ("sel1", "sel2", "sel3", "sel5", "word_edges", "w5x100", "w2048", "w4095", "h130"):
        assert len({AC.oracle_flags(name, i).tobytes() for i in range(3)}) == 3, name


def _selected(name, i=0):
    h, w = np.nonzero(AC.np_assoc(*_args(name, i)) >= 0)
    return h, w


def _args(name, i=0):
    c = AC.BY_NAME[name]
    return c.scan(i), c.p4, c.bmin, c.bmax, c.radius, c.sel


@pytest.mark.parametrize("sel", [1, 2, 3, 5])
def test_sel_cases_sit_on_the_threshold(sel):
    name = "sel%d" % sel
    counts = set(AC.ring_counts(AC.hits_of(name)).tolist())
    assert {2 * sel - 1, 2 * sel, 2 * sel + 1, 3 * sel + 2} <= counts      # none; the threshold exactly; step 1 just above it; step > 1
    assert (3 * sel + 2) // (sel + 1) > 1 and (2 * sel + 1) // (sel + 1) == 1
    assert max(counts) > 128 and AC.word_occupancy(AC.hits_of(name)).sum(axis=2).max() == 5      # a run over five mask words
    _, w = _selected(name)
    assert (w % 32 == 0).any() and (w % 32 == 31).any()


def test_word_edges_are_reached():
    hits = AC.hits_of("word_edges")
    h, w = _selected("word_edges")
    assert (w % 32 == 0).any() and (w % 32 == 31).any()
    assert (w == 0).any() and hits[..., 0].any() and hits[..., 319].any()          # runs from column 0 and to column W - 1
    assert hits[1, 0, 30:35].all() and not hits[1, 0, 29] and not hits[1, 0, 35]     # columns 30-34: across the boundary of words 0 and 1
    assert {30, 31} <= set(w[h == 0].tolist())
    run = hits[8, 2]                                                                # ring 2, columns 200 .. 215 with a NaN gap in the middle
    assert run[200:204].all() and not run[204:210].any() and run[210:216].all() and run.sum() == 10
    assert set(w[h == 2].tolist()) >= {202, 211}                                    # ranks 3 and 6 of that list lie on both sides of the gap
    alt = hits[9, 2, 232:251]
    assert alt[0::2].all() and not alt[1::2].any()                                  # the lanes of one word are not contiguous
    assert (AC.word_occupancy(hits).sum(axis=2) >= 2).sum() >= 5


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.group == "widths"])
def test_width_cases_are_in_their_regime(name):
    c = AC.BY_NAME[name]
    hits, occ = AC.hits_of(name), AC.word_occupancy(AC.hits_of(name))
    wpr, oshift = AC.wpr_of(c.W), AC.oshift_of(c.W)
    assert occ.shape[2] == wpr
    if name in AC.WIDE:
        assert (wpr, oshift) == AC.WIDE[name]
        assert occ[..., wpr - 1].any()                                              # hits in the last word
        assert hits[..., c.W - 1].any()
    else:
        assert oshift == 0 and wpr <= 4
    if name == "w2048":
        assert wpr == 64 and occ[..., 63].any()                                     # occupancy bit 63
    if oshift:
        pairs = np.zeros(occ.shape[:2] + (2 * ((wpr + 1) // 2),), bool)
        pairs[..., :wpr] = occ
        even, odd = pairs[..., 0::2], pairs[..., 1::2]
        assert (even & odd).any() and (odd & ~even).any()                           # both words of an occupancy pair; the odd word alone
        assert (wpr % 2 == 1) == (name in ("w2049", "w2080"))                       # an unpaired last word
        assert (c.W % 32 != 0) == (name in ("w2049", "w4095"))                       # a partial last word
    if name == "w5x100":
        assert c.H * c.W == 500 and c.H * c.W % 256 != 0 and c.W % 64 != 0           # two workgroups, the second partly idle; a wavefront spans two rings
        assert hits[:, :, 90:].any() and hits[:, :, :10].any()
    if name == "w1":
        assert hits.any() and AC.ring_counts(hits).max() == 1
    if name == "w33":
        assert occ[..., 1].any() and hits[..., 32].any()
    _, w = _selected(name)
    if name in ("w2080", "w4095"):
        assert (w >= 32 * (wpr - 1)).any()                                          # a column selected in the last word


def test_ring_and_plane_count_cases_are_in_their_regime():
    assert AC.BY_NAME["h1"].H == 1 and AC.BY_NAME["h130"].H == 130
    h, _ = _selected("h130")
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= set(h.tolist())
    for P in (255, 256, 257, 513):
        f = AC.np_assoc(*_args("planes%d" % P))
        ids = set(f[f >= 0].tolist())
        assert P - 1 in ids and len(ids) > 20                                       # the last plane
        if P > 256:
            assert 256 in ids and (P - 1) % AC.SA_PC == 0                           # plane 256: the first of the second chunk; the last plane alone in its chunk
        assert {p % AC.SA_PC for p in (255, 256, 257, 513)} == {255, 0, 1}          # LDS chunk tails of 255 and 1 planes, and none
    f = AC.np_assoc(*_args("planes513"))
    assert 255 in f and 256 in f and f[0, 103] == 256 and f[0, 101] == 255          # the shared column goes to the higher id


def test_overlap_highest_id_wins():
    c = AC.BY_NAME["overlap"]
    assert all(np.array_equal(c.bmin[k], c.bmin[3]) and np.array_equal(c.bmax[k], c.bmax[3]) for k in (200, 300))
    assert 3 // AC.SA_PC != 300 // AC.SA_PC                                         # in two plane chunks: two workgroups race for the flag
    f = AC.np_assoc(*_args("overlap"))
    assert set(f[0][f[0] >= 0].tolist()) == {300}
    assert f[1, 21] == 5 and f[1, 23] == 150 and f[1, 25] == 150
    hits = AC.hits_of("overlap")
    assert (hits[5] & hits[150]).any() and (hits[5] ^ hits[150]).any()


def test_grid_edge_cases_are_in_their_regime():
    assert AC.BY_NAME["grid_p1"].P == 1
    c = AC.BY_NAME["grid_empty"]
    empty = (c.bmin >= c.bmax).any(axis=1)
    assert empty.sum() == 3 and (c.bmin >= c.bmax)[empty].sum(axis=0).tolist() == [1, 1, 1]      # lo >= hi once in every axis
    assert not AC.hits_of("grid_empty")[empty].any() and AC.hits_of("grid_empty")[~empty].any()
    c = AC.BY_NAME["grid_far"]
    lo, hi = c.bmin.min(axis=0), c.bmax.max(axis=0)
    cells = np.floor((c.bmax[:-1] - lo) * (np.array([64, 64, 8]) / (hi - lo)))
    assert (cells == 0).all() and (c.P - 1) % 2 == 1 and c.bmin[-1].min() >= 1000.0       # the others share cell 0: an odd list length, two candidates per trip
    c = AC.BY_NAME["grid_bounds"]
    s = c.scan(0)
    lo, hi = c.bmin.min(axis=0), c.bmax.max(axis=0)
    assert s[0, 0, 0] == lo[0] and s[2, 99, 0] == hi[0] and s[0, 43, 1] == lo[1] and s[2, 50, 1] == hi[1]      # points exactly on the smallest lo and the largest hi
    hits = AC.hits_of("grid_bounds")
    assert not hits[:, 0, 0].any() and not hits[:, 2, 99].any() and not hits[:, 0, 43].any() and not hits[:, 2, 50].any() and not hits[:, 2, 51].any()
    assert hits[0, 0, 1:5].all() and hits[2, 2, 95:99].all() and hits[0].sum() == 4 and hits[2].sum() == 4
    c = AC.BY_NAME["grid_outside"]
    s = c.scan(0)
    lo, hi = c.bmin.min(axis=0), c.bmax.max(axis=0)
    out = ((s[..., :3] < lo) | (s[..., :3] > hi)).any(axis=2)
    assert out[0, 10:16].all() and not AC.hits_of("grid_outside")[:, out].any()
    assert AC.hits_of("grid_outside")[3, 2, 6]                                      # a hit by x, far from its column's place
    s = AC.BY_NAME["grid_nonfinite"].scan(0)
    assert np.isnan(s[0, 10, 1]) and np.isnan(s[0, 12, 2]) and not np.isnan(s[0, 10, 0]) and np.isposinf(s[1, 30, 0]) and np.isneginf(s[1, 32, 0])
    assert not AC.hits_of("grid_nonfinite")[:, ~np.isfinite(s[..., :3]).all(axis=2)].any()


def test_radius_edges_are_on_the_radius():
    z = AC.RADIUS_Z
    assert z.dtype == np.float32 and float(z[0]) == 0.25 and float(z[1]) == -0.25 and float(z[2]) > 0.25 and float(z[2]) - 0.25 < 1e-7
    hits = AC.hits_of("radius_le")
    assert hits[0, 0, 10:16].tolist() == [True, True, False, True, True, True]      # 0.25 and -0.25 hit, the next float above misses
    assert AC.BY_NAME["radius_zero"].radius == 0.0
    hits = AC.hits_of("radius_zero")
    assert hits[0, 0, 10:14].all() and hits[0].sum() == 4 and hits[1].sum() == 6


def test_chunk_sizes_are_as_stated():
    assert AC.chunk_sizes(66) == [(64, "grid"), (2, "allpairs")]
    assert AC.chunk_sizes(67) == [(64, "grid"), (3, "grid")]
    assert AC.chunk_sizes(130) == [(64, "grid"), (64, "grid"), (2, "allpairs")]
    assert [AC.chunk_sizes(S) for S in AC.BATCHES] == [[(1, "allpairs")], [(2, "allpairs")], [(3, "grid")]]


def test_hygiene_first_call_leaves_bits_that_would_show():
    a, b = AC.hits_of("hygiene_a"), AC.hits_of("hygiene_b")
    sel = AC.BY_NAME["hygiene_a"].sel
    ca, cb = a.sum(axis=2), b.sum(axis=2)
    assert ((ca > 0) & (ca < 2 * sel)).sum() >= 18 and (ca >= 2 * sel).sum() == 2    # most rings are cleared without being selected
    assert not (a & b)[:18].any()                                                   # other columns in the second call: a stale bit is not hidden behind a fresh one
    stale = AC.np_select(a | b, sel)
    assert not np.array_equal(stale, AC.np_select(b, sel))


# the wrong variants of the rule: each must differ from the oracle on at least one case
VARIANTS = {
    "step = c // sel": dict(AC.RIGHT, step=lambda c, sel: max(c // sel, 1)),
    "threshold c > 2 sel": dict(AC.RIGHT, enough=lambda c, sel: c > 2 * sel),
    "< radius": dict(AC.RIGHT, near=lambda d, r: d < r),
    "lowest id wins": dict(AC.RIGHT, ascending=False),
    "box test >= / <=": dict(AC.RIGHT, inside=lambda v, lo, hi: (v >= lo) & (v <= hi)),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_table_catches_a_wrong_flag_rule(variant):
    caught = [c.name for c in AC.CASES if not np.array_equal(AC.np_assoc(*_args(c.name), rules=VARIANTS[variant]), AC.oracle_flags(c.name))]
    print(variant, "caught by", caught)
    assert caught
    if variant == "< radius":
        assert "radius_le" in caught and "radius_zero" in caught
    if variant == "box test >= / <=":
        assert "grid_bounds" in caught
    if variant == "lowest id wins":
        assert "overlap" in caught and "planes513" in caught
    if variant in ("step = c // sel", "threshold c > 2 sel"):
        assert {"sel1", "sel2", "sel3", "sel5"} <= set(caught)


# ------------------------------------------------------------------------------------------------------------------------
# emission
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in AC.EMIT_CASES])
def test_emission_case_equals_the_oracle_and_takes_its_path(name):
    c = AC.EMIT_BY_NAME[name]
    flags, sm, raw = AC.emit_inputs(name)
    assert flags.shape == (c.S, c.H, c.W)
    want, counts = AC.emit_expected(name)
    got = AC.concat_lists([O.surfel_emit(flags[s], sm[s], raw[s]) for s in range(c.S)])
    assert AC.same_list(got, want)
    assert AC.emit_path(c.S, c.H, c.W) == c.path                                    # on any device: from n_scans * ceil(W / 128) and H alone
    assert counts.sum() > 0 and all(counts[s] == 0 for s in c.empty) and all(counts[s] > 0 for s in range(min(c.S, 5)) if s not in c.empty)
    if c.density < 1.0:
        ts = raw["timestamp"][flags != -1]
        assert (ts == 0).any() and np.signbit(ts[ts == 0]).any() and not np.signbit(ts[ts == 0]).all() and np.isnan(ts).any()      # 0.0 and -0.0 skipped, NaN kept
        assert np.isnan(want["t"]).sum() == np.isnan(ts).sum() and not (want["t"] == 0).any()
    else:
        assert counts.sum() == c.S * c.H * c.W - len(c.empty) * c.H * c.W


def test_emission_shapes_are_the_ones_asked_for():
    two = {(c.S, c.H, c.W) for c in AC.EMIT_CASES if c.path == "two_launch"}
    assert two == {(3, 130, 40), (2, 200, 9), (2049, 1, 8), (1100, 2, 130)}
    assert 130 * 40 > 1024 and 2049 > 1024 and 2049 > AC.SE_MAXWG and 1100 * 2 > AC.SE_MAXWG and 200 > AC.SE_HMAX
    fused = [(c.S, c.H, c.W) for c in AC.EMIT_CASES if c.path == "fused" and c.empty]
    assert fused == [(5, H, W) for H, W in ((1, 1), (15, 127), (17, 128), (64, 129), (65, 300), (100, 40), (128, 129))]
    assert all(c.empty == (1, 3) for c in AC.EMIT_CASES if c.path == "fused" and c.S == 5)
    assert AC.EMIT_BY_NAME["fused_full"][1:5] == (2, 128, 129, 1.0) and AC.EMIT_BY_NAME["pub_16x300"][1:4] == (16, 16, 300)
    for c in AC.EMIT_CASES:
        if c.path == "fused":
            assert c.S * -(-c.W // AC.SE_COLS) <= AC.FUSED_SAFE_WG and c.H <= AC.SE_HMAX      # never a launch meant to exceed the residency
    assert [AC.EMIT_BY_NAME[n].path for n in AC.PUB_SEQUENCE] == ["fused", "fused", "fused", "two_launch", "fused"]
    assert sorted(AC.EMIT_BY_NAME[n].path for n in AC.MAX_OUT_CASES) == ["fused", "two_launch"]


@pytest.mark.parametrize("kw", [dict(column_major=False), dict(skip_zero=False)])
def test_the_table_catches_a_wrong_emission_rule(kw):
    caught = []
    for c in AC.EMIT_CASES:
        flags, sm, raw = AC.emit_inputs(c.name)
        wrong = AC.concat_lists([AC.np_emit(flags[s], sm[s], raw[s], **kw) for s in range(c.S)])
        if not AC.same_list(wrong, AC.emit_expected(c.name)[0]):
            caught.append(c.name)
    print(kw, "caught by", caught)
    assert len(caught) >= 8


# ------------------------------------------------------------------------------------------------------------------------
# landmark <-> plane
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_planes", AC.LM_PLANES)
def test_landmark_case_is_past_one_table_trip(n_planes):
    import lvx
    P, state, q_LtoC, t_LinC, p4, bmin, bmax, want = AC.landmark_case(n_planes)
    o = O.Oracle(); lvx.load_problem(o, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    ro = O.landmark_assoc(o, state, q_LtoC, t_LinC, P["t_map"], p4, bmin, bmax, 0.05)
    L = P["n_landmarks"]
    assert len(p4) == n_planes and L >= 257 and len(ro) == L
    for l, k in want.items():
        assert ro[l] == k, (l, k, ro[l])
    won = ro[ro >= 0]
    assert (won < 256).any() and ((won >= 256).any() or n_planes == 256) and len(set(won.tolist())) >= 30      # winners on both sides of 256
    assert (ro[256:] >= 0).any() and (ro[:256] >= 0).any() and (ro == -1).sum() >= L // 2                       # in both workgroups; the second one has idle threads
    assert L % 256 != 0 and AC.LM_ONLY_256 >= 256
    N = P["n_knots"]
    assert state[7 * N + 32 + AC.LM_FAR] < 0.05 and P["lm_t0"][AC.LM_OUTSIDE] < P["t0"]
    if n_planes == 600:
        assert want[AC.LM_TWO_CHUNKS] // 256 == 2                                   # hits in the first and in the third chunk: the highest id stays
    # the boxes of the far landmark and of the one outside the spline would hold them: it is the rule that skips them
    state2 = state.copy(); state2[7 * N + 32 + AC.LM_FAR] = AC.landmark_problem()["state_true"][7 * N + 32 + AC.LM_FAR]
    assert O.landmark_assoc(o, state2, q_LtoC, t_LinC, P["t_map"], p4, bmin, bmax, 0.05)[AC.LM_FAR] == 20
