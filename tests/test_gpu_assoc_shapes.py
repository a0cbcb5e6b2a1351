"""GPU: the scan-to-surfel association, the SurfelPoint emission and the landmark <-> plane association at the shapes of tests/assoc_cases.py
(tests/test_assoc_cases.py holds each case to its regime on the CPU), through the C ABI, bit for bit against the oracle and the numpy restatements.  Everything compared
is an integer or a copied double: no tolerances.

Reached here and by no older test: sel_per_ring 1 / 3 / 5 and radius 0 / 0.25; widths 1, 31, 33 and 64 / 65 / 128 mask words per ring (oshift 0 and 1, an unpaired and a
partial last word); H = 1 and 130; H W below and across 256; LDS plane chunks with tails of 255 and 1; batches of 66 / 67 / 130 scans (a grid chunk followed by an all-pairs
chunk, the work buffer re-shaped in between); k_assoc_emit on the device at all (H > 128, more than 2 048 workgroups, more than 1 024 scans); k_assoc_emit_fused at
H = 1 .. 128 and odd widths, with empty scans between full ones; max_out smaller than the list on both paths; k_landmark_assoc past one trip of its plane table and past
one workgroup."""
import ctypes as C

import numpy as np
import pytest

import assoc_cases as AC
import lvx
from oracle import oracle as O

pytestmark = pytest.mark.gpu

UNTOUCHED = 1 << 30      # what the flag buffer holds before a call: no plane id, not -1


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _assoc(ctx, scans, p4, bmin, bmax, radius, sel, prepare):
    """lvx_surfel_assoc_batch_d on device-resident scans [S, H, W, 4]; prepare: against a grid built once by lvx_surfel_map_prepare_d."""
    import torch
    dev = torch.device("cuda", 0)
    scans = np.ascontiguousarray(scans, np.float32)
    S, H, W, P = scans.shape[0], scans.shape[1], scans.shape[2], len(p4)
    sc = torch.from_numpy(scans).to(dev)
    pl = torch.from_numpy(np.concatenate([np.asarray(a, np.float64).ravel() for a in (p4, bmin, bmax)] + [np.zeros(1)])).to(dev)
    fl = torch.full((S * H * W,), UNTOUCHED, dtype=torch.int32, device=dev)
    l = ctx._l
    if prepare:
        ctx._ck(l.lvx_surfel_map_prepare_d(ctx._h, C.c_int(P), C.c_void_p(pl.data_ptr())))
    try:
        ctx._ck(l.lvx_surfel_assoc_batch_d(ctx._h, C.c_int(S), C.c_int(H), C.c_int(W), C.c_void_p(sc.data_ptr()), C.c_int(P), C.c_void_p(pl.data_ptr()), C.c_double(radius), C.c_int(sel),
                                           C.c_void_p(fl.data_ptr())))
        ctx.synchronize()
    finally:
        l.lvx_surfel_map_release(ctx._h)
    return fl.cpu().numpy().reshape(S, H, W)


def _run_case(ctx, name, S, prepare, first=0):
    c = AC.BY_NAME[name]
    got = _assoc(ctx, c.scans(S, first), c.p4, c.bmin, c.bmax, c.radius, c.sel, prepare)
    for i in range(S):
        assert np.array_equal(got[i], AC.oracle_flags(name, first + i)), (name, S, prepare, i)
    return got


@pytest.mark.parametrize("name", AC.PARITY)
def test_flag_case_is_exact_on_all_three_paths(ctx, name):
    """S = 1: all pairs; S = 2: all pairs with blockIdx.z = 1; S = 3: the grid.  With the grid built by the call and built beforehand.  Every scan of a batch comes from
    another seed and must equal the oracle run on it alone."""
    c = AC.BY_NAME[name]
    for prepare in (False, True):
        for S in AC.BATCHES:
            got = _run_case(ctx, name, S, prepare)
            assert (got >= 0).any() != c.none
    assert np.array_equal(got[0], AC.np_assoc(c.scan(0), c.p4, c.bmin, c.bmax, c.radius, c.sel))      # the check that does not rest on the oracle


def test_batches_past_one_chunk_on_one_context(ctx):
    """66 = 64 + 2 scans (a grid chunk, then an all-pairs chunk of two: the work buffer is re-shaped in between), 67 = 64 + 3, 130 = 64 + 64 + 2; each call followed at
    once by the same call again."""
    for S in AC.CHUNK_BATCHES:
        for prepare in (False, True):
            for _ in range(2):
                _run_case(ctx, "chunks", S, prepare)


@pytest.mark.parametrize("S", AC.BATCHES)
def test_work_buffer_is_left_clean(S):
    """Two calls of one shape on one context: in the first most rings have fewer than 2 sel hits and are cleared without being selected; a bit left behind would
    change the step of the second call's rings (other columns there)."""
    c = lvx.Context(0)
    try:
        for prepare in (False, True):
            _run_case(c, "hygiene_a", S, prepare)
            _run_case(c, "hygiene_b", S, prepare)
    finally:
        c.close()


def test_argument_checks(ctx):
    c = AC.BY_NAME["grid_p1"]
    wide = np.zeros((1, 1, AC.SA_WMAX + 1, 4), np.float32)
    with pytest.raises(lvx.LvxError) as e:
        _assoc(ctx, wide, c.p4, c.bmin, c.bmax, 0.05, 2, False)
    assert e.value.code == lvx.E_ARG
    with pytest.raises(lvx.LvxError) as e:
        lvx.surfel_assoc(ctx, wide[0], c.p4, c.bmin, c.bmax, 0.05, 2)
    assert e.value.code == lvx.E_ARG
    for S in (1, 3):        # no planes: -1 everywhere
        got = _assoc(ctx, c.scans(S), c.p4[:0], c.bmin[:0], c.bmax[:0], 0.05, 2, False)
        assert (got == -1).all()
    _run_case(ctx, "grid_p1", 3, False)


# ------------------------------------------------------------------------------------------------------------------------
# emission
# ------------------------------------------------------------------------------------------------------------------------
def _emit(ctx, name):
    flags, sm, raw = AC.emit_inputs(name)
    want, counts = AC.emit_expected(name)
    got = lvx.surfel_emit(ctx, flags, sm, raw)
    assert got["n"] == len(want["t"]) and np.array_equal(got["counts"], counts), name
    assert AC.same_list(got, want), name


@pytest.mark.parametrize("name", [c.name for c in AC.EMIT_CASES])
def test_emission_case_is_bit_equal(ctx, name):
    """Synthetic flags straight into lvx_surfel_emit_d.  two_*: H > 128 or more workgroups than publication words — k_assoc_emit (count, then write) on any device;
    fused_* / pub_*: at most 64 workgroups and H <= 128 — k_assoc_emit_fused on any part with 64 CUs."""
    _emit(ctx, name)


def test_publication_words_are_restamped_not_cleared():
    """One context: 48 workgroups publish, then 1, then the 48 again (their words still hold the first launch's counts under an older epoch); then a two-launch call
    (which does not touch the words) followed by a fused one."""
    c = lvx.Context(0)
    try:
        for name in AC.PUB_SEQUENCE:
            _emit(c, name)
    finally:
        c.close()


SENTINEL_D, SENTINEL_I = -12345.678, -77


@pytest.mark.parametrize("name", AC.MAX_OUT_CASES)
def test_max_out_smaller_than_the_list(ctx, name):
    """*n_out and the per-scan counts are those of the whole list whatever max_out is; nothing at or beyond max_out is written; with max_out >= total the list is the
    one of np_emit.  (Below max_out, a list that does not fit is unspecified.)"""
    import torch
    dev = torch.device("cuda", 0)
    flags, sm, raw = AC.emit_inputs(name)
    want, counts = AC.emit_expected(name)
    total = len(want["t"])
    assert total > 64
    cap = total + 64
    for max_out in (total, total - 1, 1, total + 10):
        out = dict(pt=torch.full((3 * cap,), SENTINEL_D, dtype=torch.float64, device=dev), pt_map=torch.full((3 * cap,), SENTINEL_D, dtype=torch.float64, device=dev),
                   t=torch.full((cap,), SENTINEL_D, dtype=torch.float64, device=dev), plane=torch.full((cap,), SENTINEL_I, dtype=torch.int32, device=dev))
        r = lvx.surfel_emit(ctx, flags, sm, raw, max_out=max_out, out=out)
        assert r["n"] == total and np.array_equal(r["counts"], counts), max_out
        host = {k: v.cpu().numpy() for k, v in out.items()}
        n = min(max_out, total)
        assert (host["pt"][3 * n:] == SENTINEL_D).all() and (host["pt_map"][3 * n:] == SENTINEL_D).all() and (host["t"][n:] == SENTINEL_D).all() and (host["plane"][n:] == SENTINEL_I).all(), max_out
        if max_out >= total:
            got = dict(pt=host["pt"][:3 * total].reshape(-1, 3), pt_map=host["pt_map"][:3 * total].reshape(-1, 3), t=host["t"][:total], plane=host["plane"][:total])
            assert AC.same_list(got, want), max_out
    r = lvx.surfel_emit(ctx, flags, sm, raw, max_out=0, out=None)      # NULL outputs: the count alone
    assert r["n"] == total and np.array_equal(r["counts"], counts)


# ------------------------------------------------------------------------------------------------------------------------
# landmark <-> plane
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_planes", AC.LM_PLANES)
def test_landmark_association_past_one_table_trip(ctx, n_planes):
    """300 landmarks (two workgroups, the second with idle threads that still load the table) against 256 / 257 / 600 planes (one table trip exactly, a tail of one,
    three trips): exactly the oracle's result; the roles of assoc_cases.landmark_case come out as stated."""
    P, state, q_LtoC, t_LinC, p4, bmin, bmax, want = AC.landmark_case(n_planes)
    o = O.Oracle(); lvx.load_problem(o, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    lvx.load_problem(ctx, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    ro = O.landmark_assoc(o, state, q_LtoC, t_LinC, P["t_map"], p4, bmin, bmax, 0.05)
    rg = lvx.landmark_assoc(ctx, state, q_LtoC, t_LinC, P["t_map"], p4, bmin, bmax, 0.05)
    assert np.array_equal(rg, ro)
    for l, k in want.items():
        assert rg[l] == k, (l, k)
    assert (rg[256:] >= 0).any() and (rg[rg >= 0] < 256).any() and ((rg >= 256).any() or n_planes == 256)
