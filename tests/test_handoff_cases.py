"""CPU checks of tests/handoff_cases.py: every case of the surfel hand-off tests is what it claims to be (numpy, oracle.pipeline.select_surfels), and the pieces
of the feature that need no device (header, binding, host mirror option) are in place."""
import os

import numpy as np
import pytest

import handoff_cases as hc
import synth
from oracle import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", sorted(hc.SPLINES))
def test_splines_have_the_knot_counts_the_cases_name(N):
    P = hc.crafted(65, N=N)
    assert P["n_knots"] == N and P["dt"] == 0.02
    assert P["t0"] < P["t_map"] < P["t0"] + (N - 3) * P["dt"]
    assert len(P["t_imu"]) > 100 and len(P["rep_lm"]) == 0 and len(P["cs_lm"]) == 0   # IMU rows keep the normal equations of a solve step regular; no visual data


def test_row_counts_are_the_tile_edges():
    assert hc.ROW_COUNTS == (0, 1, 63, 64, 65, 257, 1025)   # nothing, one row, a wavefront -1 / +0 / +1, one 256-row tile + 1, four tiles + 1
    for n in hc.ROW_COUNTS:
        P = hc.crafted(n)
        assert P["surf_t"].shape == (n,) and P["surf_pt"].shape == (n, 3) and P["surf_plane"].shape == (n,) and P["surf_plane"].dtype == np.int32
        if n:
            assert P["surf_plane"].min() >= 0 and P["surf_plane"].max() < len(P["planes"])


@pytest.mark.parametrize("N", sorted(hc.SPLINES))
def test_time_patterns(N):
    n = 257
    Ps = {p: hc.crafted(n, pattern=p, N=N) for p in hc.PATTERNS}
    P = Ps["shuffled"]
    t0, dt, t_map = P["t0"], P["dt"], P["t_map"]
    key = {p: hc.knot_interval(Ps[p]["surf_t"], t0, dt, N) for p in hc.PATTERNS}
    # shuffled: not sorted, every time valid and behind t_map, many intervals
    t = Ps["shuffled"]["surf_t"]
    assert (np.diff(t) < 0).sum() > n // 4 and (t >= t_map).all() and key["shuffled"].min() >= 0 and len(np.unique(key["shuffled"])) >= min(N - 3, 16) - 5
    # all times in one interval, away from its ends
    assert (key["one_interval"] == N // 2).all() and (Ps["one_interval"]["surf_t"] >= t_map).all()
    # exactly on knots t0 + k dt, several different ones, all valid
    t = Ps["on_knots"]["surf_t"]
    k = np.rint((t - t0) / dt)
    assert np.array_equal(t, t0 + k * dt) and len(np.unique(k)) >= 10 and k.min() >= 1 and k.max() <= N - 4 and (t >= t_map).all()
    # the last valid interval [t0 + (N - 4) dt, t0 + (N - 3) dt)
    assert (key["last_interval"] == N - 4).all() and (Ps["last_interval"]["surf_t"] < t0 + (N - 3) * dt).all()
    # outside: rows before the spline, rows at or behind its end, rows inside
    t = Ps["outside"]["surf_t"]
    assert (t < t0).sum() >= n // 6 and (t >= t0 + (N - 3) * dt).sum() >= n // 6 and (key["outside"] >= 0).sum() >= n // 2 and (key["outside"] == -1).sum() == (t < t0).sum() + (t >= t0 + (N - 3) * dt).sum()


def test_plane_tables_and_the_bad_plane_id():
    assert len(hc.crafted(65, n_planes=1)["planes"]) == 1 and (hc.crafted(65, n_planes=1)["surf_plane"] == 0).all()
    P = hc.crafted(65, n_planes=40)
    assert len(P["planes"]) == 40 and len(np.unique(P["surf_plane"])) > 10
    B = hc.crafted(65, n_planes=40, bad_plane=True)
    assert (B["surf_plane"] == 40).sum() == 1 and B["surf_plane"][32] == 40 and np.array_equal(np.delete(B["surf_plane"], 32), np.delete(P["surf_plane"], 32))


def test_crafted_list_covers_what_the_issue_names():
    ids = [c[0] for c in hc.CRAFTED]
    assert len(set(ids)) == len(ids)
    kw = [dict(dict(n=None, pattern="shuffled", N=24, n_planes=40), **c[1]) for c in hc.CRAFTED]
    assert {k["n"] for k in kw} >= set(hc.ROW_COUNTS)
    assert {k["pattern"] for k in kw} == set(hc.PATTERNS)
    assert {k["N"] for k in kw} == {24, 300} and {k["n_planes"] for k in kw} == {1, 40}
    assert {c[2] for c in hc.CRAFTED} == {False, True} and {c[3] for c in hc.CRAFTED} == {None, 64}


def test_select_reference_is_select_surfels():
    rng = np.random.default_rng(3)
    pts = hc.association_like(1000, 10.0, 12.0, rng)
    for step in (1, 7, 10, 999, 1000, 5000):
        for t_map in (9.0, 10.7, 11.999, 13.0):
            a, b = hc.select_reference(pts, t_map, step), pipeline.select_surfels(pts, t_map, step)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for step in (0, -3):   # step <= 0 means 1
        assert all(np.array_equal(x, y) for x, y in zip(hc.select_reference(pts, 10.7, step), pipeline.select_surfels(pts, 10.7, 1)))
    assert len(hc.select_reference(pts, 9.0, 5000)[1]) == 1 and len(hc.select_reference(pts, 13.0, 10)[1]) == 0


@pytest.fixture(scope="module")
def sequence_association():
    S = synth.make_sequence(**hc.SEQ_KW)
    cloud = pipeline.deskew_into_map(S, S["state_true"])
    planes = pipeline.surfel_map(cloud, pipeline.DEFAULTS)
    return S, planes, pipeline.associate(S, cloud, planes, pipeline.DEFAULTS)


def test_sequence_of_the_from_association_case(sequence_association):
    S, planes, points = sequence_association
    assert len(S["scans"]) == 9 and S["n_knots"] == 93
    assert len(planes["p4"]) == 703 and len(points["t"]) == 8466
    t = points["t"]
    assert (np.diff(t) >= 0).all() and (t >= S["t_map"]).all()   # time-ordered, nothing before the map time
    _, t10, _ = pipeline.select_surfels(points, S["t_map"], 10)
    assert len(t10) == 847 and len(np.unique(hc.knot_interval(t10, S["t0"], S["dt"], S["n_knots"]))) == 46
    assert len(pipeline.select_surfels(points, S["t_map"], 1)[1]) == 8466
    assert len(pipeline.select_surfels(points, S["t_map"], 10000)[1]) == 1   # a step larger than the list: one row
    _, tm, _ = pipeline.select_surfels(points, S["t_map"] + hc.T_MAP_SHIFT, 10)
    assert 0 < len(tm) < 847                                               # the moved map time drops some points and keeps some
    assert len(pipeline.select_surfels(points, t[-1] + 1e-3, 10)[1]) == 0  # a map time behind the last point keeps nothing
    assert S["t_map"] + hc.T_MAP_SHIFT + 0.01 < S["t0"] + (S["n_knots"] - 3) * S["dt"]   # the moved map time is still a valid hub time


def test_c_abi_python_binding_and_host_mirror_name_the_hand_off():
    hdr = open(os.path.join(ROOT, "include", "lvx.h")).read()
    for name in ("lvx_set_planes_d", "lvx_set_surfel_d", "lvx_set_surfel_from_association"):
        assert ("int %s(lvx_ctx*" % name) in hdr
    import lvx
    assert callable(lvx.Context.set_planes_d) and callable(lvx.Context.set_surfel_d) and callable(lvx.set_surfel_from_association)
    mirror = open(os.path.join(ROOT, "lvi-exc_amd", "host", "lvx_calibrate.hpp")).read()
    assert "bool device_handoff = false;" in mirror and "lvx_set_surfel_from_association(ctx_" in mirror
