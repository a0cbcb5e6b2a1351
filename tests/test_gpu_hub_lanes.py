"""GPU: the hub block of k_clear — the pose at t_map of each hub set and its hub_matrix, evaluated by one WAVEFRONT per set (lvx_resid.h: hub_lanes_pairs / hub_lanes_coefs / hub_lanes_knots /
hub_lanes_matrix; the host program tests/native/hub_lanes_host_check.cpp holds the split against pose_eval + hub_matrix value for value).  Here every status and both
instantiations reach the caller: surfel set alone, camera-surfel set alone, both; t_map inside an interval and 5 us on either side of a knot; sensor time offsets locked and
free (lock mask 0: the hub carries velocity and angular velocity); a non-unit hub control point; the hub's time outside its segment and t_map outside the spline; DETERMINISTIC.

Problems of about 40 knots and 300 surfel rows; helpers and bars of tests/test_gpu_fold_chain.py / tests/fold_chain_cases.py (tests/test_gpu_time_layouts.py::_check: cost 1e-12,
residuals 1e-11, H and g 1e-10 of their maxima, block-scaled H).  Each case is held against the oracle on the first pass and on its replay; the oracle runs once per case."""
import functools

import numpy as np
import pytest

import fold_chain_cases as FC
import lvx
import synth
from oracle import oracle as O
from test_gpu_time_layouts import _check, _context

pytestmark = pytest.mark.gpu

CASES = {  # name: (sets, t_map relative to knot 12 in seconds or None (as drawn: mid-interval), locks)
    "both": ("both", None, FC.TAU),
    "surfel_only": ("surfel", None, FC.TAU),
    "camsurf_only": ("camsurf", None, FC.TAU),
    "both_offsets_free": ("both", None, 0),
    "surfel_only_offsets_free": ("surfel", None, 0),
    "behind_knot": ("both", 5e-6, FC.TAU),
    "before_knot": ("both", -5e-6, FC.TAU),
    "before_knot_offsets_free": ("both", -5e-6, 0),
}


def _small():
    return synth.make_problem(seed=4, duration=0.4, n_surfel=300, n_planes=8, n_landmarks=8, n_camsurf=6)


@functools.lru_cache(maxsize=None)
def _case(name):
    sets, dt_map, locks = CASES[name]
    P = _small()
    if sets == "surfel":
        P = dict(P); P.update(cs_lm=P["cs_lm"][:0], cs_plane=P["cs_plane"][:0])
    elif sets == "camsurf":
        P = dict(P); P.update(surf_pt=P["surf_pt"][:0], surf_t=P["surf_t"][:0], surf_plane=P["surf_plane"][:0])
    if dt_map is not None:
        P = FC._move_tmap(P, P["t0"] + FC.HUB_KNOT * P["dt"] + dt_map, False)
    s = P["state0"].copy(); s.setflags(write=False)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    return P, s, locks, o.evaluate(s, normal_eq=True)


def test_problem_size():
    P = _small()
    assert 38 <= P["n_knots"] <= 46 and len(P["surf_t"]) == 300 and len(P["cs_lm"]) > 0
    assert int(np.floor((P["t_map"] - P["t0"]) / P["dt"])) == FC.HUB_KNOT and 0.2 < (P["t_map"] - P["t0"]) / P["dt"] - FC.HUB_KNOT < 0.8


@pytest.mark.parametrize("name", list(CASES))
def test_hub_pose_against_the_oracle_first_pass_and_replay(name):
    P, s, locks, ro = _case(name)
    g = _context(P, locks)
    try:
        for label in ("first", "replay"):
            lo = _check(name, label, g.evaluate(s, normal_eq=True), ro, g)
            assert lo["exact_fallback"] == 0
    finally:
        g.close()


@pytest.mark.parametrize("name", ["both", "before_knot_offsets_free"])
def test_deterministic_bits(name):
    P, s, locks, ro = _case(name)
    g = _context(P, locks, det=True)
    try:
        a = g.evaluate(s, normal_eq=True)
        _check(name, "deterministic", a, ro, g)
        b = g.evaluate(s, normal_eq=True)
    finally:
        g.close()
    assert b["cost"] == a["cost"] and np.array_equal(b["H"], a["H"]) and np.array_equal(b["g"], a["g"])


def test_nonunit_hub_control_point():
    """Only the hub evaluates the scaled control point (the construction of fold_chain_cases.nonunit_hub_case on the small problem): -RES_NONUNIT reaches the caller."""
    P = dict(_small())
    far = P["surf_t"] > P["t_map"] + 8 * P["dt"]
    P.update(t_imu=P["t_imu"][:0], gyro=P["gyro"][:0], acc=P["acc"][:0], rep_lm=P["rep_lm"][:0], rep_uv=P["rep_uv"][:0], rep_t0=P["rep_t0"][:0],
             cs_lm=P["cs_lm"][:0], cs_plane=P["cs_plane"][:0], surf_pt=P["surf_pt"][far], surf_t=P["surf_t"][far], surf_plane=P["surf_plane"][far])
    N = P["n_knots"]
    assert far.sum() > 50
    for k in range(FC.HUB_KNOT, FC.HUB_KNOT + 4):                         # each of the hub's four control points: every pair's lane must report
        s = P["state0"].copy()
        s[3 * N + 4 * k:3 * N + 4 * k + 4] *= 1.01
        g = lvx.Context(0)
        try:
            lvx.load_problem(g, P, FC.TAU)
            with pytest.raises(lvx.LvxError) as ei:
                g.evaluate(s, normal_eq=True)
            assert ei.value.code == lvx.E_NONUNIT_QUAT, k
            r = g.evaluate(P["state0"], normal_eq=True)                   # and the context recovers on a unit state
            assert np.isfinite(r["cost"]) and r["cost"] > 0
        finally:
            g.close()


def test_hub_time_outside():
    """The hub's evaluation time t_map + offset outside its four-knot segment (a locked LiDAR offset of 30 ms in the state): the hub reports ok = 0 and every row a range
    error; t_map outside the spline is refused with the same code before any kernel runs."""
    P, s, locks, _ = _case("surfel_only")
    N = P["n_knots"]
    bad = s.copy(); bad[7 * N + 16 + 7] = 0.03
    g = _context(P, locks)
    try:
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(bad, normal_eq=True)
        assert ei.value.code == lvx.E_RANGE
        r = g.evaluate(s, normal_eq=True)
        assert np.isfinite(r["cost"]) and r["cost"] > 0
    finally:
        g.close()
    Q = dict(P, t_map=P["t0"] - 0.01)
    g = lvx.Context(0)
    try:
        with pytest.raises(lvx.LvxError) as ei:
            lvx.load_problem(g, Q, locks)
            g.evaluate(s, normal_eq=True)
        assert ei.value.code == lvx.E_RANGE
    finally:
        g.close()
