"""GPU: the fold of the pseudo pose rows onto the hub control points (k_fold_all: the dense border block in closed form by the blocks that sum its replicas, the
border rows beside them) and the hub prepass of k_clear, in the cases of tests/fold_chain_cases.py — both LiDAR sets on shared hub rows, one set alone, lock masks
(free time offsets: another border size; dead hub columns), the fallback lists, LiDAR position blocks, t_map inside an interval and on either side of a knot.

Bars.  Against the oracle: the ones of tests/test_gpu_time_layouts.py::_check.  Default pass against SERIAL = 1 (k_fold_replicas -> k_fold_border_rows ->
k_fold_border_dense, the same mathematics): both fold sums of at most 64 replicas + 12 pseudo terms in another order, 1e-13 of max|H| / max|g|.  DETERMINISTIC: bits.
The oracle's results are computed once per case (tests/test_fold_chain_cases.py holds that it evaluates every case) and shared."""
import functools

import numpy as np
import pytest

import fold_chain_cases as FC
import lidarpos_cases as lc
import lvx
from test_gpu_time_layouts import _check, _context

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _oracle(name):
    return FC.oracle_results(name)


def _ctx(name, switch=None, det=False):
    P, s, s2, locks, ex = FC.build(name)
    if switch is None:
        g = _context(P, locks, det=det)
    else:
        g = lvx.Context(0)
        g.set_switch(switch, 1)
        lvx.load_problem(g, P, locks)
    if ex["poses"] is not None:
        lc.load_case(g, ex["poses"])
    return g


def _cost_only(g, state):
    return g.evaluate(state, normal_eq=False, residuals=False)["cost"]


@pytest.mark.parametrize("name", FC.NAMES)
def test_fold_matches_the_oracle_the_serial_kernels_and_itself(name):
    P, s, s2, locks, ex = FC.build(name)
    ro, ro2 = _oracle(name)
    g = _ctx(name)
    try:
        c0 = _cost_only(g, s)                                       # a cost-only pass in front of the first normal-equation pass
        first = g.evaluate(s, normal_eq=True)
        if name == "fallback_lists":                                # that pass discovered the rows and repeated itself with the lists on
            assert 0 < g.layout()["fallback_rows"] <= 40
        runs = [("first", first, ro), ("replay", g.evaluate(s, normal_eq=True), ro), ("second_state", g.evaluate(s2, normal_eq=True), ro2),
                ("back", g.evaluate(s, normal_eq=True), ro)]
        c1 = _cost_only(g, s)
        for label, r, want in runs:
            lo = _check(name, label, r, want, g)
            assert lo["exact_fallback"] == 0
        print("FOLD_CHAIN %s: cost-only before %.17g after %.17g pass %.17g" % (name, c0, c1, first["cost"]))
        for c in (c0, c1):                                          # the same blocks summed in another order (atomics): the cost bar of _check
            assert abs(c - ro["cost"]) <= 1e-12 * abs(ro["cost"]) and abs(c - c0) <= 1e-12 * abs(c0)
    finally:
        g.close()
    h = _ctx(name, switch="SERIAL")
    try:
        if name == "fallback_lists":
            h.evaluate(s, normal_eq=True)
        rs = h.evaluate(s, normal_eq=True)
    finally:
        h.close()
    r = runs[3][1]
    dH, dg = np.abs(r["H"] - rs["H"]).max() / np.abs(rs["H"]).max(), np.abs(r["g"] - rs["g"]).max() / np.abs(rs["g"]).max()
    print("FOLD_CHAIN %s: default - SERIAL  H %.2e g %.2e cost %.2e" % (name, dH, dg, abs(r["cost"] - rs["cost"]) / abs(rs["cost"])))
    assert r["H"].shape == rs["H"].shape and dH <= 1e-13 and dg <= 1e-13


@pytest.mark.parametrize("name", FC.NAMES)
def test_deterministic_mode_repeats_bit_for_bit(name):
    """`fallback_lists`: on the parent commit two passes differed in one stored entry of H (1e-24 .. 5e-21 of max|H|) in about half of the runs — the exact kernel over
    the surfel list ran four wavefronts, and two local columns on one tangent index (the merged hub segment) added to the same entry in the order the wavefronts
    arrived.  DETERMINISTIC now sorts a list and runs the LiDAR families' exact kernel over it with one wavefront."""
    P, s, s2, locks, ex = FC.build(name)
    ro, _ = _oracle(name)
    g = _ctx(name, det=True)
    if ex["poses"] is not None:     # the library has no deterministic schedule for the position blocks and says so (run_evaluate): nothing to repeat
        with pytest.raises(lvx.LvxError) as ei:
            g.evaluate(s, normal_eq=True)
        g.close()
        assert ei.value.code == lvx.E_ARG and "DETERMINISTIC" in str(ei.value)
        return
    try:
        if name == "fallback_lists":
            g.evaluate(s, normal_eq=True)
        a = g.evaluate(s, normal_eq=True)
        _check(name, "deterministic", a, ro, g)
        b = g.evaluate(s, normal_eq=True)
    finally:
        g.close()
    h = _ctx(name, det=True)                                        # and on a fresh context
    try:
        if name == "fallback_lists":
            h.evaluate(s, normal_eq=True)
        c = h.evaluate(s, normal_eq=True)
    finally:
        h.close()
    for label, r in (("same context", b), ("fresh context", c)):
        print("FOLD_CHAIN %s deterministic, %s: cost %.2e, H entries that differ %d (max %.2e of max|H|), g entries %d" % (
            name, label, abs(r["cost"] - a["cost"]), np.count_nonzero(r["H"] != a["H"]), np.abs(r["H"] - a["H"]).max() / np.abs(a["H"]).max(), np.count_nonzero(r["g"] != a["g"])))
    for r in (b, c):
        assert r["cost"] == a["cost"]
        assert np.array_equal(r["H"], a["H"]) and np.array_equal(r["g"], a["g"])


def test_nonunit_hub_control_point_maps_to_code():
    """Only the hub prepass of k_clear evaluates the scaled control point (tests/test_fold_chain_cases.py): its status -RES_NONUNIT must reach the caller."""
    P, s, k = FC.nonunit_hub_case()
    g = lvx.Context(0)
    try:
        lvx.load_problem(g, P, FC.TAU)
        for kw in (dict(normal_eq=True), dict(normal_eq=False)):
            with pytest.raises(lvx.LvxError) as ei:
                g.evaluate(s, **kw)
            assert ei.value.code == lvx.E_NONUNIT_QUAT
        r = g.evaluate(P["state0"], normal_eq=True)                 # and the context recovers on a unit state
        assert np.isfinite(r["cost"]) and r["cost"] > 0
    finally:
        g.close()
