"""GPU: the halo samples of k_imu_own against the FP64 oracle.  Workgroup g of the fused IMU kernel walks, in front of its own (primary) samples, those of the three
knot intervals before its range, so that every band column at a range boundary has one writer; a halo window adds to the knot-indexed accumulators only.  What can go
wrong without crashing: a boundary column stored from a partial sum or counted twice, a halo sample's cost / residual / record / calibration block counted twice, a
column left to the atomic protocol that a halo window touches.  So every case compares cost, residuals, g and H entry by entry (helpers and tolerances of
tests/test_gpu_time_layouts.py: cost 1e-12, residuals 1e-11, H 1e-10 max|H| and 1e-9 block-scaled with zero where the oracle is zero, g 1e-10), on the first pass and
on its replay (owned columns are stored over the first pass's values, not cleared).

All streams use dt = 0.02 and are placed by hand (stamps moved, gyro / acc values reused, as tests/time_layout_cases.py does).  Ranges: G = ceil(n / 256) workgroups
with equal sample counts, boundaries moved up to the next interval start.  The streams begin at interval 30, away from the hub (t_map lies in interval 12: the hub
knots and their neighbours keep the atomic protocol, and so does a boundary next to them — the `hub_*` cases put one there).  Landmarks have rows of their own in
this layout (no knot loses its contiguous positions to them); the `hub_*` problems carry landmarks and surfel rows all the same."""
import functools

import numpy as np
import pytest

import lvx
import time_layout_cases as TL
from oracle import oracle as O
from test_gpu_jacobian_blocks import _check_records
from test_gpu_time_layouts import _check, _context

pytestmark = pytest.mark.gpu

K0 = 30                                 # first interval of the hand-placed streams
HUB_BOUNDARIES = (11, 13, 17, 19, 20, 22)


def _place(P, ks, rng, lo=0.02, hi=0.98, shuffle=False):
    t = TL._in_interval(P, ks, rng.uniform(lo, hi, len(ks)))
    if shuffle:
        t = t[rng.permutation(len(t))]
    TL._set_imu_times(P, t)


def _regular(n, per):
    return K0 + np.arange(n) // per


def build(name):
    """(P, state, locks, special): special = the case has a range boundary next to knots that keep the atomic protocol."""
    rng = np.random.default_rng(TL.hash_name("halo_" + name))
    locks, tau, special = TL.TAU, 0.0, False
    if name.startswith("regular_"):                       # (a) 8 per interval: 2, 3 and 5 ranges
        n = int(name.rsplit("_", 1)[1])
        P = TL._base(301, {257: 1.2, 600: 2.0, 1100: 3.3}[n], n_surfel=200)
        _place(P, _regular(n, 8), rng)
    elif name == "shuffled_600":                          # (h) the same stream in shuffled input order: residuals come out where the sample went in
        P = TL._base(301, 2.0, n_surfel=200)
        _place(P, _regular(600, 8), rng, shuffle=True)
    elif name == "dense_600":                             # (b) 40 per interval: ranges of 5 intervals, the halo is more than half of one
        P = TL._base(302, 1.0, n_surfel=100)
        _place(P, _regular(600, 40), rng)
    elif name == "short_ranges_600":                      # (c) 100 per interval: a range is two intervals, the halo reaches through the whole range before it
        P = TL._base(303, 1.0, n_surfel=100)
        _place(P, _regular(600, 100), rng)
    elif name == "halo_burst":                            # (d) 300 samples in interval 40, the last one in front of the boundary at sample 380: the halo spans batches
        P = TL._base(304, 2.0, n_surfel=200)
        ks = np.concatenate([K0 + np.arange(80) // 8, np.full(300, 40), 41 + np.arange(320) // 8])
        _place(P, ks, rng)
    elif name == "sparse":                                # (e) one sample per two to three intervals: empty halo intervals, knots no window covers; two ranges by the LDS limit
        P = TL._base(305, 9.0, n_surfel=400, n_landmarks=0)
        ks = K0 + np.cumsum(rng.integers(2, 4, 150))
        assert ks[-1] <= P["n_knots"] - 4 and ks[-1] - ks[0] + TL.IMU_WINDOW > TL.IMU_LDS_SPAN_LIMIT
        _place(P, ks, rng)
    elif name.startswith("hub_"):                         # (f) 150 samples in front of interval B, 150 behind it: the boundary of the two ranges is B
        B = int(name.rsplit("_", 1)[1])
        P = TL._base(306, 1.2, n_surfel=300, n_landmarks=12, views_per_lm=3)
        ks = np.concatenate([np.sort(rng.integers(B - 3, B, 150)), B + np.arange(150) // 6])
        assert len(np.unique(ks[:150])) == 3 and int(TL.interval(P, P["t_map"])) == 12
        _place(P, ks, rng)
        special = True
    elif name in ("tau_pos", "tau_neg"):                  # (g) t + tau_imu stays inside the interval (the middle 20 %), three ranges
        P = TL._base(307, 2.6, n_surfel=200)
        _place(P, _regular(600, 6), rng, 0.4, 0.6)
        tau = (0.3 if name == "tau_pos" else -0.3) * TL.DT
    elif name == "lock_r3":                               # (k) Solve #0, positions locked: gyroscope blocks alone, no fused kernel, no ownership (tests/test_gpu_eval.py::test_so3_only_solve0)
        P = TL._base(301, 2.0, n_surfel=0, n_planes=1, n_landmarks=0)
        _place(P, _regular(600, 8), rng)
        locks = TL.TAU | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS
    else:
        raise KeyError(name)
    state = P["state0"].copy()
    if tau:
        state[TL.tau_imu_slot(P)] = tau
    return P, state, locks, special


ORACLE_CASES = (["regular_257", "regular_600", "regular_1100", "shuffled_600", "dense_600", "short_ranges_600", "halo_burst", "sparse"] +
                ["hub_%d" % b for b in HUB_BOUNDARIES] + ["tau_pos", "tau_neg", "lock_r3"])
RECORD_CASES = ["regular_600", "short_ranges_600"]
DET_CASES = ["regular_600", "short_ranges_600", "sparse"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(P, state, locks, special, oracle result) — computed once per case and shared, never modified."""
    P, state, locks, special = build(name)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    if locks & lvx.LOCK_R3:
        o.set_so3_only(True)                            # the device has no accelerometer rows under LOCK_R3; the oracle drops them for the SO3-only estimator
    return P, state, locks, special, o.evaluate(state, normal_eq=True)


def _assert_no_fallback(lo, special):
    if not special:
        assert lo["exact_fallback"] == 0 and lo["fallback_rows"] == 0


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_halo_pass_matches_the_oracle_twice(name):
    P, state, locks, special, ro = _case(name)
    g = _context(P, locks)
    for label in ("first", "replay"):
        r = g.evaluate(state, normal_eq=True)
        _assert_no_fallback(_check(name, label, r, ro, g), special)
    # (h) cost alone: halo samples are not evaluated at all, every sample is counted once
    c = g.evaluate(state, residuals=False)
    print("IMU_HALO %s cost_only: %.2e" % (name, abs(c["cost"] - ro["cost"]) / abs(ro["cost"])))
    assert abs(c["cost"] - ro["cost"]) <= 1e-12 * abs(ro["cost"])
    _assert_no_fallback(g.layout(), special)
    r = g.evaluate(state, normal_eq=True)              # and the normal equations after a pass that stored nothing
    _assert_no_fallback(_check(name, "after_cost_only", r, ro, g), special)
    g.close()


@pytest.mark.parametrize("name", RECORD_CASES)
def test_halo_samples_write_one_record(name):
    P, state, locks, special, ro = _case(name)
    g = _context(P, locks)
    rb = g.evaluate(state, normal_eq=True, jac_blocks=True)
    _assert_no_fallback(_check(name, "records_pass", rb, ro, g), special)
    _check_records(g, state, rb["jac_blocks"])
    g.close()


@pytest.mark.parametrize("name", DET_CASES)
def test_deterministic_mode_keeps_its_bits(name):
    P, state, locks, special, ro = _case(name)
    g = _context(P, locks, det=True)
    a = g.evaluate(state, normal_eq=True)
    _assert_no_fallback(_check(name, "deterministic", a, ro, g), special)
    b = g.evaluate(state, normal_eq=True)
    g.close()
    h = _context(P, locks, det=True)                    # and on a fresh context
    c = h.evaluate(state, normal_eq=True)
    h.close()
    for r in (b, c):
        assert r["cost"] == a["cost"]
        assert np.array_equal(r["H"], a["H"]) and np.array_equal(r["g"], a["g"]) and np.array_equal(r["residuals"], a["residuals"])
