"""GPU: the window walk of the fused IMU kernel's MFMA assembly (imu_assemble in csrc/lvx_eval.hip) and of the panel-major branch of k_family_mfma against the FP64
oracle.  A window is the RUN of valid lanes of one knot interval inside a panel (its key read from the first lane, its rows masked by the span alone: rows of an
invalid lane or of an earlier trip lie outside every span), and it scatters straight from the byte offsets of the lane's table (k_imu_rtab): slots without a
target add to the lane's dummy slot, a halo window sends the calibration-only slots there too, and nothing tests the top of the accumulator range.  What can go
wrong without crashing: a stale panel row read unmasked, a window cut at a 16- / 32- / 64-lane border counted twice or not at all, a tile value
added to a wrong accumulator entry, a halo window adding to the sums over the IMU calibration.  So every case compares cost, residuals, g and H entry by entry with
the helpers and tolerances of tests/test_gpu_time_layouts.py (cost 1e-12, residuals 1e-11, H 1e-10 max|H| and 1e-9 block-scaled with zero where the oracle is zero,
g 1e-10), on the first pass and on its replay.

Streams are placed by hand as in tests/test_gpu_imu_halo.py: dt = 0.02, first interval 30 (away from the hub), G = ceil(n / 256) workgroups, batches of at most 256
samples spanning at most 32 intervals, wavefront slices of at most 64 samples on interval starts.

  sizes            intervals of 1, 3, 7, 8, 9, 15, 16, 17 and 33 samples (twice) and one of 70: windows across the 16-, 32- and 64-lane borders of a trip, the
                   70-sample interval over two trips (two workgroups: the second walks a halo)
  short_last       three intervals of 64 samples, a gap longer than a batch's reach, one interval of 5: wavefront 0 walks a trip of 64 valid lanes and then one of 5, whose
                   other 59 lanes sit over the rows of the trip before (one wavefront walks all four trips in deterministic mode)
  top              32 intervals of 8 samples: one batch whose last windows add to the top rows of the accumulator window (offset 32 of 37 knots)
  wide_pair        5 samples per interval, control point 50 turned by 2 rad: the samples of the intervals 47 .. 50 (their four knots hold a pair beyond the small-angle
                   polynomials) are invalid lanes in the middle of their panels and go to the fallback list, their neighbours stay in the assembly
  last_M / last_halo_M   sample counts that leave a last batch of M intervals behind a full one: one workgroup, 6 per interval (no halo); two workgroups, 4 per
                   interval — the first range ends with a batch of M intervals, the second one (three halo intervals in front) with one of M + 3
  gyro_only        Solve #0 (positions locked): the gyroscope blocks alone, through the panel-major branch of k_family_mfma
  reproj           a small problem with landmark tracks: the reprojection side passes run the same branch"""
import functools

import numpy as np
import pytest

import lvx
import synth
import time_layout_cases as TL
from oracle import oracle as O
from test_gpu_time_layouts import _check, _context

pytestmark = pytest.mark.gpu

K0 = 30
SIZES = (1, 3, 7, 8, 9, 15, 16, 17, 33)
LAST = (1, 5, 6)
LAST_HALO = (1, 2, 3, 5, 6)


def _place(P, ks, rng):
    ks = np.asarray(ks)
    assert ks.max() <= P["n_knots"] - 4
    TL._set_imu_times(P, TL._in_interval(P, ks, np.sort(rng.uniform(0.02, 0.98, len(ks)))))   # (keys ascend; sorted fractions keep the stamps ascending inside an interval)


def build(name):
    """(P, state, locks, fallback): fallback = the case sends rows to the exact kernels on purpose."""
    rng = np.random.default_rng(TL.hash_name("windows_" + name))
    locks, fallback = TL.TAU, False
    if name == "sizes":
        P = TL._base(401, 1.5, n_surfel=200)
        counts = list(SIZES) + [70] + list(SIZES)
        _place(P, np.repeat(K0 + np.arange(len(counts)), counts), rng)
    elif name == "short_last":
        P = TL._base(402, 2.0, n_surfel=400)
        _place(P, np.concatenate([np.repeat(K0 + np.arange(3), 64), np.full(5, K0 + 45)]), rng)
    elif name == "top":
        P = TL._base(403, 1.5, n_surfel=200)
        _place(P, K0 + np.arange(256) // 8, rng)
    elif name == "wide_pair":
        P = TL._base(404, 1.5, n_surfel=200)
        _place(P, K0 + np.arange(200) // 5, rng)
        fallback = True
    elif name.startswith("last_halo_"):
        m = int(name.rsplit("_", 1)[1])
        P = TL._base(405, 2.4, n_surfel=300)
        _place(P, K0 + np.arange(2 * (32 + m) * 4) // 4, rng)
        assert len(P["t_imu"]) > 256
    elif name.startswith("last_"):
        m = int(name.rsplit("_", 1)[1])
        P = TL._base(406, 1.6, n_surfel=200)
        _place(P, K0 + np.arange((32 + m) * 6) // 6, rng)
        assert len(P["t_imu"]) <= 256
    elif name == "gyro_only":
        P = TL._base(407, 1.5, n_surfel=0, n_planes=1, n_landmarks=0)
        counts = list(SIZES) + [70]
        _place(P, np.repeat(K0 + np.arange(len(counts)), counts), rng)
        locks = TL.TAU | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS
    elif name == "reproj":
        P = TL._base(408, 1.5, n_surfel=100, n_landmarks=40, views_per_lm=5)
    else:
        raise KeyError(name)
    state = P["state0"].copy()
    if name == "wide_pair":
        N, k = P["n_knots"], 50
        q = state[3 * N + 4 * k:3 * N + 4 * k + 4].copy()
        state[3 * N + 4 * k:3 * N + 4 * k + 4] = synth.qmul(synth.q_from_rotvec(np.array([0.0, 0.0, 2.0])), q)
    return P, state, locks, fallback


CASES = (["sizes", "short_last", "top", "wide_pair"] + ["last_%d" % m for m in LAST] + ["last_halo_%d" % m for m in LAST_HALO] + ["gyro_only", "reproj"])
DET_CASES = ["short_last", "sizes"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(P, state, locks, fallback, oracle result) — computed once per case and shared, never modified."""
    P, state, locks, fallback = build(name)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    if locks & lvx.LOCK_R3:
        o.set_so3_only(True)
    return P, state, locks, fallback, o.evaluate(state, normal_eq=True)


def _assert_fallback(lo, fallback):
    assert lo["exact_fallback"] == 0                    # never the whole pass
    if not fallback:
        assert lo["fallback_rows"] == 0
    else:
        assert 0 < lo["fallback_rows"]


@pytest.mark.parametrize("name", CASES)
def test_windows_match_the_oracle_twice(name):
    P, state, locks, fallback, ro = _case(name)
    g = _context(P, locks)
    for label in ("first", "replay"):
        r = g.evaluate(state, normal_eq=True)
        _assert_fallback(_check(name, label, r, ro, g), fallback)
    g.close()


def test_wide_pair_sends_only_its_own_samples_to_the_fallback_list():
    """The gyroscope block of every sample of the intervals 47 .. 50 is listed (the sample: its accelerometer block goes with it), the surfel rows and views in those intervals too."""
    P, state, locks, fallback, ro = _case("wide_pair")
    g = _context(P, locks)
    g.evaluate(state, normal_eq=True)
    lo = g.layout()
    g.close()
    k = TL.interval(P, P["t_imu"])
    n_imu = int(((k >= 47) & (k <= 50)).sum())
    assert n_imu == 20
    others = int(((TL.interval(P, P["surf_t"]) >= 46) & (TL.interval(P, P["surf_t"]) <= 51)).sum()) + len(P["rep_lm"])
    print("IMU_WINDOWS wide_pair: fallback_rows %d, IMU samples behind the pair %d, rows of other families that may be %d" % (lo["fallback_rows"], n_imu, others))
    assert n_imu <= lo["fallback_rows"] <= 2 * n_imu + others   # (at most: both blocks of a sample counted)


@pytest.mark.parametrize("name", DET_CASES)
def test_deterministic_mode_two_passes_bitwise_equal(name):
    P, state, locks, fallback, ro = _case(name)
    g = _context(P, locks, det=True)
    a = g.evaluate(state, normal_eq=True)
    _assert_fallback(_check(name, "deterministic", a, ro, g), fallback)
    b = g.evaluate(state, normal_eq=True)
    g.close()
    assert b["cost"] == a["cost"]
    assert np.array_equal(b["H"], a["H"]) and np.array_equal(b["g"], a["g"]) and np.array_equal(b["residuals"], a["residuals"])
