"""CPU: the irregular time layouts of tests/time_layout_cases.py are what they claim to be (the premise of every case, asserted on the built inputs), and the
oracle alone evaluates them — or throws the reference's range_error where a non-zero IMU time offset makes it (TAU_ORACLE_RAISES, which the GPU test relies on)."""
import numpy as np
import pytest

import lvx
import time_layout_cases as TL
from oracle import oracle as O


def _runs_of_empty(counts, lo, hi):
    """Lengths of the maximal runs of empty intervals inside [lo, hi], by first interval."""
    runs, k = {}, lo
    while k <= hi:
        if counts[k] == 0:
            a = k
            while k <= hi and counts[k] == 0:
                k += 1
            runs[a] = k - a
        else:
            k += 1
    return runs


def _counts(P, t):
    k = TL.interval(P, t)
    assert k.min(initial=0) >= 0 and k.max(initial=0) <= P["n_knots"] - 4
    return np.bincount(k, minlength=P["n_knots"])


def _premise(name, P, state, ex):
    N = P["n_knots"]
    assert P["dt"] == 0.02 and N <= 800
    ci, cs = _counts(P, P["t_imu"]), _counts(P, P["surf_t"])
    ki = TL.interval(P, P["t_imu"])
    if name == "imu_gap_long":
        runs = _runs_of_empty(ci, ki.min(), ki.max())
        assert list(runs.values()) == [65] and 65 >= 60 > 32 + 5          # one hole inside the stream, longer than IMU_CR + 5
        a, n = next(iter(runs.items()))
        assert (a, a + n) == ex["gap"] and cs[a:a + n].sum() >= 60           # surfel rows continue through it
    elif name == "imu_gaps_short":
        assert _runs_of_empty(ci, ki.min(), ki.max()) == {30: 1, 50: 4, 80: 5}
    elif name == "imu_burst":
        kb = ex["burst"]
        assert ci.argmax() == kb and ci[kb] >= 3 * 256 and ci[kb] >= 700
        assert ci[kb - 1] == 0 and ci[kb + 1] == 3
        assert np.median(ci[ki.min():kb - 1]) == 8                          # the rest is the normal stream
    elif name in ("imu_sparse", "imu_sparse_nosurf"):
        n = len(P["t_imu"])
        assert N >= 700 and 130 <= n <= 150 and n / (N - 3) <= 0.3
        d = np.diff(np.sort(ki))
        assert d.min() >= 3 and d.max() <= 7 and len(set(d)) >= 4           # irregular spacing of 3 - 7 intervals
        assert (len(P["surf_t"]) > 0) == (name == "imu_sparse")
        # The first partition of ensure_layout is G = ceil(n / 256) = 1 workgroup range over all samples; its knot span is (last interval - first interval) + 37
        # (TL.IMU_WINDOW), and imu_fused_lds_bytes(span) = 115 088 + 148 * span exceeds 160 KB from span = 330 on (TL.IMU_LDS_SPAN_LIMIT): the G *= 2 loop runs.
        assert (n + 255) // 256 == 1
        assert ki.max() - ki.min() + TL.IMU_WINDOW > TL.IMU_LDS_SPAN_LIMIT
        assert 115088 + 148 * TL.IMU_LDS_SPAN_LIMIT <= 160 * 1024 < 115088 + 148 * (TL.IMU_LDS_SPAN_LIMIT + 1)
        # ... and still at G = 2 (two halves of the samples, each over ~350 intervals)
        half = np.sort(ki)[:n // 2]
        assert half.max() - half.min() + TL.IMU_WINDOW > TL.IMU_LDS_SPAN_LIMIT
    elif name.startswith("imu_counts_"):
        assert len(P["t_imu"]) == ex["n"] and np.all(np.diff(P["t_imu"]) > 0)
    elif name == "imu_shuffled_dups":
        t = P["t_imu"]
        assert np.any(np.diff(t) < 0) and np.count_nonzero(np.diff(t) < 0) > len(t) // 4      # not monotone (a permutation, not a swap)
        u, inv, cnt = np.unique(t, return_inverse=True, return_counts=True)
        assert len(t) - len(u) >= 20
        for j in np.flatnonzero(cnt > 1):                                   # equal stamps carry different measurements
            rows = np.flatnonzero(inv == j)
            assert len(np.unique(P["gyro"][rows], axis=0)) == len(rows) and len(np.unique(P["acc"][rows], axis=0)) == len(rows)
    elif name == "imu_on_knots":
        al = ex["aligned"]
        assert len(al) >= 30 and np.isin(al, P["t_imu"]).all()
        on = P["t0"] + P["dt"] * np.arange(20, 60)
        assert np.isin(al, on).sum() >= 30                                  # stamps exactly t0 + k dt, as the host forms them
        assert np.isin(al, np.nextafter(on, np.inf)).sum() + np.isin(al, np.nextafter(on, -np.inf)).sum() >= 30
        assert len(P["t_imu"]) - len(al) >= 500                             # mixed into a normal stream
    elif name.startswith("imu_tau_"):
        tau = state[TL.tau_imu_slot(P)]
        assert tau == ex["tau"] and tau != 0.0
        crossing = np.count_nonzero(TL.interval(P, P["t_imu"] + tau) != ki)
        if name.startswith("imu_tau_inside"):
            assert abs(tau) == 0.3 * P["dt"] and crossing == 0
            u = (P["t_imu"] - P["t0"]) / P["dt"] - ki
            assert u.min() >= 0.4 and u.max() <= 0.6
        elif name.startswith("imu_tau_crossing"):
            assert abs(tau) == 0.3 * P["dt"] and crossing >= 10
        else:
            assert tau == 1.5 * P["dt"] and crossing == len(ki)
    elif name == "surf_burst":
        kb = ex["burst"]
        assert cs[kb] >= 3 * 512 and cs[kb] >= 2000 and cs[kb - 1] == 0 and cs[kb + 1] == 0
        assert 50 <= len(P["surf_t"]) - cs[kb] <= 300 and np.count_nonzero(cs) >= 40          # a sparse remainder elsewhere
    elif name == "surf_ends":
        km, last = ex["hub"], ex["last"]
        assert km == TL.interval(P, P["t_map"]) and last == N - 4
        assert set(np.flatnonzero(cs)) == {km, km + 1, last} and min(cs[km], cs[km + 1], cs[last]) >= 50
        assert P["surf_t"].min() > P["t_map"] and P["surf_t"].max() < TL.max_time(P)
    elif name.startswith("surf_counts_"):
        ks = TL.interval(P, P["surf_t"])
        assert len(ks) == ex["n"]
        if ex["n"] >= 63:
            assert ks.max() - ks.min() >= 0.8 * (N - 3 - TL.interval(P, P["t_map"]))         # spread over the whole spline
    elif name == "surf_shuffled_dups":
        t = P["surf_t"]
        assert np.count_nonzero(np.diff(t) < 0) > len(t) // 4
        u, inv, cnt = np.unique(t, return_inverse=True, return_counts=True)
        assert len(t) - len(u) >= 20
        assert sum(len(set(P["surf_plane"][inv == j])) > 1 for j in np.flatnonzero(cnt > 1)) >= 20   # duplicate stamps on different planes
    elif name == "rep_shuffled_unused":
        lm = P["rep_lm"]
        cnt = np.bincount(lm, minlength=P["n_landmarks"])
        assert sorted(np.flatnonzero(cnt == 0)) == ex["unused"] and len(ex["unused"]) >= 3
        assert cnt[ex["single"]] == 1 and list(np.flatnonzero(cnt == 1)) == [ex["single"]]
        r7 = np.flatnonzero(lm == ex["twice"])
        tt, c7 = np.unique(P["rep_t0"][r7], return_counts=True)
        assert sorted(c7) == [1] * (len(c7) - 1) + [2] and tt[c7 == 2][0] == ex["twice_frame"]
        assert not np.array_equal(P["rep_uv"][r7][P["rep_t0"][r7] == ex["twice_frame"]][0], P["rep_uv"][r7][P["rep_t0"][r7] == ex["twice_frame"]][1])
        assert np.count_nonzero(np.diff(lm) < 0) > len(lm) // 4             # blocks in random order: landmarks neither sorted nor grouped
        assert len(set(np.flatnonzero(np.diff(lm) != 0))) > 2 * P["n_landmarks"]
    else:
        raise KeyError(name)


def test_every_case_of_the_issue_is_built():
    assert len(set(TL.NAMES)) == len(TL.NAMES) == 28
    assert {n for n in TL.NAMES if n.startswith("imu_tau_")} == set(TL.TAU_ORACLE_RAISES)


@pytest.mark.parametrize("name", TL.NAMES)
def test_premise_holds_and_the_oracle_decides(name):
    P, state, locks, ex = TL.build(name)
    assert locks == lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
    assert ex["tau_imu"] == (name in TL.TAU_ORACLE_RAISES) and ex["tau_imu"] == (state[TL.tau_imu_slot(P)] != 0.0)
    if not ex["tau_imu"]:
        assert np.array_equal(state, P["state0"])
    _premise(name, P, state, ex)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    if ex["oracle_raises"]:
        with pytest.raises(IndexError):
            o.evaluate(state)
    else:
        r = o.evaluate(state)
        assert r["residuals"].shape == (6 * len(P["t_imu"]) + len(P["surf_t"]) + 2 * len(P["rep_lm"]) + len(P["cs_lm"]),)
        assert np.isfinite(r["residuals"]).all() and np.isfinite(r["cost"]) and r["cost"] > 0
    assert ex["oracle_raises"] == TL.TAU_ORACLE_RAISES.get(name, False)


def test_builds_are_repeatable():
    """The GPU tests build a case more than once (one context per test): same arrays every time."""
    for name in ("imu_sparse", "imu_shuffled_dups", "imu_on_knots", "rep_shuffled_unused"):
        a, b = TL.build(name), TL.build(name)
        assert np.array_equal(a[1], b[1])
        for k in ("t_imu", "gyro", "acc", "surf_t", "surf_plane", "rep_lm", "rep_uv", "rep_t0"):
            assert np.array_equal(a[0][k], b[0][k]), (name, k)
