"""Cases of the surfel hand-off tests (lvx_set_planes_d / lvx_set_surfel_d / lvx_set_surfel_from_association against the host setters): problem builders shared by
tests/test_handoff_cases.py (CPU: every case is what it claims, checked with numpy and oracle.pipeline.select_surfels) and tests/test_gpu_handoff.py (the two routes
on two contexts).

A crafted case is a synth.make_problem without visual data (IMU + surfel family) whose surfel TIMES are replaced by one of the patterns below; points and plane ids
stay the generator's, so residuals are finite numbers that the two routes must reproduce bit for bit — whether they are small is not the subject here.

Splines: N = 24 knots (dt 0.02, 0.29 s + 2 x 0.06 s pad) and N = 300 (5.53 s + 2 x 0.2 s).  Row counts 0, 1, 63, 64, 65, 257, 1025: one wavefront minus / plus one,
one 256-row compaction tile plus one, four tiles plus one."""
import numpy as np

import synth

ROW_COUNTS = (0, 1, 63, 64, 65, 257, 1025)
PATTERNS = ("shuffled", "one_interval", "on_knots", "last_interval", "outside")
SPLINES = {24: dict(duration=0.29, pad=0.06), 300: dict(duration=5.53, pad=0.2)}
SEQ_KW = dict(seed=50, duration=1.2, W=450, n_reproj=300)   # the from-association sequence: 9 scans, 93 knots
T_MAP_SHIFT = 0.4                                              # the moved map time of the from-association case


def knot_interval(t, t0, dt, N):
    """Knot interval of a time as the layout keys it: floor((t - t0) / dt) inside [t0, t0 + (N - 3) dt), -1 outside (times within 1e-9 intervals of a knot may land on
    either side of it: the tests never assert those)."""
    t = np.asarray(t, dtype=np.float64)
    k = np.floor((t - t0) / dt).astype(np.int64)
    inside = (t >= t0) & (t < t0 + (N - 3) * dt)
    return np.where(inside, np.clip(k, 0, N - 4), -1)


def times(pattern, n, P, rng):
    """n surfel times of one pattern for the spline of problem P (all >= P["t_map"] except the out-of-range ones of "outside")."""
    t0, dt, N, t_map = P["t0"], P["dt"], P["n_knots"], P["t_map"]
    t_hi = t0 + (N - 3) * dt
    k_map = int(np.floor((t_map - t0) / dt)) + 1   # first interval that lies wholly behind t_map
    if pattern == "shuffled":
        return rng.permutation(np.linspace(t_map + 1e-4, t_hi - 2e-3, n)) if n else np.zeros(0)   # (2 ms from the end: a free time offset pads every row by its 1 ms bound)
    if pattern == "one_interval":
        return t0 + ((N // 2) + rng.uniform(0.05, 0.95, n)) * dt
    if pattern == "on_knots":
        return t0 + (k_map + (np.arange(n) * 7) % (N - 3 - k_map)).astype(np.float64) * dt
    if pattern == "last_interval":
        return t0 + ((N - 4) + rng.uniform(0.01, 0.99, n)) * dt
    if pattern == "outside":
        t = t0 + ((N // 2) + rng.uniform(0.05, 0.95, n)) * dt
        t[0::5] = t0 - 0.5 * dt - rng.uniform(0, 1, len(t[0::5]))      # before the spline
        t[1::5] = t_hi + rng.uniform(0, 1, len(t[1::5]))                # at or after its end
        return t
    raise KeyError(pattern)


def crafted(n, pattern="shuffled", N=24, n_planes=40, seed=0, bad_plane=False):
    """Problem dict (synth.make_problem keys) with n surfel rows of the pattern on an N-knot spline; bad_plane: row n // 2 names plane n_planes."""
    P = synth.make_problem(seed=31 + seed, dt=0.02, n_surfel=max(n, 1), n_planes=n_planes, n_landmarks=0, n_camsurf=0, **SPLINES[N])
    assert P["n_knots"] == N
    rng = np.random.default_rng(1000 + 17 * seed + n)
    P["surf_t"] = np.ascontiguousarray(times(pattern, n, P, rng), dtype=np.float64)
    P["surf_pt"] = np.ascontiguousarray(P["surf_pt"][:n], dtype=np.float64).reshape(n, 3)
    P["surf_plane"] = np.ascontiguousarray(P["surf_plane"][:n], dtype=np.int32)
    if bad_plane:
        P["surf_plane"][n // 2] = n_planes
    return P


# (id, arguments of crafted(), LiDAR time offset free, CHUNK_ROWS or None): what tests/test_gpu_handoff.py runs through both routes
CRAFTED = [("n%d" % n, dict(n=n), False, None) for n in ROW_COUNTS] + [
    ("one_interval", dict(n=257, pattern="one_interval"), False, None),
    ("on_knots", dict(n=257, pattern="on_knots"), False, None),
    ("last_interval", dict(n=65, pattern="last_interval"), False, None),
    ("outside", dict(n=257, pattern="outside"), False, None),
    ("one_plane", dict(n=65, n_planes=1), False, None),
    ("tau_free", dict(n=257), True, None),
    ("chunk64", dict(n=1025), False, 64),
    ("N300", dict(n=1025, N=300), False, None),
    ("N300_tau_free_chunk64", dict(n=1025, N=300, pattern="on_knots"), True, 64),
    ("N300_one_interval_chunk64", dict(n=257, N=300, pattern="one_interval"), False, 64),
]


def association_like(n, t_start, t_end, rng, n_planes=50):
    """A chronological SurfelPoint list as lvx_get_surfel_points returns it (pt, t, plane), for checks of the selection rule alone."""
    return dict(pt=rng.standard_normal((n, 3)), t=np.sort(rng.uniform(t_start, t_end, n)), plane=rng.integers(0, n_planes, n).astype(np.int32))


def select_reference(points, t_map, step):
    """The issue's statement of lvx_set_surfel_from_association in numpy: indices 0, step, 2 step, ... (step <= 0: 1), those with t >= t_map, in order."""
    idx = np.arange(0, len(points["t"]), step if step > 0 else 1)
    idx = idx[points["t"][idx] >= t_map]
    return points["pt"][idx], points["t"][idx], points["plane"][idx]
