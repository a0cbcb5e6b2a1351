"""Cases and float64 reference of the calibration covariance (lvx_calibration_covariance), shared by tests/test_gpu_calib_cov.py and the generator of the reference's own
accuracy, tests/golden/make_calib_cov_ref.py.  Not a test module.

Definition (include/lvx.h): with F the free tangent scalars of a lock mask, s = 1 / (1 + sqrt(diag H_FF)) (or 1) and lmd = clip(diag(s H_FF s), 1e-6, 1e32),
    A_R = s H_FF s + diag(lmd) / R,    cov = [ s A_R^-1 s ] restricted to the calibration scalars tangent 6 N .. 6 N + 21,
and the scaled marginal information T = A_cc - A_cb A_bb^-1 A_bc (b = the free scalars that are not calibration scalars)."""
import numpy as np

from oracle import lm as LM
from oracle import oracle as O

N_CALIB = 22
TAU = O.LOCK_LIDAR_TAU | O.LOCK_CAM_TAU
SOLVE2 = TAU
SOLVE1 = TAU | O.LOCK_CAM_Q | O.LOCK_CAM_P | O.LOCK_LANDMARKS
SOLVE3 = TAU | O.LOCK_TRAJ | O.LOCK_LIDAR_Q | O.LOCK_LIDAR_P
MASKS = {"solve1": SOLVE1, "solve2": SOLVE2, "solve3": SOLVE3}
RADII = (1e4, 1e8)
SMALL = dict(seed=14, duration=0.4, n_surfel=200, n_planes=10, n_landmarks=12, n_camsurf=5)   # 44 knots
# the leaves + separators plan: the IMU-only shape of tests/test_gpu_solver_nd.py (seed 7, no LiDAR, no camera: 22 border scalars, narrow leaves only), cut from 40 s to
# 1.2 s.  The dense export the reference is built from is n_tangent^2 doubles — 4.6 GB at 40 s — and the plan is active from two leaves on when SOLVER_ND = 1 asks for it.
ND = dict(seed=7, duration=1.2, n_surfel=0, n_landmarks=0, n_camsurf=0)
ND_LOCKS = TAU | O.LOCK_LIDAR_Q | O.LOCK_LIDAR_P | O.LOCK_CAM_Q | O.LOCK_CAM_P


def case_name(mask, radius, scaling):
    return "%s_R%g_%s" % (mask, radius, "scaled" if scaling else "plain")


def free_sets(n_knots, n_landmarks, locks):
    """free tangent indices, positions (within them) of the free calibration scalars, and those scalars' numbers c."""
    free = LM.free_tangent_indices(n_knots, n_landmarks, locks)
    is_c = (free >= 6 * n_knots) & (free < 6 * n_knots + N_CALIB)
    return free, np.nonzero(is_c)[0], free[is_c] - 6 * n_knots


def damped_system(H, free, radius, scaling):
    Hf = H[np.ix_(free, free)]
    d = np.diag(Hf)
    s = 1.0 / (1.0 + np.sqrt(d)) if scaling else np.ones(len(free))
    A = Hf * s[:, None] * s[None, :]
    A = A + np.diag(np.clip(np.diag(A), 1e-6, 1e32) / radius)
    return A, s


def reference(H, n_knots, n_landmarks, locks, radius, scaling):
    """float64: cov over the free calibration scalars (Cholesky of A_R, one triangular solve), the scaled marginal information T, the scale of those scalars, their c."""
    import scipy.linalg as sl
    free, pos, cidx = free_sets(n_knots, n_landmarks, locks)
    A, s = damped_system(H, free, radius, scaling)
    L = np.linalg.cholesky(A)
    E = np.zeros((len(free), len(pos))); E[pos, np.arange(len(pos))] = 1.0
    X = sl.solve_triangular(L, E, lower=True)
    cov = (X.T @ X) * s[pos][:, None] * s[pos][None, :]
    rest = np.setdiff1d(np.arange(len(free)), pos)
    T = A[np.ix_(pos, pos)]
    if len(rest):
        W = sl.solve_triangular(np.linalg.cholesky(A[np.ix_(rest, rest)]), A[np.ix_(rest, pos)], lower=True)
        T = T - W.T @ W
    return dict(cov=cov, T=0.5 * (T + T.T), scale=s[pos], cidx=cidx)


def rel_err(cov, ref):
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(cov - ref) / (d[:, None] * d[None, :])))
