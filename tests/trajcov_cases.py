"""Cases, numpy restatements and float64 reference of lvx_trajectory_covariance, shared by tests/test_trajcov_host.py, tests/test_gpu_trajcov.py and the generator of
the reference's own accuracy, tests/golden/make_trajcov_ref.py.  Not a test module.

Definition (include/lvx.h): with F the free tangent scalars, A_R = s H_FF s + diag(lmd) / R as calib_cov_cases.damped_system builds it, Sigma = s A_R^-1 s; the pose at
a time depends on at most 31 tangent scalars (window_idx), window_cov = Sigma over them, cov = J window_cov J^T."""
import numpy as np

import calib_cov_cases as CC
import lvx
import synth

W = 31
TAU = CC.TAU
R3_LOCKS = TAU | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS | lvx.LOCK_LIDAR_Q | lvx.LOCK_LIDAR_P | lvx.LOCK_CAM_Q | lvx.LOCK_CAM_P   # gyro + prior: 3 scalars per knot


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the selected inverse, restated.  Factor layout of the sequential route: Lb[j, d] = L(j + d, j) (d <= bw), Z[r, j] = (L^-1 A_bc)(j, r), S = A_cc - Zc^T Zc (unfactored).
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def random_system(rng, nb, bw, nbd):
    """SPD matrix over (band, border) whose band has half-bandwidth min(bw, nb - 1), as G G^T of a random factor with that pattern; returns (A, Lb, Z, S)."""
    n = nb + nbd
    G = np.tril(rng.uniform(-1, 1, (n, n)))
    for j in range(nb):
        G[j + bw + 1:nb, j] = 0.0
    G[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    A = G @ G.T
    L = np.linalg.cholesky(A)
    Lb = np.zeros((max(nb, 1), bw + 1))
    for j in range(nb):
        for d in range(min(bw, nb - 1 - j) + 1):
            Lb[j, d] = L[j + d, j]
    Z = L[nb:, :nb].copy()
    S = np.tril(A[nb:, nb:] - Z @ Z.T)
    return A, Lb, Z, S


def border_inverse(S):
    Sf = np.tril(S) + np.tril(S, -1).T
    Li = np.linalg.inv(np.linalg.cholesky(Sf)) if len(Sf) else np.zeros((0, 0))
    return Li.T @ Li


def selinv_scalar(Lb, Z, S, nb, bw, nbd):
    """The recurrence column by column, on the pattern padded to bw' = max(bw, 23).  Returns band [nb, bw' + 1] (band[j, d] = Sigma(j + d, j)), zb [nbd, nb], cc."""
    bwp = max(bw, 23)
    cc = border_inverse(S)
    band = np.zeros((max(nb, 1), bwp + 1))
    zb = np.zeros((nbd, max(nb, 1)))
    for j in range(nb - 1, -1, -1):
        nr = min(bwp, nb - 1 - j)
        m = nr + nbd
        g = np.zeros(m)
        for d in range(1, nr + 1):
            g[d - 1] = Lb[j, d] if d <= bw else 0.0
        g[nr:] = Z[:, j]
        Sl = np.zeros((m, m))
        for a in range(nr):
            for b in range(a + 1):
                Sl[a, b] = Sl[b, a] = band[j + 1 + b, a - b]
            Sl[a, nr:] = Sl[nr:, a] = zb[:, j + 1 + a]
        Sl[nr:, nr:] = cc
        gjj = Lb[j, 0]
        off = -(Sl @ g) / gjj
        band[j, 1:nr + 1] = off[:nr]
        zb[:, j] = off[nr:]
        band[j, 0] = 1.0 / gjj ** 2 - (g @ off) / gjj
    return band, zb, cc


def selinv_panels(Lb, Z, S, nb, bw, nbd, lowest=0):
    """The same in k_band_selinv's order: 16-column panels back to front against the ring of the trailing window.  Returns sigb [nb, 24], zb [nbd, nb], cc."""
    up16 = lambda x: (x + 15) // 16 * 16
    TB = up16(max(bw, 23)); R = TB + 16; nbp = up16(nbd); mT = TB + nbp; M = R + nbp
    cc = border_inverse(S)
    D = np.zeros((M, M))
    D[R:R + nbd, R:R + nbd] = cc
    sigb = np.full((max(nb, 1), 24), np.nan)
    zb = np.full((nbd, max(nb, 1)), np.nan)
    j0 = (nb - 1) // 16 * 16 if nb > 0 else -16
    while j0 >= 0 and j0 + 15 >= lowest:
        nk = min(16, nb - j0)
        slot = np.array([(j0 + 16 + k) % R if k < TB else R + k - TB for k in range(mT)])
        sJ = j0 % R
        Gp = np.zeros((16 + mT, 16))
        for c in range(16):
            if c >= nk:
                Gp[c, c] = 1.0
                continue
            j = j0 + c
            for r in range(16 + TB):
                d = j0 + r - j
                if j0 + r < nb and 0 <= d <= bw:
                    Gp[r, c] = Lb[j, d]
            Gp[16 + TB:16 + TB + nbd, c] = Z[:, j]
        GT = Gp[16:]
        Wm = GT.T @ D[np.ix_(slot, slot)]
        Li = np.linalg.inv(Gp[:16])
        X = -(Li.T @ Wm)
        P = Li.T @ (np.eye(16) + Wm @ GT) @ Li
        X[nk:] = 0.0
        P[nk:] = 0.0; P[:, nk:] = 0.0
        D[np.ix_(slot, sJ + np.arange(16))] = X.T
        D[np.ix_(sJ + np.arange(16), slot)] = X
        D[sJ:sJ + 16, sJ:sJ + 16] = P
        for c in range(nk):
            for a in range(c, nk):
                sigb[j0 + c, a - c] = P[a, c]
            for i in range(TB):
                d = 16 + i - c
                if d < 24 and j0 + 16 + i < nb:
                    sigb[j0 + c, d] = X[c, i]
            zb[:, j0 + c] = X[c, TB:TB + nbd]
        j0 -= 16
    return sigb, zb, cc


def gather(pos, sigb, zb, cc, scale=None, nb=0):
    """window over positions pos (>= 0 a band position, < 0 border slot -1 - o, None constant), as k_pose_cov gathers it."""
    n = len(pos)
    Wn = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            pa, pb = pos[a], pos[b]
            if pa is None or pb is None:
                continue
            if pa >= 0 and pb >= 0:
                lo, d = min(pa, pb), abs(pa - pb)
                v = sigb[lo, d] if d < sigb.shape[1] else 0.0
            elif pa >= 0:
                v = zb[-1 - pb, pa]
            elif pb >= 0:
                v = zb[-1 - pa, pb]
            else:
                v = cc[max(-1 - pa, -1 - pb), min(-1 - pa, -1 - pb)]
            if scale is not None:
                v *= scale[pa if pa >= 0 else nb - 1 - pa] * scale[pb if pb >= 0 else nb - 1 - pb]
            Wn[a, b] = v
    return Wn


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# quaternions (x, y, z, w), EigenQuaternionParameterization::Plus, pose errors
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qplus(q, d):
    n = np.linalg.norm(d)
    if n == 0.0:
        return np.array(q, float)
    return qmul(np.concatenate([np.sin(n) / n * np.asarray(d), [np.cos(n)]]), q)


def rotvec_between(q0, q1):
    """world-frame rotation vector dphi with R1 = Exp(dphi) R0"""
    d = qmul(q1, np.array([-q0[0], -q0[1], -q0[2], q0[3]]))
    if d[3] < 0:
        d = -d
    nv = np.linalg.norm(d[:3])
    return np.zeros(3) if nv == 0.0 else 2.0 * np.arctan2(nv, d[3]) * d[:3] / nv


def plus_tangent(state, N, g, h):
    """state (+) h e_g for a knot or calibration tangent index g < 6 N + 22 (lvx_plus restricted to one scalar)."""
    x = np.array(state, float)
    if g < 6 * N:
        k, c = divmod(g, 6)
        if c < 3:
            x[3 * k + c] += h
        else:
            o = 3 * N + 4 * k
            d = np.zeros(3); d[c - 3] = h
            x[o:o + 4] = qplus(x[o:o + 4], d)
        return x
    c = g - 6 * N
    s = 7 * N
    amb = {0: 8, 1: 9, 2: 10, 3: 11, 4: 12, 5: 13, 6: 14, 7: 15, 11: 20, 12: 21, 13: 22, 14: 23, 18: 28, 19: 29, 20: 30, 21: 31}
    if c in amb:
        x[s + amb[c]] += h
    else:
        o = s + (16 if c < 11 else 24)
        d = np.zeros(3); d[c - (8 if c < 11 else 15)] = h
        x[o:o + 4] = qplus(x[o:o + 4], d)
    return x


def fd_jacobian(pose_fn, state, N, idx, h=1e-3, plus=None):
    """Central differences of the pose error by the tangent scalars idx (-1: a zero column) at steps h and h / 2 and their Richardson extrapolation.
    pose_fn(state) -> (q xyzw, p); plus(state, g, step) -> state (+) step e_g (default: plus_tangent).  Returns (J_richardson [6, len(idx)], J_half [6, len(idx)])."""
    q0, p0 = pose_fn(state)
    if plus is None:
        plus = lambda x, g, step: plus_tangent(x, N, g, step)

    def diff(g, step):
        qa, pa = pose_fn(plus(state, g, step))
        qb, pb = pose_fn(plus(state, g, -step))
        return np.concatenate([pa - pb, rotvec_between(q0, qa) - rotvec_between(q0, qb)]) / (2 * step)
    Jr = np.zeros((6, len(idx))); Jh = np.zeros((6, len(idx)))
    for c, g in enumerate(idx):
        if g < 0:
            continue
        hg = h * 1e-2 if g - 6 * N in (14, 21) else h   # a time offset moves the evaluation time: a step well inside a knot interval (dt = 0.02 s)
        d1, d2 = diff(g, hg), diff(g, hg / 2)
        Jh[:, c] = d2
        Jr[:, c] = (4 * d2 - d1) / 3
    return Jr, Jh


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def r3_problem():
    """gyro + orientation prior under LVX_LOCK_R3: three free scalars per knot, the band narrower than a window's reach"""
    P = synth.make_problem(**CC.ND)
    return dict(P, acc=np.zeros_like(P["acc"]))


def load_r3(obj, P):
    lvx.load_problem(obj, P, R3_LOCKS)
    obj.set_so3_only(True)
    obj.set_orientation_prior(P["t0"], np.array([np.cos(5e-5), 0, 0, np.sin(5e-5)]), 28.0)


def query_times(P):
    """The first and last interval, exactly on knots, at t_map and in the intervals around it (windows that hold a hub knot or lie next to one), a spread, unsorted; then
    MaxTime and NaN (invalid).  65 times: the callers cut n = 1, 63, 64."""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    km = int(np.floor((P["t_map"] - t0) / dt))
    t = [t0, t0 + 0.3 * dt, np.nextafter(tmax, 0.0), tmax - 0.4 * dt, t0 + 5 * dt, t0 + (N - 4) * dt, P["t_map"]]
    t += [t0 + (km + k + 0.37) * dt for k in (-5, -4, -3, -1, 0, 1, 3, 4, 5) if 0 <= km + k <= N - 4]
    rng = np.random.default_rng(5)
    t += list(rng.uniform(t0, tmax, 63 - len(t)))
    t = np.array(t)
    rng.shuffle(t)
    return np.concatenate([t, [tmax, np.nan]])


def window_indices(P, t, frame):
    """the 31 tangent indices of the pose at t in `frame` at state0 (locks not applied: window_of drops the constant ones)"""
    N = P["n_knots"]
    tau = 0.0 if frame == lvx.FRAME_TRAJECTORY else P["state0"][7 * N + (23 if frame == lvx.FRAME_LIDAR else 31)]
    i0 = int(np.floor((t + tau - P["t0"]) / P["dt"]))
    ext = [-1] * 7 if frame == lvx.FRAME_TRAJECTORY else [6 * N + (8 if frame == lvx.FRAME_LIDAR else 15) + b for b in range(7)]
    return [6 * (i0 + c // 6) + c % 6 for c in range(24)] + ext


def probe_indices(P):
    """windows the reference's own error is measured on (tests/golden/make_trajcov_ref.py): the first and last interval, on a knot, at t_map; both sensors"""
    t0, dt, N = P["t0"], P["dt"], P["n_knots"]
    tmax = t0 + (N - 3) * dt
    return [window_indices(P, t, f) for t in (t0 + 0.3 * dt, tmax - 0.4 * dt, t0 + 5 * dt, P["t_map"]) for f in (lvx.FRAME_LIDAR, lvx.FRAME_CAMERA)]


def reference_sigma(H, n_knots, n_landmarks, locks, radius, scaling):
    """float64: the full s A_R^-1 s over the free tangent scalars by Cholesky, and the free index list."""
    import scipy.linalg as sl
    free = CC.free_sets(n_knots, n_landmarks, locks)[0]
    A, s = CC.damped_system(H, free, radius, scaling)
    Li = sl.solve_triangular(np.linalg.cholesky(A), np.eye(len(free)), lower=True)
    return (Li.T @ Li) * s[:, None] * s[None, :], free


def window_of(Sig, free, idx):
    """Sigma restricted to the tangent indices idx (-1: zero row / column)."""
    where = {int(g): k for k, g in enumerate(free)}
    sel = np.array([where.get(int(g), -1) for g in idx])
    Wn = np.zeros((len(idx), len(idx)))
    ok = sel >= 0
    Wn[np.ix_(ok, ok)] = Sig[np.ix_(sel[ok], sel[ok])]
    return Wn


def window_rel_err(Wd, Wr):
    """calib_cov_cases.rel_err over the live rows of a window"""
    live = np.diag(Wr) > 0
    if not live.any():
        return 0.0
    return CC.rel_err(Wd[np.ix_(live, live)], Wr[np.ix_(live, live)])
