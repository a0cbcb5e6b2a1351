"""Cases and float64 reference of the JOINT calibration covariance (lvx_calibration_covariance_shared), shared by tests/test_gpu_joint_cov.py, tests/test_joint_cov_cases.py
and the generator of the reference's own accuracy, tests/golden/make_joint_cov_ref.py.  Not a test module.

Definition (include/lvx.h): every rank has a tangent vector [private scalars | 14 shared extrinsic scalars]; H is the joint normal matrix over the union of these vectors
with every rank's shared scalars aliased onto rank 0's (tests/test_gpu_shared.py::JointOracle.evaluate, here for any number of ranks), F its free scalars,
    s = 1 / (1 + sqrt(diag H_FF)) (or 1),   A_R = s H_FF s + diag(clip(diag(s H_FF s), 1e-6, 1e32)) / R,   cov_r = [ s A_R^-1 s ] over rank r's 8 private calibration
scalars and the 14 shared ones; M = the Schur complement of A_R onto the free shared scalars; own_r = s_sh (C_r - B_r^T A_r^-1 B_r) s_sh, rank r's term of M (private
damping inside A_r, no shared damping), so that sum_r own_r + diag(lmd_sh) / R = M."""
import numpy as np

import calib_cov_cases as CC
import lvx
import sharded
import synth
from oracle import lm as LM
from oracle import oracle as O

N_SHARED = 14
N_PRIV = CC.N_CALIB - N_SHARED
MASKS = dict(CC.MASKS, free=0)          # free: nothing locked, the time offsets are free
RADII = CC.RADII


def sequence(r, **over):
    """the smallest shapes that still have hubs, a band, landmarks and both sensors; rank r is 0.1 s longer than rank r - 1.  0.4 s is the shortest sequence
    synth.make_problem can give landmarks to: its camera frames lie in [t0 + 0.1, t1 - 0.2), which is empty at 0.3 s."""
    kw = dict(seed=40 + r, duration=0.4 + 0.1 * r, n_surfel=150, n_planes=8, n_landmarks=8, n_camsurf=0)
    kw.update(over)
    return synth.make_problem(**kw)


def sequences(world, over=None):
    """[(problem, state)] with ONE starting guess of the shared extrinsics, state [7 N + 16, 7 N + 32); over: {rank: make_problem overrides}"""
    seqs, ref = [], None
    for r in range(world):
        P = sequence(r, **(over or {}).get(r, {}))
        N = P["n_knots"]
        s = P["state0"].copy()
        if ref is None:
            ref = s[7 * N + 16:7 * N + 32].copy()
        s[7 * N + 16:7 * N + 32] = ref
        seqs.append((P, s))
    return seqs


# the sets of sequences the tests use: two ranks, three ranks of unequal length, a rank without camera data
SETS = {"w2": (2, None), "w3": (3, None), "nocam": (2, {1: dict(n_landmarks=0)})}
# cases beyond the two-rank grid MASKS x RADII x scaling: (set, mask, radius, scaling)
EXTRA = (("w3", "solve2", 1e4, True), ("nocam", "solve2", 1e8, True))


def case_name(mask, radius, scaling, key="w2"):
    return ("" if key == "w2" else key + "_") + CC.case_name(mask, radius, scaling)


def all_cases():
    return [("w2", m, R, sc) for m in MASKS for R in RADII for sc in (True, False)] + list(EXTRA)


def oracle_h(P, state, locks):
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    return o.evaluate(state, normal_eq=True)["H"]


def joint_h(Hs, Ns, Ls, locks):
    """The aliased joint H of per-rank dense matrices, its free indices, per rank the joint indices of its 22 calibration scalars, the joint indices of the shared scalars,
    and per rank the joint indices of its free private scalars."""
    nt = [H.shape[0] for H in Hs]
    off = np.concatenate([[0], np.cumsum(nt)])
    sh = [sharded.shared_tangent_indices(N) for N in Ns]
    H = np.zeros((off[-1], off[-1]))
    free, cal, priv = [], [], []
    for r, Hr in enumerate(Hs):
        idx = off[r] + np.arange(nt[r])
        idx[sh[r]] = off[0] + sh[0]
        np.add.at(H, (idx[:, None], idx[None, :]), Hr)
        fr = LM.free_tangent_indices(Ns[r], Ls[r], locks)
        priv.append(off[r] + np.setdiff1d(fr, sh[r]))
        free.append(idx[fr] if r == 0 else priv[r])
        cal.append(idx[6 * Ns[r]:6 * Ns[r] + CC.N_CALIB])
    return H, np.concatenate(free), cal, off[0] + sh[0], priv


def schur(A, elim, keep):
    """Schur complement of A onto `keep` after eliminating `elim`, in extended precision (numpy longdouble), returned as float64.  The complement is the small difference
    of large terms (at radius 1e8 its largest entry is 1e-6 of theirs): float64 products summed in different orders differ by 1e-9 of it, which would hide whether
    sum_r own_r + lmd / R = M holds; the covariance reference stays a plain float64 Cholesky."""
    order = np.concatenate([np.asarray(elim, dtype=np.int64), np.asarray(keep, dtype=np.int64)])
    B = A[np.ix_(order, order)].astype(np.longdouble)
    ne = len(elim)
    for k in range(ne):
        c = B[k + 1:, k].copy()
        B[k + 1:, k + 1:] -= np.outer(c / B[k, k], c)
    return B[ne:, ne:].astype(np.float64)


def reference(Hs, Ns, Ls, locks, radius, scaling):
    """float64: Cholesky of A_R and one triangular solve for all ranks' calibration scalars, the per-rank restriction, the shared Schur complement M, per-rank own_info
    (14 x 14 canonical slots, 0 at locked ones) and the shared damping.  ranks[r]: cov over cidx (the rank's free calibration scalars c), scale of those."""
    import scipy.linalg as sl
    H, free, cal, shared, priv = joint_h(Hs, Ns, Ls, locks)
    A, s = CC.damped_system(H, free, radius, scaling)
    where = {int(j): k for k, j in enumerate(free)}
    pos_of = lambda js: np.array([where.get(int(j), -1) for j in js], dtype=np.int64)   # noqa: E731
    cpos = [pos_of(c) for c in cal]
    upos = np.unique(np.concatenate([p[p >= 0] for p in cpos]))
    L = np.linalg.cholesky(A)
    E = np.zeros((len(free), len(upos))); E[upos, np.arange(len(upos))] = 1.0
    X = sl.solve_triangular(L, E, lower=True)
    C = X.T @ X
    col = {int(p): k for k, p in enumerate(upos)}
    ranks = []
    for p in cpos:
        cidx = np.nonzero(p >= 0)[0]
        k = np.array([col[int(q)] for q in p[cidx]])
        ranks.append(dict(cidx=cidx, cov=C[np.ix_(k, k)] * s[p[cidx]][:, None] * s[p[cidx]][None, :], scale=s[p[cidx]]))
    spos = pos_of(shared)
    slots = np.nonzero(spos >= 0)[0]
    sp = spos[slots]
    rest = np.setdiff1d(np.arange(len(free)), sp)
    M = schur(A, rest, sp)
    lmd = np.clip(np.diag(H[np.ix_(free, free)])[sp] * s[sp] ** 2, 1e-6, 1e32)
    own = []
    for r, Hr in enumerate(Hs):
        shr = sharded.shared_tangent_indices(Ns[r])[slots]
        pp = pos_of(priv[r])
        Ar = A[np.ix_(np.concatenate([pp, sp]), np.concatenate([pp, sp]))].copy()
        Ar[len(pp):, len(pp):] = Hr[np.ix_(shr, shr)] * s[sp][:, None] * s[sp][None, :]   # C_r in the joint scale, no shared damping
        T = schur(Ar, np.arange(len(pp)), len(pp) + np.arange(len(sp)))
        full = np.zeros((N_SHARED, N_SHARED))
        full[np.ix_(slots, slots)] = 0.5 * (T + T.T)
        own.append(full)
    return dict(ranks=ranks, M=0.5 * (M + M.T), own=own, lmd_shared=lmd, shared_free_slot=slots, A=A, s=s, cpos=cpos)


def rel_err(cov, ref):
    return CC.rel_err(cov, ref)
