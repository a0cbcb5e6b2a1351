"""Accuracy of the float64 reference of tests/test_gpu_calib_cov.py, per case: python tests/golden/make_calib_cov_ref.py  ->  tests/golden/calib_cov_ref.npz

For every case of tests/calib_cov_cases.py the damped system A_R is built from the ORACLE's dense H (CPU), the calibration block of s A_R^-1 s is computed once as the test
computes it (float64 Cholesky, calib_cov_cases.reference) and once with mpmath at 40 digits (Cholesky + forward substitution on the same float64 entries of A_R), and
    err = max |cov64 - cov_mp| / sqrt(cov_mp_ii cov_mp_jj)
is stored under the case's name.  The GPU test allows 10 x err (floor 1e-11) between the device's result and ITS float64 reference: two float64 eliminations in different
orders.  Pure-Python mpmath: about a minute per 300-scalar case, a few minutes for the 500-scalar ones; the cases run in a process pool."""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import calib_cov_cases as CC   # noqa: E402
import lvx                     # noqa: E402
import synth                   # noqa: E402
from oracle import oracle as O   # noqa: E402


def mp_cov(A, pos, s):
    import mpmath
    mpmath.mp.dps = 40
    n = A.shape[0]
    M = [[mpmath.mpf(float(A[i, j])) for j in range(i + 1)] for i in range(n)]
    Lr = []
    for i in range(n):
        row = M[i]
        for j in range(i + 1):
            Lj = Lr[j] if j < i else row
            t = row[j] - sum(row[k] * Lj[k] for k in range(j))
            row[j] = mpmath.sqrt(t) if j == i else t / Lj[j]
        Lr.append(row)
    X = []
    for p in pos:   # L x = e_p
        x = [mpmath.mpf(0)] * n
        for i in range(int(p), n):
            t = (mpmath.mpf(1) if i == p else mpmath.mpf(0)) - sum(Lr[i][k] * x[k] for k in range(int(p), i))
            x[i] = t / Lr[i][i]
        X.append(x)
    k = len(pos)
    return [[sum(X[a][i] * X[b][i] for i in range(n)) * mpmath.mpf(float(s[pos[a]])) * mpmath.mpf(float(s[pos[b]])) for b in range(k)] for a in range(k)]


def one(job):
    name, H, N, L, locks, radius, scaling = job
    free, pos, _ = CC.free_sets(N, L, locks)
    A, s = CC.damped_system(H, free, radius, scaling)
    c64 = CC.reference(H, N, L, locks, radius, scaling)["cov"]
    cm = mp_cov(A, pos, s)
    k = len(pos)
    err = max(abs((c64[a, b] - cm[a][b]) / (cm[a][a] * cm[b][b]) ** 0.5) for a in range(k) for b in range(k))
    print("%-28s free %4d  err %.3e" % (name, len(free), float(err)), flush=True)
    return name, float(err)


def dense_h(P, locks):
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    return o.evaluate(P["state0"], normal_eq=True)["H"]


def main():
    jobs = []
    P = synth.make_problem(**CC.SMALL)
    for mask, locks in CC.MASKS.items():
        H = dense_h(P, locks)
        for radius in CC.RADII:
            for scaling in (True, False):
                jobs.append((CC.case_name(mask, radius, scaling), H, P["n_knots"], P["n_landmarks"], locks, radius, scaling))
    Pn = synth.make_problem(**CC.ND)
    Hn = dense_h(Pn, CC.ND_LOCKS)
    for radius in CC.RADII:
        jobs.append((CC.case_name("nd", radius, True), Hn, Pn["n_knots"], Pn["n_landmarks"], CC.ND_LOCKS, radius, True))
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = dict(pool.map(one, jobs, chunksize=1))
    np.savez(os.path.join(ROOT, "tests", "golden", "calib_cov_ref.npz"), **res)


if __name__ == "__main__":
    main()
