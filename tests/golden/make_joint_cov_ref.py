"""Accuracy of the float64 reference of tests/test_gpu_joint_cov.py, per case: python tests/golden/make_joint_cov_ref.py  ->  tests/golden/joint_cov_ref.npz

The procedure of make_calib_cov_ref.py on the JOINT system: for every case of tests/joint_cov_cases.py the aliased joint H is built from the ORACLE's per-sequence dense H
(CPU), the damped system A_R from it, and the block of s A_R^-1 s over all ranks' calibration scalars is computed once as the test computes it (float64 Cholesky,
joint_cov_cases.reference) and once with mpmath at 40 digits on the same float64 entries of A_R.  Stored under the case's name: the largest, over the ranks, of
    err = max |cov64 - cov_mp| / sqrt(cov_mp_ii cov_mp_jj)
over the rank's own 8 private and the 14 shared scalars.  The GPU test allows 10 x err (floor 1e-11).  Pure-Python mpmath: a few minutes per 500-scalar case, about a
quarter of an hour for the three-rank one; the cases run in a process pool."""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import joint_cov_cases as JC          # noqa: E402
from make_calib_cov_ref import mp_cov   # noqa: E402


def one(job):
    name, Hs, Ns, Ls, locks, radius, scaling = job
    ref = JC.reference(Hs, Ns, Ls, locks, radius, scaling)
    upos = np.unique(np.concatenate([p[p >= 0] for p in ref["cpos"]]))
    cm = mp_cov(ref["A"], upos, ref["s"])
    col = {int(p): k for k, p in enumerate(upos)}
    err = 0.0
    for p, rk in zip(ref["cpos"], ref["ranks"]):
        k = [col[int(q)] for q in p[rk["cidx"]]]
        c64 = rk["cov"]
        err = max(err, max(float(abs((c64[a, b] - cm[k[a]][k[b]]) / (cm[k[a]][k[a]] * cm[k[b]][k[b]]) ** 0.5)) for a in range(len(k)) for b in range(len(k))))
    print("%-32s free %4d  err %.3e" % (name, ref["A"].shape[0], err), flush=True)
    return name, err


def main():
    jobs, H = [], {}
    for key, mask, radius, scaling in JC.all_cases():
        world, over = JC.SETS[key]
        seqs = JC.sequences(world, over)
        locks = JC.MASKS[mask]
        if (key, mask) not in H:
            H[key, mask] = [JC.oracle_h(P, s, locks) for P, s in seqs]
        jobs.append((JC.case_name(mask, radius, scaling, key), H[key, mask], [P["n_knots"] for P, _ in seqs], [P["n_landmarks"] for P, _ in seqs], locks, radius, scaling))
    jobs.sort(key=lambda j: -sum(h.shape[0] for h in j[1]))   # the longest first
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = dict(pool.map(one, jobs, chunksize=1))
    np.savez(os.path.join(ROOT, "tests", "golden", "joint_cov_ref.npz"), **res)


if __name__ == "__main__":
    main()
