"""Accuracy of the float64 reference of tests/test_gpu_landmark_cov.py, per case: python tests/golden/make_landmark_cov_ref.py  ->  tests/golden/landmark_cov_ref.npz

The rule and the pattern of make_calib_cov_ref.py and make_trajcov_ref.py (whose mpmath columns and per-case job this generator reuses).  For every case of
tests/landmark_cov_cases.py the damped system A_R is built from the ORACLE's dense H (CPU); the windows of Sigma = s A_R^-1 s of the probe landmarks
(landmark_cov_cases.probe_landmarks: the inverse depth and the 31 scalars of the camera-frame pose at the reference time) are computed once as the test computes them
(float64 Cholesky, trajcov_cases.reference_sigma) and once with mpmath at 40 digits, and
    err = max over the probe windows of max |W64 - W_mp| / sqrt(W_mp_ii W_mp_jj)
is stored under the case's name.  The GPU test allows 10 x err (floor 1e-11) between a device window and ITS float64 reference.  Pure-Python mpmath: minutes per
case; the cases run in a process pool."""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import landmark_cov_cases as LC   # noqa: E402
import make_trajcov_ref as MT     # noqa: E402


def main():
    jobs, problems, dense = [], {}, {}
    for name, (key, locks, radius, scaling) in LC.CASES.items():
        if key not in problems:
            problems[key] = LC.problem(key)
        P = problems[key]
        if (key, locks) not in dense:
            dense[(key, locks)] = MT.dense_h(P, locks)
        windows = [LC.window_indices(P, P["state0"], l) for l in LC.probe_landmarks(key, P)]
        jobs.append((name, dense[(key, locks)], P["n_knots"], P["n_landmarks"], locks, radius, scaling, windows))
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = dict(pool.map(MT.one, jobs, chunksize=1))
    np.savez(os.path.join(ROOT, "tests", "golden", "landmark_cov_ref.npz"), **res)


if __name__ == "__main__":
    main()
