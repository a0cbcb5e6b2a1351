"""Accuracy of the float64 reference of tests/test_gpu_ptcov.py, per case: python tests/golden/make_ptcov_ref.py  ->  tests/golden/ptcov_ref.npz

The rule and the pattern of make_calib_cov_ref.py, make_trajcov_ref.py and make_landmark_cov_ref.py (whose mpmath columns and per-case job this generator reuses).
For every case of tests/ptcov_cases.py the damped system A_R is built from the ORACLE's dense H (CPU); the 55-scalar windows of Sigma = s A_R^-1 s of the probe
points (ptcov_cases.probe_times: the first and the last interval, on a knot, inside the window of t_map; each with the four knots at t_map and the LiDAR's scalars) are
computed once as the test computes them (float64 Cholesky, trajcov_cases.reference_sigma) and once with mpmath at 40 digits, and
    err = max over the probe windows of max |W64 - W_mp| / sqrt(W_mp_ii W_mp_jj)
is stored under the case's name.  The GPU test allows 10 x err (floor 1e-11) between a device window and ITS float64 reference.  Pure-Python mpmath: a minute or two
per case; the cases run in a process pool."""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "lvi-exc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import make_trajcov_ref as MT   # noqa: E402
import ptcov_cases as PC        # noqa: E402


def main():
    P = PC.problem()
    windows = [PC.window_indices(P, P["state0"], t) for t in PC.probe_times(P)]
    dense = {m: MT.dense_h(P, locks) for m, locks in PC.MASKS.items()}
    jobs = [(name, dense[m], P["n_knots"], P["n_landmarks"], PC.MASKS[m], radius, scaling, windows) for name, (m, radius, scaling) in PC.CASES.items()]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = dict(pool.map(MT.one, jobs, chunksize=1))
    np.savez(os.path.join(ROOT, "tests", "golden", "ptcov_ref.npz"), **res)


if __name__ == "__main__":
    main()
