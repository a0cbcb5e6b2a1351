"""Accuracy of the float64 reference of tests/test_gpu_projcov.py, per case: python tests/golden/make_projcov_ref.py  ->  tests/golden/projcov_ref.npz

The rule and the pattern of make_ptcov_ref.py (make_trajcov_ref.py's mpmath columns and per-case job).  For every case of tests/projcov_cases.py the damped system
A_R is built from the ORACLE's dense H (CPU); the 62-scalar windows of Sigma = s A_R^-1 s of the probe images (projcov_cases.probe_times: the first and the last
interval, on a knot, t_map and just behind it; each with the four knots at t_map and both sensors' scalars) are computed once as the test computes them (float64
Cholesky, trajcov_cases.reference_sigma) and once with mpmath at 40 digits, and
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
import projcov_cases as JC      # noqa: E402


def main():
    P = JC.problem()
    windows = [JC.window_indices(P, P["state0"], t) for t in JC.probe_times(P)]
    dense = {m: MT.dense_h(P, locks) for m, locks in JC.MASKS.items()}
    jobs = [(name, dense[m], P["n_knots"], P["n_landmarks"], JC.MASKS[m], radius, scaling, windows) for name, (m, radius, scaling) in JC.CASES.items()]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = dict(pool.map(MT.one, jobs, chunksize=1))
    np.savez(os.path.join(ROOT, "tests", "golden", "projcov_ref.npz"), **res)


if __name__ == "__main__":
    main()
