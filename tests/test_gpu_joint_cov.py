"""lvx_calibration_covariance_shared on the device: the calibration covariance of the JOINT problem — several sequences with private trajectories, gravity, biases and
landmarks and SHARED rig extrinsics — against a float64 numpy Cholesky of the same damped joint system, built from every rank's own dense export and aliased as
tests/test_gpu_shared.py::JointOracle does (tests/joint_cov_cases.py).  The ranks run as threads of this process on one GPU and meet in sharded.ThreadAllReduce.

Tolerance of the covariance, the rule of tests/test_gpu_calib_cov.py: measure max |cov - ref| / sqrt(ref_ii ref_jj) over a rank's 8 private and the 14 shared scalars; a
case may use 10 x the reference's own error against mpmath at 40 digits (tests/golden/joint_cov_ref.npz, written by tests/golden/make_joint_cov_ref.py from the
oracle's H), floor 1e-11: two float64 eliminations in different orders.  Reference's own error, the bound it gives, and the figure observed on the first MI355X run
(the larger of the two ranks):
    case (two ranks)              reference vs mpmath   allowed             observed
    solve1 R 1e4  scaled / plain   3.6e-12 / 1.9e-12   3.6e-11 / 1.9e-11   4.1e-12 / 5.3e-12
    solve1 R 1e8  scaled / plain   1.4e-09 / 8.5e-10   1.4e-08 / 8.5e-09   1.6e-09 / 3.2e-09
    solve2 R 1e4  scaled / plain   4.8e-12 / 2.5e-12   4.8e-11 / 2.5e-11   2.6e-12 / 1.1e-12
    solve2 R 1e8  scaled / plain   1.4e-09 / 1.6e-09   1.4e-08 / 1.6e-08   2.7e-09 / 2.3e-09
    solve3 R 1e4  scaled / plain   9.3e-14 / 2.2e-13   1e-11 / 1e-11       2.6e-13 / 1.5e-13
    solve3 R 1e8  scaled / plain   4.6e-14 / 1.3e-13   1e-11 / 1e-11       9.4e-14 / 1.2e-13
    free   R 1e4  scaled / plain   2.3e-12 / 1.7e-12   2.3e-11 / 1.7e-11   1.8e-12 / 6.7e-13
    free   R 1e8  scaled / plain   2.1e-09 / 1.7e-09   2.1e-08 / 1.7e-08   2.5e-09 / 3.6e-09
    three ranks (930 free scalars), solve2 R 1e4 scaled:      6.6e-12, allowed 6.6e-11, observed 8.0e-12
    a rank without camera data, solve2 R 1e8 scaled:          1.3e-09, allowed 1.3e-08, observed 2.8e-09
    (every case within 3.8 x the reference's own error); sum of own_info + shared damping against V w V^T: at most 4.1e-15 of the largest entry;
    world 1 against lvx_calibration_covariance: 5.8e-10 (solve2, R 1e8), 7.9e-13 (solve1, R 1e4), 8.7e-13 (free, R 1e4); RCCL against the callback transport: 0
Spectrum and scale are held as tests/test_gpu_calib_cov.py::_compare holds them (eigenvalue to tol_case * lambda + 1e-12 * lambda_max, eigenvectors through Davis-Kahan
where the gap determines them, scale to 4 eps); the reference forms the shared Schur complement in extended precision, so its share of the eigenvalue error is nil.
The sequences are 0.4 s + 0.1 s per rank: the shortest synth.make_problem gives landmarks to.  World 1 against lvx_calibration_covariance and RCCL against the callback
transport compare two device results of the one-sequence problem: the tolerance of the two-rank case of the same mask and radius is used, whose system contains it."""
import os
import subprocess
import threading

import numpy as np
import pytest

import calib_cov_cases as CC
import joint_cov_cases as JC
import lvx
import sharded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "joint_cov_ref.npz")))
TAU = CC.TAU
_SEQS, _RUNS = {}, {}
_EXPORT = threading.Lock()


def _evaluate_dense(g, x):
    """evaluate with the dense export, one rank at a time: the export copies on the legacy stream, which HIP refuses while another thread's context captures its pass"""
    with _EXPORT:
        return g.evaluate(x, normal_eq=True, residuals=False)["H"]


def _tol(name):
    return max(10.0 * float(REF_ERR[name]), 1e-11)


def _seqs(key):
    if key not in _SEQS:
        _SEQS[key] = JC.sequences(*JC.SETS[key])
    return _SEQS[key]


def _run_ranks(seqs, body, locks, switches=()):
    """body(rank, ctx, allreduce) in one thread per rank; locks: one mask or one per rank.  Returns the per-rank results; a rank left inside a reduction fails the join."""
    world = len(seqs)
    ar = sharded.ThreadAllReduce(world)
    res, err = [None] * world, [None] * world
    lk = list(locks) if isinstance(locks, (list, tuple)) else [locks] * world

    def work(r):
        try:
            g = lvx.Context(0)
            for k, v in switches:
                g.set_switch(k, v)
            lvx.load_problem(g, seqs[r][0], lk[r])
            res[r] = body(r, g, ar.rank_fn(r))
            g.close()
        except BaseException as e:   # noqa: BLE001
            err[r] = e
            ar.bar.abort()
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank did not come back from the call"
    for e in err:
        if e is not None:
            raise e
    return res


def _joint(key, mask, radius, scaling):
    """one run of the case on the device and its reference, shared by the tests that read it: (records per rank, reference)"""
    k = (key, mask, radius, scaling)
    if k not in _RUNS:
        seqs, locks = _seqs(key), JC.MASKS[mask]

        def body(r, g, allreduce):
            H = _evaluate_dense(g, seqs[r][1])
            allreduce(np.zeros(1), "sum")   # every rank has its export before any goes on
            return H, g.calibration_covariance_shared(allreduce, radius, scaling), g.layout()
        res = _run_ranks(seqs, body, locks)
        ref = JC.reference([h for h, _, _ in res], [P["n_knots"] for P, _ in seqs], [P["n_landmarks"] for P, _ in seqs], locks, radius, scaling)
        _RUNS[k] = ([rec for _, rec, _ in res], ref, [lo for _, _, lo in res])
    return _RUNS[k]


def _compare(recs, ref, layouts, radius, tol, label):
    """every rank's record against the reference: covariance, constants, scale, spectrum.  Returns the largest covariance error."""
    slots = ref["shared_free_slot"]
    w, V = np.linalg.eigh(ref["M"])
    worst = 0.0
    for r, (rec, rk) in enumerate(zip(recs, ref["ranks"])):
        cidx = rk["cidx"]
        assert list(rec["free_index"]) == list(cidx) and list(rec["shared_free_slot"]) == list(slots) and rec["radius"] == radius and rec["world"] == len(recs)
        assert rec["n_hub_eliminated"] == layouts[r]["n_border"] - 22
        err = JC.rel_err(rec["cov"][np.ix_(cidx, cidx)], rk["cov"])
        eig_err = np.abs(rec["info_eig"] - w) / (tol * w + 1e-12 * w[-1])
        print("%-30s rank %d  cov err %.3e (allowed %.3e)  eig err / allowed %.3f  sweeps %d  eig %.3e .. %.3e" % (label, r, err, tol, eig_err.max(), rec["sweeps"], rec["info_eig"][0], rec["info_eig"][-1]))
        worst = max(worst, err)
        assert err <= tol
        const = np.setdiff1d(np.arange(22), cidx)
        assert not rec["cov"][const, :].any() and not rec["cov"][:, const].any() and not rec["sigma"][const].any()
        assert np.array_equal(rec["sigma"], np.sqrt(np.diag(rec["cov"])))
        assert np.abs(rec["scale"][cidx] / rk["scale"] - 1).max() <= 4 * np.finfo(float).eps
        assert (rec["info_eig"] > 0).all() and (np.diff(rec["info_eig"]) >= 0).all()
        assert eig_err.max() <= 1.0
        n = len(w)
        assert np.abs(rec["info_vec"].T @ rec["info_vec"] - np.eye(n)).max() <= 1e-13
        for k in range(n):
            nb = [j for j in (k - 1, k + 1) if 0 <= j < n]
            if all(abs(w[k] - w[j]) > 1e-6 * max(w[k], w[j]) for j in nb):
                angle = max((tol * max(w[k], w[j]) + 1e-12 * w[-1]) / abs(w[k] - w[j]) for j in nb) if nb else 0.0
                if angle <= 0.05:
                    assert 1 - abs(rec["info_vec"][:, k] @ V[:, k]) <= 0.5 * (4 * angle) ** 2 + 1e-13, (label, r, k, angle)
    return worst


GRID = [(m, R, sc) for m in JC.MASKS for R in JC.RADII for sc in (True, False)]


# 1. parity with the dense joint system, two ranks
@pytest.mark.parametrize("mask,radius,scaling", GRID)
def test_parity_with_the_dense_joint_system(mask, radius, scaling):
    recs, ref, lo = _joint("w2", mask, radius, scaling)
    name = JC.case_name(mask, radius, scaling)
    _compare(recs, ref, lo, radius, _tol(name), name)
    assert all(l["solver_fallbacks"] == 0 for l in lo)


# 2. one set of shared results
@pytest.mark.parametrize("mask,radius,scaling", GRID)
def test_shared_block_is_identical_on_all_ranks(mask, radius, scaling):
    (a, b), _, _ = _joint("w2", mask, radius, scaling)
    assert a["world"] == 2 and b["world"] == 2
    assert np.array_equal(a["cov"][8:, 8:], b["cov"][8:, 8:]) and np.array_equal(a["sigma"][8:], b["sigma"][8:]) and np.array_equal(a["scale"][8:], b["scale"][8:])
    assert np.array_equal(a["info_eig"], b["info_eig"]) and np.array_equal(a["info_vec"], b["info_vec"]) and a["sweeps"] == b["sweeps"]


# 3. what each sequence contributed adds up to the decomposed matrix
@pytest.mark.parametrize("mask,radius,scaling", GRID)
def test_own_info_of_all_ranks_and_the_shared_damping_rebuild_the_matrix(mask, radius, scaling):
    recs, ref, _ = _joint("w2", mask, radius, scaling)
    sl = recs[0]["shared_free_slot"]
    M = (recs[0]["info_vec"] * recs[0]["info_eig"]) @ recs[0]["info_vec"].T
    S = sum(rec["own_info"][np.ix_(sl, sl)] for rec in recs) + np.diag(ref["lmd_shared"]) / radius
    tol = max(_tol(JC.case_name(mask, radius, scaling)), 1e-12)
    err = np.abs(S - M).max() / np.abs(M).max()
    print("%s: sum of own_info + shared damping against V w V^T: %.3e (allowed %.3e)" % (JC.case_name(mask, radius, scaling), err, tol))
    assert err <= tol
    locked = np.setdiff1d(np.arange(14), sl)
    for rec, own in zip(recs, ref["own"]):
        assert not rec["own_info"][locked, :].any() and not rec["own_info"][:, locked].any() and np.array_equal(rec["own_info"], rec["own_info"].T)
        assert np.abs(rec["own_info"] - own).max() <= tol * np.abs(M).max() + 1e-12 * np.abs(own).max()


# 4. three ranks of unequal length
def test_three_ranks_of_unequal_length():
    key, mask, radius, scaling = JC.EXTRA[0]
    recs, ref, lo = _joint(key, mask, radius, scaling)
    assert len(recs) == 3 and len({l["n_band"] for l in lo}) == 3
    name = JC.case_name(mask, radius, scaling, key)
    _compare(recs, ref, lo, radius, _tol(name), name)
    assert np.array_equal(recs[0]["cov"][8:, 8:], recs[2]["cov"][8:, 8:]) and np.array_equal(recs[1]["info_vec"], recs[2]["info_vec"])


# 5. a rank without camera data
def test_rank_without_camera_data_contributes_nothing_to_the_camera():
    """Rank 1 has no landmark, the camera extrinsics are free: its own_info has nothing in the camera's rows and columns (slots 7 .. 12; exactly 0, no row of its
    problem touches them), the joint camera covariance is that of the reference (rank 0's data decide it), and with that rank ALONE the camera slots sit at the LM floor
    1e-6 / R, as in tests/test_gpu_calib_cov.py::test_unobserved_camera_extrinsics_show_in_the_spectrum."""
    key, mask, radius, scaling = JC.EXTRA[1]
    recs, ref, lo = _joint(key, mask, radius, scaling)
    name = JC.case_name(mask, radius, scaling, key)
    _compare(recs, ref, lo, radius, _tol(name), name)
    cam = np.arange(7, 13)
    assert list(recs[1]["shared_free_slot"]) == list(range(6)) + list(cam)
    assert not recs[1]["own_info"][cam, :].any() and not recs[1]["own_info"][:, cam].any() and (np.diag(recs[0]["own_info"])[cam] > 0).all()
    P, x = _seqs(key)[1]
    g = lvx.Context(0)
    g.set_switch("DETERMINISTIC", 1)
    lvx.load_problem(g, P, JC.MASKS[mask])
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    a = g.calibration_covariance_shared(lambda buf, op: None, radius)
    g.close()
    assert a["world"] == 1 and list(a["shared_free_slot"]) == list(range(6)) + list(cam)
    assert np.abs(a["info_eig"][:6] / (1e-6 / radius) - 1).max() <= 1e-10
    assert not a["info_vec"][:6, :6].any() and not a["info_vec"][6:, 6:].any()
    assert np.abs(np.diag(a["cov"])[15:21] / (radius / 1e-6) - 1).max() <= 1e-10 and not a["cov"][15:21, :15].any()


# 6. one rank is the single-sequence problem
@pytest.mark.parametrize("mask,radius", [("solve2", 1e8), ("solve1", 1e4), ("free", 1e4)])
def test_world_of_one_equals_the_single_sequence_call(mask, radius):
    """The identity callback makes a joint problem of one rank: the same damped system as lvx_calibration_covariance on a context that takes no part in a joint solve,
    eliminated in another order (hub, private, then the shared 14 decomposed; there all 22 decomposed at once)."""
    P, x = _seqs("w2")[1]
    rec = []
    for joint in (True, False):
        g = lvx.Context(0)
        lvx.load_problem(g, P, JC.MASKS[mask])
        g.evaluate(x, normal_eq=True, dense=False, residuals=False)
        rec.append(g.calibration_covariance_shared(lambda buf, op: None, radius) if joint else g.calibration_covariance(radius))
        if joint:
            none = g.calibration_covariance_shared(None, radius)     # no callback, no communicator: the same joint problem of one rank
            fi = none["free_index"]
            assert none["world"] == 1 and JC.rel_err(none["cov"][np.ix_(fi, fi)], rec[0]["cov"][np.ix_(fi, fi)]) <= _tol(JC.case_name(mask, radius, True))
        g.close()
    a, b = rec
    idx = b["free_index"]
    tol = _tol(JC.case_name(mask, radius, True))
    err = JC.rel_err(a["cov"][np.ix_(idx, idx)], b["cov"][np.ix_(idx, idx)])
    print("world 1 against lvx_calibration_covariance, %s R %g: %.3e (allowed %.3e)" % (mask, radius, err, tol))
    assert list(a["free_index"]) == list(idx) and a["world"] == 1 and err <= tol
    assert np.abs(a["scale"] / b["scale"] - 1).max() <= 4 * np.finfo(float).eps
    assert np.abs(a["sigma"][idx] / b["sigma"][idx] - 1).max() <= tol


# 7. transports
def test_rccl_and_callback_transports_agree_on_one_rank():
    """Both transports on the same sequence, world of one (all a single-GPU node can form; the multi-rank protocol is the one the thread transport tests above): pack -> ncclAllReduce ->
    decomposition queued on the stream, against the message staged through the host."""
    P, x = _seqs("w2")[0]
    radius = 1e8
    g = lvx.Context(0)
    lvx.load_problem(g, P, TAU)
    g.evaluate(x, normal_eq=True, dense=False, residuals=False)
    a = g.calibration_covariance_shared(lambda buf, op: None, radius)
    g.rccl_init(g.rccl_unique_id(), 0, 1)
    g.collective_count(reset=True)
    b = g.calibration_covariance_shared(None, radius)
    assert g.collective_count() == 2 and g.joint_shared_count() == 14
    g.rccl_finalize()
    g.close()
    idx = a["free_index"]
    tol = _tol(JC.case_name("solve2", radius, True))
    err = JC.rel_err(b["cov"][np.ix_(idx, idx)], a["cov"][np.ix_(idx, idx)])
    print("RCCL against callback transport: %.3e (allowed %.3e)" % (err, tol))
    assert err <= tol and b["world"] == 1 and list(b["free_index"]) == list(idx)
    assert np.abs(b["info_eig"] / a["info_eig"] - 1).max() <= tol + 1e-12 * a["info_eig"][-1] / a["info_eig"][0]


# 8. collectives and failures: codes on every rank, nobody left inside a reduction
def test_two_collectives_per_call_and_every_failure_leaves_together():
    seqs = _seqs("w2")

    def codes(body, locks=TAU):
        def wrapped(r, g, allreduce):
            g.evaluate(seqs[r][1], normal_eq=True, dense=False, residuals=False)
            return body(r, g, allreduce)
        return _run_ranks(seqs, wrapped, locks)

    def attempt(g, allreduce, **kw):
        try:
            return g.calibration_covariance_shared(allreduce, 1e4, **kw)["sweeps"]
        except lvx.LvxError as e:
            return e

    def counted(r, g, allreduce):
        g.collective_count(reset=True)
        g.calibration_covariance_shared(allreduce, 1e4)
        n1 = g.collective_count()
        g.calibration_covariance_shared(allreduce, 1e8, jacobi_scaling=False)
        return n1, g.collective_count()
    assert codes(counted) == [(2, 4), (2, 4)]

    # the sweep cap of ONE rank: the smallest cap applies everywhere, every rank reports the decomposition that did not converge; the contexts stay usable
    def capped(r, g, allreduce):
        first = attempt(g, allreduce, max_sweeps=1 if r == 1 else None)
        return first, attempt(g, allreduce)
    for first, second in codes(capped):
        assert isinstance(first, lvx.LvxError) and first.code == lvx.E_NOTPD and "not converged after 1 sweeps" in str(first)
        assert isinstance(second, int) and second > 1

    # a rank without an evaluation
    def unevaluated(r, g, allreduce):
        return attempt(g, allreduce)
    res = _run_ranks(seqs, lambda r, g, ar: (g.evaluate(seqs[r][1], normal_eq=True, dense=False, residuals=False) if r == 0 else None, unevaluated(r, g, ar))[1], TAU)
    assert all(isinstance(e, lvx.LvxError) and e.code == lvx.E_STATE for e in res)

    # a shared scalar locked on one rank only
    res = codes(lambda r, g, ar: attempt(g, ar), locks=[TAU, TAU | lvx.LOCK_CAM_P])
    assert all(isinstance(e, lvx.LvxError) and e.code == lvx.E_ARG and "locked on some ranks" in str(e) for e in res)


def test_lost_pivot_on_the_reduction_route_is_redone_sequentially_on_every_rank():
    """TEST_BAD_PIVOT declares a pivot failure behind the block chain: the vote travels with the message, every rank repeats the elimination with the sequential band
    Cholesky (one more collective) and the result is that of the plain run."""
    seqs, radius = _seqs("w2"), 1e4

    def body(r, g, allreduce):
        H = _evaluate_dense(g, seqs[r][1])
        allreduce(np.zeros(1), "sum")
        g.collective_count(reset=True)
        return H, g.calibration_covariance_shared(allreduce, radius), g.layout(), g.collective_count()
    res = _run_ranks(seqs, body, TAU, (("TEST_BAD_PIVOT", 1),))
    ref = JC.reference([h for h, _, _, _ in res], [P["n_knots"] for P, _ in seqs], [P["n_landmarks"] for P, _ in seqs], TAU, radius, True)
    name = JC.case_name("solve2", radius, True)
    _compare([rec for _, rec, _, _ in res], ref, [lo for _, _, lo, _ in res], radius, _tol(name), "redo " + name)
    assert all(lo["solver_fallbacks"] == 1 and n == 3 for _, _, lo, n in res)


# 9. no side effects
def test_call_leaves_the_normal_equations_and_the_next_shared_step_alone():
    seqs = _seqs("w2")

    def body(r, g, allreduce):
        g.evaluate(seqs[r][1], normal_eq=True, dense=False, residuals=False)
        d0, m0 = g.solve_step_shared(1e4, allreduce)
        ck0 = g.normal_eq_checksum()
        seen = []

        def spying(buf, op):   # inside a reduction of the joint call the context takes part in a joint solve: the single-sequence call refuses
            try:
                g.calibration_covariance()
                seen.append(None)
            except lvx.LvxError as e:
                seen.append(e.code)
            allreduce(buf, op)
        rec = g.calibration_covariance_shared(spying, 1e8)
        ck1 = g.normal_eq_checksum()
        d1, m1 = g.solve_step_shared(1e4, allreduce)
        g.calibration_covariance_shared(allreduce, 1e4, jacobi_scaling=False)
        d2, m2 = g.solve_step_shared(1e4, allreduce)
        return rec["sweeps"] >= 1, ck0 == ck1 == g.normal_eq_checksum(), np.array_equal(d0, d1) and m0 == m1, np.array_equal(d0, d2) and m0 == m2, seen
    for swept, same_eq, same_step, same_step2, seen in _run_ranks(seqs, body, TAU, (("DETERMINISTIC", 1),)):
        assert swept and same_eq and same_step and same_step2
        assert len(seen) == 2 and all(c == lvx.E_STATE for c in seen)


# 10. host formatter
def _write_ranks(path, seqs, locks):
    out = [float(len(seqs))]

    def vec(a):
        a = np.asarray(a, dtype=np.float64).ravel()
        out.append(float(len(a))); out.extend(a.tolist())
    for P, x in seqs:
        c = P["camera"]
        out += [P["t0"], P["dt"], float(P["n_knots"]), float(locks)]
        out += [float(c[k]) for k in ("rows", "cols", "readout", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]
        out += [float(P[k]) for k in ("w_gyro", "w_acc", "t_map", "huber_surf", "w_surf", "huber_rep", "w_rep")]
        for k in ("t_imu", "gyro", "acc", "planes", "surf_pt", "surf_t", "surf_plane", "lm_uv", "lm_t0", "rep_lm", "rep_uv", "rep_t0"):
            if k == "t_imu":
                vec(x)
            vec(P[k])
    np.asarray(out, dtype="<f8").tofile(path)


def test_host_formatter_prints_the_record_of_a_two_rank_run(tmp_path):
    """tests/native/joint_cov_demo.cpp: two contexts in one process, the callback exchanging through a barrier.  The lines of FormatJointCalibrationUncertainty (%.6e) carry
    the record's numbers: 2 sigma 180 / pi degrees for a rotation, sigma metres for a translation, the smallest joint eigenvalue, and per sensor this sequence's share
    own_info_kk / (sum_q w_q V_kq^2) of the joint information, in [0, 1]; the shared lines are the same on both ranks and the two shares of a scalar stay below 1."""
    import build as lvx_build
    lvx_build.build()
    libdir = os.path.join(ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "joint_cov_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "native", "joint_cov_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    seqs = _seqs("w2")
    pin = str(tmp_path / "ranks.bin")
    _write_ranks(pin, seqs, TAU)
    r = subprocess.run([exe, pin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blocks = [b.strip().splitlines() for b in r.stdout.split("END\n") if b.strip()]
    assert len(blocks) == 2
    shares, shared_lines = [], []
    for rank, b in enumerate(blocks):
        head = b[0].split()
        assert int(head[1]) == rank and int(head[3]) == 2 and int(head[5]) == 20 and float(head[7]) == 1e8 and [int(v) for v in head[9:]] == list(range(14)) + list(range(15, 21))
        sigma = np.array([float(v) for v in b[1].split()[1:]])
        slots = [int(v) for v in b[2].split()[1:]]
        eig = np.array([float(v) for v in b[3].split()[1:]])
        V = np.array([float(v) for v in b[4].split()[1:]]).reshape(len(slots), len(slots))
        own = np.array([float(v) for v in b[5].split()[1:]])
        assert slots == list(range(6)) + list(range(7, 13)) and (eig > 0).all()
        lines = b[6:]
        assert [ln.split()[0] for ln in lines] == ["[LiDAR]", "[Share]", "[Camera]", "[Share]", "[Spectrum]"]
        diag = (V * V) @ eig
        share = []
        for tag_line, share_line, c0, name in ((lines[0], lines[1], 8, "LiDAR"), (lines[2], lines[3], 15, "Camera")):
            num = [float(v.rstrip(";")) for v in tag_line.replace("(deg):", " ").replace("(m):", " ").split() if v[0].isdigit()]
            want = np.concatenate([2 * sigma[c0:c0 + 3] * 180 / np.pi, sigma[c0 + 3:c0 + 6]])
            assert len(num) == 6 and np.allclose(num, want, rtol=1e-6, atol=0)
            assert share_line.split()[1] == name
            sh = [float(v.rstrip(";")) for v in share_line.replace("rotation:", " ").replace("translation:", " ").split()[2:]]
            k = [slots.index(c0 - 8 + j) for j in range(6)]
            assert len(sh) == 6 and np.allclose(sh, own[c0 - 8:c0 - 2] / diag[k], rtol=1e-6, atol=0) and all(0.0 <= v <= 1.0 for v in sh)
            share += sh
        shares.append(np.array(share))
        sp = lines[4]
        assert abs(float(sp.split("eigenvalue:")[1].split()[0]) / eig[0] - 1) <= 1e-6 and float(sp.split("(radius")[1].split(")")[0]) == 1e8
        dom = 8 + slots[int(np.argmax(np.abs(V[:, 0])))]
        assert sp.rstrip().endswith("(c = %d)" % dom)
        shared_lines.append([lines[0], lines[2], lines[4]])
        print("rank %d\n%s" % (rank, "\n".join(lines)))
    assert shared_lines[0] == shared_lines[1] and (shares[0] + shares[1] <= 1.0 + 1e-6).all()   # (two numbers printed to 5e-7 relative each)
