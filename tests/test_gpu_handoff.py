"""Surfel hand-off on the device (lvx_set_planes_d, lvx_set_surfel_d, lvx_set_surfel_from_association) against the host setters: two contexts with the
same spline, IMU, state and locks — A fed by lvx_set_planes / lvx_set_surfel, B by the device calls — must be indistinguishable afterwards.

Bit-equal: residuals (input order), status codes, lvx_get_layout, error and plane statistics, Jacobian rows and blocks; with DETERMINISTIC = 1 also cost, gradient, the
dense normal equations, their checksums and one LM step (that needs the host's permutation and chunk tables).  In the default mode the sums are FP64 atomics in no
fixed order; the bar is the one tests/test_host_estimator.py documents for two runs of one problem: cost to 1e-12 relative.  For H and g the same bound follows per
entry: a reordered sum of n <= 4 000 terms moves by at most n eps sum|terms| = 4.4e-13 sum|terms|, and Cauchy-Schwarz bounds sum|J_i J_j| by max diag(H) and
sum|J_i r| by sqrt(max diag(H) * 2 cost) — so 1e-12 of those two scales.

Cases: tests/handoff_cases.py (checked on the CPU by tests/test_handoff_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import handoff_cases as hc
import lvx
import synth
from oracle import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "lvi-exc_amd")
LOCKS_TAU_FREE = lvx.LOCK_CAM_TAU
LOCKS_DEFAULT = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _context(P, tau_free=False, chunk_rows=None):
    g = lvx.Context(0)
    g.set_spline(P["t0"], P["dt"], P["n_knots"])
    g.set_camera(**P["camera"])
    g.set_imu(P["t_imu"], P["gyro"], P["acc"], P["w_gyro"], P["w_acc"])
    g.set_locks(LOCKS_TAU_FREE if tau_free else LOCKS_DEFAULT)
    if chunk_rows:
        g.set_switch("CHUNK_ROWS", chunk_rows)
    return g


def _feed_host(g, P):
    g.set_planes(P["planes"])
    g.set_surfel(P["surf_pt"], P["surf_t"], P["surf_plane"], P["t_map"], P["huber_surf"], P["w_surf"])


def _feed_device(g, P):
    pl, pt, t, pid = _dev(np.asarray(P["planes"], np.float64)), _dev(np.asarray(P["surf_pt"], np.float64)), _dev(np.asarray(P["surf_t"], np.float64)), _dev(np.asarray(P["surf_plane"], np.int32))
    g.set_planes_d(len(P["planes"]), pl.data_ptr())
    g.set_surfel_d(len(P["surf_t"]), pt.data_ptr(), t.data_ptr(), pid.data_ptr(), P["t_map"], P["huber_surf"], P["w_surf"])
    g.synchronize()   # the caller's buffers may go after this
    del pl, pt, t, pid


def _call(fn):
    try:
        return lvx.OK, "", fn()
    except lvx.LvxError as e:
        return e.code, str(e), None


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_status(a, b):
    assert a[0] == b[0] and a[1] == b[1], (a[:2], b[:2])
    if a[0] != lvx.OK:
        print("both routes:", a[0], a[1])
    return a[0] == lvx.OK


# lvx_layout fields that describe the context's last evaluations and solves, not the layout: equal only on two contexts with the same history (fresh pairs)
LAYOUT_HISTORY = ("exact_fallback", "solver_fallbacks", "fallback_rows", "solver_separators", "solver_leaves", "lm_elim_kernel")


def _layout_fields(lo, with_history):
    return {k: v for k, v in lo.items() if with_history or k not in LAYOUT_HISTORY}


def _same_stats(A, B, x, n_planes):
    sa, sb = _call(lambda: A.error_statistics(x)), _call(lambda: B.error_statistics(x))
    if not _same_status(sa, sb):
        return
    assert sa[2]["cost"] == sb[2]["cost"]
    for name in lvx.FAMILY_NAMES:
        for k, v in sa[2][name].items():
            assert _bits(v) == _bits(sb[2][name][k]), (name, k)
    for u, v in zip(A.plane_stats(n_planes), B.plane_stats(n_planes)):
        assert _bits(u) == _bits(v)


def _compare(A, B, x, n_planes, jac=True, det=True, fresh=True):
    """Everything the module docstring lists, A against B, at state x.  Returns the status code of the evaluation (the same on both)."""
    la, lb = _call(A.layout), _call(B.layout)
    if not _same_status(la, lb):
        return la[0]
    assert _layout_fields(la[2], fresh) == _layout_fields(lb[2], fresh)
    ra, rb = _call(lambda: A.evaluate(x)), _call(lambda: B.evaluate(x))
    _same_stats(A, B, x, n_planes)
    if not _same_status(ra, rb):
        return ra[0]
    assert _bits(ra[2]["residuals"]) == _bits(rb[2]["residuals"])
    assert A.family_rows() == B.family_rows()
    # default mode: the run-to-run bar
    ea, eb = A.evaluate(x, normal_eq=True), B.evaluate(x, normal_eq=True)
    assert _bits(ea["residuals"]) == _bits(eb["residuals"])
    cost = ea["cost"]
    assert abs(ea["cost"] - eb["cost"]) <= 1e-12 * cost
    hs = np.abs(np.diag(ea["H"])).max()
    print("default mode: cost rel %.2e  H %.2e  g %.2e (of their scales)" % (abs(ea["cost"] - eb["cost"]) / cost, np.abs(ea["H"] - eb["H"]).max() / hs, np.abs(ea["g"] - eb["g"]).max() / np.sqrt(hs * 2 * cost)))
    assert np.abs(ea["H"] - eb["H"]).max() <= 1e-12 * hs
    assert np.abs(ea["g"] - eb["g"]).max() <= 1e-12 * np.sqrt(hs * 2 * cost)
    if jac:
        ja, jb = A.evaluate(x, jac=True), B.evaluate(x, jac=True)
        assert _bits(ja["jac_cols"]) == _bits(jb["jac_cols"]) and _bits(ja["jac_vals"]) == _bits(jb["jac_vals"])
        ja, jb = A.evaluate(x, jac_blocks=True), B.evaluate(x, jac_blocks=True)   # (the two requests are exclusive)
        for (ka, va), (kb, vb) in zip(ja["jac_blocks"], jb["jac_blocks"]):
            assert _bits(ka) == _bits(kb) and _bits(va) == _bits(vb)
    if not det:
        return lvx.OK
    # deterministic mode: equal bits, and one LM step
    for g in (A, B):
        g.set_switch("DETERMINISTIC", 1)
    assert _layout_fields(A.layout(), fresh) == _layout_fields(B.layout(), fresh)
    ea, eb = A.evaluate(x, normal_eq=True), B.evaluate(x, normal_eq=True)
    assert ea["cost"] == eb["cost"] and _bits(ea["residuals"]) == _bits(eb["residuals"])
    assert _bits(ea["g"]) == _bits(eb["g"]) and _bits(ea["H"]) == _bits(eb["H"])
    assert A.normal_eq_checksum() == B.normal_eq_checksum()
    (da, ma), (db, mb) = A.solve_step(1e4), B.solve_step(1e4)
    assert _bits(da) == _bits(db) and ma == mb and np.abs(da).max() > 0
    for g in (A, B):
        g.set_switch("DETERMINISTIC", 0)
    return lvx.OK


@pytest.mark.gpu
@pytest.mark.parametrize("case", hc.CRAFTED, ids=[c[0] for c in hc.CRAFTED])
def test_device_setters_equal_the_host_setters(case):
    _, kw, tau_free, chunk_rows = case
    P = hc.crafted(**kw)
    A, B = _context(P, tau_free, chunk_rows), _context(P, tau_free, chunk_rows)
    try:
        _feed_host(A, P)
        _feed_device(B, P)
        rc = _compare(A, B, P["state0"], len(P["planes"]))
        assert rc == (lvx.E_RANGE if kw.get("pattern") == "outside" else lvx.OK)
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_a_plane_id_outside_the_table_fails_in_the_same_call():
    P, Q = hc.crafted(65, bad_plane=True), hc.crafted(65, seed=1)
    A, B = _context(P), _context(P)
    try:
        _feed_host(A, Q); _feed_device(B, Q)       # a valid family first: the failing call must leave it as it is
        ea, eb = _call(lambda: _feed_host(A, P)), _call(lambda: _feed_device(B, P))
        assert ea[0] == lvx.E_ARG and _same_status(ea, eb) is False and "plane id out of range" in ea[1]
        assert _compare(A, B, Q["state0"], len(Q["planes"]), jac=False) == lvx.OK
        # the table replaced by a shorter one afterwards: the layout's range check, from the call that triggers the layout
        A.set_planes(Q["planes"][:10])
        pl = _dev(Q["planes"][:10]); B.set_planes_d(10, pl.data_ptr())
        la, lb = _call(A.layout), _call(B.layout)
        assert la[0] == lvx.E_ARG and _same_status(la, lb) is False and "out of range for the current plane table" in la[1]
        A.set_planes(Q["planes"]); B.set_planes(Q["planes"])   # host planes under device-origin rows
        assert _compare(A, B, Q["state0"], len(Q["planes"]), jac=False) == lvx.OK
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_argument_errors_clearing_and_replacement():
    P, Q = hc.crafted(257), hc.crafted(65, seed=1, pattern="one_interval")
    A, B = _context(P), _context(P)
    try:
        l, h = B._l, B._h
        import ctypes as C
        one = _dev(np.zeros(3))
        assert l.lvx_set_planes_d(None, C.c_int(1), C.c_void_p(one.data_ptr())) == lvx.E_ARG
        assert l.lvx_set_planes_d(h, C.c_int(-1), C.c_void_p(one.data_ptr())) == lvx.E_ARG and l.lvx_set_planes_d(h, C.c_int(1), None) == lvx.E_ARG
        assert l.lvx_set_surfel_d(h, C.c_int(-1), None, None, None, C.c_double(0), C.c_double(5), C.c_double(1)) == lvx.E_ARG
        assert l.lvx_set_surfel_d(h, C.c_int(1), C.c_void_p(one.data_ptr()), None, C.c_void_p(one.data_ptr()), C.c_double(0), C.c_double(5), C.c_double(1)) == lvx.E_ARG
        _feed_host(A, P); _feed_device(B, P)
        assert B.layout()["n_residuals"] == A.layout()["n_residuals"]
        # device planes under host rows, and the other way round
        pl = _dev(np.asarray(Q["planes"], np.float64)); B.set_planes_d(len(Q["planes"]), pl.data_ptr())
        B.set_surfel(Q["surf_pt"], Q["surf_t"], Q["surf_plane"], Q["t_map"], Q["huber_surf"], Q["w_surf"])
        _feed_host(A, Q)
        assert _compare(A, B, Q["state0"], len(Q["planes"]), jac=False) == lvx.OK
        _feed_device(B, P); B.set_planes(P["planes"])
        _feed_host(A, P)
        assert _compare(A, B, P["state0"], len(P["planes"]), jac=False) == lvx.OK
        # n = 0 clears the family; a host call after a device one replaces it
        for g, feed in ((A, _feed_host), (B, _feed_device)):
            feed(g, hc.crafted(0))
        assert A.layout() == B.layout() and A.family_rows() == B.family_rows() and A.family_rows()[lvx.FAM_SURFEL + 1] == A.family_rows()[lvx.FAM_SURFEL]
        _feed_device(B, P); _feed_host(B, Q); _feed_host(A, Q)
        assert _compare(A, B, Q["state0"], len(Q["planes"]), jac=False) == lvx.OK
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_spline_set_or_changed_after_the_hand_off():
    """The call computes the knot intervals for the spline it finds; a spline that arrives or changes afterwards makes the layout compute them again."""
    P = hc.crafted(1025, N=300, pattern="on_knots")
    A, B = _context(P), lvx.Context(0)
    try:
        B.set_camera(**P["camera"])
        B.set_imu(P["t_imu"], P["gyro"], P["acc"], P["w_gyro"], P["w_acc"])
        B.set_locks(LOCKS_DEFAULT)
        _feed_host(A, P); _feed_device(B, P)                       # B has no spline yet
        B.set_spline(P["t0"], P["dt"], P["n_knots"])
        assert _compare(A, B, P["state0"], len(P["planes"]), jac=False) == lvx.OK
        for g in (A, B):                                           # the same knots counted from half an interval earlier: every row changes its interval or its u
            g.set_spline(P["t0"] - 0.5 * P["dt"], P["dt"], P["n_knots"])
        assert _compare(A, B, P["state0"], len(P["planes"]), jac=False) == lvx.OK
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_switches_after_a_device_hand_off():
    P = hc.crafted(1025, N=300)
    A, B = _context(P), _context(P)
    try:
        _feed_host(A, P); _feed_device(B, P)
        for name, value in (("CHUNK_R", 8), ("FORCE_LEGACY", 1)):
            for g in (A, B):
                g.set_switch(name, value)
            # (the per-segment kernels over a whole family add in no fixed order, DETERMINISTIC or not)
            assert _compare(A, B, P["state0"], len(P["planes"]), jac=False, det=(name != "FORCE_LEGACY")) == lvx.OK
            for g in (A, B):
                g.set_switch(name, 0)
        # lvx_lm_solve: equal bits under DETERMINISTIC (bitwise-repeatable LM iterates).  In the default mode two runs of ONE route already differ — the
        # crafted rows are far off their planes, so the steps are long and amplify the atomics' order — and only the documented cost bar (1e-8 relative) is held.
        for g in (A, B):
            g.set_switch("DETERMINISTIC", 1)
        (xa, sa), (xb, sb) = A.lm_solve(P["state0"], max_iterations=3), B.lm_solve(P["state0"], max_iterations=3)
        assert _bits(xa) == _bits(xb) and sa["iterations"] == sb["iterations"] == 3 and sa["termination"] == sb["termination"] and sa["final_cost"] == sb["final_cost"]
        assert _bits(sa["cost_history"]) == _bits(sb["cost_history"]) and _bits(sa["accepted"]) == _bits(sb["accepted"])
        for g in (A, B):
            g.set_switch("DETERMINISTIC", 0)
        (xa, sa), (xb, sb) = A.lm_solve(P["state0"], max_iterations=3), B.lm_solve(P["state0"], max_iterations=3)
        print("default mode LM: final cost rel %.2e, state %.2e" % (abs(sa["final_cost"] - sb["final_cost"]) / sa["final_cost"], np.abs(xa - xb).max()))
        assert sa["iterations"] == sb["iterations"] and sa["termination"] == sb["termination"] and abs(sa["final_cost"] - sb["final_cost"]) <= 1e-8 * sa["final_cost"]
    finally:
        A.close(); B.close()


# ---- from the association --------------------------------------------------------------------------------------------------------------------------------------

def _lvi_inputs(g, S):
    """What trajInitFromLVIdata has beside the surfel blocks: IMU, landmarks, reprojection blocks (the state holds the sequence's inverse depths)."""
    g.set_imu(S["t_imu"], S["gyro"], S["acc"], 28.0, 18.0)
    g.set_landmarks(S["lm_uv"], S["lm_t0"])
    g.set_reproj(S["rep_lm"], S["rep_uv"], S["rep_t0"], 5.0, 1.0)
    g.set_locks(LOCKS_DEFAULT)


@pytest.fixture(scope="module")
def assoc():
    """One context with the sequence's scans and ONE association at the true state; its planes and SurfelPoints on the host for the host route."""
    S = synth.make_sequence(**hc.SEQ_KW)
    g = lvx.Context(0)
    g.set_spline(S["t0"], S["dt"], S["n_knots"])
    g.set_camera(**S["camera"])
    _lvi_inputs(g, S)
    raw = np.zeros(S["scans"].shape, dtype=lvx.POINT_XYZIT)
    for k in ("x", "y", "z", "timestamp"):
        raw[k] = S["scans"][k]
    lvx.set_scans(g, raw, S["H"], S["W"])
    x = np.ascontiguousarray(S["state_true"], np.float64)
    npl, npt = lvx.data_association(g, x, S["t_map"])
    planes, points = lvx.get_surfel_map(g, npl), lvx.get_surfel_points(g, npt)
    yield dict(S=S, g=g, x=x, planes=planes, points=points, npl=npl, npt=npt)
    g.close()


def _host_route(S, planes, points, step, t_map):
    A = lvx.Context(0)
    A.set_spline(S["t0"], S["dt"], S["n_knots"])
    A.set_camera(**S["camera"])
    _lvi_inputs(A, S)
    pt, t, pid = pipeline.select_surfels(points, t_map, step)
    A.set_planes(np.ascontiguousarray(planes["Pi"]))
    A.set_surfel(pt, t, pid, t_map, 5.0, 10.0)
    return A, len(t)


@pytest.mark.gpu
def test_state_error_before_any_association():
    g = lvx.Context(0)
    try:
        g.set_spline(100.0, 0.02, 30)
        e = _call(lambda: lvx.set_surfel_from_association(g, 10, 100.1, 5.0, 10.0))
        assert e[0] == lvx.E_STATE and "no data association" in e[1]
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("step,shift", [(10, 0.0), (1, 0.0), (100000, 0.0), (10, hc.T_MAP_SHIFT)], ids=["step10", "step1", "one_row", "t_map_moved"])
def test_from_association_equals_fetch_select_and_set(assoc, step, shift):
    S, B = assoc["S"], assoc["g"]
    assert assoc["npl"] > 100 and assoc["npt"] > 1000 and (np.diff(assoc["points"]["t"]) >= 0).all()
    t_map = S["t_map"] + shift
    A, n_ref = _host_route(S, assoc["planes"], assoc["points"], step, t_map)
    try:
        n_used = lvx.set_surfel_from_association(B, step, t_map, 5.0, 10.0)
        assert n_used == n_ref == len(hc.select_reference(assoc["points"], t_map, step)[1])
        if step == 100000:
            assert n_used == 1
        if shift:
            n_all = len(range(0, assoc["npt"], step))
            assert 0 < n_used < n_all, "the moved map time must drop some of the strided points and keep some"
        assert _compare(A, B, assoc["x"], assoc["npl"], jac=(step == 10), fresh=False) == lvx.OK   # (B is the module's context: it has solved before)
    finally:
        A.close()


@pytest.mark.gpu
def test_from_association_behind_the_last_point_clears_the_family(assoc):
    S, B = assoc["S"], assoc["g"]
    lvx.set_surfel_from_association(B, 10, S["t_map"], 5.0, 10.0)
    rows = B.family_rows()
    assert rows[lvx.FAM_SURFEL + 1] - rows[lvx.FAM_SURFEL] > 0
    t_far = float(assoc["points"]["t"][-1]) + 1e-3
    assert lvx.set_surfel_from_association(B, 10, t_far, 5.0, 10.0) == 0
    A, n_ref = _host_route(S, assoc["planes"], assoc["points"], 10, t_far)
    try:
        assert n_ref == 0
        la, lb = _call(A.layout), _call(B.layout)
        assert _same_status(la, lb) and _layout_fields(la[2], False) == _layout_fields(lb[2], False)
        rows = B.family_rows()
        assert rows == A.family_rows() and rows[lvx.FAM_SURFEL + 1] == rows[lvx.FAM_SURFEL]
    finally:
        A.close()


@pytest.mark.gpu
def test_a_later_association_does_not_disturb_the_family(assoc):
    S, B, x = assoc["S"], assoc["g"], assoc["x"]
    n_used = lvx.set_surfel_from_association(B, 10, S["t_map"], 5.0, 10.0)
    before = B.evaluate(x)
    try:
        x0 = np.ascontiguousarray(S["state0"], np.float64)
        npl2, npt2 = lvx.data_association(B, x0, S["t_map"])     # another map, other lists, the same device buffers
        assert (npl2, npt2) != (assoc["npl"], assoc["npt"])
        B.set_switch("CHUNK_ROWS", 64)                             # a new layout from the family's own copies
        after = B.evaluate(x)
        assert _bits(after["residuals"]) == _bits(before["residuals"])
        rows = B.family_rows()
        assert rows[lvx.FAM_SURFEL + 1] - rows[lvx.FAM_SURFEL] == n_used
    finally:
        B.set_switch("CHUNK_ROWS", 0)
        assert lvx.data_association(B, x, S["t_map"]) == (assoc["npl"], assoc["npt"])   # the module's association again


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def handoff_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("handoff") / "calibrate_handoff")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(LIBDIR, "host"), os.path.join(ROOT, "tests", "native", "calibrate_handoff.cpp"),
                           "-o", out, "-L" + LIBDIR, "-llvx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def _write_sequence(path, S, refine_iterations, lvi, camsurf, step):
    """The flat problem file of tests/native/calibrate_demo.cpp / calibrate_handoff.cpp."""
    c = S["camera"]
    parts = [np.array([S["t0"], S["dt"], S["n_knots"], S["t_map"], S["H"], S["W"], len(S["scans"]), refine_iterations, lvi, camsurf, step, 0,
                       c["rows"], c["cols"], c["readout"], c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"], c["k3"]], dtype=np.float64)]

    def vec(a):
        a = np.asarray(a, dtype=np.float64).ravel()
        parts.extend([np.array([len(a)], dtype=np.float64), a])
    vec(S["state0"])
    for k in ("t_imu", "gyro", "acc", "lm_uv", "lm_t0", "rep_lm", "rep_uv", "rep_t0"):
        vec(S[k])
    for sc in S["scans"]:
        vec(np.stack([sc["x"], sc["y"], sc["z"]], axis=1)); vec(sc["timestamp"])
    np.concatenate(parts).tofile(path)


def test_hand_off_driver_compiles_against_the_c_abi(handoff_binary):
    assert subprocess.run([handoff_binary], capture_output=True).returncode == 2


@pytest.mark.gpu
def test_calibrator_with_device_handoff_runs_the_same_schedule(handoff_binary, tmp_path):
    S = synth.make_sequence(**hc.SEQ_KW)
    pin = str(tmp_path / "seq.bin")
    _write_sequence(pin, S, refine_iterations=2, lvi=1, camsurf=0, step=10)   # two association rounds (the second on the one-stop chain: its planes stay on the device), then LVI
    env = dict(os.environ, LVX_DETERMINISTIC="1")
    runs = []
    for flag in ("0", "1"):
        pout = str(tmp_path / ("res%s.bin" % flag))
        r = subprocess.run([handoff_binary, pin, pout, flag], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        out = np.fromfile(pout)
        ns = int(out[0])
        runs.append((out[1:1 + 7 * ns].reshape(ns, 7), out[1 + 7 * ns:]))
    (ra, xa), (rb, xb) = runs
    assert ra.shape == rb.shape and len(ra) == 3 and len(xa) == len(S["state0"])   # trajInitFromSurfel twice, trajInitFromLVIdata
    print(ra)
    assert (ra[:, 5] > 100).all() and (ra[:, 4] > 100).all()
    for col, name in ((0, "iterations"), (1, "termination"), (4, "planes"), (5, "surfel points used"), (6, "cam-surfel blocks")):
        assert np.array_equal(ra[:, col], rb[:, col]), name
    assert _bits(ra[:, 2:4]) == _bits(rb[:, 2:4])   # initial and final cost of every stage
    assert _bits(xa) == _bits(xb)
