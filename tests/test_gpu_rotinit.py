"""Rotation initialisation on the device (lvi-exc_amd/csrc/lvx_rotinit.hip): lvx_estimate_rotation and lvx_estimate_rotation_d against the g++ build of the same header
(bit for bit) and against the numpy restatement of InertialInitializer::EstimateRotation (tests/rotinit_cases.py: eigenvalues 1e-12 lambda_max, quaternion angle
2e-12 lambda_max / (lambda[2] - lambda[3]) rad, counts / ok / first_ok exact), repeated calls and switches, the sizes around the 64-pair tile and the 256-pair
workgroup, the error codes, and lvx_host::Calibrator's "Initialization" stage end to end.  Every test prints its figures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
import rotinit_cases as rc
import traj_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    """The short problem loaded into one context (read-only), the long one as a spline alone."""
    P, PL = tc.problem(), rc.long_problem()
    g, gl = lvx.Context(0), lvx.Context(0)
    lvx.load_problem(g, P, tc.TAU)
    gl.set_spline(PL["t0"], PL["dt"], PL["n_knots"])
    yield {id(P): g, id(PL): gl}
    g.close()
    gl.close()


def _device_d(g, state, t, q, prefix_len, tau, opt, resident=False):
    """lvx_estimate_rotation_d on torch buffers filled with a pattern first."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    t_d, q_d, s_d, pl_d, ta_d = up(t, np.float64), up(q, np.float64), up(state, np.float64), up(prefix_len, np.int32), up(tau, np.float64)
    n_prefix, n_tau = (0 if prefix_len is None else len(prefix_len)), (0 if tau is None else len(tau))
    res_d = torch.full((max(n_tau, 1) * max(n_prefix, 1) * 80,), 0x5A, dtype=torch.uint8, device=dev)
    first_d = torch.full((max(n_tau, 1),), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lvx.estimate_rotation_d(g, t_d.data_ptr(), q_d.data_ptr(), len(t), res_d.data_ptr(), first_d.data_ptr(), None if pl_d is None else pl_d.data_ptr(), n_prefix,
                            None if ta_d is None else ta_d.data_ptr(), n_tau, opt, None if resident else s_d.data_ptr())
    return res_d, first_d, (max(n_tau, 1), max(n_prefix, 1))


def _fetch(res_d, first_d, shape):
    return np.frombuffer(res_d.cpu().numpy().tobytes(), lvx.ROTINIT_DTYPE).reshape(shape), first_d.cpu().numpy()


@pytest.mark.parametrize("name", ["n3_on", "n3_off", "n17_on", "n17_off", "n65_on", "n65_off", "n257_off", "tail", "sign_scale", "huber", "huber_half", "prefixes_short", "prefixes",
                                  "shifts"])
def test_cases_match_the_host_build_bit_for_bit_and_the_restatement(ctxs, name):
    """Every case of tests/test_rotinit_host.py: the records of lvx_estimate_rotation, of a second call and of lvx_estimate_rotation_d are the bytes the g++ build of
    lvx_rotinit.h gives, and meet the bars against the restatement."""
    c = rc.cases()[name]
    g = ctxs[id(c["P"])]
    args = (c["state"], c["t"], c["q"], c["prefix_len"], c["tau"], c["opt"])
    host, hfirst, st = rc.host_estimate(c["P"], *args)
    assert st == 0
    res, first = lvx.estimate_rotation(g, *args)
    worst = rc.check_case(name, res, first)
    print("%s: worst fraction of the bars: lambda %.3f, angle %.3f" % (name, worst[0], worst[1]))
    diff = np.flatnonzero(np.frombuffer(res.tobytes(), np.uint8) != np.frombuffer(host.tobytes(), np.uint8))
    print("%s: %d of %d bytes differ from the host build" % (name, len(diff), res.nbytes), "" if not len(diff) else "first at record %d byte %d" % (diff[0] // 80, diff[0] % 80))
    assert res.tobytes() == host.tobytes() and np.array_equal(first, hfirst)
    res2, first2 = lvx.estimate_rotation(g, *args)
    assert res2.tobytes() == res.tobytes() and np.array_equal(first2, first)
    rd, fd = _fetch(*_device_d(g, *args))
    g.synchronize()
    assert rd.tobytes() == res.tobytes() and np.array_equal(fd, first)


def test_resident_state_and_switches_do_not_matter(ctxs):
    """The _d call on the state of lvx_set_state, and the calls under the elimination and determinism switches: the same bytes."""
    c = rc.cases()["tail"]
    g = ctxs[id(c["P"])]
    args = (c["state"], c["t"], c["q"], c["prefix_len"], c["tau"], c["opt"])
    res, first = lvx.estimate_rotation(g, *args)
    g.set_state(c["state"])
    rd, fd = _fetch(*_device_d(g, *args, resident=True))
    g.synchronize()
    assert rd.tobytes() == res.tobytes() and np.array_equal(fd, first)
    g2 = lvx.Context(0)
    try:
        g2.set_spline(c["P"]["t0"], c["P"]["dt"], c["P"]["n_knots"])
        for sw in ("DETERMINISTIC", "SOLVER_ND", "SOLVER_SEQ", "FORCE_LEGACY", "SERIAL", "NO_GRAPH"):
            g2.set_switch(sw, 1)
            r2, f2 = lvx.estimate_rotation(g2, *args)
            assert r2.tobytes() == res.tobytes() and np.array_equal(f2, first), sw
    finally:
        g2.close()


SEAM_PREFIXES = [1, 2, 10, 65, 66, 100, 257, 300, 10 ** 6]   # clipped to n: ends inside a tile (66, 100, 300), on a tile edge (65: 64 pairs) and on a workgroup edge (257: 256 pairs)


@pytest.mark.parametrize("pairs", [1, 63, 64, 65, 257, 513])
def test_sizes_across_the_seams_of_the_reduction(ctxs, pairs):
    """Pairs = 1, 63, 64, 65 (the 64-pair tile), 257 and 513 (one and two 256-pair workgroups + 1) on the 6 s spline; 1 and 13 shifts, 1 and 9 prefixes: every combination
    the bytes of the host build; 9 prefixes x 1 shift and 1 prefix x 13 shifts also against the restatement."""
    P = rc.long_problem()
    g = ctxs[id(P)]
    n = pairs + 1
    t = rc.stamps(P, n, False)
    q = rc.odometry(P, t)
    pl = np.minimum(n, SEAM_PREFIXES).astype(np.int32)
    taus = rc.SHIFTS * 0.1
    for prefix_len in (None, pl):
        for tau in (None, taus):
            host, hfirst, st = rc.host_estimate(P, P["state_true"], t, q, prefix_len, tau)
            res, first = lvx.estimate_rotation(g, P["state_true"], t, q, prefix_len, tau)
            assert st == 0 and res.tobytes() == host.tobytes() and np.array_equal(first, hfirst), (prefix_len is None, tau is None)
            if (prefix_len is None) != (tau is None):
                refs = [[rc.np_estimate(P, P["state_true"], t, q, int(m), tv) for m in ([n] if prefix_len is None else pl)] for tv in ([0.0] if tau is None else taus)]
                worst = rc.check_refs(res, first, refs, "pairs=%d" % pairs)
                print("pairs=%d prefixes=%s shifts=%s: worst fraction of the bars %s" % (pairs, prefix_len is not None, tau is not None, worst))


def test_error_codes(ctxs):
    c = rc.cases()["n17_off"]
    g = ctxs[id(c["P"])]
    s, t, q = (np.ascontiguousarray(a, np.float64) for a in (c["state"], c["t"], c["q"]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    res, first = np.zeros(1, lvx.ROTINIT_DTYPE), np.zeros(1, np.int32)
    call = lambda state, n, tt, qq, npf, plen, rr, ff: g._l.lvx_estimate_rotation(g._h, state, C.c_int(n), tt, qq, C.c_int(npf), plen, C.c_int(0), None, None, rr, ff)   # noqa: E731
    assert call(p(s), 17, p(t), p(q), 0, None, p(res), p(first)) == lvx.OK
    assert call(None, 17, p(t), p(q), 0, None, p(res), p(first)) == lvx.E_ARG
    assert call(p(s), 17, None, p(q), 0, None, p(res), p(first)) == lvx.E_ARG
    assert call(p(s), 17, p(t), None, 0, None, p(res), p(first)) == lvx.E_ARG
    assert call(p(s), 17, p(t), p(q), 0, None, None, p(first)) == lvx.E_ARG
    assert call(p(s), 17, p(t), p(q), 0, None, p(res), None) == lvx.E_ARG
    assert call(p(s), 0, p(t), p(q), 0, None, p(res), p(first)) == lvx.E_ARG
    res3 = np.zeros(3, lvx.ROTINIT_DTYPE)
    for bad in ([17, 16, 17], [0, 5, 17], [5, 17, 18]):
        assert call(p(s), 17, p(t), p(q), 3, p(np.array(bad, np.int32)), p(res3), p(first)) == lvx.E_ARG, bad
    assert g._l.lvx_estimate_rotation_d(g._h, None, C.c_int(0), p(t), p(q), C.c_int(0), None, C.c_int(0), None, None, p(res), p(first)) == lvx.E_ARG
    fresh = lvx.Context(0)
    try:
        with pytest.raises(lvx.LvxError) as e:
            lvx.estimate_rotation(fresh, s, t, q)
        assert e.value.code == lvx.E_STATE
    finally:
        fresh.close()


def test_nonunit_control_quaternion(ctxs):
    """Control point 40 scaled by 1.001 (traj_cases.nonunit_case's knot): LVX_E_NONUNIT_QUAT; the pairs with an evaluation time in its window are skipped and counted in
    n_skipped, the others are counted as before; records the bytes of the host build and within the bars of the restatement.  The _d variant reports through
    lvx_synchronize, once."""
    c = rc.cases()["n65_off"]
    P = c["P"]
    g = ctxs[id(P)]
    s = np.array(c["state"], np.float64)
    N = P["n_knots"]
    s[3 * N + 4 * tc.NONUNIT_KNOT:3 * N + 4 * tc.NONUNIT_KNOT + 4] *= tc.NONUNIT_SCALE
    pl = [20, 65]
    with pytest.raises(lvx.LvxError) as e:
        lvx.estimate_rotation(g, s, c["t"], c["q"], pl)
    assert e.value.code == lvx.E_NONUNIT_QUAT
    res, first = e.value.partial
    host, hfirst, st = rc.host_estimate(P, s, c["t"], c["q"], pl)
    assert st == 2 and res.tobytes() == host.tobytes() and np.array_equal(first, hfirst)
    hit = tc.nonunit_window(P, c["t"])
    n_bad = int(np.count_nonzero(hit[1:] | hit[:-1]))
    assert 0 < n_bad < 10 and res[0, 1]["n_skipped"] == n_bad and res[0, 1]["n_pairs"] == 64 - n_bad and res[0, 0]["n_pairs"] == 19 and res[0, 0]["n_skipped"] == 0
    refs = [[rc.np_estimate(P, s, c["t"], c["q"], m, skip=lambda tt: tc.nonunit_window(P, tt)) for m in pl]]
    rc.check_refs(res, first, refs, "non-unit")
    ok, _ = lvx.estimate_rotation(g, c["state"], c["t"], c["q"], pl)   # the flag does not outlive the call
    assert ok[0, 1]["n_pairs"] == 64
    rd, fd, shape = _device_d(g, s, c["t"], c["q"], pl, None, None)
    with pytest.raises(lvx.LvxError) as e:
        g.synchronize()
    assert e.value.code == lvx.E_NONUNIT_QUAT and _fetch(rd, fd, shape)[0].tobytes() == res.tobytes()
    g.synchronize()   # reported once


def _write_sequence(path, S, state, scan_t, init):
    cam = S["camera"]
    parts = [[S["t0"], S["dt"], S["n_knots"], init, cam["rows"], cam["cols"], cam["readout"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]]]
    for a in (state, S["t_imu"], S["gyro"], S["acc"], S["lm_uv"], S["lm_t0"], scan_t):
        a = np.asarray(a, np.float64).ravel()
        parts += [[len(a)], a]
    np.concatenate([np.asarray(x, np.float64) for x in parts]).tofile(path)


def test_calibrator_initialization_stage_end_to_end(tmp_path):
    """tests/native/rotinit_demo.cpp over lvx_host::Calibrator: a 6 s sequence (synth.make_sequence: LiDAR mounted with rpy 2, -3, 91 degrees), LOAM poses with 2 mm /
    0.5 mrad of noise, the state started at identity rotations and zero positions, solve0_so3_from_gyro and init_lidar_rotation on.  The "Initialization" report's prefix
    index and record equal what the restatement gives on the state Solve #0 left (the bars of rotinit_cases.py); q_LtoI of the state is conj(q_ItoS); its distance to the
    planted rotation is at most twice the restatement's own, which was measured as 5.85e-3 rad on this sequence (prefix 40 of 30, 40, 50: sigma[2] 0.231, 0.254, 0.277;
    Calibrator 5.85e-3 rad as well, 3.5e-16 rad from the restatement).  With init_lidar_rotation off Run reports the same
    stages without "Initialization" and leaves the LiDAR quaternion alone."""
    S = synth.make_sequence(seed=50, duration=6.0, H=2, W=36, n_reproj=200)
    N = S["n_knots"]
    scan_t, stamp, p, q_wxyz, _ = synth.sequence_loam_poses(S, noise_m=2e-3, noise_rad=5e-4, seed=7)
    pose_file = str(tmp_path / "loam_poses.txt")
    synth.write_loam_pose_file(pose_file, stamp, p, q_wxyz)
    x0 = np.array(S["state0"], np.float64)
    x0[:3 * N] = 0.0
    x0[3 * N:7 * N] = np.tile([0.0, 0.0, 0.0, 1.0], N)
    x0[7 * N + 16:7 * N + 20] = [0.0, 0.0, 0.0, 1.0]
    libdir = os.path.join(tc.ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "rotinit_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(tc.ROOT, "tests", "native", "rotinit_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    runs = {}
    for init in (1, 0):
        pin, pout = str(tmp_path / ("in%d.bin" % init)), str(tmp_path / ("out%d.bin" % init))
        _write_sequence(pin, S, x0, scan_t, init)
        r = subprocess.run([exe, pin, pout, pose_file], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        runs[init] = (r.stdout.splitlines(), np.fromfile(pout))
    lines, x1 = runs[1]
    assert [l for l in lines if l.startswith("stage")] == ["stage initialSO3TrajWithGyro", "stage Initialization"]
    assert runs[0][0] == ["stage initialSO3TrajWithGyro"] and np.array_equal(runs[0][1][7 * N + 16:7 * N + 20], [0, 0, 0, 1])
    d0 = np.abs(runs[0][1][3 * N:7 * N] - x1[3 * N:7 * N]).max()
    print("SO3 control points of the two runs' Solve #0: max |diff| = %.3e" % d0)
    assert d0 <= 1e-7   # the same Solve #0 (the default evaluation pass orders its FP64 atomics freely: tests/test_gpu_pipeline_oracle.py holds it at 1e-7 against the oracle's LM)
    f = [l for l in lines if l.startswith("init ")][0].split()[1:]
    rec = np.zeros(1, lvx.ROTINIT_DTYPE)[0]
    prefix_index = int(f[0])
    rec["n_poses"], rec["n_pairs"], rec["n_skipped"], rec["ok"] = (int(v) for v in f[1:5])
    rec["q_ItoS_xyzw"], rec["sigma"] = [float(v) for v in f[5:9]], [float(v) for v in f[9:13]]
    # the restatement on the state Solve #0 left, over the reference's schedule 30, 40, ...
    q_odo = np.column_stack([q_wxyz[:, 1:], q_wxyz[:, 0]])
    t_odo = stamp.astype(np.float64) * 1e-9
    assert np.array_equal((scan_t * 1e9).astype(np.int64), stamp)
    sched = list(range(30, len(scan_t) + 1, 10))
    refs = [rc.np_estimate(S, x1, scan_t, q_odo, m) for m in sched]
    print("restatement sigma[2] over the schedule %s: %s" % (sched, [r["sigma"][2] for r in refs]))
    first = [k for k, r in enumerate(refs) if r["ok"]][0]
    assert prefix_index == first and rec["n_poses"] == sched[first]
    rc.check_record(rec, refs[first], "Initialization")
    assert np.abs(t_odo - scan_t).max() < 1e-6
    qx = rec["q_ItoS_xyzw"]
    assert np.array_equal(x1[7 * N + 16:7 * N + 20], [-qx[0], -qx[1], -qx[2], qx[3]])
    q_true = S["state_true"][7 * N + 16:7 * N + 20]

    def dist(x_ItoS):
        d = synth.qmul(np.array([-x_ItoS[0], -x_ItoS[1], -x_ItoS[2], x_ItoS[3]]), synth.qconj(q_true))
        return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))
    e_ref, e_got = dist(refs[first]["x"]), dist(qx)
    print("distance to the planted q_LtoI: restatement %.6e rad, Calibrator %.6e rad (planted angle %.3f rad)" % (e_ref, e_got, 2 * np.arccos(abs(q_true[3]))))
    assert e_got <= 2.0 * e_ref and 2 * np.arccos(abs(q_true[3])) > 1.5
