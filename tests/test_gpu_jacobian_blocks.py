"""GPU: per-block Jacobian records (LVX_EVAL_JACOBIAN_BLOCKS) from the fused kernels against the debug rows (LVX_EVAL_JACOBIAN, per-segment
kernels) of the same state.  Column c of a record is column c of the per-segment kernel's row, so the two compare element by element at the
tolerance _compare of test_gpu_eval uses (1e-9 of the family's largest entry); the keys must give the debug row's column indices."""
import ctypes as C

import numpy as np
import pytest

import lvx
import synth
from test_gpu_eval import TAU_LOCKS, _pair

pytestmark = pytest.mark.gpu
NR = [3, 3, 1, 1, 2, 1]


def _check_records(g, state, blocks, full_keys=True):
    """blocks: g.evaluate(..., jac_blocks=True)["jac_blocks"]; compared with the debug rows of a second evaluation at the same state."""
    rd = g.evaluate(state, jac=True)
    row0 = g.family_rows()
    N = g.layout()["n_knots"]
    jmax = max(np.abs(rd["jac_vals"]).max(), 1e-300)
    for f in range(6):
        keys, vals = blocks[f]
        n = (row0[f + 1] - row0[f]) // NR[f]
        assert keys.shape == (n, 3) and vals.shape[:2] == (n, NR[f])
        if n == 0:
            continue
        W = vals.shape[2]
        dc = rd["jac_cols"][row0[f]:row0[f + 1]].reshape(n, NR[f], -1)
        dv = rd["jac_vals"][row0[f]:row0[f + 1]].reshape(n, NR[f], -1)
        ev = keys[:, 0] >= 0
        assert ev.all(), "family %d: %d blocks not evaluated" % (f, (~ev).sum())
        assert (dc[:, :, W:] == -1).all()
        assert np.abs(vals - dv[:, :, :W]).max() <= 1e-9 * jmax, "family %d" % f
        idx = range(n) if full_keys or n <= 2000 else np.random.default_rng(f).choice(n, 2000, replace=False)
        for i in idx:
            cols = lvx.jacobian_block_cols(f, N, W, keys[i])
            live = dc[i, 0, :W] >= 0
            assert (cols[live] == dc[i, 0, :W][live]).all(), "family %d block %d" % (f, i)
            assert not vals[i][:, ~live].any()   # constant columns: 0.0
    return rd


def _problem(seed=21):
    return synth.make_problem(seed=seed, duration=1.0, n_surfel=600, n_planes=8, n_landmarks=24, n_camsurf=8)


@pytest.mark.parametrize("locks,switch", [(TAU_LOCKS, None), (0, None), (TAU_LOCKS | lvx.LOCK_R3, None), (TAU_LOCKS | lvx.LOCK_LANDMARKS, None), (0, "FORCE_LEGACY"),
                                         (TAU_LOCKS, "REP_FUSED"), (0, "REP_FUSED")])
def test_records_match_the_debug_rows(locks, switch):
    P = _problem()
    o, g = _pair(P, locks)
    if switch:
        g.set_switch(switch, 1)
    s = P["state0"].copy()
    N = P["n_knots"]
    if not (locks & lvx.LOCK_LIDAR_TAU):
        s[7 * N + 16 + 7] = 3e-4
    if not (locks & lvx.LOCK_CAM_TAU):
        s[7 * N + 24 + 7] = -2e-4
    rb = g.evaluate(s, normal_eq=True, jac_blocks=True)
    rp = g.evaluate(s, normal_eq=True)                    # the same pass without the bit
    assert np.array_equal(rb["residuals"], rp["residuals"])
    assert np.abs(rb["H"] - rp["H"]).max() <= 1e-10 * np.abs(rp["H"]).max()
    widths = [v.shape[2] for _, v in rb["jac_blocks"]]
    assert widths[3] == 54 + (0 if locks & lvx.LOCK_LIDAR_TAU else 1) and widths[4] == 55 + (0 if locks & lvx.LOCK_CAM_TAU else 1)
    if locks & lvx.LOCK_R3:
        assert rb["jac_blocks"][lvx.FAM_ACCEL][0].shape == (0, 3)
    _check_records(g, s, rb["jac_blocks"])
    g.close()


def test_the_bit_is_exclusive_with_the_debug_rows_and_needs_a_request():
    P = _problem()
    _, g = _pair(P, TAU_LOCKS)
    g.evaluate(P["state0"])
    with pytest.raises(lvx.LvxError) as ei:
        g.jacobian_blocks(lvx.FAM_SURFEL)
    assert ei.value.code == lvx.E_STATE
    g.evaluate(P["state0"], jac_blocks=True)
    assert g.jacobian_blocks(lvx.FAM_SURFEL)[0].shape[0] == len(P["surf_t"])
    with pytest.raises(lvx.LvxError) as ei:
        g.evaluate(P["state0"], jac=True, jac_blocks=True)
    assert ei.value.code == lvx.E_ARG
    with pytest.raises(lvx.LvxError) as ei:
        g.jacobian_blocks(lvx.FAM_SURFEL)        # the failed call left nothing to read, not the records of the pass before it
    assert ei.value.code == lvx.E_STATE
    g.evaluate(P["state0"], jac_blocks=True)
    g.evaluate(P["state0"])                      # a pass without the bit
    with pytest.raises(lvx.LvxError) as ei:
        g.jacobian_blocks(lvx.FAM_SURFEL)
    assert ei.value.code == lvx.E_STATE
    g.close()


@pytest.mark.parametrize("case", ["merged_hub", "large_rotation"])
def test_fallback_rows_come_from_the_exact_kernel(case):
    """The states of test_gpu_eval's fallback tests on a fresh context: the listed rows are evaluated by k_family, and their records still match."""
    if case == "merged_hub":
        P = synth.make_problem(seed=31, duration=1.0, n_surfel=400, n_planes=6, n_landmarks=0, n_camsurf=0)
        P["t_map"] = P["t0"] + 12 * P["dt"] - 5e-6
        P["surf_t"] = np.sort(np.concatenate([P["t_map"] + np.linspace(2e-3, 0.03, 40), P["surf_t"][40:]]))
        _, g = _pair(P, TAU_LOCKS, prior=False)
        s = P["state0"].copy()
        s[7 * P["n_knots"] + 16 + 7] = 8e-6
    else:
        P = synth.make_problem(seed=33, duration=1.5, n_surfel=500, n_planes=8, n_landmarks=20, n_camsurf=6)
        _, g = _pair(P, TAU_LOCKS, prior=False)
        N = P["n_knots"]
        s = P["state0"].copy()
        k = N // 2
        q = s[3 * N + 4 * k:3 * N + 4 * k + 4].copy()
        s[3 * N + 4 * k:3 * N + 4 * k + 4] = synth.qmul(synth.q_from_rotvec(np.array([0.0, 0.0, 2.0])), q)
    rb = g.evaluate(s, normal_eq=True, jac_blocks=True)
    lo = g.layout()
    assert lo["exact_fallback"] == 0 and lo["fallback_rows"] > 0
    _check_records(g, s, rb["jac_blocks"])
    rb2 = g.evaluate(s, normal_eq=True, jac_blocks=True)   # lists in place from the start
    for f in range(6):
        assert np.array_equal(rb["jac_blocks"][f][0], rb2["jac_blocks"][f][0]) and np.array_equal(rb["jac_blocks"][f][1], rb2["jac_blocks"][f][1])
    g.close()


@pytest.mark.parametrize("det", [0, 1])
def test_the_bit_does_not_disturb_the_pass(det):
    P = _problem(seed=23)
    _, g = _pair(P, 0)
    g.set_switch("DETERMINISTIC", det)
    s = P["state0"].copy()
    s[7 * P["n_knots"] + 16 + 7] = 2e-4
    r0 = g.evaluate(s, normal_eq=True)
    g0, d0 = g.gradient()
    r1 = g.evaluate(s, normal_eq=True, jac_blocks=True)
    g1, d1 = g.gradient()
    r2 = g.evaluate(s, normal_eq=True, dense=False, jac_blocks=True)
    assert np.array_equal(r0["residuals"], r1["residuals"])
    if det:
        # cost and residuals are bitwise those of the pass without the bit.  The normal equations are not: an IMU-only problem already shows it (the fused IMU
        # kernel's export instantiation, k_imu_own<true>, is register-allocated differently — 248 against 243 AGPRs — and its Jacobian rounds differently in the
        # last bit), band, border rows and dense border differing by at most 1.7e-16 of max|H|.  Checked at 1e-15 relative instead.
        assert r0["cost"] == r1["cost"]
        assert np.abs(r1["H"] - r0["H"]).max() <= 1e-15 * np.abs(r0["H"]).max()
        assert np.abs(g1 - g0).max() <= 1e-15 * np.abs(g0).max() and np.abs(d1 - d0).max() <= 1e-15 * np.abs(d0).max()
    for f in range(6):   # records involve no atomics: bitwise repeatable in every mode
        assert np.array_equal(r1["jac_blocks"][f][0], r2["jac_blocks"][f][0]) and np.array_equal(r1["jac_blocks"][f][1], r2["jac_blocks"][f][1])
    g.close()


def test_full_size_records_match_the_debug_rows():
    P = synth.make_bench_problem(seed=4)
    g = lvx.Context(0)
    lvx.load_problem(g, P, TAU_LOCKS)
    rb = g.evaluate(P["state0"], residuals=False, jac_blocks=True)
    _check_records(g, P["state0"], rb["jac_blocks"], full_keys=False)
    g.close()


def test_ceres_seam_in_blocks_mode_hands_out_the_ambient_blocks():
    """test_ceres_shim's ambient-fixture check, with the callback in JacobianRows::kBlocks."""
    import test_ambient_pin as A
    import test_jacobian_blocks as TB
    lib = TB.build_blocks_lib()
    P = A._load()
    N, L = P["n_knots"], P["n_landmarks"]
    g = lvx.Context(0)
    lvx.load_problem(g, P, A.TAU)
    g.set_orientation_prior(P["prior_t"], P["prior_q_wxyz"], P["prior_w"])
    ns, nres = g.state_size, g.layout()["n_residuals"]
    res, J = np.zeros(nres), np.zeros((nres, ns))
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    state = np.ascontiguousarray(P["state"], np.float64)
    keep = [np.ascontiguousarray(P[k], np.float64) for k in ("t_imu", "surf_t", "rep_t0", "lm_t0")] + [np.ascontiguousarray(P[k], np.int32) for k in ("rep_lm", "cs_lm")]
    rc = lib.shim_check_all_blocks(g._h, d(state), C.c_int(ns), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(N), C.c_int(L), C.c_double(P["camera"]["readout"]), C.c_uint(A.TAU),
                                   C.c_int(len(P["t_imu"])), keep[0].ctypes.data_as(C.c_void_p), C.c_int(1), C.c_double(P["prior_t"]), C.c_int(len(P["surf_t"])), keep[1].ctypes.data_as(C.c_void_p),
                                   C.c_double(P["t_map"]), C.c_int(len(P["rep_lm"])), keep[4].ctypes.data_as(C.c_void_p), keep[2].ctypes.data_as(C.c_void_p), keep[3].ctypes.data_as(C.c_void_p),
                                   C.c_int(len(P["cs_lm"])), keep[5].ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), J.ctypes.data_as(C.c_void_p))
    assert rc == 0
    g.close()
    r_ref, Jt_ref, _, _, _ = A._reference_system(P, A._free(P, A.TAU))
    assert np.abs(res - r_ref).max() <= 1e-11 * max(np.abs(r_ref).max(), 100.0)
    T = A._tangent_map(P["state"], N, L)
    Jt = J @ T
    fmax = np.array([np.abs(Jt_ref[P["row_family"] == f]).max() for f in P["row_family"]])[:, None]
    scale = np.maximum(np.abs(Jt_ref).max(axis=1, keepdims=True), 1e-6 * fmax)
    locked = np.ones(Jt.shape[1], bool); locked[A._free(P, A.TAU)] = False
    assert (np.abs(Jt - Jt_ref)[:, ~locked] / scale).max() <= 1e-9



def _shim_dense(fn, g, P, locks):
    """Every block of P through the shim (fn: shim_check_all of the debug route or shim_check_all_blocks) -> (residuals, dense ambient J)."""
    ns, nres = g.state_size, g.layout()["n_residuals"]
    res, J = np.zeros(nres), np.zeros((nres, ns))
    f64 = lambda k: np.ascontiguousarray(P.get(k, np.zeros(0)), np.float64)
    i32 = lambda k: np.ascontiguousarray(P.get(k, np.zeros(0)), np.int32)
    keep = [np.ascontiguousarray(P["state"], np.float64), f64("t_imu"), f64("surf_t"), f64("rep_t0"), f64("lm_t0"), i32("rep_lm"), i32("cs_lm")]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = fn(g._h, p(keep[0]), C.c_int(ns), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(P["n_knots"]), C.c_int(P["n_landmarks"]), C.c_double(P["camera"]["readout"]), C.c_uint(locks),
            C.c_int(len(keep[1])), p(keep[1]), C.c_int(0), C.c_double(0.0), C.c_int(len(keep[2])), p(keep[2]), C.c_double(P["t_map"]), C.c_int(len(keep[5])), p(keep[5]), p(keep[3]), p(keep[4]),
            C.c_int(len(keep[6])), p(keep[6]), p(res), p(J))
    assert rc == 0
    return res, J


def test_ceres_seam_in_blocks_mode_at_the_merged_hub_corner():
    """The shim in blocks mode on a fresh context at the state where the fused kernels hand rows to the exact fallback (lvx_evaluate selects it and
    evaluates once more): the ambient blocks equal the debug route's."""
    import os
    import subprocess
    import test_jacobian_blocks as TB
    lib_b = TB.build_blocks_lib()
    src, so = os.path.join(TB.NATIVE, "ceres_shim_check.cpp"), os.path.join(TB.NATIVE, "libceres_shim_check.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (src, os.path.join(TB.LIBDIR, "host", "lvx_ceres_shim.hpp"), os.path.join(TB.ROOT, "include", "lvx.h"))):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.join(TB.NATIVE, "mock_ceres"), "-I" + os.path.join(TB.LIBDIR, "host"),
                               src, "-o", so, "-L" + TB.LIBDIR, "-llvx", "-Wl,-rpath," + TB.LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    lib_d = C.CDLL(so)
    P = synth.make_problem(seed=31, duration=1.0, n_surfel=400, n_planes=6, n_landmarks=0, n_camsurf=0)
    P["t_map"] = P["t0"] + 12 * P["dt"] - 5e-6
    P["surf_t"] = np.sort(np.concatenate([P["t_map"] + np.linspace(2e-3, 0.03, 40), P["surf_t"][40:]]))
    P["state"] = P["state0"].copy()
    P["state"][7 * P["n_knots"] + 16 + 7] = 8e-6
    out = []
    for fn in (lib_b.shim_check_all_blocks, lib_d.shim_check_all):
        g = lvx.Context(0)
        lvx.load_problem(g, P, TAU_LOCKS)
        out.append(_shim_dense(fn, g, P, TAU_LOCKS))
        if fn is lib_b.shim_check_all_blocks:
            lo = g.layout()
            assert lo["exact_fallback"] == 0 and lo["fallback_rows"] > 0   # the rows went to the exact kernel during the shim's evaluation
        g.close()
    (rb, Jb), (rd, Jd) = out
    assert np.abs(rb - rd).max() <= 1e-11 * np.abs(rd).max()
    assert np.abs(Jb - Jd).max() <= 1e-9 * np.abs(Jd).max()
