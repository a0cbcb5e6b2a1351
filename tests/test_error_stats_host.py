"""Error statistics without a GPU: the C ABI exports the calls, the reference's printErrorStatistics lines come out of lvx_host::FormatErrorStatistics
(lvi-exc_amd/host/lvx_estimator.hpp), and the value-only block evaluation the device kernels run (lvi-exc_amd/csrc/lvx_stats.h), built with g++, reproduces the oracle's
residual rows and — divided by the weights — the raw errors the statistics are sums of."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "lvi-exc_amd")
TAU = O.LOCK_LIDAR_TAU | O.LOCK_CAM_TAU


def test_library_exports_the_statistics_calls():
    l = lvx.lib()
    for name in ("lvx_error_statistics", "lvx_error_statistics_d", "lvx_get_plane_stats", "lvx_get_landmark_stats"):
        assert hasattr(l, name), name
    assert C.sizeof(lvx.FamilyStats) == 3 * 8 + 8 + 12 * 8 and C.sizeof(lvx.ErrorStats) == 6 * C.sizeof(lvx.FamilyStats) + 8
    # no context, no statistics: the calls are reachable only behind lvx_create, which reports a missing device instead of falling back
    h = C.c_void_p()
    rc = l.lvx_create(C.byref(h), C.c_int(0), C.c_uint32(0))
    if rc == lvx.OK:
        l.lvx_destroy(h)
    else:
        assert rc == lvx.E_NODEVICE and not h.value
    st = lvx.ErrorStats()
    assert l.lvx_error_statistics(None, None, C.byref(st)) == lvx.E_ARG
    assert l.lvx_error_statistics_d(None, None, C.byref(st)) == lvx.E_ARG
    assert l.lvx_get_plane_stats(None, C.c_int(0), None, None, None) == lvx.E_ARG
    assert l.lvx_get_landmark_stats(None, C.c_int(0), None, None, None) == lvx.E_ARG


@pytest.fixture(scope="module")
def demo_binary(tmp_path_factory):
    import build as lvx_build   # lvi-exc_amd/build.py
    lvx_build.build()
    out = str(tmp_path_factory.mktemp("stats") / "error_stats_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(LIBDIR, "host"), os.path.join(ROOT, "tests", "native", "error_stats_demo.cpp"), "-o", out,
                           "-L" + LIBDIR, "-llvx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_format_matches_the_reference_lines(demo_binary):
    """The reference streams `size << "; " << (sum / size).transpose()` (trajectory_manager_lvi.cpp:624-694; the accelerometer line with two blanks): Eigen writes a row
    vector with 6 significant digits, one blank between coefficients, each right-aligned to the widest.  Hand-filled sums: mean |e| for gyro / accel / LiDAR, the signed
    mean times the weight for the camera; a family without blocks prints nothing."""
    r = subprocess.run([demo_binary, "format"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [
        "============== Before optimization ================",
        "[Gyro]  Error size, average: 4000; 0.00123457        0.5      12.25",
        "[Accel] Error size, average: 4000;    0.25 0.0625  1e-07",
        "[LiDAR] Error size, average: 123456; 0.015625",
        "[CAMERA] Error size, average: 200; -0.75   1.5",
        "============== After optimization ================",
        "[Gyro]  Error size, average: 8; 0 2 0",
        "[CAMERA] Error size, average: 2;  7.5 -2.5",
    ]
    assert subprocess.run([demo_binary], capture_output=True).returncode == 2   # usage only: nothing touches a device


@pytest.fixture(scope="module")
def stats_check_lib():
    src = os.path.join(ROOT, "tests", "native", "stats_host_check.cpp")
    so = os.path.join(ROOT, "tests", "native", "libstats_host_check.so")
    deps = [src] + [os.path.join(LIBDIR, "csrc", f) for f in ("lvx_math.h", "lvx_resid.h", "lvx_stats.h")] + [os.path.join(ROOT, "oracle", "orc_problem.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
    return C.CDLL(so)


def _rows_by_family(o, P, so3_only):
    n_imu = len(P["t_imu"])
    cnt = [n_imu, 0 if so3_only else n_imu, 1, len(P["surf_t"]), len(P["rep_lm"]), len(P["cs_lm"])]
    nr = [3, 3, 1, 1, 2, 1]
    off = np.concatenate([[0], np.cumsum([c * k for c, k in zip(cnt, nr)])])
    assert off[-1] == o.num_residuals
    return cnt, nr, off


@pytest.mark.parametrize("locks,so3_only", [(TAU, False), (0, False), (TAU | O.LOCK_R3, True)])
def test_value_only_blocks_match_the_oracle(stats_check_lib, locks, so3_only):
    if so3_only:
        P = synth.make_problem(seed=7, duration=1.0, n_surfel=0, n_planes=1, n_landmarks=0)
    else:
        P = synth.make_problem(seed=4, duration=1.0, n_surfel=300, n_planes=6, n_landmarks=12, n_camsurf=8)
    P["huber_surf"], P["huber_rep"], P["huber_cs"] = 0.4, 2.0, 0.5
    o = O.Oracle(); lvx.load_problem(o, P, locks)
    o.set_orientation_prior(P["t0"], np.array([np.cos(5e-5), 0, 0, np.sin(5e-5)]), 28.0)
    o.set_so3_only(so3_only)
    W = stats_check_lib.hs_record_width()
    weights = [P["w_gyro"], P["w_acc"], 28.0, P["w_surf"], P["w_rep"], P["w_cs"]]
    hubers = [0, 0, 0, P["huber_surf"], P["huber_rep"], P["huber_cs"]]
    for name in ("state0",):   # the perturbed state: at the truth the noise-free camera-surfel rows are rounding noise of metre-sized terms, no scale to be relative to
        s = P[name].copy()
        N = P["n_knots"]
        if not (locks & O.LOCK_LIDAR_TAU):
            s[7 * N + 23] = 3e-4
        if not (locks & O.LOCK_CAM_TAU):
            s[7 * N + 31] = -2e-4
        ro = o.evaluate(s)["residuals"]
        res = np.zeros(o.num_residuals); rec = np.zeros((6, W))
        assert stats_check_lib.hs_evaluate(o._h, O._p(O._d(s)), O._p(res), O._p(rec)) == 0
        cnt, nr, off = _rows_by_family(o, P, so3_only)
        for f in range(6):
            rows = ro[off[f]:off[f + 1]].reshape(-1, nr[f])
            mine = res[off[f]:off[f + 1]].reshape(-1, nr[f])
            if cnt[f] == 0:
                assert not rec[f].any()
                continue
            scale = np.abs(rows).max()
            assert np.abs(mine - rows).max() <= 1e-11 * scale
            e = rows / weights[f]
            sq = (rows ** 2).sum(axis=1)
            out = (sq > hubers[f] ** 2) if hubers[f] > 0 else np.zeros(len(sq), bool)
            assert rec[f, 0] == cnt[f] and rec[f, 1] == out.sum()
            cost = 0.5 * np.where(out, 2 * hubers[f] * np.sqrt(sq) - hubers[f] ** 2, sq).sum()
            assert abs(rec[f, 2] - cost) <= 1e-12 * abs(cost)
            tol = 1e-11 * scale / weights[f]
            k = nr[f]
            assert np.abs(rec[f, 3:3 + k] / cnt[f] - e.mean(axis=0)).max() <= tol
            assert np.abs(rec[f, 6:6 + k] / cnt[f] - np.abs(e).mean(axis=0)).max() <= tol
            assert np.abs(rec[f, 9:9 + k] / cnt[f] - (e ** 2).mean(axis=0)).max() <= 2 * tol * np.abs(e).max()
            assert np.abs(rec[f, 12:12 + k] - np.abs(e).max(axis=0)).max() <= tol
            assert not rec[f, 3 + k:6].any() and not rec[f, 12 + k:15].any()
