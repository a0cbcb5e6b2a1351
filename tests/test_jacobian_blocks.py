"""Per-block Jacobian records (LVX_EVAL_JACOBIAN_BLOCKS, include/lvx.h) on the host side, no GPU needed:
* lvx_jacobian_block_cols against a restatement of the column table in lvx.h, every family, both widths;
* the blocks route of the Ceres shim (JacobianRows::kBlocks) against its debug-row route: random records for every block of the ambient fixture
  problem, expanded into 64-wide debug rows, scattered both ways through LvxRowBlock::Evaluate — the ambient blocks must be bitwise identical."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "lvi-exc_amd")

NR = {lvx.FAM_GYRO: 3, lvx.FAM_ACCEL: 3, lvx.FAM_PRIOR: 1, lvx.FAM_SURFEL: 1, lvx.FAM_REPROJ: 2, lvx.FAM_CAMSURF: 1}
WIDTH = {lvx.FAM_GYRO: (15,), lvx.FAM_ACCEL: (29,), lvx.FAM_PRIOR: (12,), lvx.FAM_SURFEL: (54, 55), lvx.FAM_REPROJ: (55, 56), lvx.FAM_CAMSURF: (60, 61)}


def _table_cols(fam, N, width, key):
    """The table of include/lvx.h, restated: 6 tangent scalars per knot (position | rotation), 4 knots from k0 (then k1); calibration base 6 N:
    roll, pitch, b_a (3), b_g (3), LiDAR theta p tau (8..14), camera theta p tau (15..21), rho_l at 6 N + 22 + l."""
    k0, k1, lm = key
    C0 = 6 * N
    knots = lambda k: [6 * (k + j) + s for j in range(4) for s in range(6)]
    rot = lambda k: [6 * (k + j) + 3 + s for j in range(4) for s in range(3)]
    if fam == lvx.FAM_GYRO:
        cols = rot(k0) + [C0 + 5, C0 + 6, C0 + 7]
    elif fam == lvx.FAM_ACCEL:
        cols = knots(k0) + [C0 + 0, C0 + 1, C0 + 2, C0 + 3, C0 + 4]
    elif fam == lvx.FAM_PRIOR:
        cols = rot(k0)
    elif fam == lvx.FAM_SURFEL:
        cols = knots(k0) + knots(k1) + [C0 + 8 + i for i in range(6)] + [C0 + 14]
    elif fam == lvx.FAM_REPROJ:
        cols = knots(k0) + knots(k1) + [C0 + 15 + i for i in range(6)] + [C0 + 22 + lm, C0 + 21]
    else:
        cols = knots(k0) + knots(k1) + [C0 + 15 + i for i in range(6)] + [C0 + 8 + i for i in range(6)] + [C0 + 21]
    return np.array(cols[:width], dtype=np.int32)


def test_block_cols_follow_the_table_in_the_header():
    rng = np.random.default_rng(5)
    N = 40
    for fam, widths in WIDTH.items():
        for w in widths:
            for _ in range(25):
                key = np.array([rng.integers(0, N - 3), rng.integers(0, N - 3), rng.integers(0, 30)], dtype=np.int32)
                if fam not in (lvx.FAM_SURFEL, lvx.FAM_REPROJ, lvx.FAM_CAMSURF):
                    key[1] = -1
                if fam != lvx.FAM_REPROJ:
                    key[2] = -1
                got = lvx.jacobian_block_cols(fam, N, w, key)
                assert got.shape == (w,)
                assert (got == _table_cols(fam, N, w, key)).all(), (fam, w, key)
    # a width the family does not have, an unknown family
    for fam, w in ((lvx.FAM_GYRO, 16), (lvx.FAM_SURFEL, 64), (6, 10)):
        with pytest.raises(lvx.LvxError):
            lvx.jacobian_block_cols(fam, N, w, [0, 0, 0])


def test_block_cols_shared_knots_map_twice():
    """Both poses in one interval (the merged-segment corner): the two knot column groups map to the same tangent scalars — the consumer adds them."""
    cols = lvx.jacobian_block_cols(lvx.FAM_SURFEL, 20, 54, [7, 7, -1])
    assert (cols[:24] == cols[24:48]).all()


def build_blocks_lib():
    """tests/native/ceres_blocks_check.cpp against the mock Ceres interfaces and liblvx (also used by the GPU seam test)."""
    import build as lvx_build
    lvx_build.build()
    src, so = os.path.join(NATIVE, "ceres_blocks_check.cpp"), os.path.join(NATIVE, "libceres_blocks_check.so")
    deps = [src, os.path.join(LIBDIR, "host", "lvx_ceres_shim.hpp"), os.path.join(ROOT, "include", "lvx.h"), os.path.join(NATIVE, "mock_ceres", "ceres", "ceres.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.join(NATIVE, "mock_ceres"), "-I" + os.path.join(LIBDIR, "host"),
                               src, "-o", so, "-L" + LIBDIR, "-llvx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def blocks_lib():
    return build_blocks_lib()


def _scatter_compare(lib, P, locks, tau_free, seed):
    d = lambda a: np.ascontiguousarray(a, np.float64)
    i = lambda a: np.ascontiguousarray(a, np.int32)
    keep = [d(P["state"]), d(P["t_imu"]), d(P["surf_t"]), i(P["rep_lm"]), d(P["rep_t0"]), d(P["lm_t0"]), i(P["cs_lm"])]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    shared, skipped = C.c_int(0), C.c_int(0)
    rc = lib.blocks_scatter_compare(p(keep[0]), C.c_double(P["t0"]), C.c_double(P["dt"]), C.c_int(P["n_knots"]), C.c_int(P["n_landmarks"]), C.c_double(P["camera"]["readout"]),
                                    C.c_uint(locks), C.c_int(len(P["t_imu"])), p(keep[1]), C.c_int(1), C.c_double(P["prior_t"]), C.c_int(len(P["surf_t"])), p(keep[2]),
                                    C.c_double(P["t_map"]), C.c_int(len(P["rep_lm"])), p(keep[3]), p(keep[4]), p(keep[5]), C.c_int(len(P["cs_lm"])), p(keep[6]),
                                    C.c_int(tau_free), C.c_uint(seed), C.byref(shared), C.byref(skipped))
    return rc, shared.value, skipped.value


@pytest.mark.parametrize("tau_free", [0, 1])
def test_shim_blocks_route_scatters_bitwise_like_the_debug_rows(blocks_lib, tau_free):
    import test_ambient_pin as A
    P = A._load()
    rc, shared, skipped = _scatter_compare(blocks_lib, P, A.TAU, tau_free, seed=11 + tau_free)
    assert rc == 0
    assert shared > 0 and skipped > 0   # records whose two poses share knots, and blocks that were not evaluated, were both exercised
