"""Calibration covariance without a GPU: the C ABI exports the calls and the record has the header's layout, NULL arguments are refused, and the Jacobi eigen-solver the
device kernel k_calib_cov runs in LDS (lvi-exc_amd/csrc/lvx_symeig.h) — built with g++ as a stand-alone program, one lane, no barrier — agrees with LAPACK
(numpy.linalg.eigh) on random, graded and degenerate matrices of every size class the kernel meets."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import lvx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_library_exports_the_calls_and_the_record_matches_the_header():
    l = lvx.lib()
    for name in ("lvx_calib_cov_default_options", "lvx_calibration_covariance"):
        assert hasattr(l, name), name
    # lvx_calib_cov of include/lvx.h, member by member
    src = open(os.path.join(ROOT, "include", "lvx.h")).read()
    body = re.search(r"typedef struct lvx_calib_cov \{(.*?)\} lvx_calib_cov;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for typ, names in re.findall(r"\b(int32_t|double)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(.*)\])?\s*$", n)
            decl.append((m.group(1), typ, eval(m.group(2)) if m.group(2) else 1))   # noqa: S307 — "22 * 22" of the project's own header
    assert decl == [("n_free", "int32_t", 1), ("free_index", "int32_t", 22), ("cov", "double", 484), ("sigma", "double", 22), ("info_eig", "double", 22),
                    ("info_vec", "double", 484), ("scale", "double", 22), ("radius", "double", 1), ("sweeps", "int32_t", 1), ("n_hub_eliminated", "int32_t", 1)]
    assert [(n, C.sizeof(t)) for n, t in lvx.CalibCov._fields_] == [(n, (4 if t == "int32_t" else 8) * k) for n, t, k in decl]
    assert lvx.CalibCov.cov.offset == 96 and C.sizeof(lvx.CalibCov) == 96 + 8 * (484 + 22 + 22 + 484 + 22) + 8 + 4 + 4
    assert C.sizeof(lvx.CalibCovOptions) == 16
    opt = lvx.CalibCovOptions()
    assert l.lvx_calib_cov_default_options(C.byref(opt)) == lvx.OK
    assert (opt.radius, opt.jacobi_scaling, opt.max_sweeps) == (1e8, 1, 30)


def test_null_arguments_are_refused():
    l = lvx.lib()
    opt, rec = lvx.CalibCovOptions(), lvx.CalibCov()
    assert l.lvx_calib_cov_default_options(None) == lvx.E_ARG
    l.lvx_calib_cov_default_options(C.byref(opt))
    assert l.lvx_calibration_covariance(None, C.byref(opt), C.byref(rec)) == lvx.E_ARG
    assert l.lvx_calibration_covariance(None, None, C.byref(rec)) == lvx.E_ARG
    assert l.lvx_calibration_covariance(None, C.byref(opt), None) == lvx.E_ARG


@pytest.fixture(scope="module")
def symeig(tmp_path_factory):
    d = tmp_path_factory.mktemp("symeig")
    exe = str(d / "symeig_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "native", "symeig_host_check.cpp"), "-o", exe])

    def run(mats, max_sweeps=30):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(mats)))
            for A in mats:
                f.write(struct.pack("<ii", A.shape[0], max_sweeps))
                f.write(np.ascontiguousarray(A, dtype="<f8").tobytes())
        subprocess.check_call([exe, fin, fout])
        b, o, res = open(fout, "rb").read(), 0, []
        for A in mats:
            n = A.shape[0]
            rc, sweeps = struct.unpack_from("<ii", b, o)
            off = struct.unpack_from("<d", b, o + 8)[0]
            w = np.frombuffer(b, "<f8", n, o + 16)
            V = np.frombuffer(b, "<f8", n * n, o + 16 + 8 * n).reshape(n, n)
            o += 16 + 8 * n + 8 * n * n
            res.append(dict(rc=rc, sweeps=sweeps, off=off, w=w, V=V))
        assert o == len(b)
        return res
    return run


def _spd(rng, n):
    X = rng.standard_normal((n + 5, n))
    return X.T @ X


def _check(A, r, rel):
    n = A.shape[0]
    wn = np.linalg.eigh(A)[0]
    assert r["rc"] == 0 and r["off"] <= EPS and 0 <= r["sweeps"] <= 12
    assert np.all(np.diff(r["w"]) >= 0)
    assert np.abs(r["w"] / wn - 1).max() <= rel, np.abs(r["w"] / wn - 1).max()
    V = r["V"]
    assert np.abs(V.T @ V - np.eye(n)).max() <= 64 * EPS
    assert np.abs(A @ V - V * r["w"]).max() <= 64 * EPS * n * wn[-1]   # backward stable: residual against the norm


@pytest.mark.parametrize("n", [1, 2, 14, 20, 22])
def test_random_spd_matrices_of_every_size(symeig, n):
    """n = 1 (no pair), 2 (one), odd-free even sizes of the lock masks (14: solve3's free calibration scalars, 20, 22); condition numbers of a few hundred, where
    LAPACK's eigenvalues are good to n eps cond: 1e-11 relative leaves two decades."""
    rng = np.random.default_rng(100 + n)
    mats = [_spd(rng, n) for _ in range(4)]
    for A, r in zip(mats, symeig(mats)):
        _check(A, r, 1e-11)


def test_odd_size_takes_the_bye(symeig):
    rng = np.random.default_rng(7)
    mats = [_spd(rng, n) for n in (3, 13, 21)]
    for A, r in zip(mats, symeig(mats)):
        _check(A, r, 1e-11)


def test_graded_matrix_keeps_relative_accuracy(symeig):
    """D B D with B of unit diagonal (condition ~50) and D from 1 down to 1e-6: entries and eigenvalues graded over 12 decades, large to small — the order in which
    LAPACK's tridiagonal reduction keeps the small eigenvalues relatively accurate too (measured against mpmath at 40 digits: LAPACK 7e-14, this routine 1e-14), so
    the comparison can be held to 1e-12 RELATIVE for every eigenvalue."""
    rng = np.random.default_rng(3)
    n = 22
    B = _spd(rng, n)
    d = 1 / np.sqrt(np.diag(B))
    B = B * d[:, None] * d[None, :]
    D = 10.0 ** (-np.linspace(0, 6, n))
    A = B * D[:, None] * D[None, :]
    r, = symeig([A])
    wn = np.linalg.eigh(A)[0]
    assert wn[-1] / wn[0] > 1e11
    assert r["rc"] == 0 and np.abs(r["w"] / wn - 1).max() <= 1e-12, np.abs(r["w"] / wn - 1).max()
    V = r["V"]
    assert np.abs(V.T @ V - np.eye(n)).max() <= 64 * EPS
    # every eigenpair to ITS OWN scale, in the graded metric: D^-1 (A v - w v) against w |D^-1 v| ... the residual column by column relative to w_k |v_k|_D
    R = (A @ V - V * r["w"]) / D[:, None]
    assert (np.abs(R).max(axis=0) <= 1e-12 * np.abs(B).sum(axis=1).max() * np.abs(V * D[:, None]).max(axis=0)).all()


def test_repeated_eigenvalue_and_inert_directions(symeig):
    """Q diag(3, 3, 3, 1, ...) Q^T: a triple eigenvalue (the eigenvectors are any basis of the eigenspace: checked as a projector); and the calibration block's own
    degenerate shape, six decoupled slots at the LM floor 1e-6 / 1e8 beside an order-one block: no rotation touches them, they come out exact."""
    rng = np.random.default_rng(11)
    n = 14
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = np.concatenate([[3.0, 3.0, 3.0], np.linspace(0.5, 2.0, n - 3)])
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    B = np.zeros((22, 22))
    B[:16, :16] = _spd(rng, 16) / 16
    B[16:, 16:] = np.eye(6) * 1e-14
    ra, rb = symeig([A, B])
    assert ra["rc"] == 0 and np.abs(np.sort(lam) - ra["w"]).max() <= 32 * EPS * 3
    top = ra["V"][:, -3:]
    assert np.abs(top @ top.T - Q[:, :3] @ Q[:, :3].T).max() <= 1e-13
    assert rb["rc"] == 0 and (rb["w"][:6] == 1e-14).all()
    assert (rb["V"][:16, :6] == 0).all() and (np.abs(rb["V"][16:, :6]).sum(axis=0) == 1).all()
    assert np.abs(rb["w"][6:] / np.linalg.eigh(B[:16, :16])[0] - 1).max() <= 1e-11


def test_sweep_cap_is_reported(symeig):
    rng = np.random.default_rng(5)
    A = _spd(rng, 22)
    r, = symeig([A], max_sweeps=1)
    assert r["rc"] == 1 and r["sweeps"] == 1 and r["off"] > 1e-8
