"""The joint calibration covariance without a GPU: the float64 reference of tests/joint_cov_cases.py (what tests/test_gpu_joint_cov.py holds the device against) on the
ORACLE's dense H, the stored accuracy figures of tests/golden/joint_cov_ref.npz, and the ABI of lvx_joint_calib_cov."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import calib_cov_cases as CC
import joint_cov_cases as JC
import lvx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ERR = dict(np.load(os.path.join(ROOT, "tests", "golden", "joint_cov_ref.npz")))
_H = {}


def _case(key, mask):
    """sequences of the set and their oracle H under the mask (computed once)"""
    if (key, mask) not in _H:
        seqs = JC.sequences(*JC.SETS[key])
        _H[key, mask] = (seqs, [JC.oracle_h(P, s, JC.MASKS[mask]) for P, s in seqs])
    seqs, Hs = _H[key, mask]
    return Hs, [P["n_knots"] for P, _ in seqs], [P["n_landmarks"] for P, _ in seqs]


def test_golden_file_has_every_case():
    names = [JC.case_name(m, R, sc, key) for key, m, R, sc in JC.all_cases()]
    assert len(names) == 18 and sorted(names) == sorted(REF_ERR)
    assert all(0 < float(v) < 1e-8 for v in REF_ERR.values())


@pytest.mark.parametrize("key,mask,radius,scaling", JC.all_cases())
def test_reference_reproduces_its_stored_error(key, mask, radius, scaling):
    """The stored figure is the float64 reference against mpmath at 40 digits (minutes per case).  Here the same float64 result is measured against the inverse formed
    in extended precision (64-bit mantissa: its own error is 1 / 2048 of the float64 one, so it reads the figure to a part in a thousand): within a factor 2 of the
    stored one — the figure belongs to THIS reference on THIS system."""
    Hs, Ns, Ls = _case(key, mask)
    ref = JC.reference(Hs, Ns, Ls, JC.MASKS[mask], radius, scaling)
    A, s = ref["A"], ref["s"]
    n = A.shape[0]
    upos = np.unique(np.concatenate([p[p >= 0] for p in ref["cpos"]]))
    aug = np.zeros((n + len(upos), n + len(upos)))
    aug[:n, :n] = A
    aug[upos, n + np.arange(len(upos))] = 1.0
    aug[n + np.arange(len(upos)), upos] = 1.0
    cx = -JC.schur(aug, np.arange(n), n + np.arange(len(upos))) * s[upos][:, None] * s[upos][None, :]   # E^T A^-1 E
    col = {int(p): k for k, p in enumerate(upos)}
    err = 0.0
    for p, rk in zip(ref["cpos"], ref["ranks"]):
        k = np.array([col[int(q)] for q in p[rk["cidx"]]])
        err = max(err, JC.rel_err(rk["cov"], cx[np.ix_(k, k)]))
    stored = float(REF_ERR[JC.case_name(mask, radius, scaling, key)])
    print("%-30s stored %.3e  measured %.3e" % (JC.case_name(mask, radius, scaling, key), stored, err))
    assert stored / 2 <= err <= 2 * stored


@pytest.mark.parametrize("key,mask,radius,scaling", JC.all_cases())
def test_contributions_and_shared_damping_add_up_to_the_schur_complement(key, mask, radius, scaling):
    Hs, Ns, Ls = _case(key, mask)
    ref = JC.reference(Hs, Ns, Ls, JC.MASKS[mask], radius, scaling)
    sl = ref["shared_free_slot"]
    S = sum(o[np.ix_(sl, sl)] for o in ref["own"]) + np.diag(ref["lmd_shared"]) / radius
    assert np.abs(S - ref["M"]).max() <= 1e-12 * np.abs(ref["M"]).max()
    locked = np.setdiff1d(np.arange(JC.N_SHARED), sl)
    assert all(not o[locked, :].any() and not o[:, locked].any() for o in ref["own"])
    assert (np.linalg.eigvalsh(ref["M"]) > 0).all()


@pytest.mark.parametrize("mask", list(JC.MASKS))
def test_one_rank_is_the_single_sequence_reference(mask):
    Hs, Ns, Ls = _case("w2", mask)
    for radius in JC.RADII:
        for scaling in (True, False):
            a = JC.reference(Hs[:1], Ns[:1], Ls[:1], JC.MASKS[mask], radius, scaling)
            b = CC.reference(Hs[0], Ns[0], Ls[0], JC.MASKS[mask], radius, scaling)
            assert list(a["ranks"][0]["cidx"]) == list(b["cidx"])
            assert CC.rel_err(a["ranks"][0]["cov"], b["cov"]) <= 1e-12 and np.array_equal(a["ranks"][0]["scale"], b["scale"])


def test_library_exports_the_call_and_the_record_matches_the_header(tmp_path):
    l = lvx.lib()
    assert hasattr(l, "lvx_calibration_covariance_shared")
    src = open(os.path.join(ROOT, "include", "lvx.h")).read()
    body = re.search(r"typedef struct lvx_joint_calib_cov \{(.*?)\} lvx_joint_calib_cov;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for typ, names in re.findall(r"\b(int32_t|double)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(.*)\])?\s*$", n)
            decl.append((m.group(1), typ, eval(m.group(2)) if m.group(2) else 1))   # noqa: S307 — "22 * 22" of the project's own header
    assert decl == [("n_free", "int32_t", 1), ("free_index", "int32_t", 22), ("cov", "double", 484), ("sigma", "double", 22), ("n_shared_free", "int32_t", 1),
                    ("shared_free_slot", "int32_t", 14), ("info_eig", "double", 14), ("info_vec", "double", 196), ("own_info", "double", 196), ("scale", "double", 22),
                    ("radius", "double", 1), ("sweeps", "int32_t", 1), ("n_hub_eliminated", "int32_t", 1), ("world", "int32_t", 1)]
    assert [(n, C.sizeof(t)) for n, t in lvx.JointCalibCov._fields_] == [(n, (4 if t == "int32_t" else 8) * k) for n, t, k in decl]
    # sizeof and every offset as the C compiler lays the header's struct out
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lvx.h"\nint main(void) {\n  printf("%zu", sizeof(lvx_joint_calib_cov));\n'
                    + "".join('  printf(" %%zu", offsetof(lvx_joint_calib_cov, %s));\n' % n for n, _, _ in decl) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(lvx.JointCalibCov)] + [getattr(lvx.JointCalibCov, n).offset for n, _, _ in decl]
    assert got[0] == 7656 and lvx.JointCalibCov.cov.offset == 96 and lvx.JointCalibCov.info_eig.offset == 4208 and lvx.JointCalibCov.world.offset == 7648


def test_null_arguments_are_refused():
    l = lvx.lib()
    opt, rec = lvx.CalibCovOptions(), lvx.JointCalibCov()
    l.lvx_calib_cov_default_options(C.byref(opt))
    assert l.lvx_calibration_covariance_shared(None, C.byref(opt), None, None, C.byref(rec)) == lvx.E_ARG
