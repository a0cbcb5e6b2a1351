"""GPU parity of the landmark rows (k_reproj_lmrows, csrc/lvx_eval.hip) by blocks per landmark: 1, 4, 5, 16, 17, 64 and 65 blocks — either side of the old trip of four, of the
group of 16 blocks whose records are requested together and of the 64 lanes that fetch the indices —, the camera time offset free (records of 57), landmarks whose blocks are all or
partly skipped, and blocks whose two poses share knots (LDS adds of one instruction collide).  Cases: tests/lmrows_depth_cases.py, their premises on the CPU in
tests/test_lmrows_depth_cases.py.  Compared the way tests/test_gpu_landmark_tracks.py compares: evaluation (H carries the landmark rows) at two states on one context against the
oracle with that file's bars, and the eliminated system through solve_step against the dense reference (step 1e-7 of max |d|, model cost change 1e-8)."""
import numpy as np
import pytest

import landmark_cases as LC
import lmrows_depth_cases as DC
import lvx
from oracle import lm
from oracle import oracle as O
from test_gpu_landmark_tracks import _compare_eval, _say

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle_at(name, key):
    """Oracle evaluation of a case at P[key]: computed once, shared, never written to."""
    if name not in _ORACLE:
        P, locks, _ = DC.build(name)
        o = O.Oracle(); lvx.load_problem(o, P, locks)
        _ORACLE[name] = (o, {})
    o, ev = _ORACLE[name]
    if key not in ev:
        ev[key] = o.evaluate(DC.build(name)[0][key], normal_eq=True)
    return ev[key]


def _ctx(name, **switches):
    P, locks, _ = DC.build(name)
    g = lvx.Context(0)
    for k, v in switches.items():
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


@pytest.mark.parametrize("name", DC.NAMES)
def test_rows_against_the_oracle(name):
    """state0, state_true and state0 again on ONE context: a row is stored whole every pass (zeros included), so nothing of the pass before may show."""
    P, locks, _ = DC.build(name)
    R = LC.track_regime(P, locks)
    g = _ctx(name)
    for key in ("state0", "state_true", "state0"):
        g.set_profiling(True); g.kernel_ms()
        rg = g.evaluate(P[key], normal_eq=True)
        _, launches = g.kernel_ms()
        g.set_profiling(False)
        assert launches[lvx.KERNEL_REP_LMROWS] == 1 and launches[lvx.KERNEL_REP_FUSED] == 0
        _compare_eval("depth", name, rg, _oracle_at(name, key))
    lo = g.layout()
    assert lo["lm_row_width"] == R["lm_wl"] and lo["rep_groups"] == len(R["groups"])
    g.close()


@pytest.mark.parametrize("name", DC.NAMES)
def test_eliminated_system(name):
    P, locks, _ = DC.build(name)
    ro = _oracle_at(name, "state0")
    free = lm.free_tangent_indices(P["n_knots"], P["n_landmarks"], locks)
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(ro["H"])[free], 0)))
    d_ref, m_ref, _ = lm.solve_step(ro["H"], ro["g"], free, 1e4, scale)
    g = _ctx(name)
    g.evaluate(P["state0"], normal_eq=True, dense=False)
    d, m = g.solve_step(1e4, True)
    e_d, e_m = np.abs(d - d_ref).max() / np.abs(d_ref).max(), abs(m - m_ref) / abs(m_ref)
    _say("depth.step", name, e_d); _say("depth.model", name, e_m)
    assert g.layout()["solver_fallbacks"] == 0
    assert e_d <= 1e-7 and e_m <= 1e-8
    g.close()


@pytest.mark.parametrize("name", ["counts", "collide"])
def test_deterministic_bits(name):
    P, locks, _ = DC.build(name)
    runs = []
    for _ in range(2):
        g = _ctx(name, DETERMINISTIC=1)
        for _ in range(2):
            r = g.evaluate(P["state0"], normal_eq=True)
            runs.append((r, g.normal_eq_checksum()))
        g.close()
    for r, chk in runs[1:]:
        assert chk == runs[0][1] and r["cost"] == runs[0][0]["cost"]
        assert np.array_equal(r["H"], runs[0][0]["H"]) and np.array_equal(r["g"], runs[0][0]["g"])
    _compare_eval("depth.det", name, runs[0][0], _oracle_at(name, "state0"))
