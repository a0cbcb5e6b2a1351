"""GPU parity of everything behind k_reproj_jac on the hand-placed visual tracks of tests/landmark_cases.py: the cross-term groups (k_reproj_cross: cap splits, trips of 8, panel
offsets, w1 < w0, strays), the landmark rows (k_reproj_lmrows), the landmark elimination by groups and per landmark (k_lm_schur_grp / k_lm_schur, the latter through the test switch
TEST_LM_SCHUR_ONE and — long_track — by itself), k_lm_back and the LM loop's in-place elimination; through lvx.Context, against the oracle and the dense numpy step / loop of oracle/lm.py.

Bars (the project's existing ones): residuals 1e-11 of max(|r|, 100 px), cost 1e-12, H and g 1e-10 of their maxima, every H entry 1e-9 of sqrt(H_ii H_jj) (tests/test_gpu_reproj_paths.py);
step 1e-7 of max |d|, model cost change 1e-8 (tests/test_gpu_solver.py); LM: same accept / reject sequence and termination, cost history 1e-7.  Every comparison prints its
measured figure (lines "LMTRACK ...") before it asserts."""
import numpy as np
import pytest

import landmark_cases as LC
import lvx
from oracle import lm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(name):
    """The oracle of a case with its evaluations at state0 / state_true: computed once, shared by every test, never written to."""
    if name not in _ORACLE:
        P, locks, _ = LC.build(name)
        o = O.Oracle(); lvx.load_problem(o, P, locks)
        _ORACLE[name] = (o, {})
    o, ev = _ORACLE[name]

    def at(key):
        if key not in ev:
            ev[key] = o.evaluate(LC.build(name)[0][key], normal_eq=True)
        return ev[key]
    return o, at


def _ctx(name, **switches):
    P, locks, _ = LC.build(name)
    g = lvx.Context(0)
    for k, v in switches.items():
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _say(what, name, value):
    print("LMTRACK %-14s %-26s %.3e" % (what, name, value))


def _compare_eval(tag, name, rg, ro, normal_eq=True):
    rs = max(np.abs(ro["residuals"]).max(), 100.0)
    e_r = np.abs(rg["residuals"] - ro["residuals"]).max() / rs
    e_c = abs(rg["cost"] - ro["cost"]) / abs(ro["cost"])
    _say(tag + ".res", name, e_r); _say(tag + ".cost", name, e_c)
    out = [e_r <= 1e-11, e_c <= 1e-12]
    if normal_eq:
        e_h = np.abs(rg["H"] - ro["H"]).max() / np.abs(ro["H"]).max()
        e_g = np.abs(rg["g"] - ro["g"]).max() / np.abs(ro["g"]).max()
        dg = np.diag(ro["H"])
        # A landmark seen in its reference view only has both poses equal: its derivatives cancel and H_ll is ROUNDING NOISE of an exact zero (measured 1e-27 next to
        # diagonals of 1e2, tests/test_landmark_cases.py), on the device as in the oracle — no scale to compare entries against.  Such a row must be noise on the device too
        # (<= 1e-20 of the largest diagonal) and stays under the 1e-10-of-max bar above; the entry-scaled bar holds every other row and column.
        noise = (dg > 0.0) & (dg <= 1e-20 * dg.max())
        assert (np.diag(rg["H"])[noise] <= 1e-20 * dg.max()).all()
        d = np.sqrt(np.maximum(np.where(noise, 0.0, dg), 0.0))
        scale = np.outer(d, d)
        err = np.abs(rg["H"] - ro["H"])
        err[noise, :] = 0.0; err[:, noise] = 0.0
        e_e = (err / np.maximum(scale, 1e-300))[err > 1e-300].max(initial=0.0)
        _say(tag + ".H", name, e_h); _say(tag + ".g", name, e_g); _say(tag + ".H_entry", name, e_e)
        if e_e > 1e-9:
            i, j = np.unravel_index(np.argmax(err / np.maximum(scale, 1e-300) * (err > 1e-300)), err.shape)
            print("LMTRACK worst entry of %s: H[%d, %d] device %.17g oracle %.17g" % (name, i, j, rg["H"][i, j], ro["H"][i, j]))
        out += [e_h <= 1e-10, e_g <= 1e-10, e_e <= 1e-9]
    assert all(out), (tag, name, out)


def _check_plan(g, name):
    P, locks, _ = LC.build(name)
    R = LC.track_regime(P, locks)
    lo = g.layout()
    assert lo["exact_fallback"] == 0
    assert (lo["rep_groups"], lo["lm_groups"], lo["lm_group_spread"], lo["lm_row_width"]) == (len(R["groups"]), len(R["elim_groups"]), R["elim_spread"], R["lm_wl"]), (lo, name)
    assert (lo["n_band"], lo["n_border"], lo["n_hub_knots"]) == (R["n_band"], R["n_border"], R["n_hub"])
    return R


def _check_eval(name, mode):
    P, locks, _ = LC.build(name)
    o, at = _oracle(name)
    g = _ctx(name, REP_FUSED=mode)
    tag = "eval" if mode < 0 else "fused"
    for key in ("state0", "state_true"):
        g.set_profiling(True); g.kernel_ms()
        rg = g.evaluate(P[key], normal_eq=True)
        _, launches = g.kernel_ms()
        g.set_profiling(False)
        if mode > 0:
            assert launches[lvx.KERNEL_REP_FUSED] == 1 and launches[lvx.KERNEL_REP_JAC] == 0
        else:
            assert launches[lvx.KERNEL_REP_FUSED] == 0 and launches[lvx.KERNEL_REP_JAC] == 1 and launches[lvx.KERNEL_REP_CROSS] == 1 and launches[lvx.KERNEL_REP_LMROWS] == 1
        _compare_eval(tag, name, rg, at(key))
        rc = g.evaluate(P[key], normal_eq=False)                       # the cost-only pass: the same kernels without their assembly half
        _compare_eval(tag + "_cost", name, rc, at(key), normal_eq=False)
        _check_plan(g, name)
    g.close()


@pytest.mark.parametrize("name", LC.NAMES)
def test_evaluation_on_the_chain(name):
    _check_eval(name, -1)


@pytest.mark.parametrize("name", LC.GROUP_SIZE_CASES)
def test_evaluation_fused(name):
    """The single-launch kernel (REP_FUSED = 1) on the group-size cases; 63 / 64 / 65 blocks in a pair sit on either side of its 64-lane groups."""
    _check_eval(name, 1)


@pytest.mark.parametrize("name", LC.DETERMINISTIC_CASES)
def test_deterministic_bits(name):
    """DETERMINISTIC: the cap split (two groups of one window pair), the mirrored pairs ((w0, w1) and (w1, w0) add to the same entries) and 65 landmarks on a frame (three
    elimination groups on the same band rows): two evaluations and two steps give the same bits, on a fresh context too, and all of them are within the bars of the oracle."""
    P, locks, _ = LC.build(name)
    o, at = _oracle(name)
    ro = at("state0")
    free = lm.free_tangent_indices(P["n_knots"], P["n_landmarks"], locks)
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(ro["H"])[free], 0)))
    d_ref, m_ref, _ = lm.solve_step(ro["H"], ro["g"], free, 1e4, scale)
    R = LC.track_regime(P, locks)
    runs = []
    for c in range(2):
        g = _ctx(name, DETERMINISTIC=1)
        for _ in range(2):
            r = g.evaluate(P["state0"], normal_eq=True)
            chk = g.normal_eq_checksum()
            d, m = g.solve_step(1e4, True)
            runs.append((r, chk, d, m))
        lo = g.layout()
        assert lo["solver_fallbacks"] == 0
        assert lo["rep_colours"] == len(set(R["colours"])), (lo["rep_colours"], R["colours"])          # the colouring itself: bits that repeat do not prove it (two additions commute)
        g.close()
    for r, chk, d, m in runs[1:]:
        assert chk == runs[0][1] and r["cost"] == runs[0][0]["cost"]
        assert np.array_equal(r["H"], runs[0][0]["H"]) and np.array_equal(r["g"], runs[0][0]["g"]) and np.array_equal(r["residuals"], runs[0][0]["residuals"])
        assert np.array_equal(d, runs[0][2]) and m == runs[0][3], "solve_step not repeatable: max diff %.3e" % np.abs(d - runs[0][2]).max()
    _compare_eval("det", name, runs[0][0], ro)
    e_d, e_m = np.abs(runs[0][2] - d_ref).max() / np.abs(d_ref).max(), abs(runs[0][3] - m_ref) / abs(m_ref)
    _say("det.step", name, e_d); _say("det.model", name, e_m)
    assert e_d <= 1e-7 and e_m <= 1e-8


def _step_refs(name, radius, scaling):
    P, locks, _ = LC.build(name)
    ro = _oracle(name)[1]("state0")
    free = lm.free_tangent_indices(P["n_knots"], P["n_landmarks"], locks)
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(ro["H"])[free], 0))) if scaling else None
    d_ref, m_ref, _ = lm.solve_step(ro["H"], ro["g"], free, radius, scale)
    return d_ref, m_ref


def _check_step(name, radius, scaling):
    """evaluate + solve_step against the dense reference, once with the kernel solve_local picks and once under TEST_LM_SCHUR_ONE (k_lm_schur, one workgroup per landmark)."""
    P, locks, _ = LC.build(name)
    d_ref, m_ref = _step_refs(name, radius, scaling)
    R = LC.track_regime(P, locks)
    for switch, kernel in ((0, R["elim_kernel"]), (1, 2)):
        g = _ctx(name, TEST_LM_SCHUR_ONE=switch)
        g.evaluate(P["state0"], normal_eq=True, dense=False)
        d, m = g.solve_step(radius, scaling)
        lo = g.layout()
        e_d, e_m = np.abs(d - d_ref).max() / np.abs(d_ref).max(), abs(m - m_ref) / abs(m_ref)
        tag = "step%d" % kernel + ("" if switch == 0 else "s")
        _say(tag, "%s r=%g%s" % (name, radius, "" if scaling else " ns"), e_d); _say(tag + ".model", "%s r=%g%s" % (name, radius, "" if scaling else " ns"), e_m)
        assert lo["lm_elim_kernel"] == kernel and lo["solver_fallbacks"] == 0 and lo["exact_fallback"] == 0, lo
        if e_d > 1e-7:
            N = P["n_knots"]
            w = int(np.argmax(np.abs(d - d_ref)))
            print("LMTRACK worst step entry of %s: tangent %d (%s) device %.12e reference %.12e" % (name, w, "knot %d" % (w // 6) if w < 6 * N else "calibration" if w < 6 * N + 22 else "landmark %d" % (w - 6 * N - 22), d[w], d_ref[w]))
        assert e_d <= 1e-7 and e_m <= 1e-8
        g.close()


@pytest.mark.parametrize("name", LC.STEP_CASES)
def test_step_against_the_dense_solve(name):
    assert (LC.track_regime(*LC.build(name)[:2])["elim_kernel"] == 2) == (name == "long_track")         # long_track reports the per-landmark kernel without the switch
    _check_step(name, 3.0 if name in LC.STEP_SMALL_RADIUS_ONLY else 1e4, True)


@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("name", LC.STEP_SWEEP_CASES)
def test_step_radius_and_scaling(name, radius, scaling):
    _check_step(name, radius, scaling)


def test_no_landmark_elimination_reports_zero():
    """lm_elim_kernel = 0 when the landmarks are locked: nothing is eliminated."""
    P, locks, _ = LC.build("L_5")
    g = lvx.Context(0)
    lvx.load_problem(g, P, locks | lvx.LOCK_LANDMARKS)
    g.evaluate(P["state0"], normal_eq=True, dense=False)
    g.solve_step(1e4, True)
    assert g.layout()["lm_elim_kernel"] == 0
    g.close()


@pytest.mark.parametrize("name", LC.LOOP_CASES)
def test_lm_loop(name):
    """lvx_lm_solve (the in-place elimination) against oracle/lm.py; afterwards an evaluation on the same context equals a fresh context's: the fill the elimination writes across
    a landmark's whole reach is cleared."""
    P, locks, _ = LC.build(name)
    N, L = P["n_knots"], P["n_landmarks"]
    o, at = _oracle(name)
    free = lm.free_tangent_indices(N, L, locks)
    xo, so = lm.lm_solve(o, P["state0"], free, max_iterations=8, n_knots=N, n_landmarks=L)
    g = _ctx(name)
    xg, sg = g.lm_solve(P["state0"], max_iterations=8)
    print("LMTRACK loop %s: iterations %d / %d, termination %s / %s, accepted %s / %s" % (name, sg["iterations"], so["iterations"], sg["termination"], so["termination"], list(sg["accepted"]), list(so["accepted"])))
    assert sg["iterations"] == so["iterations"] and sg["termination"] == so["termination"]
    assert list(sg["accepted"]) == list(so["accepted"])
    e = np.abs(sg["cost_history"] - so["cost_history"]).max() / so["cost_history"].max()
    _say("loop.cost", name, e)
    assert e <= 1e-7
    lo = g.layout()
    assert lo["solver_fallbacks"] == 0 and lo["lm_elim_kernel"] == LC.track_regime(P, locks)["elim_kernel"]
    ra = g.evaluate(P["state0"], normal_eq=True)
    h = _ctx(name)
    rb = h.evaluate(P["state0"], normal_eq=True)
    _compare_eval("loop.after", name, ra, rb)
    _compare_eval("loop.oracle", name, ra, at("state0"))
    g.close(); h.close()
