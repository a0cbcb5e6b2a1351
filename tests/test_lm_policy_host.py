"""The LM loop's decisions without a GPU: lvi-exc_amd/csrc/lvx_lm_policy.h — the trust-region schedule and the projected Armijo line search lvx_lm_solve_shared decides
with — built here with g++ (tests/native/lm_policy_host_check.cpp, no library load) and held against oracle/lm.py decision by decision.
(a) ArmijoSearch / poly_fit against projected_line_search / interpolating_polynomial on scalar functions phi(alpha) whose minimum lies far inside (0, 1).
(b) TrustRegion against lm_solve: a small dense LM of this file's own takes every step from oracle.lm.solve_step and every decision from the header.
Bars: counts, outcomes, terminations and accepted flags exact; trial steps 1e-7 relative (sqrt(eps) = 1.5e-8, the conditioning of a polynomial's minimiser, with a
margin of 7: both sides do the same operations but for numpy's dot product in the back substitution; seen here: 1.2e-8 at most, zero in most cases); radius histories 4 ulp
(seen: 0); fitted polynomials 1e-12 of the largest sample."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lvx
from oracle import lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(max_iterations=50, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, jacobi_scaling=1, verbose=0)   # lvx_lm_default_options
VERDICT = ["parameter_tolerance", "function_tolerance", "accept", "reject"]


@pytest.fixture(scope="module")
def lp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lm_policy") / "lm_policy_host_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "native", "lm_policy_host_check.cpp"), "-o", so])
    l = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    l.lp_poly_fit.argtypes = [C.c_int, dp, dp, dp, ip, dp]
    l.lp_search_needed.argtypes = [C.c_double] * 3
    l.lp_search_new.argtypes = [C.c_double] * 5; l.lp_search_new.restype = C.c_void_p
    l.lp_search_next.argtypes = [C.c_void_p, dp]
    l.lp_search_report.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
    l.lp_search_trials.argtypes = [C.c_void_p]
    l.lp_search_free.argtypes = [C.c_void_p]; l.lp_search_free.restype = None
    l.lp_tr_new.argtypes = [C.POINTER(lvx.LmOptions)]; l.lp_tr_new.restype = C.c_void_p
    l.lp_tr_radius.argtypes = [C.c_void_p]; l.lp_tr_radius.restype = C.c_double
    l.lp_tr_step_valid.argtypes = [C.c_int, C.c_double]
    l.lp_tr_invalid.argtypes = [C.c_void_p]
    l.lp_tr_classify.argtypes = [C.c_void_p] + [C.c_double] * 5 + [dp]
    l.lp_tr_accepted.argtypes = [C.c_void_p, C.c_double]; l.lp_tr_accepted.restype = None
    l.lp_tr_rejected.argtypes = [C.c_void_p]
    l.lp_tr_free.argtypes = [C.c_void_p]; l.lp_tr_free.restype = None
    return l


def test_constants_restate_the_oracles_defaults(lp):
    d, i = (C.c_double * 4)(), (C.c_int32 * 2)()
    lp.lp_constants(d, i)
    kw = {k: v.default for k, v in inspect.signature(lm.projected_line_search).parameters.items()}
    assert list(d) == [kw["sufficient_decrease"], kw["max_contraction"], kw["min_contraction"], kw["min_step"]] == [1e-4, 1e-3, 0.6, 1e-9]
    assert list(i) == [kw["max_trials"], 5] == [20, 5]


# ---- (a) the line search ----
def quartic(a):
    t = a - 0.3
    return t ** 4 + 0.1 * t * t, 4 * t ** 3 + 0.2 * t


def expmin(k, m):
    """exp(k a) - k exp(k m) a: the minimum at a = m, the slope at 1 of order k exp(k)."""
    c = k * np.exp(k * m)
    return lambda a: (np.exp(k * a) - c * a, k * np.exp(k * a) - c)


def never(a):
    """rises by a where the linear prediction (g0 = -1, given beside it) promises a decrease of a: Armijo fails at every step"""
    return a, 1.0


def walled(lo, hi):
    return lambda a: (np.inf, 0.0) if lo < a < hi else quartic(a)


# name: (phi, g0 or None: phi'(0), dinf, trials the oracle evaluates, outcome: the index of the trial that passes or None)
LS_CASES = {
    "quartic": (quartic, None, 1.0, 1, 1),
    "exp_0.3": (expmin(10, 0.3), None, 1.0, 2, 2),
    "exp_0.1_third_trial_passes": (expmin(25, 0.1), None, 1.0, 3, 3),
    "exp_0.05": (expmin(50, 0.05), None, 1.0, 4, 4),
    "exp_0.002": (expmin(300, 0.002), None, 1.0, 8, 8),
    "trial_returns_inf": (walled(0.25, 1.0), None, 1.0, 2, 2),            # the first trial (0.454) cannot be evaluated: the second contracts from it without a new sample
    "gives_up_under_1e-9": (expmin(300, 0.002), None, 1e-7, 6, None),     # the seventh step (5.4e-3) x dinf < 1e-9
    "never_passes_gives_up": (never, -1.0, 1.0, 10, None),
    # all twenty: every trial contracts by at least 0.6, so the twentieth step is at most 0.6^20 = 3.7e-5 (here 1.2e-18); the give-up (step x dinf < 1e-9) stays out
    # of the way only with a LARGE dinf
    "spends_all_twenty": (never, -1.0, 1e12, 20, None),
}


def run_oracle(phi, g0, dinf):
    steps = []
    f0, d0 = phi(0.0)
    f1, d1 = phi(1.0)

    def ev(a):
        steps.append(a)
        return phi(a)
    a, fa, trials = lm.projected_line_search(ev, f0, d0 if g0 is None else g0, f1, d1, direction_max_norm=dinf)
    return steps, a, fa, trials


def run_header(lp, phi, g0, dinf):
    f0, d0 = phi(0.0)
    f1, d1 = phi(1.0)
    d0 = d0 if g0 is None else g0
    if not lp.lp_search_needed(f0, f1, d0):
        return [], 1.0, f1, 0
    s = lp.lp_search_new(f0, d0, f1, d1, dinf)
    steps, a, out = [], C.c_double(0.0), (1.0, f1)
    while lp.lp_search_next(s, C.byref(a)):
        steps.append(a.value)
        f, df = phi(a.value)
        if lp.lp_search_report(s, f, df, int(not np.isfinite(f))):
            out = (a.value, f)
            break
    trials = lp.lp_search_trials(s)
    lp.lp_search_free(s)
    return steps, out[0], out[1], trials


@pytest.mark.parametrize("name", list(LS_CASES))
def test_line_search_follows_the_oracle(lp, name):
    phi, g0, dinf, n_eval, passes = LS_CASES[name]
    so, ao, fo, to = run_oracle(phi, g0, dinf)
    sh, ah, fh, th = run_header(lp, phi, g0, dinf)
    assert len(so) == n_eval and (to == passes if passes else (ao == 1.0 and to == 20)), (so, ao, to)   # the case reaches the branch it is named for
    if name == "trial_returns_inf":
        assert not np.isfinite(phi(so[0])[0]) and 1e-3 * so[0] <= so[1] <= 0.6 * so[0]
    if name.startswith("gives_up") or name.startswith("never"):
        assert len(so) < 20 and so[-1] * dinf >= 1e-9 and 0.6 * so[-1] * dinf < 1e-7   # not out of trials: the next step fell under the bar
    assert len(sh) == len(so)
    assert (ah == 1.0) == (ao == 1.0) and (th == to if passes else ah == 1.0 and fh == fo)
    rel = max([abs(x / y - 1) for x, y in zip(sh + [ah], so + [ao])])
    print("%s: %d trials, max relative step difference %.3e" % (name, len(so), rel))
    assert rel <= 1e-7
    assert fh == (phi(ah)[0] if passes else fo)


def test_full_step_is_kept_when_it_satisfies_armijo_or_cannot_be_judged(lp):
    """the entry condition, against projected_line_search's own first line: g0 >= 0, a candidate that is not finite, a sufficient decrease"""
    for f0, g0, f1 in [(1.0, -1.0, 0.5), (1.0, -1.0, 1.0 - 1e-4), (1.0, -1.0, 1.0 - 0.99e-4), (1.0, 0.0, 2.0), (1.0, 1.0, 2.0), (1.0, -1.0, np.inf), (1.0, -1.0, np.nan), (1.0, -1.0, 2.0)]:
        calls = []
        lm.projected_line_search(lambda a: (calls.append(a), (np.inf, 0.0))[1], f0, g0, f1, 0.0)
        assert bool(lp.lp_search_needed(f0, f1, g0)) == bool(calls), (f0, g0, f1)


@pytest.mark.parametrize("n", [2, 3])
def test_poly_fit_against_interpolating_polynomial(lp, n):
    """the samples of a search: (0, f0, g0) and one or two trials with their derivatives -> a cubic / a quintic through values and slopes"""
    worst = 0.0
    for phi, xs in [(quartic, [0.0, 0.27, 1.0]), (expmin(10, 0.3), [0.0, 0.6, 1.0]), (expmin(50, 0.05), [0.0, 0.1243, 0.2686]), (expmin(300, 0.002), [0.0, 0.005351, 0.01228])]:
        xs = [xs[0], xs[2]] if n == 2 else xs
        smp = [(x,) + tuple(float(v) for v in phi(x)) for x in xs]
        co = lm.interpolating_polynomial(smp)
        x, f, df = (np.array([s[k] for s in smp]) for k in range(3))
        out, has = np.zeros(2 * n), np.ones(n, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        assert lp.lp_poly_fit(n, x.ctypes.data_as(dp), f.ctypes.data_as(dp), df.ctypes.data_as(dp), has.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(dp)) == 2 * n == len(co)
        bar = 1e-12 * np.abs(f).max()
        for c in (out, co):
            assert np.abs(np.polyval(c, x) - f).max() <= bar, (np.polyval(c, x), f)
        worst = max(worst, np.abs(np.polyval(out, x) - np.polyval(co, x)).max() / np.abs(f).max())
        assert np.abs(np.polyval(out, x) - np.polyval(co, x)).max() <= bar
    print("%d samples: max difference of the fitted values / largest sample %.3e" % (n, worst))


# ---- (b) the schedule ----
class Fake:
    """a two-variable least-squares problem with the oracle's interface: evaluate(x, normal_eq) -> cost, H = J^T J, g = J^T r; plus"""
    tangent_size = 2

    def __init__(self, kind):
        self.kind = kind

    def res(self, x):
        if self.kind == "rosenbrock":
            return np.array([10.0 * (x[1] - x[0] ** 2), 1.0 - x[0]]), np.array([[-20.0 * x[0], 10.0], [-1.0, 0.0]])
        if self.kind == "powell":   # singular at the solution
            d = 2 * np.sqrt(5.0) * (x[0] - x[1])
            return np.array([x[0] + 10 * x[1], np.sqrt(5.0) * (x[0] - x[1]) ** 2]), np.array([[1.0, 10.0], [d, -d]])
        e0, e1 = np.exp(x[0]), np.exp(x[0] * x[1])
        return np.array([e0 - 2.0, e1 - 3.0, 0.1 * x[1]]), np.array([[e0, 0.0], [x[1] * e1, x[0] * e1], [0.0, 0.1]])

    def evaluate(self, x, normal_eq=False):
        with np.errstate(over="ignore", invalid="ignore"):
            r, J = self.res(x)
        if not np.all(np.isfinite(r)):
            raise ValueError("range")
        return {"cost": 0.5 * float(r @ r), "H": J.T @ J, "g": J.T @ r}

    def plus(self, x, d):
        return x + d


def policy_lm(lp, fake, x0, **kw):
    """lm_solve's loop with solve_step for the step and the header's TrustRegion for every decision"""
    opt = lvx.LmOptions(**dict(DEFAULTS, **kw))
    tr = lp.lp_tr_new(C.byref(opt))
    free = np.arange(2)
    x = np.array(x0, dtype=np.float64)
    ev = fake.evaluate(x, normal_eq=True)
    cost, H, g = ev["cost"], ev["H"], ev["g"]
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
    lm_diag, it, term = None, 0, None
    hist = {"radius": [], "accepted": []}

    def record(flag):
        hist["radius"].append(lp.lp_tr_radius(tr)); hist["accepted"].append(flag)
    if np.abs(g).max() <= opt.gradient_tolerance:
        term = "gradient_tolerance"
    while term is None:
        if it >= opt.max_iterations:
            term = "max_iterations"
            break
        it += 1
        try:
            delta, model, lm_diag = lm.solve_step(H, g, free, lp.lp_tr_radius(tr), scale, lm_diag)
            notpd = False
        except np.linalg.LinAlgError:
            notpd, model = True, 0.0
        if not lp.lp_tr_step_valid(int(notpd), model):
            if not lp.lp_tr_invalid(tr):
                term = "failure"
                break
            record(-1)
            continue
        xc = fake.plus(x, delta)
        try:
            cand = fake.evaluate(xc)["cost"]
        except ValueError:
            cand = np.inf
        rho = C.c_double(0.0)
        v = VERDICT[lp.lp_tr_classify(tr, cost, cand, model, np.linalg.norm(xc - x), np.linalg.norm(x), C.byref(rho))]
        if v in ("parameter_tolerance", "function_tolerance"):
            term = v
            record(0)
        elif v == "accept":
            x = xc
            ev = fake.evaluate(x, normal_eq=True)
            cost, H, g = ev["cost"], ev["H"], ev["g"]
            lm_diag = None
            lp.lp_tr_accepted(tr, rho.value)
            record(1)
            if np.abs(g).max() <= opt.gradient_tolerance:
                term = "gradient_tolerance"
        else:
            alive = lp.lp_tr_rejected(tr)
            record(0)
            if not alive:
                term = "min_trust_region_radius"
    lp.lp_tr_free(tr)
    return x, dict(termination=term, iterations=it, radius_history=np.array(hist["radius"]), accepted=np.array(hist["accepted"]))


# name: (problem, start, options, what the oracle's run must show: the case reaches the branch it is named for)
def _rosenbrock(s):
    return s["termination"] == "parameter_tolerance" and s["iterations"] == 36 and list(s["accepted"][:3]) == [0, 0, 0] and list(s["radius_history"][:3]) == [5e3, 1.25e3, 156.25] and 0 in s["accepted"][4:] and 1 in s["accepted"]


SCHEDULE_CASES = {
    "rosenbrock_rejections_then_mixed": ("rosenbrock", (-1.2, 1.0), {}, _rosenbrock),
    "rosenbrock_min_radius": ("rosenbrock", (-1.2, 1.0), dict(min_radius=1e3), lambda s: s["termination"] == "min_trust_region_radius" and s["iterations"] == 3),
    "rosenbrock_max_iterations_on_an_accept": ("rosenbrock", (-1.2, 1.0), dict(max_iterations=4), lambda s: s["termination"] == "max_iterations" and s["iterations"] == 4 and s["accepted"][-1] == 1),
    "powell_radius_times_three": ("powell", (3.0, -1.0), {}, lambda s: list(s["accepted"]) == [1] * 15 and np.allclose(s["radius_history"][1:] / s["radius_history"][:-1], 3.0, rtol=1e-12, atol=0)),
    "powell_max_radius_clamps": ("powell", (3.0, -1.0), dict(max_radius=1e6), lambda s: (s["accepted"] == 1).all() and s["radius_history"][3] == 8.1e5 and (s["radius_history"][4:] == 1e6).all()),
    "exp_function_tolerance": ("exp", (3.0, 2.0), {}, lambda s: s["termination"] == "function_tolerance" and s["iterations"] == 9),
}


@pytest.mark.parametrize("name", list(SCHEDULE_CASES))
def test_schedule_follows_the_oracle(lp, name):
    kind, x0, kw, reaches = SCHEDULE_CASES[name]
    xo, so = lm.lm_solve(Fake(kind), np.array(x0), np.arange(2), mask=np.ones(2, bool), constrained=[], **kw)
    assert reaches(so), (so["termination"], so["iterations"], list(so["accepted"]), list(so["radius_history"]))
    xh, sh = policy_lm(lp, Fake(kind), x0, **kw)
    assert (sh["termination"], sh["iterations"]) == (so["termination"], so["iterations"])
    assert list(sh["accepted"]) == list(so["accepted"])
    ulp = np.abs(sh["radius_history"] - so["radius_history"]) / np.spacing(so["radius_history"])
    print("%s: %s after %d, radius history within %.1f ulp" % (name, so["termination"], so["iterations"], ulp.max(initial=0.0)))
    assert ulp.max(initial=0.0) <= 4
    assert np.array_equal(xh, xo)   # same steps, same decisions: the same iterate


def test_five_invalid_steps_in_a_row_fail_and_a_valid_one_resets_the_count(lp):
    """oracle/lm.py:206-214: the radius is halved four times, the fifth invalid step fails the solve (and leaves the radius alone)"""
    opt = lvx.LmOptions(**DEFAULTS)
    tr = lp.lp_tr_new(C.byref(opt))
    for k in range(1, 5):
        assert lp.lp_tr_invalid(tr) == 1 and lp.lp_tr_radius(tr) == 1e4 * 0.5 ** k
    assert lp.lp_tr_invalid(tr) == 0 and lp.lp_tr_radius(tr) == 625.0
    lp.lp_tr_free(tr)
    tr = lp.lp_tr_new(C.byref(opt))
    rho = C.c_double(0.0)
    for k in range(4):
        assert lp.lp_tr_invalid(tr) == 1
    assert VERDICT[lp.lp_tr_classify(tr, 2.0, 1.0, 1.0, 1.0, 1.0, C.byref(rho))] == "accept" and rho.value == 1.0   # a valid step in between
    for k in range(4):
        assert lp.lp_tr_invalid(tr) == 1
    assert lp.lp_tr_invalid(tr) == 0 and lp.lp_tr_radius(tr) == 1e4 * 0.5 ** 8
    lp.lp_tr_free(tr)
    # what makes a step invalid: a failed factorisation, a model change that is not finite, or not positive
    assert [lp.lp_tr_step_valid(*a) for a in [(0, 1.0), (1, 1.0), (0, 0.0), (0, -1.0), (0, np.inf), (0, np.nan)]] == [1, 0, 0, 0, 0, 0]
