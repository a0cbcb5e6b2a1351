"""GPU: the fused surfel kernel's MFMA windows against the FP64 oracle.  A window is the local column space of up to three consecutive knot intervals; the
three hub pseudo-position columns are no panel columns — their accumulator slots are rebuilt from the knot sums before the flush — so every case compares the
whole of H and g: row densities from one window per wave batch to one row per window, hand-placed row times (one interval, k / k + 3 which must split, k .. k + 2,
the spline's first and last interval, the hub's neighbours, a long empty run), row counts around lane / batch / chunk edges, Huber outliers (the rebuilt slots
come from scaled rows), the free and the locked non-zero LiDAR time offset, DETERMINISTIC (same bits twice) and the smallest / largest accumulator window.

Tolerances are those of tests/test_gpu_eval.py::_compare, relative to the oracle's magnitudes: residuals 1e-11 max|r|, cost 1e-12, H and g 1e-10 of their maxima,
and every H entry to 1e-9 of its own scale sqrt(H_ii H_jj).  Every comparison prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import lvx
import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TAU_LOCKS = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
DT = 0.02
K0 = 40            # an interval well inside the spline (about 100 intervals), away from the hub's


def _assert_blockscaled(Hg, Ho, tol=1e-9):
    """Every entry against ITS OWN scale sqrt(H_ii H_jj) (the Cauchy-Schwarz bound of |H_ij|)."""
    d = np.sqrt(np.maximum(np.diag(Ho), 0.0))
    scale = np.outer(d, d)
    bad = np.abs(Hg - Ho) > tol * scale + 1e-300
    assert not bad.any(), "worst entry-scaled error %.3e" % (np.abs(Hg - Ho)[bad] / np.maximum(scale[bad], 1e-300)).max()


def _base(n_surfel, seed=31):
    return synth.make_problem(seed=seed, duration=2.0, dt=DT, imu_rate=100.0, n_surfel=n_surfel, n_planes=12, n_landmarks=6, views_per_lm=4)


def _place(P, ks, seed=7):
    """Row i into knot interval ks[i], anywhere inside it — in the hub's interval behind t_map: the reference rejects a row before the map time ("time span out of
    range") — points and planes stay as generated."""
    u = np.random.default_rng(seed).uniform(0.05, 0.95, len(ks))
    u = np.where(np.asarray(ks) == _hub_interval(P), 0.55 + 0.4 * u, u)
    P["surf_t"] = np.sort(P["t0"] + (np.asarray(ks) + u) * P["dt"])
    return P


def _hub_interval(P):
    return int(np.floor((P["t_map"] - P["t0"]) / P["dt"]))


def _lidar_normals(P):
    """Unit plane normal of every surfel row in ITS LiDAR frame, from the oracle: the residual is w n . p + const in the LiDAR point."""
    o = O.Oracle()
    lvx.load_problem(o, P, TAU_LOCKS)
    r0 = o.evaluate(P["state_true"])["residuals"]
    cols = []
    for j in range(3):
        Q = dict(P); Q["surf_pt"] = P["surf_pt"].copy(); Q["surf_pt"][:, j] += 1.0
        o2 = O.Oracle()
        lvx.load_problem(o2, Q, TAU_LOCKS)
        cols.append(o2.evaluate(P["state_true"])["residuals"] - r0)
    d = np.stack(cols, axis=1)
    rows = np.flatnonzero(np.abs(d).max(axis=1) > 0)
    assert len(rows) == len(P["surf_t"])
    n = d[rows] / P["w_surf"]
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    return n


def _problem(name):
    """(P, locks, states) of a case."""
    kind, _, arg = name.partition(":")
    locks = TAU_LOCKS
    if kind == "density":
        P = _base(int(arg))
    elif kind == "placed":
        P = _base(600)
        n, last = 600, P["n_knots"] - 4
        i = np.arange(n)
        if arg == "one":
            ks = np.full(n, K0)
        elif arg == "k_k3":
            ks = np.where(i % 2 == 0, K0, K0 + 3)
        elif arg == "k_k1_k2":
            ks = K0 + i % 3
        elif arg == "ends":                                       # the first and the last interval a row may lie in: the hub's own (no row precedes t_map) and N - 4
            ks = np.where(i % 2 == 0, _hub_interval(P), last)
        elif arg == "hub_adjacent":                               # the hub's interval and its neighbour (the one before it admits no row)
            ks = _hub_interval(P) + i % 2
        elif arg == "gap":
            ks = np.where(i < n // 2, 20 + i % 10, 55 + i % 10)   # intervals 30 .. 54 stay empty
        else:
            raise KeyError(name)
        _place(P, ks)
    elif kind == "rows":
        n = int(arg)
        P = _place(_base(n), K0 + np.arange(n) % 3)
    elif kind == "huber":
        P = _base(2500)
        nL = _lidar_normals(P)
        out = np.arange(len(nL)) % 10 == 3
        P["surf_pt"] = P["surf_pt"] + np.where(out[:, None], 1.0, 0.0) * nL   # 1 m off the plane: |r| grows by w = 10 > the Huber width 5
    elif kind == "tau":
        P = _base(2500)
        locks = 0 if arg == "free" else TAU_LOCKS
    else:
        raise KeyError(name)
    states = [P["state0"].copy(), P["state_true"].copy()]
    if kind == "tau":
        for s in states:
            s[7 * P["n_knots"] + 16 + 7] = 3e-4 if arg == "free" else 8e-6
    return P, locks, states


@functools.lru_cache(maxsize=None)
def _case(name):
    """Problem, lock mask, the two states (perturbed start, ground truth) and the oracle's result at each: computed once per case and shared, never modified."""
    P, locks, states = _problem(name)
    o = O.Oracle()
    lvx.load_problem(o, P, locks)
    return P, locks, states, [o.evaluate(s, normal_eq=True) for s in states]


def _context(P, locks, **switches):
    g = lvx.Context(0)
    for k, v in switches.items():
        g.set_switch(k, v)
    lvx.load_problem(g, P, locks)
    return g


def _check(label, r, ro, g=None):
    d = np.sqrt(np.maximum(np.diag(ro["H"]), 0.0))
    sc = np.outer(d, d)
    dH = np.abs(r["H"] - ro["H"])
    fig = dict(cost=abs(r["cost"] - ro["cost"]) / abs(ro["cost"]), r=np.abs(r["residuals"] - ro["residuals"]).max() / np.abs(ro["residuals"]).max(),
               H=dH.max() / np.abs(ro["H"]).max(), Hblk=(dH[sc > 0] / sc[sc > 0]).max(), g=np.abs(r["g"] - ro["g"]).max() / np.abs(ro["g"]).max())
    lo = g.layout() if g is not None else {"exact_fallback": -1, "fallback_rows": -1}
    print("SURFEL_WINDOWS %s: cost %.2e r %.2e H %.2e H_blockscaled %.2e g %.2e exact_fallback %d fallback_rows %d"
          % (label, fig["cost"], fig["r"], fig["H"], fig["Hblk"], fig["g"], lo["exact_fallback"], lo["fallback_rows"]))
    assert r["residuals"].shape == ro["residuals"].shape
    assert fig["r"] <= 1e-11
    assert fig["cost"] <= 1e-12
    assert fig["H"] <= 1e-10
    assert fig["g"] <= 1e-10
    _assert_blockscaled(r["H"], ro["H"])


def _run(name, **switches):
    P, locks, states, ref = _case(name)
    g = _context(P, locks, **switches)
    out = []
    for tag, s, ro in zip(("state0", "state_true"), states, ref):
        r = g.evaluate(s, normal_eq=True)
        _check("%s %s %s" % (name, switches or "", tag), r, ro, g)
        out.append(r)
    g.close()
    return out


@pytest.mark.parametrize("n_surfel", [8000, 4000, 2500, 600, 100])
def test_row_density(n_surfel):
    """About 80, 40, 25, 6 and 1 rows per interval: a wave batch of 64 sorted rows spans 1, 2, 3 (one window each), about 10 (several windows) or 64 intervals
    (one row per window)."""
    _run("density:%d" % n_surfel)


@pytest.mark.parametrize("layout", ["one", "k_k3", "k_k1_k2", "ends", "hub_adjacent", "gap"])
def test_hand_placed_times(layout):
    _run("placed:" + layout)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 513])
def test_row_counts(n):
    """n rows in three consecutive intervals: the last lane, wave batch and chunk hold one row or miss one."""
    _run("rows:%d" % n)


def test_huber_outliers():
    """Every tenth point 1 m off its plane: scale != 1 on those rows, so the rebuilt slots must come from the scaled rows."""
    _run("huber:")


@pytest.mark.parametrize("mode", ["free", "locked_nonzero"])
def test_lidar_time_offset(mode):
    """Lock mask 0: the free-offset instantiation (one more panel column); a locked non-zero offset moves rows across interval edges."""
    _run("tau:" + mode)


def test_deterministic_is_bit_reproducible():
    P, locks, states, ref = _case("density:4000")
    default = _run("density:4000")
    g = _context(P, locks, DETERMINISTIC=1)
    for tag, s, ro, rd in zip(("state0", "state_true"), states, ref, default):
        a = g.evaluate(s, normal_eq=True)
        b = g.evaluate(s, normal_eq=True)
        assert a["cost"] == b["cost"]
        assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"])
        _check("deterministic vs oracle " + tag, a, ro, g)
        _check("deterministic vs default path " + tag, a, rd)
    g.close()


@pytest.mark.parametrize("chunk_r", [8, 16])
def test_chunk_size(chunk_r):
    """The smallest and the largest accumulator window, at about 40 rows per interval."""
    _run("density:4000", CHUNK_R=chunk_r)
