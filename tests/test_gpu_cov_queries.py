"""The three covariance queries on the selected inverse (lvx_trajectory_covariance, lvx_landmark_covariance, lvx_map_point_covariance) as neighbours: their host forms
stage inputs and outputs through ONE device buffer and ONE pinned mirror of the context, laid out per call from the arrays the caller asks for.  What the per-query
files (test_gpu_trajcov.py, test_gpu_landmark_cov.py, test_gpu_ptcov.py) do not cross-check:
  1. calls of the three interleaved on one context, the staged sizes growing and shrinking: every result is the bits of the same call on a fresh context;
  2. every subset {valid} and {valid, one array} of the outputs, through ctypes (the Python methods always ask for most arrays): an array that is asked for holds the
     bits of the all-outputs call, an array that is not asked for is a NULL pointer and the call returns all the same.
Problem, times, points and directions are test_gpu_ptcov.py's (calib_cov_cases.SMALL: 44 knots, 12 landmarks, surfel rows that set t_map)."""
import ctypes as C

import numpy as np
import pytest

import calib_cov_cases as CC
import lvx
import test_gpu_ptcov as TP

pytestmark = pytest.mark.gpu
RADIUS = 1e4


def _evaluated():
    P = TP._problem()
    g = TP._context(P, CC.SOLVE2, (("DETERMINISTIC", 1),))   # two contexts hold the same bits of the normal equations only without the assembly's atomics
    g.evaluate(P["state0"], normal_eq=True, dense=False, residuals=False)
    return g


def test_interleaved_calls_are_the_calls_on_a_fresh_context():
    P = TP._problem()
    t, pts, dirs = TP._times(P, 257), TP._points(257), TP._dirs(257)   # 257: one past a 256-point workgroup
    calls = [lambda g: g.trajectory_covariance(t[:3], lvx.FRAME_LIDAR, RADIUS, window=True),
             lambda g: g.landmark_covariance(RADIUS),
             lambda g: g.map_point_covariance(pts, t, dirs, RADIUS, window=True),
             lambda g: g.trajectory_covariance(t[:1], lvx.FRAME_LIDAR, RADIUS, window=True),
             lambda g: g.map_point_covariance(pts[:1], t[:1], dirs[:1], RADIUS, window=True),
             lambda g: g.landmark_covariance(RADIUS, ids=[7, 2])]
    g = _evaluated()
    got = [call(g) for call in calls]
    ck = g.normal_eq_checksum()
    g.close()
    assert len(got[1]["valid"]) == P["n_landmarks"] and all(r["valid"].all() for r in got)
    for k, call in enumerate(calls):
        f = _evaluated()
        want = call(f)
        assert f.normal_eq_checksum() == ck
        f.close()
        assert set(want) == set(got[k])
        for key in want:
            assert np.array_equal(got[k][key], want[key]), (k, key)


def _options(g, cls, default_fn):
    opt = cls()
    assert getattr(g._l, default_fn)(C.byref(opt)) == lvx.OK
    opt.radius = RADIUS
    return opt


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# form -> (record class, its arrays before `valid` as (name, entries per query, dtype), the call: (g, n, record) -> return code)
def _forms(P):
    n = 5
    t, pts, dirs = TP._times(P, n), TP._points(n), TP._dirs(n)
    ids = np.array([7, 2, 11, 0, 2], np.int32)

    def traj(g, rec):
        opt = _options(g, lvx.TrajCovOptions, "lvx_traj_cov_default_options")
        return g._l.lvx_trajectory_covariance(g._h, C.byref(opt), C.c_int(lvx.FRAME_LIDAR), C.c_int(n), _ptr(t), C.byref(rec))

    def landmark(g, rec):
        opt = _options(g, lvx.LandmarkCovOptions, "lvx_landmark_cov_default_options")
        return g._l.lvx_landmark_covariance(g._h, C.byref(opt), C.c_int(n), _ptr(ids), C.byref(rec))

    def point(g, rec, d=dirs):
        opt = _options(g, lvx.PointCovOptions, "lvx_point_cov_default_options")
        return g._l.lvx_map_point_covariance(g._h, C.byref(opt), C.c_int(n), _ptr(pts), _ptr(t), _ptr(d), C.byref(rec))
    f8, i4 = np.float64, np.int32
    return n, {"trajectory": (lvx.TrajCov, [("cov", 36, f8), ("sigma", 6, f8), ("window_cov", 31 * 31, f8), ("window_idx", 31, i4)], traj),
               "landmark": (lvx.LandmarkCov, [("var_rho", 1, f8), ("sigma_rho", 1, f8), ("point", 3, f8), ("point_cov", 9, f8), ("window_cov", 32 * 32, f8), ("window_idx", 32, i4)],
                            landmark),
               "point": (lvx.PointCov, [("point", 3, f8), ("cov", 9, f8), ("sigma", 3, f8), ("sigma_max", 1, f8), ("var_dir", 1, f8), ("window_cov", 55 * 55, f8),
                                        ("window_idx", 55, i4)], point)}


def _ask(g, n, rec_cls, arrays, call, names, **kw):
    """one call that asks for `names` and valid; every array starts at 7"""
    out = {name: np.full((n, w), 7, dt) for name, w, dt in arrays if name in names}
    valid = np.full(n, 7, np.uint8)
    rec = rec_cls(*[out[name].ctypes.data if name in out else None for name, _, _ in arrays], valid.ctypes.data)
    assert call(g, rec, **kw) == lvx.OK
    out["valid"] = valid
    return out


@pytest.mark.parametrize("form", ["trajectory", "landmark", "point"])
def test_every_subset_of_the_outputs_holds_the_bits_of_the_full_call(form):
    P = TP._problem()
    n, forms = _forms(P)
    rec_cls, arrays, call = forms[form]
    names = [a[0] for a in arrays]
    g = _evaluated()
    full = _ask(g, n, rec_cls, arrays, call, names)
    assert (full["valid"] == 1).all()
    for name, _, _ in arrays:
        assert not (full[name] == 7).all(), name
    for asked in [[]] + [[name] for name in names]:
        r = _ask(g, n, rec_cls, arrays, call, asked)
        for key in r:
            assert np.array_equal(r[key], full[key]), (form, asked, key)
    if form == "point":
        r = _ask(g, n, rec_cls, arrays, call, ["cov", "sigma_max"])   # directions given, their variances not asked for
        assert np.array_equal(r["cov"], full["cov"]) and np.array_equal(r["sigma_max"], full["sigma_max"]) and np.array_equal(r["valid"], full["valid"])
        r = _ask(g, n, rec_cls, arrays, call, ["cov", "var_dir"], d=None)   # the reverse: without directions var_dir is not written
        assert (r["var_dir"] == 7).all() and np.array_equal(r["cov"], full["cov"]) and np.array_equal(r["valid"], full["valid"])
    g.close()
