"""Rotation initialisation without a GPU: the C ABI exports the calls, refuses a NULL context and has the struct sizes of include/lvx.h; the header the kernels run
(lvi-exc_amd/csrc/lvx_rotinit.h, built here with g++ -O2 -ffp-contract=off: tests/native/rotinit_host_check.cpp) against a numpy restatement of
InertialInitializer::EstimateRotation (tests/rotinit_cases.py) on odometry with a planted mounting rotation of 2.7 rad.
Bars (rotinit_cases.py): eigenvalues 1e-12 lambda_max absolute, quaternion angle 2e-12 lambda_max / (lambda[2] - lambda[3]) rad; counts, ok and first_ok exact."""
import ctypes as C

import numpy as np
import pytest

import lvx
import synth
import rotinit_cases as rc
import traj_cases as tc


def test_library_exports_the_calls_and_struct_sizes():
    l = lvx.lib()
    for name in ("lvx_rotinit_default_options", "lvx_estimate_rotation", "lvx_estimate_rotation_d"):
        assert hasattr(l, name), name
    assert C.sizeof(lvx.RotInitOptions) == 24 and C.sizeof(lvx.RotInitResult) == 80 and lvx.ROTINIT_DTYPE.itemsize == 80
    o = lvx.default_rotinit_options()
    assert (o.huber_deg, o.min_pairs, o.reserved, o.min_sigma) == (1.0, 15, 0, 0.25)
    assert l.lvx_rotinit_default_options(None) == lvx.E_ARG
    r, f = lvx.RotInitResult(), C.c_int32(0)
    assert l.lvx_estimate_rotation(None, None, C.c_int(1), None, None, C.c_int(0), None, C.c_int(0), None, None, C.byref(r), C.byref(f)) == lvx.E_ARG
    assert l.lvx_estimate_rotation_d(None, None, C.c_int(1), None, None, C.c_int(0), None, C.c_int(0), None, None, C.byref(r), C.byref(f)) == lvx.E_ARG
    so, sr = C.c_int(0), C.c_int(0)
    rc.host_lib().rh_sizes(C.byref(so), C.byref(sr))
    assert (so.value, sr.value) == (24, 80)


def _host(name):
    c = rc.cases()[name]
    res, first, st = rc.host_estimate(c["P"], c["state"], c["t"], c["q"], c["prefix_len"], c["tau"], c["opt"])
    assert st == 0
    return c, res, first


@pytest.mark.parametrize("name", ["n3_on", "n3_off", "n17_on", "n17_off", "n65_on", "n65_off", "n257_off"])
def test_poses_on_and_off_the_knots(name):
    """3, 17, 65 and 257 poses: the whole list as one prefix.  3 poses are fewer than 15 pairs: ok = 0, identity, zero sigmas.  From 17 poses on the quaternion is the
    planted one: exact odometry leaves lambda[3] = 0."""
    c, res, first = _host(name)
    rc.check_case(name, res, first)
    n = len(c["t"])
    assert res[0, 0]["n_poses"] == n and res[0, 0]["n_pairs"] == (n - 1 if n > 3 else 2) and res[0, 0]["n_skipped"] == 0
    if n > 3:
        want = synth.qconj(rc.Q_LTOI)
        want = want if want[3] >= 0 else -want
        d = np.linalg.norm(res[0, 0]["q_ItoS_xyzw"] - want)
        print("distance to conj(q_LtoI): %.3e" % d)
        assert d <= 2e-12 * rc.gap_ratio(rc.reference(name)[0][0])   # the convention: x = q_ItoS = conj(q_LtoI)


def test_prefixes_cross_the_singular_value_test():
    """6 s at 10 Hz: the restatement's sigma[2] stays below 0.25 up to 24 poses and is above it from 36 on, each at least 0.05 away; first_ok is the fifth prefix.  A prefix
    of 1 and one of fewer than 15 pairs come first."""
    c, res, first = _host("prefixes")
    refs = rc.reference("prefixes")[0]
    s2 = np.array([r["sigma"][2] for r in refs])
    print("restatement sigma[2] per prefix:", s2)
    assert [r["ok"] for r in refs] == [0, 0, 0, 0, 1, 1, 1] and [r["n_pairs"] for r in refs] == [0, 15, 19, 23, 35, 39, 59]
    assert (np.abs(s2[1:] - 0.25) >= 0.05).all()
    rc.check_case("prefixes", res, first)
    assert first[0] == 4 and list(res[0]["ok"]) == [0, 0, 0, 0, 1, 1, 1] and list(res[0]["n_poses"]) == rc.LONG_PREFIXES


def test_short_prefixes_and_bad_lists():
    """Prefixes of 1, 2, 15 (14 pairs: below min_pairs), 16 (15 pairs: solved), a repeated entry; a decreasing list, an entry of 0 and one above n are refused."""
    c, res, first = _host("prefixes_short")
    rc.check_case("prefixes_short", res, first)
    assert list(res[0]["n_pairs"]) == [0, 1, 14, 15, 32, 64, 64] and not res[0]["sigma"][:3].any() and res[0]["sigma"][3:, 0].all()
    assert res[0, 5].tobytes() == res[0, 6].tobytes()
    for bad in ([20, 10], [0, 10], [10, 66]):
        assert rc.host_estimate(c["P"], c["state"], c["t"], c["q"], bad)[2] == -1


def test_tail_breaks_the_list_and_early_stamps_are_skipped():
    """Two stamps before MinTime, 65 inside, then MaxTime, MaxTime + 0.3, a stamp in the middle of the range and NaN.  The pairs (0, 1) and (1, 2) are skipped and counted;
    the pair that ends at MaxTime ends the list: no prefix gains a pair behind it, not even the in-range stamp."""
    c, res, first = _host("tail")
    rc.check_case("tail", res, first)
    assert list(res[0]["n_pairs"]) == [0, 17, 64, 64, 64, 64, 64] and list(res[0]["n_skipped"]) == [2] * 7
    for k in range(3, 7):
        assert res[0, k]["sigma"].tobytes() == res[0, 2]["sigma"].tobytes() and res[0, k]["q_ItoS_xyzw"].tobytes() == res[0, 2]["q_ItoS_xyzw"].tobytes()


@pytest.mark.parametrize("name,weight", [("huber", 1.0 / 3.0), ("huber_half", 0.5 / 3.0)])
def test_huber_weight_of_a_planted_step(name, weight):
    """One odometry step turned 3 degrees further about its own axis: the restatement weights that pair huber_deg / 3 and every other pair 1."""
    c, res, first = _host(name)
    w = rc.reference(name)[0][0]["weights"]
    assert abs(w[29] - weight) < 1e-9 and (np.delete(w, 29) == 1.0).all()
    rc.check_case(name, res, first)
    clean = rc.reference("n65_off")[0][0]
    assert res[0, 0]["sigma"][3] > 1e-3 > clean["sigma"][3]   # the outlier shows in the smallest singular value


def test_signs_and_norms_of_the_input_do_not_matter():
    c, res, first = _host("sign_scale")
    rc.check_case("sign_scale", res, first)
    plain = _host("n65_off")[1]
    assert res[0, 0]["q_ItoS_xyzw"][3] >= 0
    print("against the unscaled input: max |d sigma^2| = %.3e" % np.abs(res[0, 0]["sigma"] ** 2 - plain[0, 0]["sigma"] ** 2).max())
    rc.check_refs(res, first, rc.reference("n65_off"), "sign_scale vs plain reference")


def test_shift_sweep_finds_the_planted_offset():
    """Odometry whose poses belong to the spline 30 ms after their stamps, shifts -60 .. +60 ms in 10 ms steps, prefixes of 20 and 41 poses: every record against the
    restatement; sigma[3] is smallest at +30 ms and strictly larger at both neighbours — asserted on the restatement first, then on the result."""
    c, res, first = _host("shifts")
    refs = rc.reference("shifts")
    k = int(np.flatnonzero(c["tau"] == rc.SHIFT_TRUE)[0])
    for b in range(2):
        s3 = np.array([row[b]["sigma"][3] for row in refs])
        print("restatement sigma[3] over the shifts, prefix %d:" % b, s3)
        assert np.argmin(s3) == k and s3[k - 1] > 100 * s3[k] and s3[k + 1] > 100 * s3[k]
    rc.check_case("shifts", res, first)
    for b in range(2):
        g3 = res[:, b]["sigma"][:, 3]
        print("header sigma[3] over the shifts, prefix %d:" % b, g3)
        assert np.argmin(g3) == k and g3[k - 1] > 100 * g3[k] and g3[k + 1] > 100 * g3[k]


def test_eigen_solver_on_hard_spectra():
    """rot_eigen4 alone against numpy.linalg.eigh: a random matrix, a rank-1 one, two equal eigenvalues, a diagonal one, zeros."""
    rng = np.random.default_rng(3)
    B = rng.standard_normal((9, 4))
    v = rng.standard_normal(4)
    Q = np.linalg.qr(rng.standard_normal((4, 4)))[0]
    mats = [B.T @ B, np.outer(v, v), Q @ np.diag([3.0, 1.0, 1.0, 0.0]) @ Q.T, np.diag([1.0, 4.0, 2.0, 3.0]), np.zeros((4, 4))]
    for M in mats:
        s10 = np.ascontiguousarray(M[np.triu_indices(4)])
        lam, V = np.zeros(4), np.zeros((4, 4))
        rc.host_lib().rh_eigen4(rc._p(s10), rc._p(lam), rc._p(V))
        ref = np.linalg.eigvalsh(M)[::-1]
        scale = max(abs(ref).max(), 1e-300)
        assert (np.diff(lam) <= 0).all() and np.abs(lam - ref).max() <= 1e-14 * scale * 10
        assert np.abs(V.T @ V - np.eye(4)).max() <= 1e-14 and np.abs(M @ V - V * lam).max() <= 1e-13 * scale


def test_own_trigonometry_is_accurate_to_a_few_ulp():
    """rot_sincos on [0, 5 pi / 4] and rot_atan2_pos on the upper half plane against numpy: 4 ulp of the result (the polynomials are FDLIBM's, good to 1 ulp; the plain
    argument reduction costs the rest), with the break points and their neighbours among the arguments."""
    rng = np.random.default_rng(1)
    edges = np.array([0.0, 0.3, 0.78125, np.pi / 4, 3 * np.pi / 4, np.pi / 2, np.pi, 5 * np.pi / 4, 1e-9, 1e-4])
    x = np.concatenate([rng.uniform(0, 5 * np.pi / 4, 20000), edges, np.nextafter(edges, 9.0), np.nextafter(edges[1:], 0.0)])
    x = x[x <= 3.9269908169872414]
    ratio = np.concatenate([10.0 ** rng.uniform(-12, 12, len(x) - 12), [0.4375, 0.6875, 1.1875, 2.4375, 1.0, 1e-300, 1e300, 0.0, 0.4374999, 0.68751, 1.18751, 2.43751]])
    w = rng.choice([-1.0, 1.0], len(x)) * rng.uniform(0.1, 2.0, len(x))
    y = np.abs(w) * ratio
    out = np.zeros((len(x), 3))
    rc.host_lib().rh_trig(C.c_int(len(x)), rc._p(np.ascontiguousarray(x)), rc._p(np.ascontiguousarray(y)), rc._p(np.ascontiguousarray(w)), rc._p(out))
    ref = np.column_stack([np.sin(x), np.cos(x), np.arctan2(y, w)])
    # near a zero of sin / cos the error is held against the argument's own half ulp (the reduction subtracts pi / 2 in two pieces, 2e-27 short of it), not the result's
    ulp = np.maximum(np.spacing(np.abs(ref)), np.column_stack([np.spacing(x), np.spacing(x), np.zeros(len(x))]))
    worst = (np.abs(out - ref) / ulp).max(axis=0)
    print("worst error in ulp: sin %.2f cos %.2f atan2 %.2f" % tuple(worst))
    assert (worst <= 4.0).all()
