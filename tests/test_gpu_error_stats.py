"""Error statistics on the device (lvx_error_statistics, lvx_get_plane_stats, lvx_get_landmark_stats) against the CPU oracle.

One seeded problem of ~40 knots: 300 IMU samples, 700 surfel rows over 6 planes (one without rows, one with more than 256; no count a multiple of 64), 150
reprojection blocks over 12 landmarks (one unused, one with more than 64 blocks, one block whose view lies outside the spline), 20 camera-surfel blocks, the
orientation prior.  Expected values: numpy over the ORACLE's residual rows (oracle.Oracle.evaluate), split by family_rows() and divided by the family weights.

The block with the view outside the spline.  A view whose SPAN leaves the spline is refused by the layout (LVX_E_RANGE before anything runs, as CheckTimeSpans); the
evaluator skips a block (k = -1 in k_reproj_jac) when the span is inside and the view's row time, moved by the locked camera time offset, is not.  lvx_evaluate then
returns LVX_E_RANGE (the reference throws std::range_error) and so does the oracle, which returns no rows at all.  The statistics call returns the code of lvx_evaluate
and still fills its output with the sums over the blocks it evaluated: that block is counted in n_blocks and not in n_evaluated.  The oracle's rows therefore come from the same problem WITHOUT that one block; every other case runs on
the problem without it, where the call succeeds.

Tolerances.  A row of the device is within eps_f = 1e-11 * (largest |row| of the family) of the oracle's (tests/test_gpu_fullsize_oracle.py); a raw error is the row
over the weight w, so a mean of raw errors is within eps_f / w, a maximum likewise, and a mean of squares within 2 max|e| eps_f / w + (eps_f / w)^2.  Costs: 1e-12
relative (tests/test_gpu_eval.py).  Counts are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
from oracle import oracle as O

TAU_LOCKS = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
PRIOR_W = 28.0
NR = [3, 3, 1, 1, 2, 1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "lvi-exc_amd")


def make_case():
    """The problem of this file and the index of the reprojection block whose view lies outside the spline."""
    P = synth.make_problem(seed=17, duration=0.75, n_surfel=700, n_planes=5, n_landmarks=12, views_per_lm=14, cam_rate=40.0, n_camsurf=20, pad=0.02)
    rng = np.random.default_rng(5)
    # planes: the 5 surfel planes, one plane nobody points at, then the camera-surfel planes
    n_cs_planes = len(P["planes"]) - 5
    P["planes"] = np.concatenate([P["planes"][:5], [[0.0, 0.0, 3.0]], P["planes"][5:]])
    P["cs_plane"] = (P["cs_plane"] + 1).astype(np.int32)
    assert n_cs_planes == len(P["cs_lm"])
    # surfel rows: 160 rows of planes 1..4 re-labelled to plane 0 (metres off it: Huber outliers) -> plane 0 holds more than 256 rows
    sid = P["surf_plane"].copy()
    move = rng.permutation(np.flatnonzero(sid > 0))[:160]
    sid[move] = 0
    P["surf_plane"] = sid
    # reprojection: landmark 11 loses its blocks, landmark 0 gets copies of its own with pixel noise until it has 70, 149 blocks in all
    keep = P["rep_lm"] != 11
    lm, uv, t0 = P["rep_lm"][keep], P["rep_uv"][keep], P["rep_t0"][keep]
    own = np.flatnonzero(lm == 0)
    extra = own[rng.integers(0, len(own), 70 - len(own))]
    lm = np.concatenate([lm, lm[extra]]); uv = np.concatenate([uv, uv[extra] + rng.normal(0, 3.0, (len(extra), 2))]); t0 = np.concatenate([t0, t0[extra]])
    others = rng.permutation(np.flatnonzero(lm != 0))[:79]
    assert len(others) == 79
    order = rng.permutation(np.concatenate([np.flatnonzero(lm == 0), others]))
    lm, uv, t0 = lm[order], uv[order], t0[order]
    # ... and block 77: a view whose padded span [t0 - 1 ms, t0 + readout + 1 ms] ends 1 us inside the spline — the layout accepts it — observed in the last image row: with
    # the camera offset of CAM_TAU (locked) its row time lies behind the spline's end and the evaluator skips the block
    skip = 77
    cam = P["camera"]
    t_end = P["t0"] + (P["n_knots"] - 3) * P["dt"]
    lm = np.insert(lm, skip, 3); uv = np.insert(uv, skip, [400.0, cam["rows"] - 1.0], axis=0); t0 = np.insert(t0, skip, t_end - cam["readout"] - 1e-3 - 1e-6)
    P["rep_lm"], P["rep_uv"], P["rep_t0"] = lm.astype(np.int32), uv, t0
    # camera-surfel: 20 blocks on the landmarks whose reference view is not on a knot (with a locked non-zero camera offset the {t, t} span of a view ON a knot leaves its
    # 4-knot segment: range_error, as in the reference) — the consistent (landmark, plane) pairs, then landmarks paired with another landmark's plane (off it: outliers)
    frac = np.mod((P["lm_t0"] - P["t0"]) / P["dt"], 1.0)
    good = [(l, p) for l, p in zip(P["cs_lm"], P["cs_plane"]) if 0.1 < frac[l] < 0.9]
    assert len(good) >= 5
    pairs = list(good)
    k = 0
    while len(pairs) < 20:
        pairs.append((good[k % len(good)][0], good[(k + 1 + k // len(good)) % len(good)][1])); k += 1
    P["cs_lm"] = np.array([a for a, _ in pairs], dtype=np.int32); P["cs_plane"] = np.array([b for _, b in pairs], dtype=np.int32)
    # Huber deltas between the small and the large residuals of the perturbed state (asserted on the oracle's rows below)
    P["huber_surf"], P["huber_rep"], P["huber_cs"] = 2.0, 8.0, 6.0
    return P, skip


def without_block(P, i):
    Q = dict(P)
    for k in ("rep_lm", "rep_uv", "rep_t0"):
        Q[k] = np.delete(P[k], i, axis=0)
    return Q


CAM_TAU = 1.2e-3   # a locked, non-zero camera time offset: legal inside the spans' 1 ms margins + the knot interval, except for the block above


def state_of(P, locks, name="state0"):
    s = P[name].copy()
    N = P["n_knots"]
    s[7 * N + 31] = CAM_TAU
    if not (locks & lvx.LOCK_LIDAR_TAU):
        s[7 * N + 23] = 3e-4
    if not (locks & lvx.LOCK_CAM_TAU):
        s[7 * N + 31] = -2e-4
    return s


def _prior(P):
    return (P["t0"], np.array([np.cos(5e-5), 0, 0, np.sin(5e-5)]), PRIOR_W)


def _load(obj, P, locks, prior=True):
    lvx.load_problem(obj, P, locks)
    if prior:
        obj.set_orientation_prior(*_prior(P))


def _expected(P, rows_all, fam_rows, locks, so3_only=False):
    """numpy statistics of the oracle's rows: per family (n, outliers, cost, mean, mean |e|, mean e^2, max |e|, eps) and the rows themselves."""
    w = [P["w_gyro"], P["w_acc"], PRIOR_W, P["w_surf"], P["w_rep"], P["w_cs"]]
    h = [0, 0, 0, P["huber_surf"], P["huber_rep"], P["huber_cs"]]
    out = []
    for f in range(6):
        rows = rows_all[fam_rows[f]:fam_rows[f + 1]].reshape(-1, NR[f])
        n = len(rows)
        if n == 0:
            out.append(None)
            continue
        sq = (rows ** 2).sum(axis=1)
        outl = sq > h[f] ** 2 if h[f] > 0 else np.zeros(n, bool)
        cost = 0.5 * np.where(outl, 2 * h[f] * np.sqrt(sq) - h[f] ** 2, sq).sum()
        e = rows / w[f]
        out.append(dict(n=n, outliers=int(outl.sum()), cost=cost, mean=e.mean(axis=0), mean_abs=np.abs(e).mean(axis=0), mean_sq=(e ** 2).mean(axis=0), max_abs=np.abs(e).max(axis=0),
                        eps=1e-11 * np.abs(rows).max() / w[f], e=e))
    return out


def _check_families(st, exp, n_blocks=None):
    total = 0.0
    for f, name in enumerate(lvx.FAMILY_NAMES):
        s, x = st[name], exp[f]
        if x is None:
            assert s["n_blocks"] == 0 and s["n_evaluated"] == 0 and s["n_outliers"] == 0 and s["cost"] == 0.0
            assert not s["sum"].any() and not s["sum_abs"].any() and not s["sum_sq"].any() and not s["max_abs"].any()
            continue
        k, n = NR[f], x["n"]
        print(name, "n", s["n_blocks"], s["n_evaluated"], "outliers", s["n_outliers"], x["outliers"], "cost", s["cost"], x["cost"], "mean |e|", s["sum_abs"][:k] / n, x["mean_abs"],
              "max |e|", s["max_abs"][:k], "eps", x["eps"])
        assert s["n_blocks"] == (n if n_blocks is None else n_blocks[f]) and s["n_evaluated"] == n and s["n_outliers"] == x["outliers"]
        assert abs(s["cost"] - x["cost"]) <= 1e-12 * abs(x["cost"])
        assert np.abs(s["sum"][:k] / n - x["mean"]).max() <= x["eps"]
        assert np.abs(s["sum_abs"][:k] / n - x["mean_abs"]).max() <= x["eps"]
        assert np.abs(s["sum_sq"][:k] / n - x["mean_sq"]).max() <= 2 * x["max_abs"].max() * x["eps"] + x["eps"] ** 2
        assert np.abs(s["max_abs"][:k] - x["max_abs"]).max() <= x["eps"]
        assert not s["sum"][k:].any() and not s["sum_abs"][k:].any() and not s["sum_sq"][k:].any() and not s["max_abs"][k:].any()
        total += x["cost"]
    assert abs(st["cost"] - total) <= 1e-12 * abs(total)


def _check_segments(g, P, exp):
    """per-plane and per-landmark statistics against the oracle's rows grouped by the INPUT plane_id / landmark_id"""
    n, sa, mx = g.plane_stats()
    assert len(n) == len(P["planes"])
    es = exp[lvx.FAM_SURFEL]
    for p in range(len(P["planes"])):
        rows = np.flatnonzero(P["surf_plane"] == p) if es is not None else []
        if len(rows) == 0:
            assert n[p] == 0 and sa[p] == 0.0 and mx[p] == 0.0
            continue
        a = np.abs(es["e"][rows, 0])
        assert n[p] == len(rows)
        assert abs(sa[p] / n[p] - a.mean()) <= es["eps"] and abs(mx[p] - a.max()) <= es["eps"]
    n, sq, mn = g.landmark_stats()
    assert len(n) == P["n_landmarks"]
    er = exp[lvx.FAM_REPROJ]
    for l in range(P["n_landmarks"]):
        rows = np.flatnonzero(P["rep_lm"] == l) if er is not None else []
        if len(rows) == 0:
            assert n[l] == 0 and sq[l] == 0.0 and mn[l] == 0.0
            continue
        q = (er["e"][rows] ** 2).sum(axis=1)
        big = np.sqrt(q.max())
        assert n[l] == len(rows)
        assert abs(sq[l] / n[l] - q.mean()) <= 2 * np.sqrt(2) * big * er["eps"] + 2 * er["eps"] ** 2   # |e|^2 of a 2-vector whose components are each within eps
        assert abs(mn[l] - big) <= np.sqrt(2) * er["eps"]
    return n


@pytest.fixture(scope="module")
def case():
    """The problem, the oracle's rows at the perturbed state for the default lock mask (computed once, never changed) and their numpy statistics."""
    P, skip = make_case()
    Q = without_block(P, skip)
    o = O.Oracle()
    _load(o, Q, TAU_LOCKS)
    s = state_of(P, TAU_LOCKS)
    rows = o.evaluate(s)["residuals"]
    rows.setflags(write=False)
    n = len(P["t_imu"])
    fam_rows = np.cumsum([0, 3 * n, 3 * n, 1, len(Q["surf_t"]), 2 * len(Q["rep_lm"]), len(Q["cs_lm"])])
    return dict(P=P, Q=Q, skip=skip, state=s, rows=rows, exp=_expected(Q, rows, fam_rows, TAU_LOCKS), fam_rows=fam_rows)


def test_problem_has_the_shapes_the_kernels_can_go_wrong_at(case):
    P, Q = case["P"], case["Q"]
    assert 38 <= P["n_knots"] <= 46 and len(P["t_imu"]) == 300 and len(P["surf_t"]) == 700 and len(P["rep_lm"]) == 150 and len(P["cs_lm"]) == 20
    cnt = np.bincount(P["surf_plane"], minlength=len(P["planes"]))[:6]
    assert cnt.sum() == 700 and (cnt == 0).sum() == 1 and cnt.max() > 256 and all(c % 64 for c in cnt if c)
    lc = np.bincount(P["rep_lm"], minlength=12)
    assert (lc == 0).sum() == 1 and lc.max() > 64
    t_end = P["t0"] + (P["n_knots"] - 3) * P["dt"]
    k = case["skip"]
    row_time = P["rep_t0"][k] + CAM_TAU + P["rep_uv"][k, 1] * P["camera"]["readout"] / P["camera"]["rows"]
    assert P["rep_t0"][k] + P["camera"]["readout"] + 1e-3 < t_end <= row_time - 1e-5   # span inside, row time (also after the t - 1e-5 retry) outside
    for f in (lvx.FAM_SURFEL, lvx.FAM_REPROJ, lvx.FAM_CAMSURF):   # every lossy family has inliers and outliers at this state
        x = case["exp"][f]
        assert 0 < x["outliers"] < x["n"], (f, x["outliers"], x["n"])


@pytest.mark.gpu
def test_family_statistics_and_the_skipped_block(case):
    P, Q = case["P"], case["Q"]
    g = lvx.Context(0)
    _load(g, P, TAU_LOCKS)
    assert g.family_rows()[-1] == len(case["rows"]) + 2   # the problem with the extra block
    rc, st, _ = g.error_statistics(case["state"], raw=True)
    assert rc == lvx.E_RANGE                              # what lvx_evaluate returns for this problem
    with pytest.raises(lvx.LvxError) as ei:
        g.evaluate(case["state"])
    assert ei.value.code == lvx.E_RANGE
    nb = [len(P["t_imu"]), len(P["t_imu"]), 1, 700, 150, 20]
    _check_families(st, case["exp"], n_blocks=nb)
    assert st["reproj"]["n_blocks"] - st["reproj"]["n_evaluated"] == 1
    # the segment statistics leave the skipped block out as well
    lm_n = _check_segments(g, Q, case["exp"])
    assert lm_n[3] == np.count_nonzero(P["rep_lm"] == 3) - 1
    g.close()


@pytest.mark.gpu
def test_plane_and_landmark_statistics(case):
    Q = case["Q"]
    g = lvx.Context(0)
    _load(g, Q, TAU_LOCKS)
    assert g.family_rows() == [int(v) for v in case["fam_rows"]]
    st = g.error_statistics(case["state"])
    _check_families(st, case["exp"])
    n = _check_segments(g, Q, case["exp"])
    assert n[11] == 0 and n[0] > 64
    pn, _, _ = g.plane_stats()
    assert pn[5] == 0 and pn[0] > 256 and pn[6:].sum() == 0   # the camera-surfel planes carry no surfel rows
    # resident state, no host copy of it: the same bits
    g.set_state(case["state"])
    rc, st2, raw2 = g.error_statistics(None, raw=True)
    rc1, st1, raw1 = g.error_statistics(case["state"], raw=True)
    assert rc == 0 and rc1 == 0 and bytes(raw1) == bytes(raw2)
    g.close()


def _variant(P, locks, so3_only=False, prior=True, bounds=False, state=None):
    o, g = O.Oracle(), lvx.Context(0)
    for obj in (o, g):
        _load(obj, P, locks, prior=prior)
    o.set_so3_only(so3_only)
    if bounds:
        g.set_time_offset_bounds(0.01, 0.001)   # the oracle's bounds (trajectory_manager_lvi.h:118-119), set explicitly
    s = state_of(P, locks) if state is None else state
    rows = o.evaluate(s)["residuals"]
    fr = g.family_rows()
    assert fr[-1] == len(rows)
    exp = _expected(P, rows, fr, locks)
    if not prior:
        assert exp[lvx.FAM_PRIOR] is None
    st = g.error_statistics(s)
    _check_families(st, exp)
    _check_segments(g, P, exp)
    lo = g.layout()
    g.close()
    return st, lo


@pytest.mark.gpu
@pytest.mark.parametrize("locks", [0, TAU_LOCKS], ids=["free_offsets", "default"])
def test_lock_masks(case, locks):
    st, _ = _variant(case["Q"], locks, bounds=locks == 0)
    assert st["accel"]["n_evaluated"] == 300 and st["camsurf"]["n_evaluated"] == 20


@pytest.mark.gpu
def test_so3_only_gyro_and_prior(case):
    """Solve #0: LVX_LOCK_R3, gyroscope blocks and the orientation prior; no accelerometer family and no LiDAR / camera family at all (families with zero blocks)."""
    Q = dict(case["Q"])
    Q["surf_pt"], Q["surf_t"], Q["surf_plane"] = np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int32)
    Q["rep_lm"], Q["rep_uv"], Q["rep_t0"] = np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0)
    Q["cs_lm"], Q["cs_plane"] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    st, _ = _variant(Q, TAU_LOCKS | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS, so3_only=True)
    assert st["gyro"]["n_evaluated"] == 300 and st["prior"]["n_evaluated"] == 1 and st["accel"]["n_blocks"] == 0 and st["surfel"]["n_blocks"] == 0


@pytest.mark.gpu
def test_merged_hub_segment_corner():
    """The construction of test_merged_hub_segment_corner_takes_the_exact_fallback (tests/test_gpu_eval.py): t_map 5 us before a knot, a locked LiDAR offset of 8 us, 40 rows
    right behind t_map whose spans merge with the map-time span — inside them the map-time pose has another interpolation amount than the shared one."""
    P = synth.make_problem(seed=31, duration=1.0, n_surfel=400, n_planes=6, n_landmarks=0, n_camsurf=0)
    P["t_map"] = P["t0"] + 12 * P["dt"] - 5e-6
    assert P["surf_t"].min() > P["t_map"]
    P["surf_t"] = np.sort(np.concatenate([P["t_map"] + np.linspace(2e-3, 0.03, 40), P["surf_t"][40:]]))
    s = P["state0"].copy()
    s[7 * P["n_knots"] + 16 + 7] = 8e-6
    st, _ = _variant(P, TAU_LOCKS, prior=False, state=s)
    assert st["surfel"]["n_evaluated"] == 400 and st["reproj"]["n_blocks"] == 0


@pytest.mark.gpu
def test_two_calls_give_identical_bits_and_leave_the_evaluation_alone(case):
    Q, s = case["Q"], case["state"]
    g = lvx.Context(0)
    _load(g, Q, TAU_LOCKS)
    rc, _, a = g.error_statistics(s, raw=True)
    pa, la = g.plane_stats(), g.landmark_stats()
    rc2, _, b = g.error_statistics(s, raw=True)
    pb, lb = g.plane_stats(), g.landmark_stats()
    assert rc == 0 and rc2 == 0 and bytes(a) == bytes(b)
    for x, y in zip(pa + la, pb + lb):
        assert x.tobytes() == y.tobytes()
    g.close()
    # between two evaluations of the normal equations (fixed summation order): the second one's checksums are those of a run without the statistics call
    sums = []
    for with_stats in (False, True):
        g = lvx.Context(0)
        _load(g, Q, TAU_LOCKS)
        g.set_switch("DETERMINISTIC", 1)
        g.evaluate(s, normal_eq=True, dense=False, residuals=False)
        if with_stats:
            g.error_statistics(s)
        g.evaluate(s, normal_eq=True, dense=False, residuals=False)
        sums.append(g.normal_eq_checksum())
        g.close()
    assert sums[0] == sums[1]


@pytest.mark.gpu
def test_errors(case):
    Q = dict(case["Q"])
    g = lvx.Context(0)
    _load(g, Q, TAU_LOCKS)
    with pytest.raises(lvx.LvxError) as ei:      # nothing evaluated yet
        g.plane_stats()
    assert ei.value.code == lvx.E_STATE
    with pytest.raises(lvx.LvxError) as ei:
        g.landmark_stats()
    assert ei.value.code == lvx.E_STATE
    g.error_statistics(case["state"])
    g.plane_stats()
    with pytest.raises(lvx.LvxError) as ei:      # another count than the table's
        g.plane_stats(3)
    assert ei.value.code == lvx.E_ARG
    Q["t_imu"] = Q["t_imu"].copy()
    Q["t_imu"][-1] = Q["t0"] + (Q["n_knots"] - 3) * Q["dt"] + 0.5   # beyond MaxTime: std::range_error in the reference
    g.set_imu(Q["t_imu"], Q["gyro"], Q["acc"], Q["w_gyro"], Q["w_acc"])
    with pytest.raises(lvx.LvxError) as ei:      # the problem changed since the statistics call
        g.plane_stats()
    assert ei.value.code == lvx.E_STATE
    with pytest.raises(lvx.LvxError) as ei:
        g.error_statistics(case["state"])
    assert ei.value.code == lvx.E_RANGE
    g.close()


@pytest.fixture(scope="module")
def demo_binary(tmp_path_factory):
    import build as lvx_build
    lvx_build.build()
    out = str(tmp_path_factory.mktemp("stats") / "error_stats_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(LIBDIR, "host"), os.path.join(ROOT, "tests", "native", "error_stats_demo.cpp"), "-o", out,
                           "-L" + LIBDIR, "-llvx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.gpu
def test_cpp_estimator_error_statistics(case, demo_binary, tmp_path):
    """TrajectoryEstimator::ErrorStatistics() on the same problem, built measurement by measurement in C++: the struct of the ctypes path, bit for bit, and the
    reference's lines from FormatErrorStatistics."""
    Q, s = case["Q"], case["state"]
    c = Q["camera"]
    t, q, w = _prior(Q)
    parts = [np.array([Q["t0"], Q["dt"], Q["n_knots"], TAU_LOCKS, c["rows"], c["cols"], c["readout"], c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"], c["k3"],
                       Q["w_gyro"], Q["w_acc"], Q["t_map"], Q["huber_surf"], Q["w_surf"], Q["huber_rep"], Q["w_rep"], Q["huber_cs"], Q["w_cs"], t, q[0], q[1], q[2], q[3], w], dtype=np.float64)]
    for a in (s, Q["t_imu"], Q["gyro"], Q["acc"], Q["planes"], Q["surf_pt"], Q["surf_t"], Q["surf_plane"], Q["lm_uv"], Q["lm_t0"], Q["rep_lm"], Q["rep_uv"], Q["rep_t0"], Q["cs_lm"], Q["cs_plane"]):
        a = np.asarray(a, dtype=np.float64).ravel()
        parts += [np.array([len(a)], dtype=np.float64), a]
    pin, pout = str(tmp_path / "p.bin"), str(tmp_path / "st.bin")
    np.concatenate(parts).tofile(pin)
    r = subprocess.run([demo_binary, "estimator", pin, pout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = lvx.Context(0)
    _load(g, Q, TAU_LOCKS)
    rc, st, raw = g.error_statistics(s, raw=True)
    g.close()
    assert rc == 0 and open(pout, "rb").read() == bytes(raw)
    lines = r.stdout.splitlines()
    assert lines[0] == "============== Before optimization ================" and len(lines) == 5
    for line, head, fam, key, k in zip(lines[1:], ("[Gyro]  Error size, average: 300; ", "[Accel] Error size, average: 300;  ", "[LiDAR] Error size, average: 700; ", "[CAMERA] Error size, average: 149; "),
                                       ("gyro", "accel", "surfel", "reproj"), ("sum_abs", "sum_abs", "sum_abs", "sum"), (3, 3, 1, 2)):
        assert line.startswith(head), line
        vals = np.array([float(v) for v in line[len(head):].split()])
        want = st[fam][key][:k] / st[fam]["n_evaluated"] * (Q["w_rep"] if fam == "reproj" else 1.0)
        assert len(vals) == k and np.abs(vals - want).max() <= 1e-5 * np.abs(want).max()   # six significant digits


@pytest.mark.gpu
def test_calibrator_collects_statistics_around_every_stage(demo_binary, tmp_path):
    """CalibrateOptions::error_statistics on the short sequence of tests/test_gpu_pipeline.py (one association round + trajInitFromSurfel, then trajInitFromLVIdata): every
    stage carries a before and an after record, the cost does not go up, and the records are the solver's own initial / final cost."""
    def _write(path, S, refine_iterations, lvi, camsurf, step=10, solve0=0):   # the file format of tests/native/calibrate_demo.cpp
        c = S["camera"]
        parts = [np.array([S["t0"], S["dt"], S["n_knots"], S["t_map"], S["H"], S["W"], len(S["scans"]), refine_iterations, lvi, camsurf, step, solve0,
                           c["rows"], c["cols"], c["readout"], c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"], c["k3"]], dtype=np.float64)]

        def vec(a):
            a = np.asarray(a, dtype=np.float64).ravel()
            parts.extend([np.array([len(a)], dtype=np.float64), a])
        vec(S["state0"])
        for k in ("t_imu", "gyro", "acc", "lm_uv", "lm_t0", "rep_lm", "rep_uv", "rep_t0"):
            vec(S[k])
        for sc in S["scans"]:
            vec(np.stack([sc["x"], sc["y"], sc["z"]], axis=1)); vec(sc["timestamp"])
        np.concatenate(parts).tofile(path)
    S = synth.make_sequence(seed=51, range_noise=0.0, lidar_err_deg=0.0, lidar_err_m=0.0, cam_err_deg=0.0, cam_err_m=0.0, cp_noise=(0.0, 0.0))
    pin, pout = str(tmp_path / "seq.bin"), str(tmp_path / "res.bin")
    _write(pin, S, refine_iterations=1, lvi=1, camsurf=0)
    r = subprocess.run([demo_binary, "calibrate", pin, pout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(pout)
    ns = int(out[0])
    rep = out[1:1 + 7 * ns].reshape(ns, 7)
    assert ns == 2
    for has, before, after, lm0, lm1, nb, ne in rep:
        print(before, after, lm0, lm1, nb, ne)
        assert has == 1.0 and nb > 0 and ne == nb
        assert after <= before
        assert abs(before - lm0) <= 1e-9 * lm0 and abs(after - lm1) <= 1e-9 * lm1   # (the solver's pass sums with atomics in another order)
    assert r.stdout.count("============== Before optimization ================") == ns and r.stdout.count("[LiDAR] Error size, average: ") == 2 * ns
