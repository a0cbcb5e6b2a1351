"""The visual-track cases of tests/landmark_cases.py on the CPU: every case reaches the regime it is named for (asserted from track_regime, the numpy restatement of the host's
layout rules, alone), the oracle is held against finite differences and a numpy J^T J on the ground it never walked before (reference view last / in the middle, both poses on
the same knots, two observations in a frame), the sparsity of its landmark rows is the one the table predicts, and the dense step reference the GPU tests compare against carries
the bar they hold it to."""
import numpy as np
import pytest

import landmark_cases as LC
import lvx
from oracle import lm
from oracle import oracle as O


def _regime(name):
    P, locks, ex = LC.build(name)
    return P, locks, ex, LC.track_regime(P, locks, ex["tau"])


@pytest.fixture(scope="module")
def oracle_eval():
    """Oracle evaluation (H, g, J) of a case at its state0, computed once per case."""
    cache = {}

    def get(name, jac=False):
        key = (name, jac)
        if key not in cache:
            P, locks, _ = LC.build(name)
            o = O.Oracle(); lvx.load_problem(o, P, locks)
            cache[key] = (o, o.evaluate(P["state0"], jac=jac, normal_eq=True))
        return cache[key]
    return get


# ---- regimes -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LC.GROUP_SIZES + LC.FUSED_SIZES)
def test_group_sizes_trips_and_cap_splits(n):
    P, locks, ex, R = _regime("grp_%d" % n)
    assert R["pair_sizes"] == {ex["pair"]: n}
    sizes = [c for _, c, _, _ in R["groups"]]
    assert sizes == [32] * (n // 32) + ([n % 32] if n % 32 else [])                 # the cap: 33 = 32 | 1, 65 = 32 | 32 | 1
    assert R["last_trips"][-1] == (n - 1) % 32 % 8 + 1
    assert R["nks"][-1] == {1: 1, 2: 1, 3: 2, 5: 3, 7: 4, 8: 4, 6: 3, 4: 2}[R["last_trips"][-1]]
    fused = [c for _, c, _, _ in R["fused_groups"]]
    assert fused == [64] * (n // 64) + ([n % 64] if n % 64 else [])
    assert len(set(R["colours"])) == len(R["groups"])                               # groups of one pair never share a launch


def test_group_size_table_hits_every_named_trip():
    last = {n: LC.track_regime(*LC.build("grp_%d" % n)[:2])["last_trips"][-1] for n in LC.GROUP_SIZES}
    assert last == {1: 1, 2: 2, 3: 3, 5: 5, 7: 7, 8: 8, 9: 1, 31: 7, 32: 8, 33: 1, 65: 1}
    nks = lambda r: (2 * r + 3) >> 2                                                # noqa: E731
    assert [nks(r) for r in (1, 2, 3, 5)] == [1, 1, 2, 3] and [(2 * r) >> 2 for r in (1, 2, 3, 5)] == [0, 1, 1, 2]   # without the "+ 3" the trips of 1, 3, 5 lose their last k-step


def test_same_window_and_same_interval():
    P, locks, ex, R = _regime("same_interval")
    assert all((a0, a1) == (ex["window"], ex["window"]) for _, _, a0, a1 in R["groups"])
    same = (R["k0"] == R["k1"]) & (R["k0"] == ex["interval"])
    assert same.sum() >= 2 and (R["k0"] != R["k1"]).any()
    assert not (np.asarray(P["rep_t0"])[same] == P["lm_t0"][P["rep_lm"][same]]).any()        # not the reference observation: two different views on the same four knots


def test_reference_observation_as_a_block_and_twice_in_a_frame():
    P, _, _, R = _regime("ref_as_block")
    is_ref = np.array([P["rep_t0"][i] == P["lm_t0"][l] and np.array_equal(P["rep_uv"][i], P["lm_uv"][l]) for i, l in enumerate(P["rep_lm"])])
    assert is_ref.sum() == 2 and (R["k0"][is_ref] == R["k1"][is_ref]).all()
    P, _, _, R = _regime("twice_in_frame")
    for l in range(2):
        t = P["rep_t0"][P["rep_lm"] == l]
        u, c = np.unique(t, return_counts=True)
        assert c.max() == (2 if l == 0 else 3)                                      # two (three) observations share a frame time and differ in their pixels
    assert len(np.unique(P["rep_uv"], axis=0)) == len(P["rep_uv"])


def test_adjacent_windows_and_panel_offsets():
    P, _, ex, R = _regime("adjacent_windows")
    assert R["pair_sizes"] == {ex["pair"]: 16} and ex["pair"][1] == ex["pair"][0] + 1
    assert sorted(set(zip(R["k0"] & 3, R["k1"] & 3))) == [(a, b) for a in range(4) for b in range(4)]
    P, _, ex, R = _regime("panel_offsets")
    assert R["pair_sizes"] == {ex["pair"]: 4}
    assert sorted(zip(R["k0"] & 3, R["k1"] & 3)) == [(0, 0), (0, 3), (3, 0), (3, 3)]


def test_first_and_last_interval():
    P, _, ex, R = _regime("first_last_interval")
    last = ex["last"]
    assert last == P["n_knots"] - 4
    assert 0 in R["k0"] and 0 in R["k1"] and last in R["k0"] and last in R["k1"]
    assert R["k0"].min() >= 0 and R["k1"].max() <= last and R["kmin"].min() == 0 and R["kmax"].max() == P["n_knots"] - 1


@pytest.mark.parametrize("name", ["ref_last", "ref_middle", "long_track"])
def test_reference_view_not_first(name):
    P, _, _, R = _regime(name)
    lm = P["rep_lm"]
    w0, w1 = R["k0"] >> 2, R["k1"] >> 2
    assert (w1 < w0).any()                                                          # the cross kernel gets w1 < w0
    for l in (range(P["n_landmarks"]) if name != "long_track" else [0]):
        t = P["rep_t0"][lm == l]
        if name == "ref_last":
            assert (t <= P["lm_t0"][l]).all() and (t < P["lm_t0"][l]).sum() == 5
        else:
            assert (t < P["lm_t0"][l]).sum() >= 3 and (t > P["lm_t0"][l]).sum() >= 3
        assert R["lm_first"][l] < LC.interval(P, P["lm_t0"][l] - LC.MARGIN)          # the landmark's span starts before its reference frame


def test_mirrored_pairs_collide_in_the_colour_keys():
    P, _, ex, R = _regime("mirrored_pairs")
    pairs = [(a0, a1) for _, _, a0, a1 in R["groups"]]
    assert len(set(P["rep_lm"][R["order"][[g[0] for g in R["groups"]]]])) == 4          # from different landmarks
    for a, b in ex["mirrored"]:
        ia, ib = pairs.index(a), pairs.index(b)
        assert R["colour_keys"][ia] == R["colour_keys"][ib] and R["colours"][ia] != R["colours"][ib]
        ordered = lambda p: {(p[0] + x, p[1] + y) for x in range(2) for y in range(2)}   # noqa: E731
        assert not (ordered(a) & ordered(b))                                        # an ORDERED key would let the two share a launch


@pytest.mark.parametrize("mode", ["locked", "free"])
@pytest.mark.parametrize("kind", LC.STRAYS)
def test_strays(kind, mode):
    P, locks, ex, R = _regime("stray_%s_%s" % (kind, mode))
    assert bool(locks & lvx.LOCK_CAM_TAU) == (mode == "locked") and P["state0"][LC.tau_cam_slot(P)] == ex["tau"] != 0.0
    assert not LC.track_regime(P, locks, 0.0)["strays"].any()                       # the layout (tau = 0) has them inside their windows
    assert int(R["strays"].sum()) == ex["strays"]
    sizes = [c for _, c, _, _ in R["groups"]]
    sides = [s for s in R["stray_side"] if s]
    if kind == "alone":
        assert sizes == [1] and sides == ["obs"]
    elif kind == "two_in_trip":
        assert sizes == [8] and sides == ["obs", "obs"]
    elif kind == "ref_side":
        assert sides == ["ref", "ref"] and len(sizes) == 1
    else:
        assert sides == ["obs"] and len(sizes) == 1
    # 0.2 ms inside the window edge
    rd = LC.row_delta(P)
    te = np.concatenate([P["rep_t0"] + P["rep_uv"][:, 1] * rd, P["lm_t0"] + P["lm_uv"][:, 1] * rd])
    frac = (te - P["t0"]) / (4 * LC.DT)
    assert np.isclose((np.ceil(frac) - frac) * 4 * LC.DT, 2e-4, atol=1e-9).any()


def test_blocks_per_landmark():
    P, _, ex, R = _regime("lm_counts")
    assert [len(b) for b in R["lm_blocks"]] == ex["counts"] == [0, 1, 2, 3, 4, 0, 5, 8, 9, 40, 0]
    assert list(P["rep_lm"]) != sorted(P["rep_lm"])                                 # rep_lm shuffled
    long_ = ex["counts"].index(40)
    span = lambda l: R["ord"][6 * R["lm_last"][l] + 5] - R["ord"][6 * R["lm_first"][l]] + 1   # noqa: E731
    assert R["lm_wl"] == span(long_) and span(1) < R["lm_wl"] // 2                  # the long one sets the row width: the one-view landmark's row is mostly zeros
    assert R["lm_last"][0] == -1 and all(0 not in g and 5 not in g and 10 not in g for g in R["elim_groups"])


@pytest.mark.parametrize("n", LC.L_SIZES)
def test_landmark_counts(n):
    P, _, _, R = _regime("L_%d" % n)
    assert P["n_landmarks"] == n and all(len(b) == 3 for b in R["lm_blocks"])
    assert (n + 3) // 4 == {1: 1, 3: 1, 4: 1, 5: 2, 33: 9}[n]                        # workgroups of k_reproj_lmrows / k_lm_back (4 landmarks each)


def test_hub_coupling():
    P, _, _, R = _regime("hub_coupled")
    assert R["n_hub"] == 5 and R["hub0"] == 12 and R["n_border"] == 52
    assert R["hub_coupled"][0] and R["band_sides"][0] == (True, True)               # border slots and band couplings on both sides of the hub gap
    assert R["ord"][6 * 11] + 6 == R["ord"][6 * 17]                                  # the gap: knot 17 follows knot 11 in the band
    Q, _, _, S = _regime("hub_coupled_nosurf")
    assert S["n_hub"] == 0 and S["n_border"] == 22 and not any(S["hub_coupled"])
    assert S["lm_wl"] == R["lm_wl"] + 30                                            # the same tracks: without a hub its five knots are band scalars of the widest row


def test_lock_masks():
    P, locks, _, R = _regime("locks_cam_dead")
    N = P["n_knots"]
    assert all(R["ord"][6 * N + 15 + c] == -(1 << 30) for c in range(7))
    P, locks, _, R = _regime("locks_tau_free")
    assert R["ord"][6 * N + 21] == -1 - (R["n_border"] - 1) and all(6 * N + 21 in c for c in R["cols_required"])   # record width 57
    P, locks, _, R = _regime("locks_traj")
    assert R["n_band"] == 0 and R["lm_wl"] == 1 and R["elim_spread"] == 0 and len(R["elim_groups"]) == 1            # no band: every coupling in the border
    assert all(c == set(range(6 * N + 15, 6 * N + 21)) for c in R["cols_required"])
    P, locks, _, R = _regime("locks_r3")
    assert len(P["t_imu"]) == 0 and R["n_band"] == 3 * (N - R["n_hub"])                                           # 3 band scalars per knot
    assert R["ord"][6 * 30 + 3] == R["ord"][6 * 29 + 3] + 3 and R["ord"][6 * 30] == -(1 << 30)


@pytest.mark.parametrize("n", LC.FRAME_SIZES)
def test_landmarks_on_one_frame(n):
    P, _, ex, R = _regime("frame_%d" % n)
    assert len(set(P["lm_t0"][:n])) == 1 and len(set(R["lm_p0"][:n])) == 1
    sizes = [len(g) for g in R["elim_groups"] if g[0] < n]
    assert sizes == [32] * (n // 32) + ([n % 32] if n % 32 else [])
    assert all(all(l >= n for l in g) for g in R["elim_groups"] if g[0] >= n)       # the ordinary landmarks form groups of their own
    assert R["elim_kernel"] == 1


@pytest.mark.parametrize("name,per_knot", [("frames_shifted", 6), ("frames_shifted_r3", 3)])
def test_shifted_frames(name, per_knot):
    P, _, ex, R = _regime(name)
    p0 = R["lm_p0"]
    assert sorted(set(p0 - p0.min())) == [0, 6, 24, 30]
    assert [per_knot * (k - ex["frame_knots"][0]) for k in ex["frame_knots"]] == [0, 6, 24, 30]
    assert [len(g) for g in R["elim_groups"]] == ex["groups"] and R["elim_spread"] == ex["spread"] == 24
    assert sorted(set(p0[R["elim_groups"][0]] - p0.min())) == [0, 6, 24]            # one group, rows shifted inside it; 30 starts a new one


def test_row_reaches_both_ends_of_its_span():
    """reach_ends: the widest landmark couples to the first AND the last knot of its padded span: the group elimination writes an entry at distance exactly `bandwidth`."""
    P, _, _, R = _regime("reach_ends")
    mine = P["rep_lm"] == 0
    assert R["k0"][mine][0] == R["lm_first"][0] and R["k1"][mine].max() + 3 == R["lm_last"][0]
    assert R["lm_wl"] == 6 * (R["lm_last"][0] - R["lm_first"][0] + 1) and all(R["lm_last"][l] - R["lm_first"][l] < R["lm_last"][0] - R["lm_first"][0] for l in range(1, 4))
    cols = sorted(c for c in R["cols_required"][0] if c < 6 * P["n_knots"])
    assert R["ord"][cols[-1]] - R["ord"][cols[0]] == R["lm_wl"] - 1


def test_lds_on_either_side_of_160_kb():
    for name in LC.STEP_CASES:
        P, locks, _, R = _regime(name)
        ne_max = R["lm_wl"] + R["elim_spread"] + R["n_border"] + 12
        assert R["lds_g"] == 32 * (ne_max + 1) * 8 + 32 * 8 + 2 * ne_max * 4 + 16   # solve_local
        assert (R["lds_g"] > 160 * 1024) == (name == "long_track") and R["elim_kernel"] == (2 if name == "long_track" else 1)
    P, _, _, R = _regime("long_track")
    assert P["n_knots"] >= 180 and len(R["lm_blocks"][0]) == 41 and R["lm_last"][0] - R["lm_first"][0] + 1 >= 105 and P["n_landmarks"] == 21
    assert R["lm_wl"] >= 6 * 105


# ---- the oracle on ground it never walked --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.ORACLE_CASES)
def test_oracle_jacobian_against_finite_differences(name, oracle_eval):
    """As tests/test_oracle_kat.py::test_dual_number_jacobians_match_finite_differences, at its bar."""
    P, locks, _ = LC.build(name)
    o, r0 = oracle_eval(name, jac=True)
    s0 = P["state0"]
    J = O.dense_jacobian(r0["jac_cols"], r0["jac_vals"], o.tangent_size)
    free = lm.free_tangent_indices(P["n_knots"], P["n_landmarks"], locks)
    rng = np.random.default_rng(0)
    rows = slice(6 * len(P["t_imu"]) + len(P["surf_t"]), None)                      # the reprojection rows, and all rows
    for _ in range(3):
        d = np.zeros(o.tangent_size); d[free] = rng.standard_normal(len(free))
        h = 1e-6
        fd = (o.evaluate(o.plus(s0, h * d))["residuals"] - o.evaluate(o.plus(s0, -h * d))["residuals"]) / (2 * h)
        Jd = J @ d
        print(name, "fd error, all rows %.3e reprojection rows %.3e (relative to max |J d|)" % (np.abs(fd - Jd).max() / np.abs(Jd).max(), np.abs(fd - Jd)[rows].max() / np.abs(Jd[rows]).max()))
        assert np.abs(fd - Jd).max() < 1e-6 * np.abs(Jd).max()
        assert np.abs(fd - Jd)[rows].max() < 1e-6 * np.abs(Jd[rows]).max()


@pytest.mark.parametrize("name", LC.ORACLE_CASES)
def test_oracle_normal_equations_are_jtj(name, oracle_eval):
    """As tests/test_oracle_kat.py::test_normal_equations_are_jtj_with_huber_scaling, at its bar."""
    P, locks, _ = LC.build(name)
    o, r = oracle_eval(name, jac=True)
    J = O.dense_jacobian(r["jac_cols"], r["jac_vals"], o.tangent_size)
    res = r["residuals"]
    nI, nS, nR = len(P["t_imu"]), len(P["surf_t"]), len(P["rep_lm"])
    sc = np.ones(len(res))
    o0 = 6 * nI
    s = res[o0:o0 + nS] ** 2
    sc[o0:o0 + nS] = np.where(s > 25.0, np.sqrt(5.0 / np.sqrt(np.maximum(s, 1e-300))), 1.0)
    o1 = o0 + nS
    s2 = (res[o1:o1 + 2 * nR].reshape(-1, 2) ** 2).sum(axis=1)
    sc[o1:o1 + 2 * nR] = np.repeat(np.where(s2 > 25.0, np.sqrt(5.0 / np.sqrt(np.maximum(s2, 1e-300))), 1.0), 2)
    Js = J * sc[:, None]
    eh, eg = np.abs(Js.T @ Js - r["H"]).max() / np.abs(r["H"]).max(), np.abs(Js.T @ (res * sc) - r["g"]).max() / np.abs(r["g"]).max()
    print(name, "H vs J^T J %.3e, g vs J^T r %.3e" % (eh, eg))
    assert eh < 1e-12 and eg < 1e-12
    # ... and the landmark rows alone, against their own scale
    N, L = P["n_knots"], P["n_landmarks"]
    rows = slice(6 * N + 22, 6 * N + 22 + L)
    assert np.abs((Js.T @ Js)[rows] - r["H"][rows]).max() < 1e-12 * np.abs(r["H"][rows]).max()


# ---- sparsity ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.NAMES)
def test_landmark_row_sparsity(name, oracle_eval):
    """Every landmark row of the oracle's H is non-zero exactly where the table predicts: four knots per pose of every block, the camera columns the lock mask leaves free, the time
    offset when free.  (A block that IS the reference observation has both poses equal: its derivatives cancel, to zero or to rounding noise — its columns are allowed, not required.)
    The union width nn of every elimination group follows from the same pattern."""
    P, locks, ex = LC.build(name)
    P0 = P
    if ex["tau"] != 0.0:                                                           # the prediction is made from the layout's intervals: evaluate at tau = 0
        P0 = dict(P, state0=P["state0"].copy()); P0["state0"][LC.tau_cam_slot(P)] = 0.0
        o = O.Oracle(); lvx.load_problem(o, P0, locks)
        H = o.evaluate(P0["state0"], normal_eq=True)["H"]
    else:
        H = oracle_eval(name)[1]["H"]
    R = LC.track_regime(P, locks)
    N, L = P["n_knots"], P["n_landmarks"]
    nz = []
    for l in range(L):
        got = set(np.flatnonzero(H[6 * N + 22 + l, :6 * N + 22]))
        assert R["cols_required"][l] <= got <= R["cols_allowed"][l], (l, sorted(R["cols_required"][l] - got), sorted(got - R["cols_allowed"][l]))
        assert set(np.flatnonzero(H[6 * N + 22 + l, 6 * N + 22:])) <= {l}           # landmarks couple to each other through nothing
        nz.append(got)
    noise = [len(set().union(*[nz[l] for l in g])) for g in R["elim_groups"]]
    for g, n_req, n_got in zip(R["elim_groups"], R["nn_predicted"], noise):
        alw = len(set().union(*[R["cols_allowed"][l] for l in g]))
        assert n_req <= n_got <= alw
    if "nn" in ex:
        assert R["nn_predicted"] == ex["nn"] == noise
    if name == "frame_65x10":
        assert min(R["nn_predicted"][:2]) > 200 and R["nn_predicted"] == noise
    if name == "ref_only_frame":
        g = [g for g in R["elim_groups"] if g[0] in ex["ref_only"]]
        assert g == [ex["ref_only"]] and R["nn_predicted"][R["elim_groups"].index(g[0])] == 0
        d = np.diag(H)[6 * N + 22:][ex["ref_only"]]
        print("H_ll of the reference-only landmarks:", d, "against", np.diag(H)[6 * N + 22 + 3])
        assert (d <= 1e-20 * np.diag(H)[6 * N + 22 + 3]).all()                      # zero or rounding noise


def test_union_widths_hit_the_tiles():
    nn = {name: LC.track_regime(*LC.build(name)[:2])["nn_predicted"] for name in ("nn_30", "nn_48", "nn_49", "nn_traj", "nn_traj_tau")}
    assert nn == {"nn_30": [30], "nn_48": [48], "nn_49": [49], "nn_traj": [6], "nn_traj_tau": [7]}
    assert [(n + 15) >> 4 for n in (30, 48, 49, 6)] == [2, 3, 4, 1]


# ---- the step reference --------------------------------------------------------------------------------------------------------------------------------------
def _refined_solve(A, b):
    """Cholesky solve with one refinement step whose residual is formed in np.longdouble."""
    Lc = np.linalg.cholesky(A)
    solve = lambda r: np.linalg.solve(Lc.T, np.linalg.solve(Lc, r))                 # noqa: E731
    y = solve(b)
    r = (b.astype(np.longdouble) - A.astype(np.longdouble) @ y.astype(np.longdouble)).astype(np.float64)
    return y + solve(r)


def step_reference_error(name, radius, oracle_eval):
    P, locks, _ = LC.build(name)
    _, ev = oracle_eval(name)
    H, g = ev["H"], ev["g"]
    free = lm.free_tangent_indices(P["n_knots"], P["n_landmarks"], locks)
    s = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H)[free], 0)))
    d_ref, _, _ = lm.solve_step(H, g, free, radius, s)
    Hs = H[np.ix_(free, free)] * s[:, None] * s[None, :]
    A = Hs + np.diag(np.clip(np.diag(Hs), 1e-6, 1e32) / radius)
    y = _refined_solve(A, -(g[free] * s))
    return np.abs(d_ref[free] - y * s).max() / np.abs(y * s).max()


@pytest.mark.parametrize("name", LC.STEP_CASES)
def test_step_reference_carries_its_bar(name, oracle_eval):
    """lm.solve_step on the oracle's dense H (what tests/test_gpu_landmark_tracks.py holds the device's step to at 1e-7) agrees with a refined Cholesky solve to 1e-8 of max |y|
    at radius 3.0 everywhere, and at radius 1e4 wherever the GPU test uses that radius (LC.STEP_SMALL_RADIUS_ONLY lists the others — and nothing else)."""
    e_small, e_large = step_reference_error(name, 3.0, oracle_eval), step_reference_error(name, 1e4, oracle_eval)
    print(name, "step reference vs refined solve: radius 3.0 %.3e, radius 1e4 %.3e" % (e_small, e_large))
    assert e_small <= 1e-8
    assert (e_large > 1e-8) == (name in LC.STEP_SMALL_RADIUS_ONLY)
