"""CPU: holds the first-map cases of tests/firstmap_cases.py to what each one claims — key scans, absent scans, points on the zero-then-transform branch, a map that is
not empty — and the oracle (oracle/pipeline.py::first_data_association) to the numpy restatements, which do not rest on it: key lists equal, the scans in the map frame
bit for bit.  Wrong variants of the host rule (>= for >, the last SCAN for the last KEY scan, no +-360 wrap, has_pose ignored) must each change the key list of some case: a
variant no case catches means a case is missing.  tests/test_gpu_firstmap.py then runs the same cases through the C ABI."""
import numpy as np
import pytest

import firstmap_cases as FC
from oracle import pipeline

NAMES = [c.name for c in FC.CASES]


def test_case_table_is_the_one_asked_for():
    by = FC.BY_NAME
    S = FC.sequence(*FC.BASE)
    assert S["scans"].shape == (12, 3600) and S["n_knots"] == 108 and abs(S["t0"] - 99.7) < 1e-12
    assert [c.name for c in FC.CASES if c.group == "key_rule"] == ["dist_strict", "last_key", "yaw_only", "pitch_only", "roll_only", "yaw_wrap", "angle_margin", "first_absent",
                                                                   "nondefault_all", "nondefault_one"]
    for name in ("dist_strict", "last_key", "yaw_only", "pitch_only", "roll_only", "yaw_wrap", "angle_margin", "first_absent"):
        assert (by[name].key_dist, by[name].key_angle) == (0.25, 5.0), name
    assert (by["nondefault_all"].key_dist, by["nondefault_all"].key_angle) == (0.05, 1.0) and (by["nondefault_one"].key_dist, by["nondefault_one"].key_angle) == (1e9, 1e9)
    assert by["mixed"].tau == 0.25 and by["tau_tail"].tau == 0.55 and by["tau_drop"].tau == 0.65 and by["has_pose_null"].has_pose() is None
    assert [(by[n].n, by[n].H, by[n].W) for n in ("s1", "s2", "s3")] == [(1, 16, 450), (2, 16, 225), (3, 16, 225)]
    assert [(by[n].H, by[n].W) for n in ("w15", "w17", "h3")] == [(16, 15), (16, 17), (3, 225)]
    assert FC.MAY_BE_EMPTY == ["w15", "w17", "h3"]
    assert max(c.n * c.H * c.W for c in FC.CASES) == 17 * 16 * 450          # nothing larger than the denser sequence


def test_pose_builder_angles_come_back_through_r2ypr():
    rng = np.random.default_rng(3)
    for _ in range(200):
        y, p, r = rng.uniform(-179, 179), rng.uniform(-89, 89), rng.uniform(-179, 179)
        assert np.abs(np.array(FC.ypr_deg(FC.pose(y, p, r))) - [y, p, r]).max() <= 1e-6
    T = FC.pose(10, 20, 30, (1, 2, 3)).reshape(4, 4)
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-15 and list(T[:3, 3]) == [1, 2, 3] and list(T[3]) == [0, 0, 0, 1]


def test_threshold_distances_are_exact_and_angles_keep_their_margin():
    """Distances on the threshold are dyadic: the squares, their sum and the root are exact in every implementation.  Angle differences stay 1e-6 deg away from it: no case
    tests libm's rounding."""
    P = FC.BY_NAME["dist_strict"].poses()[:, [3, 7, 11]]
    assert np.linalg.norm(P[1] - P[0]) == 0.25 and np.linalg.norm(P[2] - P[0]) == 0.3125 and np.linalg.norm(P[3] - P[2]) == 0.25
    assert 0.25 < np.linalg.norm(P[4] - P[2]) < 0.25001
    for name in ("yaw_only", "pitch_only", "roll_only", "yaw_wrap", "angle_margin"):
        c = FC.BY_NAME[name]
        ypr = np.array([FC.ypr_deg(T) for T in c.poses()])
        d = ypr[:, None, :] - ypr[None, :, :]
        d = np.where(d > 180, d - 360, d); d = np.where(d < -180, d + 360, d)
        assert np.abs(np.abs(d) - c.key_angle).min() >= 0.999e-6, name


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_what_it_claims(name):
    c, e = FC.BY_NAME[name], FC.BY_NAME[name].expected()
    if c.key is not None:
        assert e["key"] == c.key
    assert tuple(np.nonzero(~e["present"])[0]) == c.absent
    assert (e["zeroed"].sum() > 0) == c.zeroed
    sc = e["scans"]
    assert np.isnan(sc[~e["present"], :, :, :3]).all() and not sc[~e["present"], :, :, 3].any()
    fin = sc[e["present"]][..., :3]
    fin = fin[~np.isnan(fin)]
    assert fin.size == 0 or np.abs(fin).max() < FC.ROOM
    if c.zeroed:        # a point on that branch sits exactly on its scan's translation, intensity 0
        s, i = np.nonzero(e["zeroed"])
        want = c.poses().reshape(-1, 4, 4)[s, :3, 3].astype(np.float32)
        flat = sc.reshape(c.n, -1, 4)
        assert np.array_equal(flat[s, i, :3], want) and not flat[s, i, 3].any()
    if c.group == "empty":
        assert e["key"] == [] and np.isnan(sc[..., :3]).all()
    if name == "tau_tail":      # the last scan is present, only its late columns are outside
        assert e["present"][11] and 0 < e["zeroed"][11].sum() < e["zeroed"].shape[1] and not e["zeroed"][:11].any()
    if name == "first_absent":  # one absence of each kind
        assert c.has_pose()[0] == 0 and c.has_pose()[1] == 1 and not FC.np_inside(c.S(), c.state(), c.scan_t())[1]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_numpy_restatement(name):
    c, e, o = FC.BY_NAME[name], FC.BY_NAME[name].expected(), FC.oracle_result(name)
    assert list(o["key"]) == e["key"]
    assert list(pipeline.key_scans(c.poses(), e["present"], c.key_dist, c.key_angle)) == e["key"]
    so = o["scans_in_map"]
    assert so.shape == e["scans"].shape == (c.n, c.H, c.W, 4) and so.dtype == np.float32
    assert np.array_equal(np.isnan(so), np.isnan(e["scans"]))
    assert so.tobytes() == e["scans"].tobytes()
    if c.group == "empty":
        assert o["planes"] is None and o["points"] is None
    elif not c.may_be_empty:
        assert len(o["planes"]["p4"]) > 0 and len(o["points"]["t"]) > 0


def test_key_scan_selection_is_visible_in_the_map():
    """One key scan and all key scans give other maps on the same scans; the default rule keeps 10 of the base sequence's 12."""
    one, every, dflt = FC.oracle_result("nondefault_one"), FC.oracle_result("all_key"), FC.oracle_result("has_pose_null")
    assert len(one["planes"]["p4"]) != len(pipeline.surfel_map(one["scans_in_map"], dict(pipeline.DEFAULTS, plane_lambda=0.6))["p4"])
    assert len(dflt["key"]) == 10 and len(dflt["planes"]["p4"]) != len(every["planes"]["p4"])


@pytest.mark.parametrize("wrong", sorted(FC.WRONG_RULES))
def test_wrong_rule_changes_some_key_list(wrong):
    rules = FC.WRONG_RULES[wrong]
    caught = []
    for c in FC.CASES:
        present = FC.np_present(c.S(), c.state(), c.scan_t(), c.has_pose(), rules)
        if FC.np_key_scans(c.poses(), present, c.key_dist, c.key_angle, rules) != c.expected()["key"]:
            caught.append(c.name)
    print(wrong, "caught by", caught)
    assert caught
    want = dict(ge={"dist_strict"}, last_scan={"last_key", "yaw_only", "pitch_only", "roll_only"}, no_wrap={"yaw_wrap"}, ignore_has_pose={"first_absent", "mixed", "empty_no_pose"})[wrong]
    assert want <= set(caught)
