"""GPU: lvx_voxelgrid_downsample and lvx_lidar_odometry (tests/odometry_cases.py has the cases and says why no test compares two free-running loops).

  a. the filter against O.voxelgrid_xyzi, bit for bit in count, order and all four floats;
  b. the odometry against its parts (PRIMARY, exact): for every step the map is rebuilt from the call's own reported poses and key flags, lvx_voxel_build runs on it,
     lvx_voxelgrid_downsample filters the scan and lvx_ndt_align starts from pose[k - 1] cast to float — final_transformation, p6, iterations, n_evaluations and score
     equal the step record and the pose bit for bit (same kernels, same order, fixed-order reductions);
  c. the map cloud equals the concatenation of PL.transform_cloud over the reported key scans bit for bit, the final grid matches O.voxel_build of that map at the
     project's bars (tests/upstream_checks.check_voxels, the bars tests/test_gpu_voxel_cases.py holds the oracle to);
  d. teacher-forced against the oracle (SECONDARY): the oracle's step() starts from the GPU's map and guess; n_src and the key flag are equal, and on the steps the CPU
     stability record calls stable the iterations are equal and max |p6 - p6_oracle| <= max(1e-6, s_k) — 1e-6 is the project's bar for lvx_ndt_align with line-search
     iterations (tests/test_gpu_ndt_align.py), s_k the oracle's measured sensitivity of that very step to a 1e-7 m change of its guess;
  e. edge cases: a scan without a finite point, a single scan, argument and state errors."""
import ctypes as C

import numpy as np
import pytest

import lvx
import odometry_cases as OC
import upstream_checks as UC
import voxel_cases as VC
from oracle import oracle as O
from oracle import pipeline as PL

pytestmark = pytest.mark.gpu
SORT_TILE = 1024     # sorted positions per workgroup of k_vx_sort_pass (the step of voxel_cases' sort-tile clouds)
RUNS = ("gentle", "lively", "gentle+predict")


@pytest.fixture(scope="module")
def ctx():
    c = lvx.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- a. the filter ------------------------------------------------------------------------------------------------------------------------------------------------
def _cloud(n, seed=3, span=6.0):
    rng = np.random.default_rng(seed + n)
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-span, span, (n, 3)) * np.array([1.0, 0.7, 0.2])
    c[:, 3] = rng.uniform(0, 255, n)
    return c


def _filter_clouds():
    out = {}
    for n in (1, 63, 64, 65, 3600, 28800, VC.leaf_tile(1) + 1, SORT_TILE + 1, 2 * SORT_TILE + 1):
        out["n_%d" % n] = (_cloud(n), 0.5)
    out["above_own_sort"] = (_cloud(VC.OWN_SORT_MAX + 1, span=40.0), 0.5)               # rocPRIM sorts
    one = _cloud(3000)
    one[:, :3] = 0.25 + 0.2 * (one[:, :3] / 6.0)
    out["one_voxel"] = (one, 0.5)
    neg = _cloud(2000)
    neg[:, :3] -= np.float32(20.0)
    out["negative"] = (neg, 0.5)
    edge = _cloud(1500)
    edge[:, :3] = np.round(edge[:, :3] / 0.5) * 0.5                                      # every coordinate exactly k * leaf
    out["on_cell_edges"] = (edge, 0.5)
    out["other_leaf"] = (_cloud(5000), 0.13)
    wide = _cloud(4000, span=300.0)
    wide[:, 2] *= 5.0
    out["wide_grid"] = (wide, 0.5)                                                       # more cells than the fresh sort covers: the key range grows and the chain runs again
    return out


FILTER = _filter_clouds()


@pytest.mark.parametrize("name", sorted(FILTER))
def test_filter_against_the_oracle(ctx, name):
    cloud, leaf = FILTER[name]
    got, ref = lvx.voxelgrid_downsample(ctx, cloud, leaf), O.voxelgrid_xyzi(cloud, leaf)
    assert len(got) == len(ref) and np.array_equal(_bits(got), _bits(ref))
    if name == "one_voxel":
        assert len(got) == 1


def test_filter_leaves_non_finite_points_out(ctx):
    cloud = _cloud(5000)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j, i in enumerate(range(0, 5000, 7)):
        cloud[i, j % 3] = bad[(j // 3) % 3]
    got, ref = lvx.voxelgrid_downsample(ctx, cloud, 0.5), O.voxelgrid_xyzi(OC.finite(cloud), 0.5)
    assert len(got) == len(ref) and np.array_equal(_bits(got), _bits(ref))
    cloud[:, 0] = np.nan
    assert len(lvx.voxelgrid_downsample(ctx, cloud, 0.5)) == 0
    assert len(lvx.voxelgrid_downsample(ctx, cloud[:0], 0.5)) == 0                      # n = 0


def test_filter_errors(ctx):
    with pytest.raises(lvx.LvxError) as e:
        lvx.voxelgrid_downsample(ctx, _cloud(10), 0.0)
    assert e.value.code == lvx.E_ARG
    far = np.zeros((2, 4), np.float32)
    far[0, :3], far[1, :3] = 0.5, 1301.5                                                 # 1 302^3 cells: more than 2^31 - 1
    with pytest.raises(lvx.LvxError, match="Leaf size is too small") as e:
        lvx.voxelgrid_downsample(ctx, far, 1.0)
    assert e.value.code == lvx.E_ARG
    cloud = _cloud(1000)                                                                 # and the context filters on
    assert np.array_equal(_bits(lvx.voxelgrid_downsample(ctx, cloud, 0.5)), _bits(O.voxelgrid_xyzi(cloud, 0.5)))


# ---- the odometry runs -------------------------------------------------------------------------------------------------------------------------------------------------
def _predict(n):
    """small fixed motions, a different one per scan"""
    P = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        a = 1e-3 * (1 + k % 3)
        P[k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        P[k, :3, 3] = 1e-3 * np.array([k % 4, -(k % 3), 0.5])
    return P


def _grid_of(ctx, n_points):
    """the context's grid as lvx.voxel_build returns it, without building"""
    info = lvx.VoxelInfo()
    ctx._ck(ctx._l.lvx_voxel_get_info(ctx._h, C.byref(info)))
    nl = info.n_leaves
    o = dict(n_leaves=nl, n_points=info.n_points, grid=np.array(list(info.min_b) + list(info.max_b) + list(info.div_b) + list(info.divb_mul), np.int32),
             leaf_key=np.zeros(nl, np.int32), leaf_n=np.zeros(nl, np.int32), mean=np.zeros((nl, 3)), cov=np.zeros((nl, 9)), icov=np.zeros((nl, 9)),
             evecs=np.zeros((nl, 9)), evals=np.zeros((nl, 3)), centroid=np.zeros((nl, 3), np.float32), offsets=np.zeros(nl + 1, np.int32), point_ids=np.zeros(max(n_points, 1), np.int32))
    ctx._ck(ctx._l.lvx_voxel_get(ctx._h, *[lvx._p(o[k]) for k in ("leaf_key", "leaf_n", "mean", "cov", "icov", "evecs", "evals", "centroid", "offsets", "point_ids")]))
    return o


_RUNS = {}


def _run(ctx, run):
    """One lvx_lidar_odometry per run, shared by the tests: poses, step records, key count, map cloud and final grid, all fetched before anything else uses the context."""
    if run not in _RUNS:
        case = OC.make_case(run.split("+")[0])
        predict = _predict(OC.N_SCANS) if run.endswith("+predict") else None
        lvx.set_scans(ctx, case["scans"], OC.H, OC.W)
        poses, steps, n_key = lvx.lidar_odometry(ctx, predict, lvx.odom_default_options(ctx))
        cloud = lvx.odometry_get_map(ctx)
        _RUNS[run] = dict(case=case, predict=predict, poses=poses, steps=steps, n_key=n_key, map=cloud, grid=_grid_of(ctx, len(cloud)))
    return _RUNS[run]


def _scan(R, k):
    return OC.scan_xyzi(R["case"]["scans"][k])


def _guess(R, k):
    return OC.guess_of(R["poses"][k - 1], None if R["predict"] is None else R["predict"][k])


def _maps(R):
    """map cloud before each step, from the call's own poses and key flags"""
    parts, before = [], []
    for k in range(OC.N_SCANS):
        before.append(len(parts))
        if R["steps"]["is_key"][k]:
            parts.append(PL.transform_cloud(_scan(R, k), R["poses"][k]))
    return parts, before


def test_default_options(ctx):
    o = lvx.odom_default_options(ctx)
    assert (o.ndt_resolution, o.downsample_leaf, o.key_dist, o.key_angle_deg) == (0.5, 0.5, 0.2, 5.0)
    assert (o.ndt.step_size, o.ndt.transformation_epsilon, o.ndt.max_iterations, o.ndt.search, o.ndt.outlier_ratio) == (0.01, 1e-3, 50, 7, 0.55)
    assert (o.min_points_per_voxel, o.min_covar_eigvalue_mult) == (6, 0.01)


# ---- c. map and grid ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS)
def test_map_and_grid(ctx, run):
    R = _run(ctx, run)
    s = R["steps"]
    assert s["is_key"][0] == 1 and s["is_key"].sum() == R["n_key"] >= 2
    assert np.array_equal(R["poses"][0], np.eye(4)) and s["converged"].all()
    parts, _ = _maps(R)
    want = np.concatenate(parts)
    assert len(R["map"]) == R["n_key"] * OC.H * OC.W
    assert np.array_equal(_bits(R["map"]), _bits(want))                                  # NaN positions included
    assert np.isnan(want[:, 0]).any()
    assert R["grid"]["n_points"] == len(want)
    UC.check_voxels(R["grid"], O.voxel_build(want, OC.RESOLUTION, 6, 0.01))


# ---- b. the odometry against its parts ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS)
def test_steps_equal_their_parts(ctx, run):
    R = _run(ctx, run)
    parts, before = _maps(R)
    built = -1
    for k in range(1, OC.N_SCANS):
        if built != before[k]:
            lvx.voxel_build(ctx, np.concatenate(parts[:before[k]]), OC.RESOLUTION, 6, 0.01, fetch=False)
            built = before[k]
        src = lvx.voxelgrid_downsample(ctx, _scan(R, k), OC.LEAF)
        r = lvx.ndt_align(ctx, src, _guess(R, k), search=7, step_size=0.01, transformation_epsilon=1e-3, max_iterations=50)
        s = R["steps"][k]
        assert s["n_src"] == len(src)
        assert np.array_equal(r["final_transformation"].astype(np.float64), R["poses"][k]), k
        assert np.array_equal(r["p"], s["p6"]) and r["score"] == s["score"] and r["trans_probability"] == s["trans_probability"], k
        assert (r["iterations"], r["n_evaluations"], int(r["converged"])) == (s["iterations"], s["n_evaluations"], s["converged"]), k
    assert R["steps"]["iterations"][1:].min() >= 1


# ---- d. teacher-forced against the oracle -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS[:2])
def test_steps_against_the_oracle_from_the_gpu_state(ctx, run):
    R = _run(ctx, run)
    s_k, unstable = OC.stability(run)
    assert unstable.sum() <= OC.MAX_UNSTABLE[run]
    HW = OC.H * OC.W
    before = _maps(R)[1]
    ndt, built, worst, skipped = None, -1, 0.0, 0
    for k in range(1, OC.N_SCANS):
        if built != before[k]:
            ndt, built = OC.aligner(R["map"][:before[k] * HW]), before[k]
        o = OC.step(None, _guess(R, k), _scan(R, k), ndt)
        s = R["steps"][k]
        assert o["n_src"] == s["n_src"], k
        assert OC.is_key(list(R["poses"][:k]) + [o["pose"]]) == bool(s["is_key"]), k
        if unstable[k]:
            skipped += 1
            continue
        assert o["iterations"] == s["iterations"], k
        d, bar = np.abs(o["p6"] - s["p6"]).max(), max(OC.P6_BAR, s_k[k])
        worst = max(worst, d / bar)
        assert d <= bar, (k, d, bar)
    print("%s: worst |p6 - p6_oracle| / max(1e-6, s_k) over the stable steps %.3g, %d unstable steps skipped" % (run, worst, skipped))


# ---- e. edge cases -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scan_without_a_finite_point_keeps_the_guess(ctx):
    scans = OC.make_case("gentle")["scans"][:4].copy()
    scans["x"][2] = np.nan
    lvx.set_scans(ctx, scans, OC.H, OC.W)
    poses, steps, n_key = lvx.lidar_odometry(ctx)
    assert steps["n_src"][2] == 0 and steps["converged"][2] == 1 and steps["n_evaluations"][2] == 0 and steps["iterations"][2] == 0
    assert np.array_equal(poses[2], poses[1]) and steps["is_key"][2] == 0
    assert np.array_equal(steps["p6"][2][:3], poses[1][:3, 3])
    assert steps["n_src"][3] > 1000 and steps["iterations"][3] >= 1


def test_a_single_scan(ctx):
    scans = OC.make_case("gentle")["scans"][:1]
    lvx.set_scans(ctx, scans, OC.H, OC.W)
    poses, steps, n_key = lvx.lidar_odometry(ctx)
    assert n_key == 1 and steps["is_key"][0] == 1 and np.array_equal(poses[0], np.eye(4))
    assert np.array_equal(_bits(lvx.odometry_get_map(ctx)), _bits(OC.scan_xyzi(scans[0])))
    UC.check_voxels(_grid_of(ctx, OC.H * OC.W), O.voxel_build(OC.scan_xyzi(scans[0]), OC.RESOLUTION, 6, 0.01))


def test_errors():
    c = lvx.Context(0)
    try:
        with pytest.raises(lvx.LvxError) as e:                                          # before lvx_set_scans
            lvx.lidar_odometry(c)
        assert e.value.code == lvx.E_STATE
        with pytest.raises(lvx.LvxError) as e:                                          # before any odometry run
            lvx.odometry_get_map(c)
        assert e.value.code == lvx.E_STATE
        scans = OC.make_case("gentle")["scans"][:2].copy()
        lvx.set_scans(c, scans, OC.H, OC.W)
        steps, poses = np.zeros(2, lvx.ODOM_STEP_DTYPE), np.zeros((2, 16))
        assert c._l.lvx_lidar_odometry(c._h, None, None, None, lvx._p(steps), None) == lvx.E_ARG
        assert c._l.lvx_lidar_odometry(c._h, None, None, lvx._p(poses), None, None) == lvx.E_ARG
        for bad in (dict(ndt_resolution=0.0), dict(downsample_leaf=-1.0)):
            with pytest.raises(lvx.LvxError) as e:
                lvx.lidar_odometry(c, None, lvx.odom_default_options(c, **bad))
            assert e.value.code == lvx.E_ARG
        o = lvx.odom_default_options(c)
        o.ndt.search = 5
        with pytest.raises(lvx.LvxError) as e:
            lvx.lidar_odometry(c, None, o)
        assert e.value.code == lvx.E_ARG
        scans["x"][0] = np.nan                                                           # a first key scan without a finite point: the map's grid has no leaf
        lvx.set_scans(c, scans, OC.H, OC.W)
        with pytest.raises(lvx.LvxError) as e:
            lvx.lidar_odometry(c)
        assert e.value.code == lvx.E_STATE
        lvx.set_scans(c, OC.make_case("gentle")["scans"][:2], OC.H, OC.W)                # and the context runs on
        assert lvx.lidar_odometry(c)[2] >= 1
    finally:
        c.close()


# ---- f. the host driver ------------------------------------------------------------------------------------------------------------------------------------------------
def test_driver_takes_its_poses_from_the_odometry(ctx, tmp_path):
    """tests/native/odometry_demo.cpp over lvx_host::Calibrator with lidar_odometry = true and no pose file, on a 2 s synth.make_sequence of 16 x 225 scans: Run goes through
    Solve #0, the first map and one surfel solve; the poses the Calibrator holds (and hands to lvx_data_association_poses as they are) equal lvx_lidar_odometry on the same
    scans bit for bit, RunLidarOdometry's LoamPoses carry the scans' stamps and Eigen's quaternion of those poses, and the first-map call — fed these poses — selects the
    odometry's own key scans."""
    import os
    import subprocess
    import synth
    S = synth.make_sequence(seed=50, duration=2.0, H=OC.H, W=OC.W, n_reproj=200)
    N, n = S["n_knots"], len(S["scans"])
    scan_t = np.array([sc["timestamp"][0] for sc in S["scans"]], np.float64)
    x0 = np.array(S["state0"], np.float64)
    cam = S["camera"]
    parts = [[S["t0"], S["dt"], N, OC.H, OC.W, cam["rows"], cam["cols"], cam["readout"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]]]
    for a in (x0, S["t_imu"], S["gyro"], S["acc"], S["lm_uv"], S["lm_t0"], scan_t):
        a = np.asarray(a, np.float64).ravel()
        parts += [[len(a)], a]
    pin, pscans, pout = (str(tmp_path / f) for f in ("in.bin", "scans.bin", "out.bin"))
    np.concatenate([np.asarray(x, np.float64) for x in parts]).tofile(pin)
    np.ascontiguousarray(S["scans"], lvx.POINT_XYZIT).tofile(pscans)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "lvi-exc_amd")
    exe = str(tmp_path / "odometry_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(root, "tests", "native", "odometry_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, pin, pscans, pout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("stage")] == ["stage initialSO3TrajWithGyro", "stage BatchOptimization"]
    out = np.fromfile(pout)
    pose16, rec, loam = out[:16 * n].reshape(n, 4, 4), out[16 * n:19 * n].reshape(n, 3), out[19 * n:].reshape(n, 8)
    lvx.set_scans(ctx, S["scans"], OC.H, OC.W)
    poses, steps, n_key = lvx.lidar_odometry(ctx)
    assert np.array_equal(pose16, poses)
    assert np.array_equal(rec, np.stack([steps["is_key"], steps["n_src"], steps["iterations"]], axis=1))
    assert int([l for l in lines if l.startswith("keys")][0].split()[1]) == n_key >= 2
    assert [int(v) for v in [l for l in lines if l.startswith("firstmap")][0].split()[1:]] == steps["is_key"].tolist()
    assert np.array_equal(loam[:, 0], (scan_t * 1e9).astype(np.int64).astype(np.float64)) and np.array_equal(loam[:, 1:4], poses[:, :3, 3])
    for k in range(n):                                                                   # q w x y z of the pose's rotation
        w, x, y, z = loam[k, 4:]
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.abs(Rq - poses[k, :3, :3]).max() <= 1e-6                               # (the float rotation of an NDT pose is orthonormal to float rounding)
