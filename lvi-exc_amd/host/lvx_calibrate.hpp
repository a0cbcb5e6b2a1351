// lvx_calibrate.hpp — the reference's offline calibration schedule over the lvx C ABI (header-only, no HIP types).
//
// What it mirrors (src/lvi_exc/test/lvi_initialize_surfel_orb.cpp): LIinitializer's stage machine
//     Initialization()      -> TrajectoryManagerLVI::initialSO3TrajWithGyro            (trajectory_manager_lvi.cpp:43-62)        Solve #0
//     DataAssociation()     -> undistortScanInMap, ndt grid of the map cloud, setSurfelMap, getAssociation per scan,
//                              averageTimeDownSmaple                                   (:1169-1210)
//     BatchOptimization() / Refinement()  -> trajInitFromSurfel                        (:1212-1243, trajectory_manager_lvi.cpp:311-351)   Solve #1, #1', ...
//     LVI refinement        -> trajInitFromLVIdata(frames, surfels)                    (trajectory_manager_lvi.cpp:138-195)       Solve #2
//     camera refinement     -> associateVisualPointsWithPlanes + trajInitFromLVIdata(frames, surfels, lm_splane)  (:197-257)     Solve #3
// DataAssociation is ONE device-resident call (lvx_data_association: de-skew of every scan into the map frame, voxel grid of the map cloud, surfel
// extraction, association of every scan, chronological SurfelPoint emission); the raw scans are handed to the context once (lvx_set_scans).
// The FIRST DataAssociation (InitializationDone branch, :1175-1178) takes its map from per-scan odometry poses — LOAM's, ReadPoseGT (lvx_loaders.hpp) — exactly as the
// reference with using_loam: CalibrateInput::loam + scan_stamps select it (lvx_data_association_poses: rotation-only de-skew with the SO3 spline of Solve #0, key-scan
// map, surfel map, association), so a recorded dataset starts from the reference's initial state (identity rotations, zero positions) with nothing hand-fitted.
// CalibrateOptions::init_lidar_rotation adds Initialization()'s EstimateRotation loop (calib_helper_lvi.cpp:55-89) after Solve #0: the LiDAR mounting rotation itself then
// starts from the odometry (lvx_estimate_rotation), e.g. for a LiDAR turned 90 degrees against the IMU, which the surfel stage alone does not recover from identity.
// CalibrateOptions::lidar_odometry: without a pose file (CalibrateInput::loam empty) the odometry poses are LiDAROdometry's own NDT scan-to-map registration
// (using_loam = false: lvx_lidar_odometry over the raw scans, as CalibrHelperLVI::Initialization feeds them, calib_helper_lvi.cpp:55-60); the first map and the rotation
// initialisation then take their poses from it (RunLidarOdometry).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lvx.h"
#include "lvx_loaders.hpp"

namespace lvx_host {

struct CalibrateInput {
  double t0 = 0, dt = 0.02; int n_knots = 0;                       // spline meta
  lvx_pinhole camera{};
  std::vector<double> imu_t, gyro, acc;                            // [n], [n][3], [n][3]
  int H = 0, W = 0;                                                // organised scans
  std::vector<std::vector<lvx_point_xyzit>> scans;                 // raw LiDAR scans, [H * W] each (row-major h * W + w), per-point timestamps
  // ... or, instead of `scans`, the recording's VLP-16 packets (velodyne_msgs/VelodyneScan: [n][1206] bytes back to back; scan s = packets [vlp16_packet_offsets[s],
  // vlp16_packet_offsets[s + 1]); vlp16_stamps[s] = the message's header stamp): the device unpacks them (lvx_set_scans_vlp16 = LioDataset's VelodyneCorrection::unpack_scan),
  // H becomes 16, W 24 x the longest scan (or the W given here, if larger), and scan_stamps defaults to vlp16_stamps
  std::vector<uint8_t> vlp16_packets; std::vector<int32_t> vlp16_packet_offsets; std::vector<double> vlp16_stamps;
  double map_time = 0;
  // first map from odometry poses (optional): the scans' header stamps and the LOAM pose file (ReadPoseGT); simulation = the reference's flag: a scan takes the pose with
  // EXACTLY its stamp (loam_poses_map_.find, :1283-1290) instead of the nearest of the poses idx - 5 .. idx + 4 (findAssociatedPose, :1246-1260)
  std::vector<double> scan_stamps; LoamPoses loam; bool simulation = true;
  // ORB results (lvx_loaders.hpp: LoadOrbResults): landmark table + observations
  std::vector<double> lm_uv, lm_t0; std::vector<int32_t> obs_landmark; std::vector<double> obs_uv, obs_t0;
};
struct CalibrateOptions {
  bool solve0_so3_from_gyro = false;     // Initialization()
  bool init_lidar_rotation = false;      // Initialization()'s EstimateRotation loop after Solve #0 (calib_helper_lvi.cpp:55-89), when odometry poses are present: q_LtoI from the odometry (lvx_estimate_rotation)
  bool lidar_odometry = false;           // no CalibrateInput::loam: the odometry poses come from lvx_lidar_odometry over the scans (feedScan with using_loam = false)
  int refine_iterations = 2;             // DataAssociation + trajInitFromSurfel rounds (the reference runs batch + 2 refinements)
  bool lvi_stage = true;                 // trajInitFromLVIdata
  bool camera_surfel_stage = false;      // the third stage with camera-landmark-to-surfel blocks
  float ndt_resolution = 0.5f;           // lvi.yaml:26
  double plane_lambda = 0.7, fit_threshold = 0.05; int min_leaf_points = 10, min_inliers = 20;
  double first_map_plane_lambda = 0.6, key_scan_dist = 0.2, key_scan_angle_deg = 5.0;   // plane_lambda_ of the constructor (:127); checkKeyScan (lidar_odometry.cpp:121-122)
  double associated_radius = 0.05; int selected_per_ring = 2, downsample_step = 10;
  double w_gyro = 28, w_acc = 18, w_surfel = 10, w_cam = 5, w_cam_surfel = 30;   // SetCalibWeights (lvi_initialize_surfel_orb.cpp:904-928)
  double w_lidar_pos = 1;                // global_opt_pos_weight (calibration.hpp:68): the LiDAR odometry position blocks of RunLidarPoses
  bool opt_time_offset = false;
  bool keep_history = false, keep_clouds = false;   // AssociationRecord per DataAssociation round (tests, diagnostics)
  bool device_handoff = false;           // trajInitFromSurfel / trajInitFromLVIdata take their surfel blocks with lvx_set_surfel_from_association: the SurfelPoint list stays on the device (fetched only for keep_history), the planes are fetched only for the camera-surfel stage
  bool error_statistics = false;   // printErrorStatistics("Before optimization") / ("After optimization") around every stage's solve (trajectory_manager_lvi.cpp:339-342): StageReport::stats_before / stats_after
  bool covariance = false;         // lvx_calibration_covariance at every stage's final state (one more LVX_EVAL_NORMAL_EQ evaluation per stage): StageReport::covariance
  double covariance_radius = 1e8;  // the radius of the damped system the covariance belongs to (what it means)
  double trajectory_covariance_step = 0;   // seconds, 0 = off: lvx_trajectory_covariance of the pose at every stage's final state, sampled with SampleTimes over the IMU span (the same evaluation as `covariance`, the same radius): StageReport::trajectory_sigma
  int trajectory_covariance_frame = LVX_FRAME_LIDAR;   // the frame of those poses.  A stage that locks the trajectory and a sensor's extrinsics (the camera-surfel stage: LiDAR) reports exact zeros for that sensor's frame
  bool landmark_covariance = false;   // lvx_landmark_covariance of every landmark at every stage's final state (the same evaluation as `covariance`, the same radius): StageReport::landmark_sigma.  A stage that holds the landmarks constant carries no record
  int verbose = 1;
};
// lvx_landmark_covariance over a list of landmarks: var_rho / sigma_rho [n] (inverse depth), point [n][3] (world), point_cov [n][9], valid [n]; rho [n] the inverse depths
// themselves where the caller gave the state (empty otherwise)
struct LandmarkUncertainty { double radius = 0; std::vector<int32_t> ids; std::vector<double> rho, var_rho, sigma_rho, point, point_cov; std::vector<uint8_t> valid; };
// lvx_trajectory_covariance over a list of times: cov [n][36], sigma [n][6] (metres, RADIANS), valid [n]
struct TrajectoryUncertainty { int frame = 0; double radius = 0; std::vector<double> t, cov, sigma; std::vector<uint8_t> valid; };
struct StageReport { std::string name; lvx_lm_summary lm; int n_planes = 0, n_surfel_points = 0, n_cam_surfel = 0;
                     std::vector<double> cost_history, radius_history; std::vector<int32_t> accepted;   // per-iteration trace of the stage's solve (lvx_lm_get_history)
                     std::vector<double> state_in;   // the state the stage's solve started from (CalibrateOptions::keep_history)
                     bool has_stats = false; lvx_error_stats stats_before{}, stats_after{};   // CalibrateOptions::error_statistics: lvx_error_statistics at the state the solve started from / ended at
                     int init_prefix = -1; lvx_rotinit_result init{};   // the "Initialization" report (CalibrateOptions::init_lidar_rotation): index into InitializationPrefixes and the record that passed
                     bool has_covariance = false; lvx_calib_cov covariance{};   // CalibrateOptions::covariance: the record at the state the stage's solve ended at (false: the option is off, or the call reported LVX_E_NOTPD)
                     bool has_trajectory_sigma = false; TrajectoryUncertainty trajectory_sigma;   // CalibrateOptions::trajectory_covariance_step: pose sigmas (trajectory_covariance_frame) along the spline at the stage's final state (false: off, or LVX_E_NOTPD)
                     bool has_landmark_sigma = false; LandmarkUncertainty landmark_sigma;   // CalibrateOptions::landmark_covariance: every landmark at the stage's final state (false: off, the stage holds the landmarks constant, or LVX_E_NOTPD)
                     int n_lidar_poses = 0; lvx_family_stats lidar_pos_before{}, lidar_pos_after{}; };   // trajInitFromLidarPose: blocks attached; with error_statistics, lvx_lidar_pose_statistics around the solve
// what one DataAssociation round produced (kept when CalibrateOptions::keep_history): the state it ran at, the surfel map, the full SurfelPoint list and —
// keep_clouds — the de-skewed scans [n_scans][H][W][4]
struct AssociationRecord { std::vector<double> state; std::vector<lvx_surfel_plane> planes; std::vector<double> pt, pt_map, t; std::vector<int32_t> plane; std::vector<float> scans_in_map; };

// LIinitializer::ReprojectPointCloudToImage's image choice (lvi_initialize_surfel_orb.cpp:1319-1327): per scan the FIRST image with img_t > scan_t and |img_t - scan_t| < 0.05,
// or -1
// The calibration scalars c = tangent - 6 N of lvx_calib_cov, by name
inline const char* CalibScalarName(int c) {
  static const char* const names[22] = {"gravity.x", "gravity.y", "acc_bias.x", "acc_bias.y", "acc_bias.z", "gyro_bias.x", "gyro_bias.y", "gyro_bias.z",
                                        "lidar_rot.x", "lidar_rot.y", "lidar_rot.z", "lidar_pos.x", "lidar_pos.y", "lidar_pos.z", "lidar_tau",
                                        "cam_rot.x", "cam_rot.y", "cam_rot.z", "cam_pos.x", "cam_pos.y", "cam_pos.z", "cam_tau"};
  return c >= 0 && c < 22 ? names[c] : "?";
}
// What a user reads off a lvx_calib_cov, one line per sensor whose extrinsics are (partly) free and one for the spectrum:
//   [LiDAR]  rotation std (deg): a b c; translation std (m): x y z            (rotation: 2 sigma 180 / pi — the tangent of a quaternion block is a half-angle; a constant scalar prints 0)
//   [Camera] ...
//   [Spectrum] smallest scaled eigenvalue: v (radius r); dominant scalar: name (c = k)
// The covariance is that of the damped system at the record's radius; an eigenvalue at 1e-6 / radius is a direction no residual row touches.
inline std::string FormatCalibrationUncertainty(const lvx_calib_cov& r) {
  std::string out;
  char buf[256];
  const double deg = 2.0 * 180.0 / 3.14159265358979323846;
  const struct { const char* tag; int c0; } sensors[2] = {{"[LiDAR] ", 8}, {"[Camera]", 15}};
  for (const auto& sn : sensors) {
    bool any = false;
    for (int k = 0; k < r.n_free; ++k) any = any || (r.free_index[k] >= sn.c0 && r.free_index[k] < sn.c0 + 6);
    if (!any) continue;
    const double* s = r.sigma + sn.c0;
    std::snprintf(buf, sizeof buf, "%s rotation std (deg): %.6e %.6e %.6e; translation std (m): %.6e %.6e %.6e\n", sn.tag, deg * s[0], deg * s[1], deg * s[2], s[3], s[4], s[5]);
    out += buf;
  }
  if (r.n_free > 0) {
    int dom = 0;
    for (int i = 1; i < r.n_free; ++i) if (std::fabs(r.info_vec[i * 22]) > std::fabs(r.info_vec[dom * 22])) dom = i;
    std::snprintf(buf, sizeof buf, "[Spectrum] smallest scaled eigenvalue: %.6e (radius %.6e); dominant scalar: %s (c = %d)\n", r.info_eig[0], r.radius, CalibScalarName(r.free_index[dom]), (int)r.free_index[dom]);
    out += buf;
  }
  return out;
}

// The same for a lvx_joint_calib_cov (lvx_calibration_covariance_shared: several sequences, shared extrinsics): the [LiDAR] / [Camera] / [Spectrum] lines of the JOINT
// problem, and per sensor this sequence's fraction of the diagonal of the joint information of the shared scalars, own_info_kk / (sum_q w_q V_kq^2):
//   [Share] LiDAR  rotation: a b c; translation: x y z                        (in [0, 1]; the fractions of all sequences and the LM prior add up to 1; a constant scalar prints 0)
inline std::string FormatJointCalibrationUncertainty(const lvx_joint_calib_cov& r) {
  std::string out;
  char buf[256];
  const double deg = 2.0 * 180.0 / 3.14159265358979323846;
  const struct { const char* tag; const char* name; int c0; } sensors[2] = {{"[LiDAR] ", "LiDAR ", 8}, {"[Camera]", "Camera", 15}};
  const int ns = r.n_shared_free;
  for (const auto& sn : sensors) {
    bool any = false;
    for (int k = 0; k < r.n_free; ++k) any = any || (r.free_index[k] >= sn.c0 && r.free_index[k] < sn.c0 + 6);
    if (!any) continue;
    const double* s = r.sigma + sn.c0;
    std::snprintf(buf, sizeof buf, "%s rotation std (deg): %.6e %.6e %.6e; translation std (m): %.6e %.6e %.6e\n", sn.tag, deg * s[0], deg * s[1], deg * s[2], s[3], s[4], s[5]);
    out += buf;
    double share[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ns; ++i) {
      const int slot = r.shared_free_slot[i], j = slot - (sn.c0 - 8);
      if (j < 0 || j >= 6) continue;
      double m = 0.0;
      for (int q = 0; q < ns; ++q) m += r.info_eig[q] * r.info_vec[i * 14 + q] * r.info_vec[i * 14 + q];
      share[j] = r.own_info[slot * 14 + slot] / m;
    }
    std::snprintf(buf, sizeof buf, "[Share] %s rotation: %.6e %.6e %.6e; translation: %.6e %.6e %.6e\n", sn.name, share[0], share[1], share[2], share[3], share[4], share[5]);
    out += buf;
  }
  if (ns > 0) {
    int dom = 0;
    for (int i = 1; i < ns; ++i) if (std::fabs(r.info_vec[i * 14]) > std::fabs(r.info_vec[dom * 14])) dom = i;
    const int c = 8 + r.shared_free_slot[dom];
    std::snprintf(buf, sizeof buf, "[Spectrum] smallest scaled eigenvalue: %.6e (radius %.6e); dominant scalar: %s (c = %d)\n", r.info_eig[0], r.radius, CalibScalarName(c), c);
    out += buf;
  }
  return out;
}

inline std::vector<int32_t> MatchScanImages(const std::vector<double>& scan_t, const std::vector<double>& image_t) {
  std::vector<int32_t> idx(scan_t.size(), -1);
  for (size_t j = 0; j < scan_t.size(); ++j)
    for (size_t i = 0; i < image_t.size(); ++i)
      if (image_t[i] > scan_t[j] && std::fabs(image_t[i] - scan_t[j]) < 0.05) { idx[j] = (int32_t)i; break; }
  return idx;
}
// RenderMap's candidate images (:729-733): i = 50, 50 + step, ... with step = size / 10 (a step of 0 — fewer than 10 images — would never advance: one candidate then)
inline std::vector<int32_t> RenderCandidates(size_t n_images) {
  std::vector<int32_t> c;
  const size_t step = n_images / 10;
  for (size_t i = 50; i < n_images && c.size() < (size_t)LVX_RENDER_MAX_IMAGES; i += step) { c.push_back((int32_t)i); if (step == 0) break; }
  return c;
}
// pcl::io::savePCDFileASCII of a PointXYZRGB cloud (:804): fields x y z rgb, unorganised (WIDTH n, HEIGHT 1).  The packed colour (a << 24 | r << 16 | g << 8 | b) is
// written as PCL >= 1.9 does, an unsigned integer with TYPE U (older writers print the same four bytes as a float, which is a NaN pattern for a = 255 and does not
// survive a text round trip); pcl::io::loadPCDFile reads both.
inline bool WritePcdAscii(const std::string& path, const std::vector<lvx_point_xyzrgb>& cloud) {
  std::FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  std::fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA ascii\n",
               cloud.size(), cloud.size());
  for (const lvx_point_xyzrgb& p : cloud) {
    const uint32_t rgb = (uint32_t)p.b | ((uint32_t)p.g << 8) | ((uint32_t)p.r << 16) | ((uint32_t)p.a << 24);
    std::fprintf(f, "%.9g %.9g %.9g %u\n", p.x, p.y, p.z, (unsigned)rgb);
  }
  return std::fclose(f) == 0;
}
struct RenderResult { std::vector<lvx_point_xyzrgb> cloud; std::vector<int32_t> candidates, valid; int64_t n_colored = 0; };

// ---- trajectory queries (lvx_sample_trajectory / lvx_compare_poses): what LIinitializer::PublishTrajectory (lvi_initialize_surfel_orb.cpp:834-902) builds on the host ----
// its sampling loop (:875-891): `t = begin; while (t < end) { ...; t += step; }` — the ACCUMULATED sum, not begin + k * step
inline std::vector<double> SampleTimes(double t_begin, double t_end, double step) {
  std::vector<double> t;
  if (!(step > 0.0)) return t;
  for (double x = t_begin; x < t_end; x += step) t.push_back(x);
  return t;
}
inline void ThrowOnError(lvx_ctx* ctx, int rc) {
  if (rc == LVX_OK) return;
  const std::string msg = ctx ? lvx_last_error(ctx) : "lvx error";
  if (rc == LVX_E_RANGE) throw std::range_error(msg);
  throw std::runtime_error(msg + " (lvx error " + std::to_string(rc) + ")");
}
// arrays [n][3] / [n][4] (x, y, z, w); acceleration stays empty for a sensor frame (lvx.h); an invalid sample holds zeros
struct TrajectorySamples { std::vector<double> t, position, velocity, acceleration, orientation_xyzw, angular_velocity; std::vector<int32_t> valid; };
inline TrajectorySamples SampleTrajectory(lvx_ctx* ctx, const std::vector<double>& state, int frame, const std::vector<double>& times) {
  TrajectorySamples r; r.t = times;
  const size_t n = times.size();
  if (n == 0) return r;
  r.position.assign(3 * n, 0.0); r.velocity.assign(3 * n, 0.0); r.orientation_xyzw.assign(4 * n, 0.0); r.angular_velocity.assign(3 * n, 0.0); r.valid.assign(n, 0);
  if (frame == LVX_FRAME_TRAJECTORY) r.acceleration.assign(3 * n, 0.0);
  lvx_traj_samples o{r.position.data(), r.velocity.data(), r.acceleration.empty() ? nullptr : r.acceleration.data(), r.orientation_xyzw.data(), r.angular_velocity.data(), r.valid.data()};
  ThrowOnError(ctx, lvx_sample_trajectory(ctx, state.data(), frame, (int)n, times.data(), &o));
  return r;
}
// lvx_trajectory_covariance at the normal equations (and the state) of the context's last LVX_EVAL_NORMAL_EQ evaluation; opts = nullptr: the defaults
inline TrajectoryUncertainty TrajectoryCovariance(lvx_ctx* ctx, int frame, const std::vector<double>& times, const lvx_traj_cov_options* opts = nullptr) {
  TrajectoryUncertainty r; r.frame = frame; r.t = times;
  lvx_traj_cov_options o; lvx_traj_cov_default_options(&o);
  if (opts) o = *opts;
  r.radius = o.radius;
  const size_t n = times.size();
  if (n == 0) return r;
  r.cov.assign(36 * n, 0.0); r.sigma.assign(6 * n, 0.0); r.valid.assign(n, 0);
  lvx_traj_cov out{r.cov.data(), r.sigma.data(), nullptr, nullptr, r.valid.data()};
  ThrowOnError(ctx, lvx_trajectory_covariance(ctx, &o, frame, (int)n, times.data(), &out));
  return r;
}
// What a user reads off it, two lines: the worst and the median position / rotation sigma (norm of the three standard deviations) over the valid samples and the
// time of the worst.  The sigmas belong to the damped system at the record's radius, as those of FormatCalibrationUncertainty.
//   [Trajectory] position std (m): worst a at t = ..., median b (n valid samples, radius r)
//   [Trajectory] rotation std (deg): worst a at t = ..., median b
inline std::string FormatTrajectoryUncertainty(const TrajectoryUncertainty& r) {
  std::vector<double> sp, sr; std::vector<size_t> at;
  for (size_t i = 0; i < r.valid.size(); ++i) if (r.valid[i]) {
    const double* s = r.sigma.data() + 6 * i;
    sp.push_back(std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])); sr.push_back(std::sqrt(s[3] * s[3] + s[4] * s[4] + s[5] * s[5])); at.push_back(i);
  }
  if (sp.empty()) return "[Trajectory] no valid sample\n";
  const size_t wp = (size_t)(std::max_element(sp.begin(), sp.end()) - sp.begin()), wr = (size_t)(std::max_element(sr.begin(), sr.end()) - sr.begin());
  auto median = [](std::vector<double> v) { std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end()); return v[v.size() / 2]; };
  const double deg = 180.0 / 3.14159265358979323846;
  char buf[512];
  std::snprintf(buf, sizeof buf, "[Trajectory] position std (m): worst %.6e at t = %.6f, median %.6e (%d valid samples, radius %.6e)\n[Trajectory] rotation std (deg): worst %.6e at t = %.6f, median %.6e\n",
                sp[wp], r.t[at[wp]], median(sp), (int)sp.size(), r.radius, deg * sr[wr], r.t[at[wr]], deg * median(sr));
  return buf;
}
// lvx_landmark_covariance at the normal equations (and the state) of the context's last LVX_EVAL_NORMAL_EQ evaluation; ids empty: every landmark in order; opts = nullptr:
// the defaults; state (the one of that evaluation): fills LandmarkUncertainty::rho, which FormatLandmarkUncertainty divides by
inline LandmarkUncertainty LandmarkCovariance(lvx_ctx* ctx, const std::vector<int32_t>& ids = {}, const lvx_landmark_cov_options* opts = nullptr, const std::vector<double>* state = nullptr) {
  LandmarkUncertainty r; r.ids = ids;
  lvx_landmark_cov_options o; lvx_landmark_cov_default_options(&o);
  if (opts) o = *opts;
  r.radius = o.radius;
  lvx_layout lo{};
  ThrowOnError(ctx, lvx_get_layout(ctx, &lo));
  if (ids.empty()) { r.ids.resize((size_t)std::max(lo.n_landmarks, 0)); for (size_t i = 0; i < r.ids.size(); ++i) r.ids[i] = (int32_t)i; }
  const size_t n = r.ids.size();
  if (n == 0) return r;
  r.var_rho.assign(n, 0.0); r.sigma_rho.assign(n, 0.0); r.point.assign(3 * n, 0.0); r.point_cov.assign(9 * n, 0.0); r.valid.assign(n, 0);
  lvx_landmark_cov out{r.var_rho.data(), r.sigma_rho.data(), r.point.data(), r.point_cov.data(), nullptr, nullptr, r.valid.data()};
  ThrowOnError(ctx, lvx_landmark_covariance(ctx, &o, (int)n, ids.empty() ? nullptr : r.ids.data(), &out));
  if (state) { r.rho.resize(n); for (size_t i = 0; i < n; ++i) r.rho[i] = state->at(7 * (size_t)lo.n_knots + 32 + (size_t)r.ids[i]); }
  return r;
}
// lvx_map_point_covariance over LiDAR points [n][3] measured at `times`: the point in the map frame [n][3], cov [n][9], sigma [n][3] (metres), sigma_max [n], valid [n];
// dirs [n][3] (optional, e.g. unit plane normals in the map frame): var_dir [n] = dir^T cov dir, the predicted variance of a surfel row
struct MapPointUncertainty { double radius = 0; std::vector<double> point, cov, sigma, sigma_max, var_dir; std::vector<uint8_t> valid; };
inline MapPointUncertainty MapPointCovariance(lvx_ctx* ctx, const std::vector<double>& points, const std::vector<double>& times, const std::vector<double>& dirs = {},
                                              const lvx_point_cov_options* opts = nullptr) {
  const size_t n = times.size();
  if (points.size() != 3 * n || (!dirs.empty() && dirs.size() != 3 * n)) throw std::invalid_argument("MapPointCovariance: three coordinates (and direction components) per time");
  MapPointUncertainty r;
  lvx_point_cov_options o; lvx_point_cov_default_options(&o);
  if (opts) o = *opts;
  r.radius = o.radius;
  if (n == 0) return r;
  r.point.assign(3 * n, 0.0); r.cov.assign(9 * n, 0.0); r.sigma.assign(3 * n, 0.0); r.sigma_max.assign(n, 0.0); r.valid.assign(n, 0);
  if (!dirs.empty()) r.var_dir.assign(n, 0.0);
  lvx_point_cov out{r.point.data(), r.cov.data(), r.sigma.data(), r.sigma_max.data(), dirs.empty() ? nullptr : r.var_dir.data(), nullptr, nullptr, r.valid.data()};
  ThrowOnError(ctx, lvx_map_point_covariance(ctx, &o, (int)n, points.data(), times.data(), dirs.empty() ? nullptr : dirs.data(), &out));
  return r;
}
// What a user reads off it, one line: the median and the largest sigma_max over the valid points, in millimetres
//   [Map] point std (mm): median a, worst b at point i (n valid of m, radius r)
inline std::string FormatMapPointUncertainty(const MapPointUncertainty& r) {
  std::vector<double> s; std::vector<size_t> at;
  for (size_t i = 0; i < r.valid.size(); ++i) if (r.valid[i]) { s.push_back(r.sigma_max[i]); at.push_back(i); }
  if (s.empty()) return "[Map] no valid point\n";
  const size_t w = (size_t)(std::max_element(s.begin(), s.end()) - s.begin());
  const double worst = s[w];
  std::nth_element(s.begin(), s.begin() + s.size() / 2, s.end());
  char buf[200];
  std::snprintf(buf, sizeof buf, "[Map] point std (mm): median %.4g, worst %.4g at point %zu (%zu valid of %zu, radius %g)\n", 1e3 * s[s.size() / 2], 1e3 * worst, at[w], at.size(),
                r.valid.size(), r.radius);
  return buf;
}
// lvx_projection_covariance over map points [n][4] float (x, y, z, intensity; the LiDAR frame at t_map, as lvx_render_map takes them) and the images taken at
// image_times: per point uv [n][2], cov [n][4] (px^2), sigma [n][2], sigma_max [n] (px), image [n] (-1: none), status [n] (0 skipped, 1 outside every image, 2
// projected); per image pose_cov [n_images][144] over (camera dp, dphi; LiDAR dp, dphi) and image_valid.  The map point is taken as given (lvx.h).
struct PixelUncertainty {
  double radius = 0; std::vector<double> uv, cov, sigma, sigma_max, pose_cov; std::vector<int32_t> image, image_valid; std::vector<uint8_t> status;
};
inline PixelUncertainty ProjectionCovariance(lvx_ctx* ctx, const std::vector<float>& map_xyzi, const std::vector<double>& image_times, const lvx_proj_cov_options* opts = nullptr) {
  if (map_xyzi.size() % 4 != 0) throw std::invalid_argument("ProjectionCovariance: four floats per map point");
  const size_t n = map_xyzi.size() / 4, ni = image_times.size();
  PixelUncertainty r;
  lvx_proj_cov_options o; lvx_proj_cov_default_options(&o);
  if (opts) o = *opts;
  r.radius = o.radius;
  if (n == 0) return r;
  r.uv.assign(2 * n, 0.0); r.cov.assign(4 * n, 0.0); r.sigma.assign(2 * n, 0.0); r.sigma_max.assign(n, 0.0); r.image.assign(n, -1); r.status.assign(n, 0);
  r.pose_cov.assign(144 * ni, 0.0); r.image_valid.assign(ni, 0);
  const lvx_proj_cov_images img{r.pose_cov.data(), nullptr, nullptr, r.image_valid.data()};
  const lvx_proj_cov out{r.uv.data(), r.cov.data(), r.sigma.data(), r.sigma_max.data(), r.image.data(), r.status.data()};
  ThrowOnError(ctx, lvx_projection_covariance(ctx, &o, (int)n, map_xyzi.data(), (int)ni, image_times.data(), &img, &out));
  return r;
}
// What a user reads off it, one line: the median, the 95 % quantile and the largest sigma_max over the projected points, in pixels
//   [Map] pixel std (px): median a, 95 % b, max c at point i (n projected of m, k images, radius r)
inline std::string FormatProjectionUncertainty(const PixelUncertainty& r) {
  std::vector<double> s; std::vector<size_t> at;
  for (size_t i = 0; i < r.status.size(); ++i) if (r.status[i] == 2) { s.push_back(r.sigma_max[i]); at.push_back(i); }
  if (s.empty()) return "[Map] no projected point\n";
  const size_t w = (size_t)(std::max_element(s.begin(), s.end()) - s.begin());
  const double worst = s[w];
  std::sort(s.begin(), s.end());
  char buf[240];
  std::snprintf(buf, sizeof buf, "[Map] pixel std (px): median %.4g, 95 %% %.4g, max %.4g at point %zu (%zu projected of %zu, %zu images, radius %g)\n", s[s.size() / 2],
                s[(size_t)(0.95 * (double)(s.size() - 1))], worst, at[w], at.size(), r.status.size(), r.image_valid.size(), r.radius);
  return buf;
}
// What a user reads off it, one line: the median and the largest relative depth sigma, sigma_rho / |rho| (to first order the relative sigma of the depth 1 / rho), over
// the valid landmarks, and which landmark is the worst.  Without LandmarkUncertainty::rho the sigmas of the inverse depth themselves.
//   [Landmarks] relative depth std: median a, max b at landmark l (n valid of m, radius r)
inline std::string FormatLandmarkUncertainty(const LandmarkUncertainty& r) {
  std::vector<double> rel; std::vector<size_t> at;
  const bool have_rho = r.rho.size() == r.valid.size();
  for (size_t i = 0; i < r.valid.size(); ++i) if (r.valid[i]) { rel.push_back(have_rho ? r.sigma_rho[i] / std::fabs(r.rho[i]) : r.sigma_rho[i]); at.push_back(i); }
  if (rel.empty()) return "[Landmarks] no valid landmark\n";
  const size_t w = (size_t)(std::max_element(rel.begin(), rel.end()) - rel.begin());
  std::vector<double> v = rel;
  std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
  char buf[320];
  std::snprintf(buf, sizeof buf, "[Landmarks] %s std: median %.6e, max %.6e at landmark %d (%d valid of %d, radius %.6e)\n", have_rho ? "relative depth" : "inverse depth",
                v[v.size() / 2], rel[w], (int)r.ids[at[w]], (int)rel.size(), (int)r.valid.size(), r.radius);
  return buf;
}
struct PoseComparison { lvx_pose_errors errors{}; std::vector<double> abs_trans, abs_rot; };
// reference poses as ReadPoseGT returns them (stamp_ns, p, q w x y z): the stamps become stamp_ns * 1e-9 seconds
inline PoseComparison ComparePoses(lvx_ctx* ctx, const std::vector<double>& state, int frame, const std::vector<PoseStamped>& poses, int align) {
  PoseComparison r;
  const size_t n = poses.size();
  if (n == 0) return r;
  std::vector<double> t(n), q(4 * n), p(3 * n);
  for (size_t i = 0; i < n; ++i) {
    t[i] = static_cast<double>(poses[i].stamp_ns) * 1e-9;
    for (int k = 0; k < 3; ++k) { p[3 * i + k] = poses[i].p[k]; q[4 * i + k] = poses[i].q_wxyz[1 + k]; }
    q[4 * i + 3] = poses[i].q_wxyz[0];
  }
  r.abs_trans.assign(n, 0.0); r.abs_rot.assign(n, 0.0);
  ThrowOnError(ctx, lvx_compare_poses(ctx, state.data(), frame, (int)n, t.data(), q.data(), p.data(), align, &r.errors, r.abs_trans.data(), r.abs_rot.data()));
  return r;
}
// LOAM's pose file, one line per pose: `stamp_ns tx ty tz qw qx qy qz`, 17 significant digits so that ReadPoseGT (lvx_loaders.hpp) reads back the same doubles.
// p [n][3], q [n][4] (x, y, z, w)
inline bool WritePoseFile(const std::string& path, const std::vector<int64_t>& stamps_ns, const std::vector<double>& p, const std::vector<double>& q_xyzw) {
  if (p.size() != 3 * stamps_ns.size() || q_xyzw.size() != 4 * stamps_ns.size()) return false;
  std::FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  for (size_t i = 0; i < stamps_ns.size(); ++i)
    std::fprintf(f, "%lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)stamps_ns[i], p[3 * i], p[3 * i + 1], p[3 * i + 2], q_xyzw[4 * i + 3], q_xyzw[4 * i], q_xyzw[4 * i + 1],
                 q_xyzw[4 * i + 2]);
  return std::fclose(f) == 0;
}

// ---- rotation initialisation (lvx_estimate_rotation): CalibrHelperLVI::Initialization's loop around InertialInitializer::EstimateRotation (calib_helper_lvi.cpp:55-89) ----
// the odometry sizes at which the reference tries (:62-64): 30, 40, ... <= n
inline std::vector<int32_t> InitializationPrefixes(int n) {
  std::vector<int32_t> p;
  for (int k = 30; k <= n; k += 10) p.push_back(k);
  return p;
}
// records [taus][prefixes]; first_ok[tau]: the first prefix that passes (-1: none — the reference's "[Initialization] fails")
struct RotationInit {
  std::vector<int32_t> prefix_len; std::vector<double> taus; std::vector<lvx_rotinit_result> results; std::vector<int32_t> first_ok;
  const lvx_rotinit_result& at(size_t tau, size_t prefix) const { return results[tau * prefix_len.size() + prefix]; }
};
// odometry stamps t [n] and rotations q [n][4] (x, y, z, w) on the reference's schedule, for every shift of `taus` (empty: the reference's single shift of 0).  Fewer than
// 30 poses: nothing is tried, first_ok = -1.
inline RotationInit EstimateRotation(lvx_ctx* ctx, const std::vector<double>& state, const std::vector<double>& t, const std::vector<double>& q_xyzw, const std::vector<double>& taus = {},
                                     const lvx_rotinit_options* opt = nullptr) {
  RotationInit r; r.prefix_len = InitializationPrefixes((int)t.size()); r.taus = taus.empty() ? std::vector<double>{0.0} : taus;
  r.first_ok.assign(r.taus.size(), -1);
  if (r.prefix_len.empty()) return r;
  if (q_xyzw.size() != 4 * t.size()) throw std::invalid_argument("EstimateRotation: one quaternion per stamp");
  r.results.assign(r.taus.size() * r.prefix_len.size(), lvx_rotinit_result{});
  ThrowOnError(ctx, lvx_estimate_rotation(ctx, state.data(), (int)t.size(), t.data(), q_xyzw.data(), (int)r.prefix_len.size(), r.prefix_len.data(), (int)r.taus.size(), r.taus.data(), opt,
                                          r.results.data(), r.first_ok.data()));
  return r;
}
// odometry poses as ReadPoseGT returns them (stamp_ns, p, q w x y z)
inline RotationInit EstimateRotation(lvx_ctx* ctx, const std::vector<double>& state, const std::vector<PoseStamped>& poses, const std::vector<double>& taus = {}) {
  std::vector<double> t(poses.size()), q(4 * poses.size());
  for (size_t i = 0; i < poses.size(); ++i) {
    t[i] = static_cast<double>(poses[i].stamp_ns) * 1e-9;
    for (int k = 0; k < 3; ++k) q[4 * i + k] = poses[i].q_wxyz[1 + k];
    q[4 * i + 3] = poses[i].q_wxyz[0];
  }
  return EstimateRotation(ctx, state, t, q, taus);
}
// Eigen's Quaternion(Matrix3d) on the rotation block of a row-major 4 x 4 pose (x, y, z, w)
inline void QuaternionOfPose(const double T[16], double q[4]) {
  const double m[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  double tr = m[0][0] + m[1][1] + m[2][2];
  if (tr > 0.0) {
    double s = std::sqrt(tr + 1.0); q[3] = 0.5 * s; s = 0.5 / s;
    q[0] = (m[2][1] - m[1][2]) * s; q[1] = (m[0][2] - m[2][0]) * s; q[2] = (m[1][0] - m[0][1]) * s;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0); q[i] = 0.5 * s; s = 0.5 / s;
    q[3] = (m[k][j] - m[j][k]) * s; q[j] = (m[j][i] + m[i][j]) * s; q[k] = (m[k][i] + m[i][k]) * s;
  }
}

// ---- LiDAR odometry (lvx_lidar_odometry): LiDAROdometry::feedScan(using_loam = false) over the scans of lvx_set_scans, the poses in the form ReadPoseGT returns ----
// `loam.all`: one pose per scan under its header stamp ((int64_t)(stamp * 1e9), what PoseOfScan looks up), q = Eigen's Quaternion(Matrix3d) of the pose; `loam.key`: the
// key scans; pose16 [n][16] row-major scan -> map and the step records as the call wrote them
struct LidarOdometry { LoamPoses loam; std::vector<double> pose16; std::vector<lvx_odom_step> steps; int32_t n_key = 0; };
inline LidarOdometry RunLidarOdometry(lvx_ctx* ctx, const std::vector<double>& scan_stamps, const lvx_odom_options* opt = nullptr) {
  LidarOdometry r;
  const size_t n = scan_stamps.size();
  if (n == 0) return r;
  r.pose16.assign(16 * n, 0.0); r.steps.assign(n, lvx_odom_step{});
  ThrowOnError(ctx, lvx_lidar_odometry(ctx, opt, nullptr, r.pose16.data(), r.steps.data(), &r.n_key));
  for (size_t s = 0; s < n; ++s) {
    const double* T = &r.pose16[16 * s];
    double q[4]; QuaternionOfPose(T, q);
    const PoseStamped ps{(int64_t)(scan_stamps[s] * 1e9), {T[3], T[7], T[11]}, {q[3], q[0], q[1], q[2]}};
    r.loam.all.push_back(ps);
    if (r.steps[s].is_key) r.loam.key.push_back(ps);
  }
  return r;
}

class Calibrator {
 public:
  // `in` is copied: the calibrator may outlive the caller's object
  Calibrator(int device, const CalibrateInput& in, const CalibrateOptions& opt) : in_(Resolved(in)), opt_(opt) {
    check(lvx_create(&ctx_, device, 0));
    check(lvx_set_spline(ctx_, in_.t0, in_.dt, in_.n_knots));
    check(lvx_set_camera(ctx_, &in_.camera));
    check(lvx_set_landmarks(ctx_, (int)in_.lm_t0.size(), in_.lm_uv.data(), in_.lm_t0.data()));
    // LioDataset::get_scan_data: the organised raw scans go to the device once
    const size_t HW = (size_t)in_.H * in_.W;
    std::vector<lvx_point_xyzit> raw(in_.scans.size() * HW);
    for (size_t s = 0; s < in_.scans.size(); ++s) {
      if (in_.scans[s].size() != HW) throw std::invalid_argument("scan size does not match H x W");
      std::copy(in_.scans[s].begin(), in_.scans[s].end(), raw.begin() + s * HW);
    }
    if (!raw.empty()) check(lvx_set_scans(ctx_, (int)in_.scans.size(), in_.H, in_.W, raw.data()));
    n_scans_ = in_.scans.size();
    if (!in_.vlp16_stamps.empty()) {   // LioDataset::read's unpack_scan per message, on the device
      check(lvx_set_scans_vlp16(ctx_, (int)in_.vlp16_stamps.size(), in_.vlp16_packet_offsets.data(), in_.vlp16_packets.data(), in_.vlp16_stamps.data(), in_.W, nullptr, &vlp16_info_));
      n_scans_ = in_.vlp16_stamps.size();
    }
  }
  ~Calibrator() { lvx_destroy(ctx_); }
  Calibrator(const Calibrator&) = delete;
  Calibrator& operator=(const Calibrator&) = delete;

  // state: flat vector of lvx.h, in / out
  std::vector<StageReport> Run(std::vector<double>* state) {
    if ((int)state->size() != lvx_state_size(ctx_)) throw std::invalid_argument("state size does not match the problem");
    std::vector<StageReport> rep;
    if (opt_.solve0_so3_from_gyro) rep.push_back(Solve0(state));
    if (opt_.lidar_odometry && in_.loam.all.empty() && n_scans_ > 0) EnsureOdometry();
    const bool have_poses = !in_.loam.all.empty() || !odom_.pose16.empty();
    if (opt_.init_lidar_rotation && have_poses) rep.push_back(InitializeRotation(state));
    for (int it = 0; it < opt_.refine_iterations; ++it) {
      if (it == 0 && have_poses) FirstDataAssociation(*state); else
      DataAssociation(*state);
      rep.push_back(SolveSurfel(state, it == 0 ? "BatchOptimization" : "Refinement"));
    }
    if (opt_.lvi_stage) rep.push_back(SolveLVI(state, false));
    if (opt_.camera_surfel_stage) rep.push_back(SolveLVI(state, true));
    return rep;
  }
  // LIinitializer::CIoptimize (lvi_initialize_surfel_orb.cpp:519-537): camera-IMU calibration alone — initialSO3TrajWithGyro, then trajInitFromVisualFrames
  // (trajectory_manager_lvi.cpp:99-136: gyroscope + accelerometer + reprojection blocks, <= 200 iterations, LiDAR extrinsics locked)
  std::vector<StageReport> RunCameraImu(std::vector<double>* state) {
    if ((int)state->size() != lvx_state_size(ctx_)) throw std::invalid_argument("state size does not match the problem");
    std::vector<StageReport> rep;
    rep.push_back(Solve0(state));
    rep.push_back(SolveVisual(state));
    return rep;
  }
  // LiDAR-IMU extrinsics from the LiDAR odometry alone, no surfel map (plane-poor scenes; a first p_LinI before DataAssociation): initialSO3TrajWithGyro, then
  // trajInitFromLidarPose (trajectory_manager_lvi.cpp:353-388) on CalibrateInput::loam — every pose, re-expressed in the frame of the first one (PosesRelativeToFirst: a
  // pose file need not start at the identity), whose stamp is the start time
  std::vector<StageReport> RunLidarPoses(std::vector<double>* state) {
    if ((int)state->size() != lvx_state_size(ctx_)) throw std::invalid_argument("state size does not match the problem");
    if (in_.loam.all.empty()) throw std::invalid_argument("RunLidarPoses: no LiDAR odometry poses (CalibrateInput::loam)");
    std::vector<StageReport> rep;
    rep.push_back(Solve0(state));
    rep.push_back(SolveLidarPose(state, PosesRelativeToFirst(in_.loam.all), (double)in_.loam.all.front().stamp_ns * 1e-9));
    return rep;
  }
  // the poses in the frame of the first one: p' = R(q_0)^T (p - p_0), q' = q_0^* q with q_0 normalised; a first pose at the identity leaves every number as it is
  static std::vector<PoseStamped> PosesRelativeToFirst(const std::vector<PoseStamped>& poses) {
    std::vector<PoseStamped> out = poses;
    if (poses.empty()) return out;
    const PoseStamped& f = poses.front();
    double w = f.q_wxyz[0], x = f.q_wxyz[1], y = f.q_wxyz[2], z = f.q_wxyz[3];
    const double nq = std::sqrt(w * w + x * x + y * y + z * z);
    if (!(nq > 0.0)) throw std::invalid_argument("PosesRelativeToFirst: the first pose has a zero quaternion");
    if (f.p[0] == 0.0 && f.p[1] == 0.0 && f.p[2] == 0.0 && x == 0.0 && y == 0.0 && z == 0.0) return out;
    w /= nq; x = -x / nq; y = -y / nq; z = -z / nq;   // conj(q_0)
    for (PoseStamped& ps : out) {
      const double d[3] = {ps.p[0] - f.p[0], ps.p[1] - f.p[1], ps.p[2] - f.p[2]};
      const double ux = 2 * (y * d[2] - z * d[1]), uy = 2 * (z * d[0] - x * d[2]), uz = 2 * (x * d[1] - y * d[0]);
      ps.p = {d[0] + w * ux + (y * uz - z * uy), d[1] + w * uy + (z * ux - x * uz), d[2] + w * uz + (x * uy - y * ux)};
      const double bw = ps.q_wxyz[0], bx = ps.q_wxyz[1], by = ps.q_wxyz[2], bz = ps.q_wxyz[3];
      ps.q_wxyz = {w * bw - x * bx - y * by - z * bz, w * bx + x * bw + y * bz - z * by, w * by + y * bw + z * bx - x * bz, w * bz + z * bw + x * by - y * bx};
    }
    return out;
  }
  // addLidarPoses (trajectory_manager_lvi.cpp:533-559): one position block per pose with both times inside [MinTime, MaxTime) (the two `continue`s of :544-545),
  // weight global_opt_pos_weight, HuberLoss(5.0); returns the blocks attached.  The blocks stay set until the next call (an empty list clears them).
  int AddLidarPoses(const std::vector<PoseStamped>& poses, double lidar_start_time) {
    const double tmin = in_.t0, tmax = in_.t0 + (double)(in_.n_knots - 3) * in_.dt;
    std::vector<double> t, p;
    for (const PoseStamped& ps : poses) {
      const double tk = (double)ps.stamp_ns * 1e-9;
      if (tmin > tk || tmax <= tk) continue;
      if (tmin > lidar_start_time || tmax <= lidar_start_time) continue;
      t.push_back(tk); p.insert(p.end(), ps.p.begin(), ps.p.end());
    }
    check(lvx_set_lidar_poses(ctx_, (int)t.size(), t.data(), p.data(), lidar_start_time, 5.0, opt_.w_lidar_pos));
    return (int)t.size();
  }
  // trajInitFromLidarPose: gyroscope + accelerometer + LiDAR position blocks, <= 50 iterations
  StageReport SolveLidarPose(std::vector<double>* state, const std::vector<PoseStamped>& poses, double lidar_start_time) {
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), in_.acc.data(), opt_.w_gyro, opt_.w_acc));
    clear_families(true, true, true);
    const int n = AddLidarPoses(poses, lidar_start_time);
    const PoseBlocksGuard guard{ctx_};   // a fresh estimator per stage: the blocks leave the shared context however this stage ends
    check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromLidarPose, opt_.opt_time_offset)));
    StageReport r{"trajInitFromLidarPose", {}};
    if (opt_.error_statistics) check(lvx_lidar_pose_statistics(ctx_, state->data(), &r.lidar_pos_before));
    r.lm = solve(state, 50);
    attach_history(&r);
    if (opt_.error_statistics) check(lvx_lidar_pose_statistics(ctx_, state->data(), &r.lidar_pos_after));
    r.n_lidar_poses = n;
    return r;
  }
  // the four-argument trajInitFromLVIdata (:259-309): gyroscope + accelerometer + LiDAR position + reprojection blocks, everything free, <= 80 iterations
  StageReport SolveLVIPoses(std::vector<double>* state, const std::vector<PoseStamped>& poses, double lidar_start_time) {
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), in_.acc.data(), opt_.w_gyro, opt_.w_acc));
    clear_families(true, false, true);
    check(lvx_set_reproj(ctx_, (int)in_.obs_landmark.size(), in_.obs_landmark.data(), in_.obs_uv.data(), in_.obs_t0.data(), /*huber*/ opt_.w_cam, /*weight*/ 1.0));   // argument swap of :525
    const int n = AddLidarPoses(poses, lidar_start_time);
    const PoseBlocksGuard guard{ctx_};
    check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromLVI, opt_.opt_time_offset)));
    StageReport r{"trajInitFromLVIdata(lidar_poses)", {}};
    r.lm = solve(state, 80);
    attach_history(&r);
    r.n_lidar_poses = n;
    return r;
  }
  // LIinitializer::RenderMap (lvi_initialize_surfel_orb.cpp:711-811) at `state`, on the de-skewed scans the last DataAssociation round left on the device (nothing is
  // downloaded but the records).  images[i]: grey, [rows][cols] of CalibrateInput::camera; the candidates are the reference's (RenderCandidates); a candidate whose time
  // lies outside the spline is passed over, the first valid one colours (with several valid ones: the lowest that sees the point).
  RenderResult RenderMap(const std::vector<double>& state, const std::vector<std::vector<uint8_t>>& images, const std::vector<double>& image_t) {
    if (images.size() != image_t.size()) throw std::invalid_argument("RenderMap: one time per image");
    RenderResult r; r.candidates = RenderCandidates(images.size());
    if (r.candidates.empty()) return r;
    const size_t px = (size_t)in_.camera.rows * in_.camera.cols;
    std::vector<uint8_t> pack(r.candidates.size() * px); std::vector<double> t(r.candidates.size());
    for (size_t k = 0; k < r.candidates.size(); ++k) {
      const std::vector<uint8_t>& im = images[(size_t)r.candidates[k]];
      if (im.size() != px) throw std::invalid_argument("RenderMap: image size does not match the camera");
      std::copy(im.begin(), im.end(), pack.begin() + k * px); t[k] = image_t[(size_t)r.candidates[k]];
    }
    r.cloud.assign(n_scans_ * (size_t)in_.H * in_.W, lvx_point_xyzrgb{});
    r.valid.assign(r.candidates.size(), 0);
    check(lvx_render_map(ctx_, state.data(), in_.map_time, 0, nullptr, (int)r.candidates.size(), pack.data(), in_.camera.cols, t.data(), nullptr, r.cloud.data(), r.valid.data(), &r.n_colored));
    return r;
  }
  // LIinitializer::ReprojectPointCloudToImage (:1307-1363): every scan with a matching image (MatchScanImages) drawn into it; masks [pairs][rows][cols], 1 where a point
  // lands; scan_of_pair / image_of_pair say which pair a mask belongs to, valid[i] = 0: a pose outside the spline (the mask is zero)
  struct Overlay { std::vector<int32_t> scan_of_pair, image_of_pair, valid; std::vector<uint8_t> masks; };
  Overlay OverlayScans(const std::vector<double>& state, const std::vector<double>& scan_t, const std::vector<double>& image_t) {
    if (scan_t.size() != n_scans_) throw std::invalid_argument("OverlayScans: one time per scan");
    Overlay o;
    const std::vector<int32_t> m = MatchScanImages(scan_t, image_t);
    std::vector<double> st, it;
    for (size_t j = 0; j < m.size(); ++j) if (m[j] >= 0) { o.scan_of_pair.push_back((int32_t)j); o.image_of_pair.push_back(m[j]); st.push_back(scan_t[j]); it.push_back(image_t[(size_t)m[j]]); }
    o.valid.assign(st.size(), 0); o.masks.assign(st.size() * (size_t)in_.camera.rows * in_.camera.cols, 0);
    if (!st.empty()) check(lvx_overlay_scans(ctx_, state.data(), (int)st.size(), o.scan_of_pair.data(), st.data(), it.data(), o.masks.data(), o.valid.data()));
    return o;
  }
  // the optimised path of PublishTrajectory (:873-891): `frame` sampled every `step` seconds from the first to the last IMU stamp (the reference: LiDAR frame, 0.05 s)
  TrajectorySamples SampleTrajectory(const std::vector<double>& state, int frame = LVX_FRAME_LIDAR, double step = 0.05) {
    if (in_.imu_t.empty()) return TrajectorySamples{};
    return lvx_host::SampleTrajectory(ctx_, state, frame, SampleTimes(in_.imu_t.front(), in_.imu_t.back(), step));
  }
  // the LOAM path beside it (:849-870): LiDAR-frame pose errors against CalibrateInput::loam (every pose, or the key poses integration_frames_lidar_), anchored at the
  // first valid pose with LVX_ALIGN_FIRST
  PoseComparison CompareWithLoam(const std::vector<double>& state, int align = LVX_ALIGN_FIRST, bool key_only = false) {
    return ComparePoses(ctx_, state, LVX_FRAME_LIDAR, key_only ? in_.loam.key : in_.loam.all, align);
  }
  // lvx_map_point_covariance over the points of raw scan `scan_index` (lvx_get_scans_raw: whichever way the scans came in), at the normal equations and the state of the
  // context's last LVX_EVAL_NORMAL_EQ evaluation; index_in_scan[i] = h * W + w of entry i.  Empty cells (NaN coordinates) are left out; every `step`-th point is taken.
  // The host route: not the hot path (lvx_map_point_covariance_xyzi_d reads device buffers).
  MapPointUncertainty MapPointCovariance(int scan_index, std::vector<int32_t>* index_in_scan = nullptr, int step = 1, const lvx_point_cov_options* opts = nullptr) {
    if (scan_index < 0 || (size_t)scan_index >= n_scans_ || step < 1) throw std::invalid_argument("MapPointCovariance: scan index outside the scans, or step < 1");
    const size_t HW = (size_t)in_.H * in_.W;
    std::vector<lvx_point_xyzit> raw(HW);
    check(lvx_get_scans_raw(ctx_, scan_index, 1, raw.data()));
    std::vector<double> pts, t;
    if (index_in_scan) index_in_scan->clear();
    for (size_t k = 0; k < HW; k += (size_t)step) {
      const lvx_point_xyzit& p = raw[k];
      if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
      pts.push_back(p.x); pts.push_back(p.y); pts.push_back(p.z); t.push_back(p.timestamp);
      if (index_in_scan) index_in_scan->push_back((int32_t)k);
    }
    return lvx_host::MapPointCovariance(ctx_, pts, t, {}, opts);
  }
  // lvx_projection_covariance over the map cloud — the de-skewed scans of the last data association (lvx_get_scans_in_map), every `step`-th cell that holds a point —
  // in the images taken at image_times, at the normal equations and the state of the context's last LVX_EVAL_NORMAL_EQ evaluation; index_in_map[i] = the cell of entry
  // i.  The host route: not the hot path (lvx_projection_covariance_d reads the resident cloud).
  PixelUncertainty ProjectionUncertainty(const std::vector<double>& image_times, std::vector<int32_t>* index_in_map = nullptr, int step = 1, const lvx_proj_cov_options* opts = nullptr) {
    if (step < 1) throw std::invalid_argument("ProjectionUncertainty: step < 1");
    const size_t np = n_scans_ * (size_t)in_.H * in_.W;
    std::vector<float> cloud(4 * np);
    check(lvx_get_scans_in_map(ctx_, cloud.data()));
    std::vector<float> pts;
    if (index_in_map) index_in_map->clear();
    for (size_t k = 0; k < np; k += (size_t)step) {
      const float* p = &cloud[4 * k];
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
      pts.insert(pts.end(), p, p + 4);
      if (index_in_map) index_in_map->push_back((int32_t)k);
    }
    return lvx_host::ProjectionCovariance(ctx_, pts, image_times, opts);
  }
  const std::vector<lvx_surfel_plane>& planes() const { return planes_; }
  const std::vector<AssociationRecord>& associations() const { return assoc_history_; }
  size_t n_scans() const { return n_scans_; }
  int scan_height() const { return in_.H; }
  int scan_width() const { return in_.W; }
  const lvx_vlp16_info& vlp16_info() const { return vlp16_info_; }   // of the constructor's lvx_set_scans_vlp16 (zero without packets)
  const std::vector<int32_t>& key_scans() const { return key_scans_; }   // of the first-map association: 1 where the scan joined the key-scan map
  const LidarOdometry& odometry() const { return odom_; }                // CalibrateOptions::lidar_odometry: what RunLidarOdometry returned (empty before Run)
  lvx_ctx* context() { return ctx_; }

 private:
  struct PoseBlocksGuard { lvx_ctx* c; ~PoseBlocksGuard() { (void)lvx_set_lidar_poses(c, 0, nullptr, nullptr, 0.0, 5.0, 1.0); } };   // clears the LiDAR-pose blocks when a stage ends, by return or by exception
  StageReport Solve0(std::vector<double>* state) {   // initialSO3TrajWithGyro: gyro blocks + one orientation prior at MinTime, SO3 spline only
    std::vector<double> zero(in_.acc.size(), 0.0);
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), zero.data(), opt_.w_gyro, opt_.w_acc));
    const double q0[4] = {std::cos(0.5e-4), 0, 0, std::sin(0.5e-4)};
    check(lvx_set_orientation_prior(ctx_, 1, in_.t0, q0, opt_.w_gyro));
    clear_families(true, true, true);
    check(lvx_set_locks(ctx_, StageLocks(Stage::SO3FromGyro, opt_.opt_time_offset)));
    StageReport r{"initialSO3TrajWithGyro", solve(state, 30)};
    attach_history(&r);
    check(lvx_set_orientation_prior(ctx_, 0, in_.t0, q0, opt_.w_gyro));
    return r;
  }
  // the scans' odometry poses from lvx_lidar_odometry, once (the scans do not change)
  void EnsureOdometry() {
    if (!odom_.pose16.empty()) return;
    if (in_.scan_stamps.size() != n_scans_) throw std::invalid_argument("scan_stamps: one header stamp per scan is needed for the LiDAR odometry");
    lvx_odom_options oo; lvx_odom_default_options(&oo);   // (oo.ndt.search: DIRECT7 as ndtInit sets it; 0 / 1 / 26 select KDTREE / DIRECT1 / DIRECT26)
    oo.ndt_resolution = opt_.ndt_resolution; oo.key_dist = opt_.key_scan_dist; oo.key_angle_deg = opt_.key_scan_angle_deg;
    odom_ = RunLidarOdometry(ctx_, in_.scan_stamps, &oo);
    if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] LiDAR odometry: %zu scans, %d key scans\n", n_scans_, (int)odom_.n_key);
  }
  // a scan's odometry pose: the pose file's (PoseOfScan), or — without one — the 4 x 4 lvx_lidar_odometry wrote for it, as it is
  bool pose_of_scan(int idx, double scan_t, double T[16]) const {
    if (in_.loam.all.empty() && !odom_.pose16.empty()) { std::copy(odom_.pose16.begin() + 16 * (size_t)idx, odom_.pose16.begin() + 16 * (size_t)idx + 16, T); return true; }
    return PoseOfScan(in_.loam, in_.simulation, idx, scan_t, T);
  }
  // Initialization()'s loop (calib_helper_lvi.cpp:55-89) on the odometry poses of the scans (the poses PoseOfScan selects; a scan without one is left out): the first
  // prefix of the schedule that passes sets q_LtoI = conj(q_ItoS); none: the reference's "[Initialization] fails"
  StageReport InitializeRotation(std::vector<double>* state) {
    if (in_.scan_stamps.empty()) throw std::invalid_argument("scan_stamps: the header stamps of the scans are needed for the rotation initialisation");
    std::vector<double> t, q;
    for (size_t s = 0; s < in_.scan_stamps.size(); ++s) {
      double T[16], qs[4];
      if (!pose_of_scan((int)s, in_.scan_stamps[s], T)) continue;
      QuaternionOfPose(T, qs);
      t.push_back(in_.scan_stamps[s]); q.insert(q.end(), qs, qs + 4);
    }
    const RotationInit ri = EstimateRotation(ctx_, *state, t, q);
    if (ri.first_ok[0] < 0) throw std::runtime_error("[Initialization] fails: no prefix of the " + std::to_string(t.size()) + " odometry poses passes the singular-value test");
    StageReport r{"Initialization", {}};
    r.init_prefix = ri.first_ok[0]; r.init = ri.at(0, (size_t)ri.first_ok[0]);
    double* ql = state->data() + 7 * (size_t)in_.n_knots + 16;
    for (int k = 0; k < 3; ++k) ql[k] = -r.init.q_ItoS_xyzw[k];
    ql[3] = r.init.q_ItoS_xyzw[3];
    if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] Initialization: %d odometry poses, q_LtoI (x y z w) %.6f %.6f %.6f %.6f, sigma[2] %.4f\n", r.init.n_poses, ql[0], ql[1], ql[2], ql[3], r.init.sigma[2]);
    return r;
  }
  lvx_assoc_options assoc_options(double plane_lambda) const {
    lvx_assoc_options ao; lvx_assoc_default_options(&ao);
    ao.ndt_resolution = opt_.ndt_resolution; ao.plane_lambda = plane_lambda; ao.fit_threshold = opt_.fit_threshold; ao.min_leaf_points = opt_.min_leaf_points;
    ao.min_inliers = opt_.min_inliers; ao.radius = opt_.associated_radius; ao.selected_per_ring = opt_.selected_per_ring;
    return ao;
  }
  // DataAssociation of the InitializationDone branch (lvi_initialize_surfel_orb.cpp:1175-1178): Mapping() with the LOAM poses, undistortScanInMap(odom_data_map), setSurfelMap
  // on the key-scan map's NDT grid, getAssociation per scan
  void FirstDataAssociation(const std::vector<double>& state) {
    const size_t S = n_scans_;
    if (in_.scan_stamps.size() != S) throw std::invalid_argument("scan_stamps: one header stamp per scan is needed for the first map");
    std::vector<double> poses(S * 16, 0.0); std::vector<int32_t> has(S, 0);
    for (size_t s = 0; s < S; ++s) has[s] = pose_of_scan((int)s, in_.scan_stamps[s], &poses[16 * s]) ? 1 : 0;
    const lvx_assoc_options ao = assoc_options(opt_.first_map_plane_lambda);
    int32_t np = 0, n = 0;
    key_scans_.assign(S, 0);
    check(lvx_data_association_poses(ctx_, state.data(), in_.scan_stamps.data(), poses.data(), has.data(), opt_.key_scan_dist, opt_.key_scan_angle_deg, &ao, &np, &n, key_scans_.data()));
    fetch_association(state, np, n);
  }
  // DataAssociation of the refinement branch (lvi_initialize_surfel_orb.cpp:1180-1188, 1192-1201)
  void DataAssociation(const std::vector<double>& state) {
    const lvx_assoc_options ao = assoc_options(opt_.plane_lambda);
    int32_t np = 0, n = 0;
    check(lvx_data_association(ctx_, state.data(), in_.map_time, &ao, &np, &n));
    fetch_association(state, np, n);
  }
  void fetch_association(const std::vector<double>& state, int32_t np, int32_t n) {
    n_planes_ = np;
    const bool want_planes = !opt_.device_handoff || opt_.keep_history || opt_.camera_surfel_stage, want_points = !opt_.device_handoff || opt_.keep_history;
    planes_.assign(want_planes ? (size_t)np : 0, lvx_surfel_plane{});
    if (want_planes && np > 0) check(lvx_get_surfel_map(ctx_, np, planes_.data()));
    const int32_t nf = want_points ? n : 0;
    sp_pt_.assign((size_t)nf * 3, 0.0); sp_map_.assign((size_t)nf * 3, 0.0); sp_t_.assign((size_t)nf, 0.0); sp_plane_.assign((size_t)nf, 0);
    if (nf > 0) check(lvx_get_surfel_points(ctx_, nf, sp_pt_.data(), sp_map_.data(), sp_t_.data(), sp_plane_.data()));
    if (opt_.keep_history) {
      AssociationRecord r; r.state = state; r.planes = planes_; r.pt = sp_pt_; r.pt_map = sp_map_; r.t = sp_t_; r.plane = sp_plane_;
      if (opt_.keep_clouds) { r.scans_in_map.assign(n_scans_ * (size_t)in_.H * in_.W * 4, 0.f); check(lvx_get_scans_in_map(ctx_, r.scans_in_map.data())); }
      assoc_history_.push_back(std::move(r));
    }
    if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] association: %d surfels, %d surfel points (every %d-th is used)\n", np, n, opt_.downsample_step);
  }
  void set_surfels() {   // addSurfMeasurement over get_surfel_points() after averageTimeDownSmaple(step) (surfel_association.cpp:240-244)
    if (opt_.device_handoff) {   // the same selection on the device, from the lists of the last association
      int32_t used = 0;
      check(lvx_set_surfel_from_association(ctx_, opt_.downsample_step, in_.map_time, 5.0, opt_.w_surfel, &used));
      n_surfel_used_ = used;
      return;
    }
    std::vector<double> Pi(planes_.size() * 3);
    for (size_t k = 0; k < planes_.size(); ++k) for (int a = 0; a < 3; ++a) Pi[3 * k + a] = planes_[k].Pi[a];
    check(lvx_set_planes(ctx_, (int)planes_.size(), Pi.data()));
    std::vector<double> pt, t; std::vector<int32_t> pid;
    for (size_t i = 0; i < sp_t_.size(); i += (size_t)std::max(1, opt_.downsample_step)) {
      if (sp_t_[i] < in_.map_time) continue;   // CheckTimeSpans: {map_time, t} must be ordered (trajectory_estimator.h:102-127) — the reference would throw
      pt.insert(pt.end(), sp_pt_.begin() + 3 * i, sp_pt_.begin() + 3 * i + 3); t.push_back(sp_t_[i]); pid.push_back(sp_plane_[i]);
    }
    n_surfel_used_ = (int)t.size();
    check(lvx_set_surfel(ctx_, (int)t.size(), pt.data(), t.data(), pid.data(), in_.map_time, 5.0, opt_.w_surfel));
  }
  StageReport SolveSurfel(std::vector<double>* state, const char* name) {   // trajInitFromSurfel
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), in_.acc.data(), opt_.w_gyro, opt_.w_acc));
    set_surfels();
    clear_families(false, true, true);
    check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromSurfel, opt_.opt_time_offset)));
    StageReport r{name, solve(state, 30)};
    attach_history(&r);
    r.n_planes = n_planes_; r.n_surfel_points = n_surfel_used_;
    return r;
  }
  StageReport SolveVisual(std::vector<double>* state) {   // trajInitFromVisualFrames
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), in_.acc.data(), opt_.w_gyro, opt_.w_acc));
    clear_families(true, false, true);
    check(lvx_set_reproj(ctx_, (int)in_.obs_landmark.size(), in_.obs_landmark.data(), in_.obs_uv.data(), in_.obs_t0.data(), /*huber*/ opt_.w_cam, /*weight*/ 1.0));   // argument swap of :525
    check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromVisualFrames, opt_.opt_time_offset)));
    StageReport r{"trajInitFromVisualFrames", solve(state, 200)};
    attach_history(&r);
    return r;
  }
  StageReport SolveLVI(std::vector<double>* state, bool camera_surfel) {   // trajInitFromLVIdata
    check(lvx_set_imu(ctx_, (int)in_.imu_t.size(), in_.imu_t.data(), in_.gyro.data(), in_.acc.data(), opt_.w_gyro, opt_.w_acc));
    set_surfels();
    check(lvx_set_reproj(ctx_, (int)in_.obs_landmark.size(), in_.obs_landmark.data(), in_.obs_uv.data(), in_.obs_t0.data(), /*huber*/ opt_.w_cam, /*weight*/ 1.0));   // argument swap of :525
    StageReport r{camera_surfel ? "trajInitFromLVIdata+lm_splane" : "trajInitFromLVIdata", {}};
    if (camera_surfel) {
      // associateVisualPointsWithPlanes with q_LtoC / t_LinC from the current extrinsics
      const int N = in_.n_knots; const double* sl = state->data() + 7 * N + 16; const double* sc = state->data() + 7 * N + 24;
      double qLC[4], tLC[3]; relative(sc, sl, qLC, tLC);
      const int L = (int)in_.lm_t0.size(), np = (int)planes_.size();
      std::vector<double> p4((size_t)np * 4), bmin((size_t)np * 3), bmax((size_t)np * 3);
      for (int k = 0; k < np; ++k) { for (int a = 0; a < 4; ++a) p4[4 * k + a] = planes_[k].p4[a]; for (int a = 0; a < 3; ++a) { bmin[3 * k + a] = planes_[k].box_min[a]; bmax[3 * k + a] = planes_[k].box_max[a]; } }
      std::vector<int32_t> pol((size_t)std::max(L, 1), -1);
      check(lvx_landmark_assoc(ctx_, state->data(), qLC, tLC, in_.map_time, np, p4.data(), bmin.data(), bmax.data(), opt_.associated_radius, pol.data()));
      std::vector<int32_t> lm, pl;
      for (int l = 0; l < L; ++l) if (pol[l] >= 0) { lm.push_back(l); pl.push_back(pol[l]); }
      check(lvx_set_camsurf(ctx_, (int)lm.size(), lm.data(), pl.data(), in_.map_time, 5.0, opt_.w_cam_surfel));
      check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromLVILandmarksOnly, opt_.opt_time_offset)));
      r.n_cam_surfel = (int)lm.size();
    } else {
      check(lvx_set_camsurf(ctx_, 0, nullptr, nullptr, in_.map_time, 5.0, opt_.w_cam_surfel));
      check(lvx_set_locks(ctx_, StageLocks(Stage::TrajFromLVI, opt_.opt_time_offset)));
    }
    r.lm = solve(state, 80);
    attach_history(&r);
    r.n_planes = n_planes_; r.n_surfel_points = n_surfel_used_;
    return r;
  }
  // LiDAR pose in the camera frame from the two sensor blocks (q_XtoI, p_XinI): q_LtoC = q_CtoI^-1 q_LtoI, t_LinC = q_CtoI^-1 (p_LinI - p_CinI)
  static void relative(const double* cam, const double* lidar, double q[4], double t[3]) {
    const double cx = -cam[0], cy = -cam[1], cz = -cam[2], cw = cam[3];
    const double lx = lidar[0], ly = lidar[1], lz = lidar[2], lw = lidar[3];
    q[0] = cw * lx + cx * lw + cy * lz - cz * ly; q[1] = cw * ly + cy * lw + cz * lx - cx * lz; q[2] = cw * lz + cz * lw + cx * ly - cy * lx; q[3] = cw * lw - cx * lx - cy * ly - cz * lz;
    const double d[3] = {lidar[4] - cam[4], lidar[5] - cam[5], lidar[6] - cam[6]};
    const double ux = 2 * (cy * d[2] - cz * d[1]), uy = 2 * (cz * d[0] - cx * d[2]), uz = 2 * (cx * d[1] - cy * d[0]);
    t[0] = d[0] + cw * ux + (cy * uz - cz * uy); t[1] = d[1] + cw * uy + (cz * ux - cx * uz); t[2] = d[2] + cw * uz + (cx * uy - cy * ux);
  }
  void clear_families(bool surfel, bool reproj, bool camsurf) {
    if (surfel) check(lvx_set_surfel(ctx_, 0, nullptr, nullptr, nullptr, in_.map_time, 5.0, opt_.w_surfel));
    if (reproj) check(lvx_set_reproj(ctx_, 0, nullptr, nullptr, nullptr, opt_.w_cam, 1.0));
    if (camsurf) check(lvx_set_camsurf(ctx_, 0, nullptr, nullptr, in_.map_time, 5.0, opt_.w_cam_surfel));
  }
  lvx_lm_summary solve(std::vector<double>* state, int max_it) {
    lvx_lm_options o; lvx_lm_default_options(&o); o.max_iterations = max_it; o.verbose = opt_.verbose > 1;
    lvx_lm_summary s{};
    if (opt_.keep_history) stage_state_in_ = *state;
    if (opt_.error_statistics) check(lvx_error_statistics(ctx_, state->data(), &stats_before_));
    check(lvx_lm_solve(ctx_, state->data(), &o, &s));
    if (opt_.error_statistics) check(lvx_error_statistics(ctx_, state->data(), &stats_after_));
    has_cov_ = false; has_tsig_ = false; has_lsig_ = false;
    const bool want_tsig = opt_.trajectory_covariance_step > 0 && !in_.imu_t.empty();
    const bool want_lsig = opt_.landmark_covariance && !in_.lm_t0.empty();
    if (opt_.covariance || want_tsig || want_lsig) {   // the normal equations at the final state (the loop's last ones may belong to a rejected candidate), then the calls
      double cost = 0.0;
      check(lvx_evaluate(ctx_, state->data(), LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, &cost, nullptr));
    }
    if (want_tsig) {
      lvx_traj_cov_options to; lvx_traj_cov_default_options(&to); to.radius = opt_.covariance_radius;
      const std::vector<double> times = SampleTimes(in_.imu_t.front(), in_.imu_t.back(), opt_.trajectory_covariance_step);
      tsig_ = TrajectoryUncertainty{}; tsig_.frame = opt_.trajectory_covariance_frame; tsig_.radius = to.radius; tsig_.t = times;
      tsig_.cov.assign(36 * times.size(), 0.0); tsig_.sigma.assign(6 * times.size(), 0.0); tsig_.valid.assign(times.size(), 0);
      lvx_traj_cov out{tsig_.cov.data(), tsig_.sigma.data(), nullptr, nullptr, tsig_.valid.data()};
      const int rc = times.empty() ? LVX_OK : lvx_trajectory_covariance(ctx_, &to, opt_.trajectory_covariance_frame, (int)times.size(), times.data(), &out);
      if (rc == LVX_E_NOTPD) { if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] trajectory covariance: %s\n", lvx_last_error(ctx_)); }   // no record for this stage; the calibration goes on
      else { check(rc); has_tsig_ = true; if (opt_.verbose) std::fputs(FormatTrajectoryUncertainty(tsig_).c_str(), stderr); }
    }
    if (want_lsig) {
      lvx_landmark_cov_options lo; lvx_landmark_cov_default_options(&lo); lo.radius = opt_.covariance_radius;
      const size_t L = in_.lm_t0.size();
      lsig_ = LandmarkUncertainty{}; lsig_.radius = lo.radius; lsig_.ids.resize(L); lsig_.rho.resize(L);
      for (size_t l = 0; l < L; ++l) { lsig_.ids[l] = (int32_t)l; lsig_.rho[l] = (*state)[7 * (size_t)in_.n_knots + 32 + l]; }
      lsig_.var_rho.assign(L, 0.0); lsig_.sigma_rho.assign(L, 0.0); lsig_.point.assign(3 * L, 0.0); lsig_.point_cov.assign(9 * L, 0.0); lsig_.valid.assign(L, 0);
      lvx_landmark_cov out{lsig_.var_rho.data(), lsig_.sigma_rho.data(), lsig_.point.data(), lsig_.point_cov.data(), nullptr, nullptr, lsig_.valid.data()};
      const int rc = lvx_landmark_covariance(ctx_, &lo, (int)L, nullptr, &out);
      if (rc == LVX_E_NOTPD) { if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] landmark covariance: %s\n", lvx_last_error(ctx_)); }   // no record for this stage; the calibration goes on
      else {
        check(rc);
        has_lsig_ = std::find(lsig_.valid.begin(), lsig_.valid.end(), (uint8_t)1) != lsig_.valid.end();   // none valid: the stage holds the landmarks constant
        if (has_lsig_ && opt_.verbose) std::fputs(FormatLandmarkUncertainty(lsig_).c_str(), stderr);
      }
    }
    if (opt_.covariance) {
      lvx_calib_cov_options co; lvx_calib_cov_default_options(&co); co.radius = opt_.covariance_radius;
      const int rc = lvx_calibration_covariance(ctx_, &co, &cov_);
      if (rc == LVX_E_NOTPD) { if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] covariance: %s\n", lvx_last_error(ctx_)); }   // no record for this stage; the calibration goes on
      else { check(rc); has_cov_ = true; if (opt_.verbose) std::fputs(FormatCalibrationUncertainty(cov_).c_str(), stderr); }
    }
    const int cap = 4 * max_it + 8;
    hist_cost_.assign((size_t)cap, 0.0); hist_radius_.assign((size_t)cap, 0.0); hist_acc_.assign((size_t)cap, 0);
    const int k = lvx_lm_get_history(ctx_, cap, hist_cost_.data(), hist_radius_.data(), hist_acc_.data());
    hist_cost_.resize((size_t)std::max(k, 0)); hist_radius_.resize(hist_cost_.size()); hist_acc_.resize(hist_cost_.size());
    if (opt_.verbose) std::fprintf(stderr, "[lvx calibrate] solve: %d iterations, cost %.6e -> %.6e, termination %d\n", s.iterations, s.initial_cost, s.final_cost, s.termination);
    return s;
  }
  void attach_history(StageReport* r) const {
    r->cost_history = hist_cost_; r->radius_history = hist_radius_; r->accepted = hist_acc_; r->state_in = stage_state_in_;
    r->has_stats = opt_.error_statistics; r->stats_before = stats_before_; r->stats_after = stats_after_;
    r->has_covariance = has_cov_; r->covariance = cov_;
    r->has_trajectory_sigma = has_tsig_; r->trajectory_sigma = tsig_;
    r->has_landmark_sigma = has_lsig_; r->landmark_sigma = has_lsig_ ? lsig_ : LandmarkUncertainty{};
  }
  void check(int rc) {
    if (rc == LVX_OK) return;
    const std::string msg = ctx_ ? lvx_last_error(ctx_) : "lvx error";
    if (rc == LVX_E_RANGE) throw std::range_error(msg);
    throw std::runtime_error(msg + " (lvx error " + std::to_string(rc) + ")");
  }
  // CalibrateInput::vlp16_*: the shape of the scans the device will unpack, and the default scan_stamps
  static CalibrateInput Resolved(CalibrateInput in) {
    if (in.vlp16_stamps.empty()) return in;
    if (!in.scans.empty()) throw std::invalid_argument("CalibrateInput: scans or vlp16_packets, not both");
    const size_t n = in.vlp16_stamps.size();
    if (in.vlp16_packet_offsets.size() != n + 1) throw std::invalid_argument("vlp16_packet_offsets: one more entry than vlp16_stamps");
    int longest = 0;
    for (size_t s = 0; s < n; ++s) longest = std::max(longest, in.vlp16_packet_offsets[s + 1] - in.vlp16_packet_offsets[s]);
    if (in.vlp16_packet_offsets[0] < 0 || (size_t)in.vlp16_packet_offsets[n] * LVX_VLP16_PACKET_BYTES > in.vlp16_packets.size())
      throw std::invalid_argument("vlp16_packet_offsets reach outside vlp16_packets");
    in.H = 16; in.W = std::max(in.W, 24 * longest);
    if (in.scan_stamps.empty()) in.scan_stamps = in.vlp16_stamps;
    return in;
  }
  lvx_ctx* ctx_ = nullptr;
  const CalibrateInput in_;
  size_t n_scans_ = 0; lvx_vlp16_info vlp16_info_{};
  CalibrateOptions opt_;
  std::vector<AssociationRecord> assoc_history_;
  std::vector<double> hist_cost_, hist_radius_, stage_state_in_; std::vector<int32_t> hist_acc_;
  std::vector<lvx_surfel_plane> planes_;
  std::vector<int32_t> key_scans_;
  LidarOdometry odom_;
  std::vector<double> sp_pt_, sp_map_, sp_t_; std::vector<int32_t> sp_plane_;
  int n_surfel_used_ = 0, n_planes_ = 0;
  lvx_error_stats stats_before_{}, stats_after_{};
  bool has_cov_ = false; lvx_calib_cov cov_{};
  bool has_tsig_ = false; TrajectoryUncertainty tsig_;
  bool has_lsig_ = false; LandmarkUncertainty lsig_;
};

}  // namespace lvx_host
