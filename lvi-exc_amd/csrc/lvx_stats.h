// lvx_stats.h — value-only evaluation of one residual block per family, for the error statistics (lvx_stats.hip).
//
// The reference judges a calibration by printErrorStatistics (src/lvi_exc/src/core/trajectory_manager_lvi.cpp:621-697): the mean absolute RAW error of every family —
// ErrorRaw of the gyroscope / accelerometer (gyroscope_measurement.h:46-48, accelerometer_measurement.h:49-51), point2plane of the surfel points
// (lidar_surfel_point.h:86-89), Error of the camera.  These functions are the value halves (NEED_J = false) of the residuals in lvx_resid.h with the segment,
// hub and time-offset semantics of the per-segment kernel (lvx_eval.hip: k_family's family policies): they return the WEIGHTED residual rows, exactly what
// lvx_evaluate writes; the raw error is the row divided by the family weight.  Host-callable, so the CPU suite checks them against the oracle.
#pragma once
#include "lvx_resid.h"

namespace lvx {

// the pose at the map time, shared by every surfel (tau = LiDAR offset) or camera-surfel (tau = camera offset) block: value only
struct StatHub { KnotRef k; v3 p; quat q; int ok; };   // ok: 1 | 0 outside the spline | -RES_NONUNIT
LVX_HD bool stat_pose(const SplineRef& sp, const KnotRef& k, v3* p, quat* q) {
  PoseEval e;
  if (!pose_eval<false>(sp, k, &e)) return false;
  *p = e.p; *q = e.so3.q;
  return true;
}
LVX_HD void stat_hub(const SplineRef& sp, double t_map, bool tau_locked, double mto, double tau, StatHub* h) {
  double s1[1][2];
  if (tau_locked) { s1[0][0] = t_map; s1[0][1] = t_map; } else { s1[0][0] = t_map - mto; s1[0][1] = t_map + mto; }
  Segs sg; h->ok = 0;
  if (!build_segments(sp, s1, 1, &sg)) return;
  if (!seg_lookup(sp, sg, t_map + tau, &h->k)) return;
  if (!stat_pose(sp, h->k, &h->p, &h->q)) { h->ok = -RES_NONUNIT; return; }
  h->ok = 1;
}
// spans of a two-pose LiDAR block, the map-time pose inside THEM (the merged-segment corner of spline_base.h:196-203 gives another interpolation amount than the shared hub)
LVX_HD int stat_two_pose(const SplineRef& sp, const StatHub& hub, double t_map, double tk, bool tau_locked, double mto, double tau, Segs* segs, PoseEval* hp) {
  const double pad = tau_locked ? 0.0 : mto;
  const double spans[2][2] = {{t_map - pad, t_map + pad}, {tk - pad, tk + pad}};
  if (!build_segments(sp, spans, 2, segs)) return RES_RANGE;
  KnotRef kh;
  if (!seg_lookup(sp, *segs, t_map + tau, &kh)) return RES_RANGE;
  hp->k = kh;
  if (hub.ok == 1 && kh.i0 == hub.k.i0 && kh.u == hub.k.u) { hp->p = hub.p; hp->so3.q = hub.q; return RES_OK; }
  return stat_pose(sp, kh, &hp->p, &hp->so3.q) ? RES_OK : RES_NONUNIT;
}

LVX_HD int stat_gyro(const SplineRef& sp, const ImuCal& imu, double t, v3 w_meas, double weight, double r[3]) {
  int i0;
  return gyro_residual<false>(sp, imu, t, w_meas, weight, &i0, r, nullptr);
}
LVX_HD int stat_accel(const SplineRef& sp, const ImuCal& imu, double t, v3 a_meas, double weight, double r[3]) {
  int i0;
  return accel_residual<false>(sp, imu, t, a_meas, weight, &i0, r, nullptr);
}
LVX_HD int stat_prior(const SplineRef& sp, double t, quat q_meas, double weight, double r[1]) {
  int i0;
  return prior_residual<false>(sp, t, q_meas, weight, &i0, r, nullptr);
}
LVX_HD int stat_surfel(const SplineRef& sp, const StatHub& hub, const SensorCal& lidar, bool tau_locked, double mto, double t_map, double tk, v3 p_L, v3 Pi, double weight, double r[1]) {
  Segs segs; PoseEval h;
  const int st = stat_two_pose(sp, hub, t_map, tk, tau_locked, mto, lidar.tau, &segs, &h);
  if (st != RES_OK) return st;
  int i0;
  return surfel_residual<false>(sp, h, segs, lidar, tk, p_L, Pi, weight, &i0, r, nullptr);
}
// LiDAR odometry position block (lvx_set_lidar_poses): the hub is the pose at the start time, with the LiDAR offset
LVX_HD int stat_lidarpos(const SplineRef& sp, const StatHub& hub, const SensorCal& lidar, bool tau_locked, double mto, double t_start, double tk, v3 p_meas, double weight, double r[3]) {
  Segs segs; PoseEval h;
  const int st = stat_two_pose(sp, hub, t_start, tk, tau_locked, mto, lidar.tau, &segs, &h);
  if (st != RES_OK) return st;
  int i0;
  return lidarpos_residual<false>(sp, h, segs, lidar, tk, p_meas, weight, &i0, r, nullptr);
}
LVX_HD int stat_reproj(const SplineRef& sp, const CamIntr& ci, const SensorCal& cam, bool tau_locked, double mto, double u_ref, double v_ref, double t0_ref,
                       double u_obs, double v_obs, double t0_obs, double rho, double weight, double r[2]) {
  int i0r, i0o;
  return reproj_residual<false>(sp, ci, cam, tau_locked, mto, u_ref, v_ref, t0_ref, u_obs, v_obs, t0_obs, rho, weight, &i0r, &i0o, r, nullptr);
}
LVX_HD int stat_camsurf(const SplineRef& sp, const StatHub& hub, const CamIntr& ci, const SensorCal& cam, const SensorCal& lidar, bool tau_locked, double mto, double t_map,
                        double u_ref, double v_ref, double t0_ref, double rho, v3 Pi, double weight, double r[1]) {
  Segs segs; PoseEval h;
  const int st = stat_two_pose(sp, hub, t_map, t0_ref, tau_locked, mto, cam.tau, &segs, &h);
  if (st != RES_OK) return st;
  int i0;
  return camsurf_residual<false>(sp, h, segs, ci, cam, lidar, u_ref, v_ref, t0_ref, rho, Pi, weight, &i0, r, nullptr);
}

// One block's contribution to its family's sums.  Slots of a record: 0 evaluated | 1 outliers | 2 cost | 3..5 sum | 6..8 sum |e| | 9..11 sum e^2 | 12..14 max |e| (raw error e = r / weight).
enum { ST_EVAL = 0, ST_OUT = 1, ST_COST = 2, ST_SUM = 3, ST_ABS = 6, ST_SQ = 9, ST_MAX = 12, ST_W = 16 };
template <int NR>
LVX_HD void stat_block(const double r[NR], double weight, double huber, double acc[ST_W]) {
  double s = 0.0;
  for (int a = 0; a < NR; ++a) s += r[a] * r[a];
  double scale;
  acc[ST_EVAL] += 1.0;
  if (huber > 0.0 && s > huber * huber) acc[ST_OUT] += 1.0;   // ceres::HuberLoss: the squared norm of the weighted residual beyond delta^2
  acc[ST_COST] += 0.5 * huber_rho(huber, s, &scale);
  for (int a = 0; a < NR; ++a) {
    const double e = r[a] / weight, ae = fabs(e);
    acc[ST_SUM + a] += e; acc[ST_ABS + a] += ae; acc[ST_SQ + a] += e * e;
    if (ae > acc[ST_MAX + a]) acc[ST_MAX + a] = ae;
  }
}

}  // namespace lvx
