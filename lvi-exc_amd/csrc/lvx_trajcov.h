// lvx_trajcov.h — the pose Jacobian of lvx_trajectory_covariance: derivative of the pose error at a time by the at most 31 tangent scalars the pose depends on.
// Host-callable (tests/native/trajcov_host_check.cpp builds it with g++ and holds it against central differences); the library runs it inside k_pose_cov
// (lvx_selinv.h).
//
// Pose error: dp = p' - p in the world frame, dphi the WORLD-frame rotation vector in radians, R' = Exp(dphi) R.  Columns:
//   6 j + a     (j = 0..3, a = 0..2)  position tangent of knot i0 + j:   dp = Bp[j] e_a (+ nothing on the rotation)
//   6 j + 3 + b                       rotation tangent of knot i0 + j (EigenQuaternionParameterization: a HALF-angle, applied on the left of the control quaternion):
//                                     q(delta) = q Exp(xi), xi = dxi[j] delta (lvx_math.h: so3_eval), so dphi = R xi, and a sensor's origin moves by dphi x (R p_rel)
//   24 .. 26    the sensor's theta: q_rel' = Exp(2 theta) q_rel, so dphi = 2 R theta        27 .. 29  the sensor's p: dp = R dp_rel
//   30          the sensor's tau: (v + omega_world x (R p_rel), omega_world) = (traj_sensor_velocity, w_world)
// LVX_FRAME_TRAJECTORY: columns 24 .. 30 are zero and idx is -1 there.  idx[c]: the tangent index of column c (locks are the caller's business: ord[]).
#pragma once
#include "lvx_traj.h"

namespace lvx {

enum { TCOV_W = 31 };

// frame: 0 trajectory (ext is not read), 1 LiDAR, 2 camera (ext: that sensor's q_rel, p_rel; tau has been added to tt by the caller).
// Returns RES_OK, RES_RANGE (J and idx are not written) or RES_NONUNIT.
LVX_HD int traj_pose_jacobian(const SplineRef& sp, int frame, const SensorCal& ext, double tt, double J[6][TCOV_W], int idx[TCOV_W]) {
  KnotRef k;
  if (!traj_knot(sp.t0, sp.dt, sp.n, tt, &k)) return RES_RANGE;
  PoseEval e;
  const bool ok = pose_eval<true, true>(sp, k, &e);
  const bool sensor = frame != 0;
  const m3 R = rotmat(e.so3.q);
  const v3 lever = sensor ? R * ext.p : mk(0, 0, 0);   // q(tt) p_rel
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < TCOV_W; ++c) J[r][c] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { J[a][6 * j + a] = e.Bp[j]; idx[6 * j + a] = 6 * (k.i0 + j) + a; idx[6 * j + 3 + a] = 6 * (k.i0 + j) + 3 + a; }
    const m3 W = R * e.so3.dxi[j];                       // dphi per unit rotation tangent
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const v3 dphi = mk(W.a[b], W.a[3 + b], W.a[6 + b]);
      const v3 dp = cross(dphi, lever);
      J[0][6 * j + 3 + b] = dp.x; J[1][6 * j + 3 + b] = dp.y; J[2][6 * j + 3 + b] = dp.z;
      J[3][6 * j + 3 + b] = dphi.x; J[4][6 * j + 3 + b] = dphi.y; J[5][6 * j + 3 + b] = dphi.z;
    }
  }
  const int c0 = 6 * sp.n + (frame == 1 ? 8 : 15);
#pragma unroll
  for (int b = 0; b < 7; ++b) idx[24 + b] = sensor ? c0 + b : -1;
  if (sensor) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int a = 0; a < 3; ++a) { J[3 + a][24 + b] = 2.0 * R.a[3 * a + b]; J[a][27 + b] = R.a[3 * a + b]; }
    const v3 ww = R * e.so3.w_body;
    const v3 vs = e.v + cross(ww, lever);
    J[0][30] = vs.x; J[1][30] = vs.y; J[2][30] = vs.z; J[3][30] = ww.x; J[4][30] = ww.y; J[5][30] = ww.z;
  }
  return ok ? RES_OK : RES_NONUNIT;
}

}  // namespace lvx
