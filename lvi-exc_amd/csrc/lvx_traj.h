// lvx_traj.h — the query side of the split spline, per sample: what Kontiki's TrajectoryView::Evaluate(t, flags) returns (position, velocity, acceleration, orientation,
// angular velocity: trajectories/uniform_r3_spline_trajectory.h:36-103, uniform_so3_spline_trajectory.h:46-125), what the IMU model predicts at a time
// (sensors/imu.h:61-101, constant_bias_imu.h:51-61) and the error of one pose against a reference pose (LIinitializer::PublishTrajectory lays the LOAM path beside the
// optimised one, src/lvi_exc/test/lvi_initialize_surfel_orb.cpp:834-902).  Host-callable (tests/native/traj_host_check.cpp builds it with g++); the library runs it inside
// the kernels of lvx_traj.hip only.
//
// Validity of a query at time tt (= t + the frame's time offset): MinTime <= tt < MaxTime with MinTime = t0, MaxTime = t0 + (N - 3) dt — the test of
// TrajectoryManagerLVI::evaluateLidarPose (trajectory_manager_lvi.cpp:401-402).  The `t - 1e-5` retry of SplineView::Evaluate (spline_base.h:196-203) is deliberately NOT
// part of a query: it exists so that a MEASUREMENT on the last knot boundary still finds its segment; a query at MaxTime is outside the trajectory and reports so.
// NaN and +-inf fail both comparisons' positive forms and are invalid.
#pragma once
#include "lvx_resid.h"

namespace lvx {

LVX_HD bool traj_time_valid(double t0, double dt, int N, double tt) {
  const double tmax = t0 + (double)(N - 3) * dt;
  return N >= 4 && tt >= t0 && tt < tmax;
}
// The knot interval as lidar_pose_dev / camera_pose_dev find it (lvx_pose.h); the interpolation amount against the interval's own origin t0 + dt i0, as Kontiki's
// segment views and the residual kernels form it (spline_base.h:153-157 with the segment's t0, :399): (tt - t0) / dt - i0 carries the rounding of a quotient near N
// (7e-15 at s = 95, i.e. 1.4e-16 s), the origin's rounding is half an ulp of the stamp (7e-15 s at t = 100 s) — with a jerk of 1e4 m/s^3 the second is 1e-10 m/s^2 of
// acceleration, and it is the one the reference's numbers carry.  Within an ulp of a knot u may come out as 1 + 4e-13 instead of 0 + ...: the same cubic, continued.
LVX_HD bool traj_knot(double t0, double dt, int N, double tt, KnotRef* k) {
  if (!traj_time_valid(t0, dt, N, tt)) return false;
  const int i0 = (int)floor((tt - t0) / dt);
  if (i0 < 0 || i0 > N - 4) return false;
  k->i0 = i0; k->u = (tt - madd_2r(dt, (double)i0, t0)) / dt;
  return true;
}

struct TrajKin { v3 p, v, a; quat q; v3 w_body, w_world; };   // w_world = q w_body: Kontiki's angular velocity is in the world frame (the gyroscope model rotates it by q*, imu.h:87-91)
// The spline itself at tt.  Returns RES_OK, RES_RANGE or RES_NONUNIT (a control quaternion pair of the window fails logq's 1e-5 unit check, as in the residual kernels).
template <bool NEED_W>
LVX_HD int traj_kinematics(const SplineRef& sp, double tt, TrajKin* o) {
  KnotRef k;
  if (!traj_knot(sp.t0, sp.dt, sp.n, tt, &k)) return RES_RANGE;
  R3Basis b; r3_basis(k.u, sp.dt, &b);
  v3 p = mk(0, 0, 0), v = mk(0, 0, 0), a = mk(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v3 cj = load_v3(sp.r3 + 3 * (size_t)(k.i0 + j));
    p = p + b.Bp[j] * cj; v = v + b.Bv[j] * cj; a = a + b.Ba[j] * cj;
  }
  o->p = p; o->v = v; o->a = a;
  quat c[4]; load_so3_cp(sp, k.i0, c);
  So3Eval e;
  if (!so3_eval<NEED_W, false>(c, k.u, sp.dt, &e)) return RES_NONUNIT;
  o->q = e.q;
  if (NEED_W) { o->w_body = e.w_body; o->w_world = qrot(e.q, e.w_body); }
  return RES_OK;
}
// velocity of a sensor origin rigidly mounted at p_S in the body frame: v + omega x (q p_S)
LVX_HD v3 traj_sensor_velocity(const TrajKin& k, v3 p_S) { return k.v + cross(k.w_world, qrot(k.q, p_S)); }

// Imu::Gyroscope / Accelerometer with the constant biases, at tt = t + tau_imu: gyro = q* omega + b_g, acc = q* (p'' + g(roll, pitch)) + b_a, g and G = -9.79 as
// accel_residual forms them (imu.h:25, 61-70)
LVX_HD int traj_predict_imu(const SplineRef& sp, const ImuCal& imu, double t, v3* gyro, v3* acc) {
  TrajKin k;
  const int st = traj_kinematics<true>(sp, t + imu.tau, &k);
  if (st != RES_OK) return st;
  *gyro = k.w_body + imu.bg;
  const double G = -9.79;
  const double cr = cos(imu.roll), sr = sin(imu.roll), cp = cos(imu.pitch), sp_ = sin(imu.pitch);
  const v3 g = mk(-sp_ * cr * G, sr * G, -cr * cp * G);
  *acc = qrot_inv(k.q, k.a + g) + imu.ba;
  return RES_OK;
}
LVX_HD ImuCal traj_load_imu(const double* state, int N) {
  const double* si = state + 7 * (size_t)N;
  ImuCal imu; imu.roll = si[8]; imu.pitch = si[9]; imu.ba = load_v3(si + 10); imu.bg = load_v3(si + 13); imu.tau = si[7];
  return imu;
}

// rigid poses (q, p): x -> q x + p
struct TrajPose { quat q; v3 p; };
LVX_HD TrajPose pose_mul(const TrajPose& a, const TrajPose& b) { TrajPose r; r.q = qmul(a.q, b.q); r.p = qrot(a.q, b.p) + a.p; return r; }
LVX_HD TrajPose pose_inv(const TrajPose& a) { TrajPose r; r.q = qconj(a.q); r.p = -qrot(r.q, a.p); return r; }
LVX_HD quat qnormalized(quat q) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return mkq(q.w / n, q.x / n, q.y / n, q.z / n);
}
// error of pose T against the reference pose R: translation |p - p'|, rotation 2 atan2(|vec(d)|, |d.w|) with d = q* (x) q' (Eigen's angularDistance, the form
// lvx_loaders.hpp's key-pose test uses)
LVX_HD void traj_pose_error(const TrajPose& T, const TrajPose& R, double* e_trans, double* e_rot) {
  const v3 d = T.p - R.p;
  *e_trans = sqrt(dot(d, d));
  const quat dq = qmul(qconj(T.q), R.q);
  *e_rot = 2.0 * atan2(sqrt(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z), fabs(dq.w));
}
// LVX_ALIGN_FIRST: A = T_a o R_a^-1 maps the reference onto the trajectory at the anchor sample (PublishTrajectory's Twl * Tl, :850-861, for a first pose that need not
// be the identity)
LVX_HD TrajPose traj_align_first(const TrajPose& T_a, const TrajPose& R_a) { return pose_mul(T_a, pose_inv(R_a)); }
// relative error of the step i -> j: T_i^-1 T_j against R_i^-1 R_j
LVX_HD void traj_rel_error(const TrajPose& Ti, const TrajPose& Tj, const TrajPose& Ri, const TrajPose& Rj, double* e_trans, double* e_rot) {
  traj_pose_error(pose_mul(pose_inv(Ti), Tj), pose_mul(pose_inv(Ri), Rj), e_trans, e_rot);
}

// One error series' running summary: terms are added in index order; the maximum keeps its LOWEST index
struct TrajSum { double sum, sumsq, max; int argmax, n; };
LVX_HD TrajSum trajsum_zero() { TrajSum s; s.sum = 0.0; s.sumsq = 0.0; s.max = 0.0; s.argmax = 0; s.n = 0; return s; }
LVX_HD void trajsum_add(TrajSum* s, double e, int index) {
  if (s->n == 0 || e > s->max || (e == s->max && index < s->argmax)) { s->max = e; s->argmax = index; }
  s->sum += e; s->sumsq += e * e; s->n += 1;
}
LVX_HD TrajSum trajsum_merge(const TrajSum& a, const TrajSum& b) {   // a + b, in this order
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  TrajSum r; r.sum = a.sum + b.sum; r.sumsq = a.sumsq + b.sumsq; r.n = a.n + b.n;
  const bool tb = b.max > a.max || (b.max == a.max && b.argmax < a.argmax);
  r.max = tb ? b.max : a.max; r.argmax = tb ? b.argmax : a.argmax;
  return r;
}

}  // namespace lvx
