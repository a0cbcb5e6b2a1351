// lvx_pose.h — sensor poses from the split spline on the device: TrajectoryManagerLVI::evaluateLidarPose / evaluateCameraPose
// (src/lvi_exc/src/core/trajectory_manager_lvi.cpp:398-408, 430-440).  One definition for the upstream kernels (lvx_upstream.hip) and the map rendering
// (lvx_render.hip); both translation units are built without FP contraction, so a pose is the same bits wherever it is evaluated.
#pragma once
#include "lvx_resid.h"

namespace lvx {

__device__ __forceinline__ bool lidar_pose_dev(const double* state, int N, double t0, double dt, double t, quat* q_LtoG, v3* p_LinG) {
  const double* sl = state + 7 * (size_t)N + 16;
  const double tt = t + sl[7];
  const double tmax = t0 + (double)(N - 3) * dt;
  if (t0 > tt || tmax <= tt) return false;                         // evaluateLidarPose range test (trajectory_manager_lvi.cpp:401-402)
  const double s = (tt - t0) / dt;
  const int i0 = (int)floor(s);
  if (N < 4 || i0 < 0 || i0 > N - 4) return false;
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  KnotRef k; k.i0 = i0; k.u = s - (double)i0;
  PoseEval e;
  if (!pose_eval<false>(sp, k, &e)) return false;
  const quat qL = load_q(sl); const v3 pL = load_v3(sl + 4);
  *q_LtoG = qmul(e.so3.q, qL);
  *p_LinG = qrot(e.so3.q, pL) + e.p;
  return true;
}
// evaluateCameraPose (trajectory_manager_lvi.cpp:430-440)
__device__ __forceinline__ bool camera_pose_dev(const double* state, int N, double t0, double dt, double t, quat* q_CtoG, v3* p_CinG) {
  const double* sc = state + 7 * (size_t)N + 24;
  const double tt = t + sc[7];
  const double tmax = t0 + (double)(N - 3) * dt;
  if (t0 > tt || tmax <= tt) return false;
  const double s = (tt - t0) / dt;
  const int i0 = (int)floor(s);
  if (N < 4 || i0 < 0 || i0 > N - 4) return false;
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  KnotRef k; k.i0 = i0; k.u = s - (double)i0;
  PoseEval e;
  if (!pose_eval<false>(sp, k, &e)) return false;
  const quat qC = load_q(sc); const v3 pC = load_v3(sc + 4);
  *q_CtoG = qmul(e.so3.q, qC);
  *p_CinG = qrot(e.so3.q, pC) + e.p;
  return true;
}

}  // namespace lvx
