// lvx_lmcov.h — the map point of a landmark and its Jacobian for lvx_landmark_covariance.  Host-callable (tests/native/lmcov_host_check.cpp builds it with g++ and
// holds it against central differences); the library runs it inside k_landmark_cov (lvx_selinv.h).
//
// A landmark is an inverse depth rho along the ray y_h = Unproject(uv_ref) of its reference view, taken at t_ref = (t0_ref + tau_C) + v_ref readout / rows (the
// reprojection residual's expression, lvx_resid.h: reproj_residual).  With (R_C, p_C) the LVX_FRAME_CAMERA pose at t_ref
//   P_w = R_C (y_h / rho) + p_C
// (reproj_residual's X / rho).  Columns of J (3 x 32):
//   0         rho:  -R_C y_h / rho^2
//   1 .. 31   the 31 scalars of the camera-frame pose at t_ref in traj_pose_jacobian's order:  dP = dp + dphi x (R_C y_h / rho) = (I, -[R_C y_h / rho]_x) J_pose
// idx[0] = 6 N + 22 + l, idx[1 + c] = traj_pose_jacobian's idx[c] (locks are the caller's business: ord[]).  rho = 0 is a point at infinity: P and J are not finite.
#pragma once
#include "lvx_trajcov.h"

namespace lvx {

enum { LCOV_W = 32 };

LVX_HD double landmark_ref_time(const CamIntr& ci, double tau_cam, double v_ref, double t0_ref) { return madd_2r(v_ref, ci.readout / (double)ci.rows, t0_ref + tau_cam); }

// Jp: the caller's room for the pose Jacobian (LDS on the device).  Returns RES_OK, RES_RANGE (nothing is written) or RES_NONUNIT.
LVX_HD int landmark_point_jacobian(const SplineRef& sp, const CamIntr& ci, const SensorCal& cam, int l, double u_ref, double v_ref, double t0_ref, double rho,
                                   double Jp[6][TCOV_W], double J[3][LCOV_W], int idx[LCOV_W], double P[3]) {
  const double tt = landmark_ref_time(ci, cam.tau, v_ref, t0_ref);
  const int st = traj_pose_jacobian(sp, 2, cam, tt, Jp, idx + 1);
  if (st == RES_RANGE) return st;
  idx[0] = 6 * sp.n + 22 + l;
  TrajKin k;
  if (traj_kinematics<false>(sp, tt, &k) != RES_OK) return RES_NONUNIT;
  const v3 yh = cam_unproject(ci, u_ref, v_ref);
  const v3 ray = (1.0 / rho) * qrot(qmul(k.q, cam.q), yh);   // R_C y_h / rho
  const v3 pc = k.p + qrot(k.q, cam.p);
  P[0] = pc.x + ray.x; P[1] = pc.y + ray.y; P[2] = pc.z + ray.z;
  J[0][0] = -ray.x / rho; J[1][0] = -ray.y / rho; J[2][0] = -ray.z / rho;
#pragma unroll 1
  for (int c = 0; c < TCOV_W; ++c) {
    const v3 dphi = mk(Jp[3][c], Jp[4][c], Jp[5][c]);
    const v3 x = cross(dphi, ray);
    J[0][1 + c] = Jp[0][c] + x.x; J[1][1 + c] = Jp[1][c] + x.y; J[2][1 + c] = Jp[2][c] + x.z;
  }
  return st;
}

}  // namespace lvx
