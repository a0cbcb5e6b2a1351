// lvx_ptcov.h — a LiDAR point carried into the map frame and its Jacobian for lvx_map_point_covariance.  Host-callable (tests/native/ptcov_host_check.cpp builds it
// with g++ and holds it against central differences); the library runs its pieces inside k_pt_hub / k_point_cov (lvx_selinv.h).
//
// The chain of LiDARSurfelPoint::reprojectPoint2map (lidar_surfel_point.h:34-69) and undistortScanInMap: with (R_Sk, p_Sk) the LVX_FRAME_LIDAR pose at t_k + tau_L and
// (R_S0, p_S0) the one at t_map + tau_L,
//   X_w = R_Sk p_L + p_Sk,     p_M = R_S0^T (X_w - p_S0)                                  (the LiDAR frame at t_map)
// With Jk, J0 the pose Jacobians of traj_pose_jacobian (lvx_trajcov.h: dp and the WORLD-frame dphi by the 31 scalars of a LiDAR-frame pose) at the two times,
// A_k = (I, -[R_Sk p_L]x) and A_0 = (I, -[X_w - p_S0]x), the 3 x 55 Jacobian of p_M is
//   J[:,  0..23] =  R_S0^T A_k Jk[:, 0..23]                          the four knots of the pose at t_k + tau_L
//   J[:, 24..47] = -R_S0^T A_0 J0[:, 0..23]                          the four knots of the pose at t_map + tau_L (hub knots: border slots of the factor)
//   J[:, 48..54] =  R_S0^T (A_k Jk[:, 24..30] - A_0 J0[:, 24..30])   the LiDAR's theta (3), p (3), tau (1)
// idx[c]: the tangent index of column c (locks are the caller's business: ord[]).  When t_k falls into the window of t_map the SAME index stands in both knot groups.
// That is correct as it stands: the window of Sigma is gathered BY INDEX, so the repeated scalar has identical rows in both places (W(a, b) = Sigma(idx a, idx b)) and
// J W J^T is the covariance under the sum of the two columns; nothing is merged or dropped.
//
// The device does not form the 3 x 55 matrix per point.  With d_k / d_0 the 31 scalars of the two poses (the LiDAR's seven in both), Gk = A_k Jk, G0 = A_0 J0 (3 x 31):
//   R_S0 cov R_S0^T = Gk Wkk Gk^T - Gk Wk0 G0^T - (Gk Wk0 G0^T)^T + G0 W00 G0^T,     Wkk = Cov(d_k, d_k), Wk0 = Cov(d_k, d_0), W00 = Cov(d_0, d_0)
// G0 W00 G0^T = A_0 (J0 W00 J0^T) A_0^T and Gk Wk0 G0^T = Gk (Wk0 J0^T) A_0^T: J0, C00 = J0 W00 J0^T are one per call, B0 = Wk0 J0^T (31 x 6) one per knot interval,
// and the per-point product is T = Gk [Wkk | B0] (pt_cov_assemble takes it from there).  Column a of the k-window is column a (a < 24) or 24 + a of the 55; column b
// of the 0-window is column 24 + b.
#pragma once
#include "lvx_symeig.h"
#include "lvx_trajcov.h"

namespace lvx {

enum { PCOV_W = 55, PCOV_TW = 38 };   // PCOV_TW: columns of T that are read: 0..30 Gk Wkk, 32..37 Gk B0

// the LVX_FRAME_LIDAR pose at tt (tau_L added by the caller): q_S = q(tt) q_LI, p_S = p(tt) + q(tt) p_LI
LVX_HD int pt_lidar_pose(const SplineRef& sp, const SensorCal& lidar, double tt, quat* q, v3* p) {
  TrajKin k;
  const int st = traj_kinematics<false>(sp, tt, &k);
  if (st != RES_OK) return st;
  *q = qmul(k.q, lidar.q); *p = k.p + qrot(k.q, lidar.p);
  return RES_OK;
}
// G = (I, -[r]x) Jp: what the pose's 31 scalars do to a point rigidly attached to the sensor at offset r (world axes)
LVX_HD void pt_lever(const double Jp[6][TCOV_W], v3 r, double G[3][TCOV_W]) {
#pragma unroll
  for (int c = 0; c < TCOV_W; ++c) {
    const v3 x = cross(mk(Jp[3][c], Jp[4][c], Jp[5][c]), r);
    G[0][c] = Jp[0][c] + x.x; G[1][c] = Jp[1][c] + x.y; G[2][c] = Jp[2][c] + x.z;
  }
}
// One point's geometry given the two sensor poses: r = R_Sk p_L, v = X_w - p_S0, p_M = R_S0^T v
LVX_HD void pt_chain(quat qk, v3 pk, quat q0, v3 p0, v3 pL, v3* r, v3* v, v3* pm) {
  *r = qrot(qk, pL);
  *v = (*r + pk) - p0;
  *pm = qrot_inv(q0, *v);
}

// Jk, J0: the caller's room for the two pose Jacobians.  Returns RES_OK, RES_RANGE (either time outside the trajectory; nothing is written) or RES_NONUNIT.
LVX_HD int map_point_jacobian(const SplineRef& sp, const SensorCal& lidar, double t_map, double t_k, v3 pL, double Jk[6][TCOV_W], double J0[6][TCOV_W],
                              double J[3][PCOV_W], int idx[PCOV_W], double P[3]) {
  KnotRef kr;
  if (!traj_knot(sp.t0, sp.dt, sp.n, t_map + lidar.tau, &kr) || !traj_knot(sp.t0, sp.dt, sp.n, t_k + lidar.tau, &kr)) return RES_RANGE;
  int ik[TCOV_W], i0[TCOV_W];
  const int s0 = traj_pose_jacobian(sp, 1, lidar, t_map + lidar.tau, J0, i0);
  const int sk = traj_pose_jacobian(sp, 1, lidar, t_k + lidar.tau, Jk, ik);
  quat qk, q0; v3 pk, p0;
  if (s0 != RES_OK || sk != RES_OK || pt_lidar_pose(sp, lidar, t_k + lidar.tau, &qk, &pk) != RES_OK || pt_lidar_pose(sp, lidar, t_map + lidar.tau, &q0, &p0) != RES_OK) return RES_NONUNIT;
  v3 r, v, pm;
  pt_chain(qk, pk, q0, p0, pL, &r, &v, &pm);
  P[0] = pm.x; P[1] = pm.y; P[2] = pm.z;
  double Gk[3][TCOV_W], G0[3][TCOV_W];
  pt_lever(Jk, r, Gk); pt_lever(J0, v, G0);
  const m3 R0 = rotmat(q0);
  for (int c = 0; c < PCOV_W; ++c) {
    const int a = c < 24 ? c : c - 24;   // the pose scalar behind column c (both poses' for c >= 48)
    v3 g;
    if (c < 24) g = mk(Gk[0][a], Gk[1][a], Gk[2][a]);
    else if (c < 48) g = mk(-G0[0][a], -G0[1][a], -G0[2][a]);
    else g = mk(Gk[0][a] - G0[0][a], Gk[1][a] - G0[1][a], Gk[2][a] - G0[2][a]);
    const v3 j = tmulv(R0, g);
    J[0][c] = j.x; J[1][c] = j.y; J[2][c] = j.z;
    idx[c] = (c >= 24 && c < 48) ? i0[a] : ik[a];
  }
  return RES_OK;
}

// cov = R_S0^T (Mkk - X - X^T + A_0 C00 A_0^T) R_S0 from T = Gk [Wkk | . | B0] (row stride ldt; columns 0..30 and 32..37 are read), every sum in index order.
//   Mkk = T[:, 0..30] Gk^T (lower triangle computed, mirrored),   X = T[:, 32..37] A_0^T,   A_0 = (I, -[v]x)
LVX_HD void pt_cov_assemble(const double Gk[3][TCOV_W], const double* T, int ldt, const double C00[36], v3 v, const m3& R0, double cov[9]) {
  const m3 K = skew(v);   // A_0 = (I, -K)
  double M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s <= r; ++s) {
      double m = 0.0;
#pragma unroll
      for (int b = 0; b < TCOV_W; ++b) m += T[r * ldt + b] * Gk[s][b];
      M[3 * r + s] = m; M[3 * s + r] = m;
    }
  double X[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      double x = T[r * ldt + 32 + s];
#pragma unroll
      for (int c = 0; c < 3; ++c) x -= T[r * ldt + 35 + c] * K.a[3 * s + c];
      X[3 * r + s] = x;
    }
  double U[18];   // A_0 C00 (3 x 6)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double u = C00[6 * r + b];
#pragma unroll
      for (int c = 0; c < 3; ++c) u -= K.a[3 * r + c] * C00[6 * (3 + c) + b];
      U[6 * r + b] = u;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s <= r; ++s) {
      double z = U[6 * r + s];
#pragma unroll
      for (int c = 0; c < 3; ++c) z -= U[6 * r + 3 + c] * K.a[3 * s + c];
      const double m = (M[3 * r + s] - (X[3 * r + s] + X[3 * s + r])) + z;
      M[3 * r + s] = m; M[3 * s + r] = m;
    }
  double Q[9];   // M R0
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) Q[3 * r + s] = M[3 * r] * R0.a[s] + M[3 * r + 1] * R0.a[3 + s] + M[3 * r + 2] * R0.a[6 + s];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s <= r; ++s) {
      const double c = R0.a[r] * Q[s] + R0.a[3 + r] * Q[3 + s] + R0.a[6 + r] * Q[6 + s];
      cov[3 * r + s] = c; cov[3 * s + r] = c;
    }
}

// sqrt of the largest eigenvalue of a symmetric 3 x 3 (row-major, both triangles): the cyclic Jacobi of lvx_symeig.h on one lane.  A matrix that is not finite gives NaN.
LVX_HD double pt_sigma_max(const double C[9]) {
  double A[9], V[9], cs[8];
  for (int e = 0; e < 9; ++e) A[e] = C[e];
  int sweeps; double off;
  symeig_jacobi(A, 3, 3, V, 3, cs, 30, 0, 1, SymeigNoSync(), &sweeps, &off);
  double m = A[0];
  if (A[4] > m) m = A[4];
  if (A[8] > m) m = A[8];
  return sqrt(m > 0.0 ? m : (m == m ? 0.0 : m));
}
// dir^T C dir, rows in order
LVX_HD double pt_var_dir(const double C[9], v3 d) {
  const v3 cd = mk(C[0] * d.x + C[1] * d.y + C[2] * d.z, C[3] * d.x + C[4] * d.y + C[5] * d.z, C[6] * d.x + C[7] * d.y + C[8] * d.z);
  return d.x * cd.x + d.y * cd.y + d.z * cd.z;
}

}  // namespace lvx
