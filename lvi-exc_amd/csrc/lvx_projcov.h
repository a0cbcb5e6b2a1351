// lvx_projcov.h — a LiDAR map point carried into an image and the pixel covariance the two poses leave there, for lvx_projection_covariance.  Host- and
// device-callable (tests/native/projcov_host_check.cpp builds it with g++ -ffp-contract=off and holds it against central differences and numpy); the library runs its
// pieces inside k_proj_hub (lvx_selinv.h) and k_proj_cov (lvx_render.hip).
//
// The chain is RenderMap's (lvx_render.h): pt_G = R_L0 x + p_L0, pt_C = R_C^T (pt_G - p_C), uv = render_project(cam, pt_C).  The map point x is TAKEN AS GIVEN (its own
// uncertainty, lvx_map_point_covariance, correlates with the image pose off the factor's pattern).  With the pose errors of lvx_trajcov.h — dp = p' - p and the
// WORLD-frame rotation vector dphi, R' = Exp(dphi) R — of the camera pose (dp_C, dphi_C) and of the LiDAR pose (dp_L, dphi_L), r = R_L0 x and v = pt_G - p_C:
//   d pt_C = R_C^T ( -dp_C + [v]x dphi_C + dp_L - [r]x dphi_L )
// so with D (2 x 3) the derivative of render_project at pt_C and G = D R_C^T, the rows of A (2 x 12) are   A_i = ( -g_i,  g_i x v,  g_i,  r x g_i ).
// pose_cov (12 x 12, k_proj_hub: J12 W J12^T over the 62-scalar window) is one per image, 78 unique entries; cov_uv = A pose_cov A^T, every sum in index order.
#pragma once
#include "lvx_render.h"

namespace lvx {

enum { PJ_W = 62, PJ_NP = 78 };   // window scalars; unique entries of the symmetric 12 x 12: P(i, j) = pc[i (i + 1) / 2 + j], i >= j

// what k_proj_hub leaves per image, and the table one k_proj_cov launch reads
struct ProjImage { RenderPose C; double pc[PJ_NP]; int32_t valid, pad; };
// status: 0 ok, 1 a lost pivot, 2 the window of t_map is off the border (or t_map has left the trajectory), 3 a non-unit control quaternion at t_map (every point is
// skipped, as lvx_render_map_d skips them)
struct ProjTable { RenderPose L0; int32_t map_valid, n_images, status, pad; ProjImage img[LVX_RENDER_MAX_IMAGES]; };
struct ProjRecord { double uv[2], cov[4], sigma[2], sigma_max; int32_t image, status; };

// D = d render_project / d pt_C (2 x 3, row-major), all five distortion terms
LVX_HD void proj_project_jacobian(const lvx_pinhole& cam, v3 pt_C, double D[6]) {
  const double iz = 1.0 / pt_C.z;
  const double x = pt_C.x * iz, y = pt_C.y * iz;
  const double r2 = x * x + y * y;
  const double d = 1 + cam.k1 * r2 + cam.k2 * r2 * r2 + cam.k3 * r2 * r2 * r2;
  const double dd = cam.k1 + 2 * cam.k2 * r2 + 3 * cam.k3 * r2 * r2;   // d' by r2
  const double ux = d + 2 * x * x * dd + 2 * cam.p1 * y + 6 * cam.p2 * x;
  const double uy = 2 * x * y * dd + 2 * cam.p1 * x + 2 * cam.p2 * y;
  const double vx = uy;
  const double vy = d + 2 * y * y * dd + 6 * cam.p1 * y + 2 * cam.p2 * x;
  // (x, y) by pt_C: (iz, 0, -x iz; 0, iz, -y iz)
  D[0] = cam.fx * ux * iz; D[1] = cam.fx * uy * iz; D[2] = -cam.fx * (ux * x + uy * y) * iz;
  D[3] = cam.fy * vx * iz; D[4] = cam.fy * vy * iz; D[5] = -cam.fy * (vx * x + vy * y) * iz;
}

// A (2 x 12) over (camera dp, dphi; LiDAR dp, dphi) for the point xyz; pt_C as render_to_camera gives it
LVX_HD void proj_pose_jacobian(const lvx_pinhole& cam, const float xyz[3], const RenderPose& L0, const RenderPose& C, v3 pt_C, double A[2][12]) {
  const double x = (double)xyz[0], y = (double)xyz[1], z = (double)xyz[2];
  const v3 r = mk(L0.R[0] * x + L0.R[1] * y + L0.R[2] * z, L0.R[3] * x + L0.R[4] * y + L0.R[5] * z, L0.R[6] * x + L0.R[7] * y + L0.R[8] * z);
  const v3 v = mk((r.x + L0.p[0]) - C.p[0], (r.y + L0.p[1]) - C.p[1], (r.z + L0.p[2]) - C.p[2]);
  double D[6];
  proj_project_jacobian(cam, pt_C, D);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double a = D[3 * i], b = D[3 * i + 1], c = D[3 * i + 2];
    const v3 g = mk(C.R[0] * a + C.R[1] * b + C.R[2] * c, C.R[3] * a + C.R[4] * b + C.R[5] * c, C.R[6] * a + C.R[7] * b + C.R[8] * c);   // (D R_C^T)_i = R_C D_i
    const v3 gv = cross(g, v), rg = cross(r, g);
    A[i][0] = -g.x; A[i][1] = -g.y; A[i][2] = -g.z; A[i][3] = gv.x; A[i][4] = gv.y; A[i][5] = gv.z;
    A[i][6] = g.x; A[i][7] = g.y; A[i][8] = g.z; A[i][9] = rg.x; A[i][10] = rg.y; A[i][11] = rg.z;
  }
}

// cov = A P A^T (row-major 2 x 2, symmetric), P from its 78 lower entries: T = A P over a ascending, then T A^T over b ascending
LVX_HD void proj_sandwich(const double A[2][12], const double* pc, double cov[4]) {
  double T[2][12];
#pragma unroll
  for (int b = 0; b < 12; ++b) {
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int a = 0; a < 12; ++a) { const double p = a >= b ? pc[a * (a + 1) / 2 + b] : pc[b * (b + 1) / 2 + a]; t0 += A[0][a] * p; t1 += A[1][a] * p; }
    T[0][b] = t0; T[1][b] = t1;
  }
  double c00 = 0.0, c10 = 0.0, c11 = 0.0;
#pragma unroll
  for (int b = 0; b < 12; ++b) { c00 += T[0][b] * A[0][b]; c10 += T[1][b] * A[0][b]; c11 += T[1][b] * A[1][b]; }
  cov[0] = c00; cov[1] = c10; cov[2] = c10; cov[3] = c11;
}

// largest eigenvalue of a symmetric 2 x 2 in closed form: the mean of the diagonal plus the radius (no cancellation: both terms are >= 0 for a PSD matrix)
LVX_HD double proj_eig_max(const double cov[4]) {
  const double m = 0.5 * (cov[0] + cov[3]), h = 0.5 * (cov[0] - cov[3]);
  return m + sqrt(h * h + cov[1] * cov[1]);
}
LVX_HD double proj_sqrt0(double x) { return sqrt(x > 0.0 ? x : (x == x ? 0.0 : x)); }   // a value below zero by rounding counts as zero; NaN stays

// One map point over the images of a table: render_point_images's rule and its decisions (render_point_pixel, the function render_point itself decides by), the
// record of the lowest-index valid image that holds the point.  rec is zero with image -1 unless the point is projected.
LVX_HD int proj_point_images(const float xyz[3], const ProjTable& tab, const lvx_pinhole& cam, double z_min, double z_max, ProjRecord* rec) {
  rec->uv[0] = rec->uv[1] = 0.0; rec->cov[0] = rec->cov[1] = rec->cov[2] = rec->cov[3] = 0.0; rec->sigma[0] = rec->sigma[1] = 0.0; rec->sigma_max = 0.0;
  rec->image = -1; rec->status = RENDER_SKIPPED;
  if (!tab.map_valid) return RENDER_SKIPPED;
  int st = RENDER_SKIPPED;
  for (int k = 0; k < tab.n_images; ++k) {
    const ProjImage& im = tab.img[k];
    if (!im.valid) continue;
    v3 pt_C; double uv[2]; int iu, iv;
    const int s = render_point_pixel(xyz, tab.L0, im.C, cam, z_min, z_max, &pt_C, uv, &iu, &iv);   // render_point's own decisions
    if (s > st) st = s;
    if (s != RENDER_COLORED) continue;
    double A[2][12];
    proj_pose_jacobian(cam, xyz, tab.L0, im.C, pt_C, A);
    proj_sandwich(A, im.pc, rec->cov);
    rec->uv[0] = uv[0]; rec->uv[1] = uv[1];
    rec->sigma[0] = proj_sqrt0(rec->cov[0]); rec->sigma[1] = proj_sqrt0(rec->cov[3]);
    rec->sigma_max = proj_sqrt0(proj_eig_max(rec->cov));
    rec->image = k;
    st = RENDER_COLORED;
    break;
  }
  rec->status = st;
  return st;
}

// The rig's LiDAR-in-camera extrinsic T_CL = T_CI^-1 T_LI (R_CL = R_CI^T R_LI, p_CL = R_CI^T (p_LI - p_CI)) and its 6 x 6 covariance over (dp, dphi) — dp = p' - p,
// R' = Exp(dphi) R, both in the camera frame: the pose-error convention above — from the 22 x 22 calibration covariance of lvx_calibration_covariance (calib_cov,
// row-major; scalars 8..10 theta_L, 11..13 p_L, 15..17 theta_C, 18..20 p_C).  A theta is a HALF-angle applied on the left (q' = Exp(2 theta) q), hence the factor 2:
//   dphi = 2 R_CI^T (theta_L - theta_C),   dp = R_CI^T (dp_L - dp_C) + 2 R_CI^T [p_LI - p_CI]x theta_C
// state: the library's state vector, N its knot count.  Host code (the device has pose_cov).
inline void lidar_in_camera_cov(const double* calib_cov, const double* state, int N, double cov36[36]) {
  const double* sl = state + 7 * (size_t)N + 16; const double* sc = sl + 8;
  const m3 Rc = rotmat(mkq(sc[3], sc[0], sc[1], sc[2]));
  const m3 K = skew(mk(sl[4] - sc[4], sl[5] - sc[5], sl[6] - sc[6]));
  static const int col[12] = {8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20};
  double J[6][12];
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 12; ++c) J[r][c] = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double rt = Rc.a[3 * b + a];   // R_CI^T (a, b)
      double rk = 0.0;
      for (int m = 0; m < 3; ++m) rk += Rc.a[3 * m + a] * K.a[3 * m + b];   // (R_CI^T K)(a, b)
      J[3 + a][b] = 2.0 * rt; J[3 + a][6 + b] = -2.0 * rt;
      J[a][3 + b] = rt; J[a][9 + b] = -rt; J[a][6 + b] = 2.0 * rk;
    }
  double T[6][12];
  for (int r = 0; r < 6; ++r) for (int b = 0; b < 12; ++b) { double s = 0.0; for (int a = 0; a < 12; ++a) s += J[r][a] * calib_cov[col[a] * 22 + col[b]]; T[r][b] = s; }
  for (int r = 0; r < 6; ++r) for (int s2 = 0; s2 <= r; ++s2) { double s = 0.0; for (int b = 0; b < 12; ++b) s += T[r][b] * J[s2][b]; cov36[6 * r + s2] = s; cov36[6 * s2 + r] = s; }
}

}  // namespace lvx
