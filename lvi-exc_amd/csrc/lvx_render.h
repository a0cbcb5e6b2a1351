// lvx_render.h — per-point math of the coloured map and of the LiDAR-to-image overlay, host- and device-callable.
//
// Restated from the reference (src/lvi_exc/test/lvi_initialize_surfel_orb.cpp):
//   LIinitializer::RenderMap                   :711-811   (per point :749-793)
//   LIinitializer::ReprojectPointCloudToImage  :1307-1363 (per point :1343-1353)
// The kernels of lvx_render.hip call these functions one lane per point; tests/native/render_host_check.cpp builds them with g++ (-ffp-contract=off, as
// lvx_render.hip is built) so that the CPU suite compares them with an independent float64 restatement and the GPU suite compares the kernels with them byte for byte.
#pragma once
#include <string.h>

#include "../../include/lvx.h"
#include "lvx_math.h"

namespace lvx {

struct RenderPose { double R[9]; double p[3]; };   // row-major rotation of the NORMALISED quaternion (q.normalize(); toRotationMatrix(): :724-727, :744-746) and translation
// what one launch reads: T_L0inG, then the candidate images' T_CinG in order (valid = 0: evaluateCameraPose failed, the image is passed over as :738-741)
struct RenderTable { RenderPose L0; int32_t map_valid, n_images; RenderPose cam[LVX_RENDER_MAX_IMAGES]; int32_t valid[LVX_RENDER_MAX_IMAGES]; };

enum { RENDER_SKIPPED = 0, RENDER_OUTSIDE = 1, RENDER_COLORED = 2 };

LVX_HD RenderPose render_pose(quat q, v3 p) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  const m3 R = rotmat(mkq(q.w / n, q.x / n, q.y / n, q.z / n));
  RenderPose o;
  for (int i = 0; i < 9; ++i) o.R[i] = R.a[i];
  o.p[0] = p.x; o.p[1] = p.y; o.p[2] = p.z;
  return o;
}

// the inline radtan projection of RenderMap (:766-779): k1, k2, k3 (r^6), p1, p2, then fx, fy, cx, cy
LVX_HD void render_project(const lvx_pinhole& cam, v3 pt_C, double uv[2]) {
  const double tmpx = pt_C.x / pt_C.z, tmpy = pt_C.y / pt_C.z;
  const double r2 = tmpx * tmpx + tmpy * tmpy;
  const double tmpdist = 1 + cam.k1 * r2 + cam.k2 * r2 * r2 + cam.k3 * r2 * r2 * r2;
  const double u = tmpx * tmpdist + 2 * cam.p1 * tmpx * tmpy + cam.p2 * (r2 + 2 * tmpx * tmpx);
  const double v = tmpy * tmpdist + cam.p1 * (r2 + 2 * tmpy * tmpy) + 2 * cam.p2 * tmpx * tmpy;
  uv[0] = cam.fx * u + cam.cx;
  uv[1] = cam.fy * v + cam.cy;
}
// int(uv) of :781-784 and :1350-1351.  The reference casts whatever the projection gave; the cast of a NaN, an infinity or a value beyond the int range is undefined
// behaviour there.  Here a coordinate that is not finite or lies beyond +-2^30 is OUTSIDE the image (no image is that wide), so the cast below is always defined.
LVX_HD bool render_trunc(double x, int* i) {
  if (!(x > -1073741824.0 && x < 1073741824.0)) return false;
  *i = (int)x;
  return true;
}

// pt_G = T_L0inG * ept (:754); pt_C = T_GtoC * pt_G (:755): the rigid inverse R_C^T (pt_G - p_CinG), not a general 4 x 4 inverse
LVX_HD v3 render_to_camera(const float xyz[3], const RenderPose& L0, const RenderPose& C) {
  const double x = (double)xyz[0], y = (double)xyz[1], z = (double)xyz[2];
  const double gx = L0.R[0] * x + L0.R[1] * y + L0.R[2] * z + L0.p[0];
  const double gy = L0.R[3] * x + L0.R[4] * y + L0.R[5] * z + L0.p[1];
  const double gz = L0.R[6] * x + L0.R[7] * y + L0.R[8] * z + L0.p[2];
  const double dx = gx - C.p[0], dy = gy - C.p[1], dz = gz - C.p[2];
  return mk(C.R[0] * dx + C.R[3] * dy + C.R[6] * dz, C.R[1] * dx + C.R[4] * dy + C.R[7] * dz, C.R[2] * dx + C.R[5] * dy + C.R[8] * dz);
}

// One map point in one image (:749-793).  rec must be all zero on entry of the FIRST image and is only ever written with the point's xyz / colour, so calling this for
// image after image until it returns RENDER_COLORED leaves the record of the lowest-index image that colours the point.
// The decisions of one map point in one image (:752-784), shared by render_point and by lvx_projection_covariance's chain (lvx_projcov.h: proj_point_images), so that
// the two cannot drift apart: RENDER_SKIPPED (a NaN coordinate, out of depth range; nothing is written), RENDER_OUTSIDE (pt_C and, when the projection is finite, uv
// are written) or RENDER_COLORED (pt_C, uv and the pixel iu, iv).
LVX_HD int render_point_pixel(const float xyz[3], const RenderPose& L0, const RenderPose& C, const lvx_pinhole& cam, double z_min, double z_max, v3* pt_C, double uv[2], int* iu,
                              int* iv) {
  if (xyz[0] != xyz[0] || xyz[1] != xyz[1] || xyz[2] != xyz[2]) return RENDER_SKIPPED;   // pcl_isnan (:752)
  const v3 pc = render_to_camera(xyz, L0, C);
  if (pc.z < z_min || pc.z > z_max) return RENDER_SKIPPED;   // :757
  *pt_C = pc;
  render_project(cam, pc, uv);
  if (!render_trunc(uv[0], iu) || !render_trunc(uv[1], iv)) return RENDER_OUTSIDE;
  if (*iu < 0 || *iv < 0 || *iu > cam.cols - 1 || *iv > cam.rows - 1) return RENDER_OUTSIDE;   // :781-784: on int(uv), so uv in (-1, 0) truncates to 0 and is INSIDE
  return RENDER_COLORED;
}

LVX_HD int render_point(const float xyz[3], const RenderPose& L0, const RenderPose& C, const lvx_pinhole& cam, const uint8_t* image, int pitch, double z_min, double z_max,
                        lvx_point_xyzrgb* rec) {
  v3 pt_C; double uv[2]; int iu = 0, iv = 0;
  const int s = render_point_pixel(xyz, L0, C, cam, z_min, z_max, &pt_C, uv, &iu, &iv);
  if (s == RENDER_SKIPPED) return s;
  rec->x = xyz[0]; rec->y = xyz[1]; rec->z = xyz[2];             // :759-762
  if (s == RENDER_OUTSIDE) return s;
  const uint8_t g = image[(size_t)iv * (size_t)pitch + (size_t)iu];                        // img.at<u_char>(int(uv[1]), int(uv[0])) (:785)
  rec->b = g; rec->g = g; rec->r = g; rec->a = 255;
  return RENDER_COLORED;
}

// One map point over the candidate images of a table: the colour of the lowest-index valid image that colours it; xyz stays when any valid image had it in depth range.
// images: the table's images [rows][pitch] back to back.  A table whose map pose is invalid (map time outside the spline, :720-723) leaves every record zero.
LVX_HD int render_point_images(const float xyz[3], const RenderTable& tab, const lvx_pinhole& cam, const uint8_t* images, int pitch, double z_min, double z_max, lvx_point_xyzrgb* rec) {
  memset(rec, 0, sizeof(*rec));
  int st = RENDER_SKIPPED;
  if (!tab.map_valid) return st;
  const size_t image_bytes = (size_t)cam.rows * (size_t)pitch;
  for (int k = 0; k < tab.n_images; ++k) {
    if (!tab.valid[k]) continue;
    const int s = render_point(xyz, tab.L0, tab.cam[k], cam, images + (size_t)k * image_bytes, pitch, z_min, z_max, rec);
    if (s > st) st = s;
    if (s == RENDER_COLORED) break;
  }
  return st;
}

// q_LtoC = q_CtoG* (x) q_LtoG, p_LinC = q_CtoG* (p_LinG - p_CinG) (:1335-1336)
LVX_HD void overlay_chain(quat q_LtoG, v3 p_LinG, quat q_CtoG, v3 p_CinG, quat* q_LtoC, v3* p_LinC) {
  *q_LtoC = qmul(qconj(q_CtoG), q_LtoG);
  *p_LinC = qrot(qconj(q_CtoG), p_LinG - p_CinG);
}
// One scan point in its image (:1343-1353): the pixel index int(v) * cols + int(u), or -1.  The bounds test differs from RenderMap's: uv < 0 is tested on the DOUBLES, so
// uv in (-1, 0) is OUTSIDE here.  The reference projects with the camodocal model (camera->spaceToPlane); this uses RenderMap's formula.
LVX_HD int overlay_point(const float xyz[3], quat q_LtoC, v3 p_LinC, const lvx_pinhole& cam) {
  const v3 pt_c = qrot(q_LtoC, mk((double)xyz[0], (double)xyz[1], (double)xyz[2])) + p_LinC;   // :1345
  if (pt_c.z < 0) return -1;                                                                    // :1346
  double uv[2];
  render_project(cam, pt_c, uv);
  int iu, iv;
  if (!render_trunc(uv[0], &iu) || !render_trunc(uv[1], &iv)) return -1;   // (a NaN point ends here: the reference's casts are undefined for it)
  if (uv[0] < 0 || uv[1] < 0 || iu > cam.cols - 1 || iv > cam.rows - 1) return -1;   // :1350-1351
  return iv * cam.cols + iu;
}

}  // namespace lvx
