// tests/native/projcov_host_check.cpp — TEST-ONLY host build of the pixel Jacobian, the 2 x 2 sandwich and eigenvalue, the decision chain and the LiDAR-in-camera
// covariance of lvx_projection_covariance (lvi-exc_amd/csrc/lvx_projcov.h), so that the CPU suite (-m "not gpu") can hold them against finite differences and numpy
// without a GPU, and the layout of the call's structs against the ctypes mirrors.  Not a CPU fallback: nothing here is linked into liblvx.so.
// Built with g++ -O2 -ffp-contract=off (as lvx_render.hip, which runs the same functions per point, is built).
#include <cmath>
#include <cstddef>

#include "../../include/lvx.h"
#include "../../lvi-exc_amd/csrc/lvx_projcov.h"

using namespace lvx;

namespace {
RenderPose pose_of(const double* q_xyzw, const double* p) { return render_pose(mkq(q_xyzw[3], q_xyzw[0], q_xyzw[1], q_xyzw[2]), mk(p[0], p[1], p[2])); }
}  // namespace

// uv [2] and A [2][12] row-major of the point xyz (float) given the camera pose (qc xyzw, pc) and the LiDAR pose at t_map (ql, pl); returns pt_C.z
extern "C" double pj_jacobian(const lvx_pinhole* cam, const double* qc, const double* pc, const double* ql, const double* pl, const float* xyz, double* uv2, double* A24) {
  const RenderPose C = pose_of(qc, pc), L0 = pose_of(ql, pl);
  const v3 pt_C = render_to_camera(xyz, L0, C);
  render_project(*cam, pt_C, uv2);
  double A[2][12];
  proj_pose_jacobian(*cam, xyz, L0, C, pt_C, A);
  for (int r = 0; r < 2; ++r) for (int c = 0; c < 12; ++c) A24[12 * r + c] = A[r][c];
  return pt_C.z;
}

// cov [4] = A P A^T with P given as a full symmetric 12 x 12 (its lower triangle is packed as the device's record holds it); out[0] = largest eigenvalue
extern "C" void pj_sandwich(const double* A24, const double* P144, double* cov4, double* out1) {
  double A[2][12], pc[PJ_NP];
  for (int r = 0; r < 2; ++r) for (int c = 0; c < 12; ++c) A[r][c] = A24[12 * r + c];
  for (int r = 0; r < 12; ++r) for (int c = 0; c <= r; ++c) pc[r * (r + 1) / 2 + c] = P144[12 * r + c];
  proj_sandwich(A, pc, cov4);
  out1[0] = proj_eig_max(cov4);
}
extern "C" double pj_eig_max(const double* cov4) { return proj_eig_max(cov4); }

// the decision chain over n_images camera poses (qc [n_images][4], pc [n_images][3], valid [n_images]) with a zero pose_cov: status, image and uv of n points
extern "C" void pj_decide(const lvx_pinhole* cam, int n_images, const double* qc, const double* pc, const int* valid, const double* ql, const double* pl, int map_valid, double z_min,
                          double z_max, int n, const float* xyzi4, unsigned char* status, int* image, double* uv) {
  static ProjTable tab;
  tab.L0 = pose_of(ql, pl); tab.map_valid = map_valid; tab.n_images = n_images; tab.status = 0;
  for (int k = 0; k < n_images; ++k) {
    tab.img[k].valid = valid[k];
    tab.img[k].C = pose_of(qc + 4 * k, pc + 3 * k);
    for (int e = 0; e < PJ_NP; ++e) tab.img[k].pc[e] = 0.0;
  }
  for (int i = 0; i < n; ++i) {
    ProjRecord r;
    proj_point_images(xyzi4 + 4 * (size_t)i, tab, *cam, z_min, z_max, &r);
    status[i] = (unsigned char)r.status; image[i] = r.image; uv[2 * i] = r.uv[0]; uv[2 * i + 1] = r.uv[1];
  }
}

extern "C" void pj_lidar_in_camera_cov(const double* calib_cov484, const double* state, int N, double* cov36) { lidar_in_camera_cov(calib_cov484, state, N, cov36); }

// sizeof and member offsets of the call's three structs, LVX_PROJ_COV_W and the timer ids
extern "C" void pj_layout(long long* out) {
  out[0] = sizeof(lvx_proj_cov_options); out[1] = offsetof(lvx_proj_cov_options, radius); out[2] = offsetof(lvx_proj_cov_options, jacobi_scaling);
  out[3] = offsetof(lvx_proj_cov_options, reserved); out[4] = offsetof(lvx_proj_cov_options, z_min); out[5] = offsetof(lvx_proj_cov_options, z_max);
  out[6] = sizeof(lvx_proj_cov_images); out[7] = offsetof(lvx_proj_cov_images, pose_cov); out[8] = offsetof(lvx_proj_cov_images, window_cov);
  out[9] = offsetof(lvx_proj_cov_images, window_idx); out[10] = offsetof(lvx_proj_cov_images, valid);
  out[11] = sizeof(lvx_proj_cov); out[12] = offsetof(lvx_proj_cov, uv); out[13] = offsetof(lvx_proj_cov, cov); out[14] = offsetof(lvx_proj_cov, sigma);
  out[15] = offsetof(lvx_proj_cov, sigma_max); out[16] = offsetof(lvx_proj_cov, image); out[17] = offsetof(lvx_proj_cov, status);
  out[18] = LVX_PROJ_COV_W; out[19] = LVX_KERNEL_PROJ_HUB; out[20] = LVX_KERNEL_PROJ_COV; out[21] = LVX_NUM_KERNELS_EXT;
}
