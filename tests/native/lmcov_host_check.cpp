// tests/native/lmcov_host_check.cpp — TEST-ONLY host build of the map point and its 3 x 32 Jacobian of lvx_landmark_covariance (lvi-exc_amd/csrc/lvx_lmcov.h), so that
// the CPU suite (-m "not gpu") can hold it against finite differences without a GPU, and the layout of the call's two structs against the ctypes mirrors.
// Not a CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2.
#include <cmath>
#include <cstddef>

#include "../../include/lvx.h"
#include "../../lvi-exc_amd/csrc/lvx_lmcov.h"

using namespace lvx;

namespace {
// cam10: fx fy cx cy k1 k2 p1 p2 k3 readout, as lvx_set_camera derives the rest (lvx_api.hip)
CamIntr intrinsics(const double* cam10, int rows, int cols) {
  CamIntr k{};
  k.fx = cam10[0]; k.fy = cam10[1]; k.cx = cam10[2]; k.cy = cam10[3]; k.k1 = cam10[4]; k.k2 = cam10[5]; k.p1 = cam10[6]; k.p2 = cam10[7]; k.k3 = cam10[8]; k.readout = cam10[9];
  k.rows = rows; k.cols = cols;
  k.inv_K11 = 1.0 / k.fx; k.inv_K13 = -k.cx / k.fx; k.inv_K22 = 1.0 / k.fy; k.inv_K23 = -k.cy / k.fy;
  k.do_distortion = (std::fabs(k.k1) > 1e-5 || std::fabs(k.k2) > 1e-5 || std::fabs(k.p1) > 1e-5 || std::fabs(k.p1) > 1e-5) ? 1 : 0;
  return k;
}
}  // namespace

// J [3][32] row-major, idx [32], P [3], yh [3]; the camera's extrinsics and rho_l are read from the state.  Returns the status (0 ok, 1 range, 2 non-unit quaternion)
extern "C" int lc_jacobian(const double* state, int N, double t0, double dt, const double* cam10, int rows, int cols, int l, double u_ref, double v_ref, double t0_ref,
                           double* J96, int* idx32, double* P3, double* yh3) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const CamIntr ci = intrinsics(cam10, rows, cols);
  const double* ss = state + 7 * (size_t)N + 24;
  SensorCal cam; cam.q = load_q(ss); cam.p = load_v3(ss + 4); cam.tau = ss[7];
  double Jp[6][TCOV_W], J[3][LCOV_W], P[3]; int idx[LCOV_W];
  const int st = landmark_point_jacobian(sp, ci, cam, l, u_ref, v_ref, t0_ref, state[7 * (size_t)N + 32 + l], Jp, J, idx, P);
  if (st == RES_RANGE) return st;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < LCOV_W; ++c) J96[r * LCOV_W + c] = J[r][c];
  for (int c = 0; c < LCOV_W; ++c) idx32[c] = idx[c];
  for (int r = 0; r < 3; ++r) P3[r] = P[r];
  const v3 yh = cam_unproject(ci, u_ref, v_ref);
  yh3[0] = yh.x; yh3[1] = yh.y; yh3[2] = yh.z;
  return st;
}

// sizeof and member offsets of lvx_landmark_cov_options (4 words) and lvx_landmark_cov (8 words), LVX_LM_COV_W
extern "C" void lc_layout(long long* out) {
  out[0] = sizeof(lvx_landmark_cov_options); out[1] = offsetof(lvx_landmark_cov_options, radius); out[2] = offsetof(lvx_landmark_cov_options, jacobi_scaling);
  out[3] = offsetof(lvx_landmark_cov_options, reserved);
  out[4] = sizeof(lvx_landmark_cov); out[5] = offsetof(lvx_landmark_cov, var_rho); out[6] = offsetof(lvx_landmark_cov, sigma_rho); out[7] = offsetof(lvx_landmark_cov, point);
  out[8] = offsetof(lvx_landmark_cov, point_cov); out[9] = offsetof(lvx_landmark_cov, window_cov); out[10] = offsetof(lvx_landmark_cov, window_idx);
  out[11] = offsetof(lvx_landmark_cov, valid); out[12] = LVX_LM_COV_W;
}
