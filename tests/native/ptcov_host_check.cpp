// tests/native/ptcov_host_check.cpp — TEST-ONLY host build of the map point, its 3 x 55 Jacobian and the factored covariance of lvx_map_point_covariance
// (lvi-exc_amd/csrc/lvx_ptcov.h), so that the CPU suite (-m "not gpu") can hold them against finite differences and numpy without a GPU, and the layout of the call's
// two structs against the ctypes mirrors.  Not a CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2.
#include <cmath>
#include <cstddef>

#include "../../include/lvx.h"
#include "../../lvi-exc_amd/csrc/lvx_ptcov.h"

using namespace lvx;

namespace {
SensorCal lidar_of(const double* state, int N) {
  const double* ss = state + 7 * (size_t)N + 16;
  SensorCal ext; ext.q = load_q(ss); ext.p = load_v3(ss + 4); ext.tau = ss[7];
  return ext;
}
}  // namespace

// J [3][55] row-major, idx [55], P [3]; the LiDAR's extrinsics are read from the state.  Returns the status (0 ok, 1 range, 2 non-unit quaternion)
extern "C" int pc_jacobian(const double* state, int N, double t0, double dt, double t_map, double t_k, const double* pL3, double* J165, int* idx55, double* P3) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  double Jk[6][TCOV_W], J0[6][TCOV_W], J[3][PCOV_W], P[3]; int idx[PCOV_W];
  const int st = map_point_jacobian(sp, lidar_of(state, N), t_map, t_k, mk(pL3[0], pL3[1], pL3[2]), Jk, J0, J, idx, P);
  if (st != RES_OK) return st;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < PCOV_W; ++c) J165[r * PCOV_W + c] = J[r][c];
  for (int c = 0; c < PCOV_W; ++c) idx55[c] = idx[c];
  for (int r = 0; r < 3; ++r) P3[r] = P[r];
  return st;
}

// cov [9] as k_pt_hub / k_point_cov form it, from a 55 x 55 window W (row-major, symmetric): C00 = J0 W00 J0^T, B0 = Wk0 J0^T, T = Gk [Wkk | B0], pt_cov_assemble.
// Column a of the k-window stands at a (a < 24) or 24 + a of the 55, column b of the 0-window at 24 + b.
extern "C" int pc_factored(const double* state, int N, double t0, double dt, double t_map, double t_k, const double* pL3, const double* W, double* cov9) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const SensorCal ext = lidar_of(state, N);
  double Jk[6][TCOV_W], J0[6][TCOV_W]; int ik[TCOV_W], i0[TCOV_W];
  if (traj_pose_jacobian(sp, 1, ext, t_map + ext.tau, J0, i0) != RES_OK || traj_pose_jacobian(sp, 1, ext, t_k + ext.tau, Jk, ik) != RES_OK) return 1;
  quat qk, q0; v3 pk, p0;
  if (pt_lidar_pose(sp, ext, t_k + ext.tau, &qk, &pk) != RES_OK || pt_lidar_pose(sp, ext, t_map + ext.tau, &q0, &p0) != RES_OK) return 1;
  v3 r, v, pm;
  pt_chain(qk, pk, q0, p0, mk(pL3[0], pL3[1], pL3[2]), &r, &v, &pm);
  double Gk[3][TCOV_W];
  pt_lever(Jk, r, Gk);
  auto ka = [](int a) { return a < 24 ? a : 24 + a; };
  auto w = [&](int A, int B) { return W[A * PCOV_W + B]; };
  double C00[36], T0[6][TCOV_W];
  for (int m = 0; m < 6; ++m) for (int b = 0; b < TCOV_W; ++b) { double s = 0.0; for (int a = 0; a < TCOV_W; ++a) s += J0[m][a] * w(24 + a, 24 + b); T0[m][b] = s; }
  for (int m = 0; m < 6; ++m) for (int q = 0; q < 6; ++q) { double s = 0.0; for (int b = 0; b < TCOV_W; ++b) s += T0[m][b] * J0[q][b]; C00[6 * m + q] = s; }
  double B0[TCOV_W][6];
  for (int a = 0; a < TCOV_W; ++a) for (int m = 0; m < 6; ++m) { double s = 0.0; for (int b = 0; b < TCOV_W; ++b) s += w(ka(a), 24 + b) * J0[m][b]; B0[a][m] = s; }
  double T[3][PCOV_TW];
  for (int rr = 0; rr < 3; ++rr) {
    for (int b = 0; b < PCOV_TW; ++b) T[rr][b] = 0.0;
    for (int b = 0; b < TCOV_W; ++b) { double s = 0.0; for (int a = 0; a < TCOV_W; ++a) s += Gk[rr][a] * w(ka(a), ka(b)); T[rr][b] = s; }
    for (int m = 0; m < 6; ++m) { double s = 0.0; for (int a = 0; a < TCOV_W; ++a) s += Gk[rr][a] * B0[a][m]; T[rr][32 + m] = s; }
  }
  pt_cov_assemble(Gk, &T[0][0], PCOV_TW, C00, v, rotmat(q0), cov9);
  return 0;
}

// out[0] = sigma_max (pt_sigma_max), out[1] = dir^T cov dir (pt_var_dir)
extern "C" void pc_summaries(const double* cov9, const double* dir3, double* out2) {
  out2[0] = pt_sigma_max(cov9);
  out2[1] = pt_var_dir(cov9, mk(dir3[0], dir3[1], dir3[2]));
}

// sizeof and member offsets of lvx_point_cov_options (4 words) and lvx_point_cov (9 words), LVX_PT_COV_W
extern "C" void pc_layout(long long* out) {
  out[0] = sizeof(lvx_point_cov_options); out[1] = offsetof(lvx_point_cov_options, radius); out[2] = offsetof(lvx_point_cov_options, jacobi_scaling);
  out[3] = offsetof(lvx_point_cov_options, reserved);
  out[4] = sizeof(lvx_point_cov); out[5] = offsetof(lvx_point_cov, point); out[6] = offsetof(lvx_point_cov, cov); out[7] = offsetof(lvx_point_cov, sigma);
  out[8] = offsetof(lvx_point_cov, sigma_max); out[9] = offsetof(lvx_point_cov, var_dir); out[10] = offsetof(lvx_point_cov, window_cov);
  out[11] = offsetof(lvx_point_cov, window_idx); out[12] = offsetof(lvx_point_cov, valid); out[13] = LVX_PT_COV_W;
}
