// tests/native/trajcov_host_check.cpp — TEST-ONLY host build of the pose Jacobian of lvx_trajectory_covariance (lvi-exc_amd/csrc/lvx_trajcov.h over lvx_traj.h), so that
// the CPU suite (-m "not gpu") can hold it against finite differences of the pose without a GPU, and the layout of the call's two structs against the ctypes mirrors.
// Not a CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2.
#include <cstddef>

#include "../../include/lvx.h"
#include "../../lvi-exc_amd/csrc/lvx_trajcov.h"

using namespace lvx;

namespace {
SensorCal sensor(const double* state, int N, int frame) {
  SensorCal s; s.q = mkq(1, 0, 0, 0); s.p = mk(0, 0, 0); s.tau = 0.0;
  if (frame == 0) return s;
  const double* ss = state + 7 * (size_t)N + (frame == 2 ? 24 : 16);
  s.q = load_q(ss); s.p = load_v3(ss + 4); s.tau = ss[7];
  return s;
}
}  // namespace

// J [6][31] row-major, idx [31]; returns traj_pose_jacobian's status (0 ok, 1 range, 2 non-unit quaternion)
extern "C" int tc_jacobian(const double* state, int N, double t0, double dt, int frame, double t, double* J186, int* idx31) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const SensorCal s = sensor(state, N, frame);
  double J[6][TCOV_W]; int idx[TCOV_W];
  const int st = traj_pose_jacobian(sp, frame, s, t + s.tau, J, idx);
  if (st == RES_RANGE) return st;
  for (int r = 0; r < 6; ++r) for (int c = 0; c < TCOV_W; ++c) J186[r * TCOV_W + c] = J[r][c];
  for (int c = 0; c < TCOV_W; ++c) idx31[c] = idx[c];
  return st;
}

// the pose itself in `frame` (q x, y, z, w; p), composed as lvx_pose.h composes a sensor pose; also the knot interval
extern "C" int tc_pose(const double* state, int N, double t0, double dt, int frame, double t, double* q4, double* p3, int* i0, double* u) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const SensorCal s = sensor(state, N, frame);
  TrajKin k;
  const int st = traj_kinematics<false>(sp, t + s.tau, &k);
  if (st != RES_OK) return st;
  KnotRef kr; traj_knot(t0, dt, N, t + s.tau, &kr);
  *i0 = kr.i0; *u = kr.u;
  const quat q = frame == 0 ? k.q : qmul(k.q, s.q);
  const v3 p = frame == 0 ? k.p : qrot(k.q, s.p) + k.p;
  q4[0] = q.x; q4[1] = q.y; q4[2] = q.z; q4[3] = q.w; p3[0] = p.x; p3[1] = p.y; p3[2] = p.z;
  return st;
}

// sizeof and member offsets of lvx_traj_cov_options (4 words) and lvx_traj_cov (6 words)
extern "C" void tc_layout(long long* out) {
  out[0] = sizeof(lvx_traj_cov_options); out[1] = offsetof(lvx_traj_cov_options, radius); out[2] = offsetof(lvx_traj_cov_options, jacobi_scaling); out[3] = offsetof(lvx_traj_cov_options, reserved);
  out[4] = sizeof(lvx_traj_cov); out[5] = offsetof(lvx_traj_cov, cov); out[6] = offsetof(lvx_traj_cov, sigma); out[7] = offsetof(lvx_traj_cov, window_cov);
  out[8] = offsetof(lvx_traj_cov, window_idx); out[9] = offsetof(lvx_traj_cov, valid);
}
