// tests/native/traj_host_check.cpp — TEST-ONLY host build of the per-sample math behind the trajectory queries (lvi-exc_amd/csrc/lvx_traj.h), so that the CPU suite
// (-m "not gpu") can hold it against the oracle without a GPU.  Not a CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2 -ffp-contract=off, as the
// device translation unit is.
#include "../../lvi-exc_amd/csrc/lvx_traj.h"

using namespace lvx;

namespace {
void put3(double* o, int i, v3 x) { if (!o) return; o[3 * i] = x.x; o[3 * i + 1] = x.y; o[3 * i + 2] = x.z; }
SensorCal sensor(const double* state, int N, int frame) {
  const double* ss = state + 7 * (size_t)N + (frame == 2 ? 24 : 16);
  SensorCal s; s.q = load_q(ss); s.p = load_v3(ss + 4); s.tau = ss[7];
  return s;
}
}  // namespace

// frame 0: the spline itself; frame 1 / 2: the sensor pose composed here as lvx_pose.h composes it (q = q(tt) q_S, p = q(tt) p_S + p(tt)), the sensor-origin velocity and
// omega.  Invalid samples: zeros and valid = 0.  Returns the OR of the samples' status bits (1 range, 2 non-unit quaternion).
extern "C" int th_sample(const double* state, int N, double t0, double dt, int frame, int n, const double* t, double* p3, double* v3_, double* a3, double* q4, double* w3, int* valid) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  int all = 0;
  for (int i = 0; i < n; ++i) {
    TrajKin k;
    const SensorCal s = sensor(state, N, frame);
    const int st = traj_kinematics<true>(sp, frame == 0 ? t[i] : t[i] + s.tau, &k);
    all |= st;
    valid[i] = st == RES_OK;
    v3 p = mk(0, 0, 0), v = p, a = p, w = p; quat q; q.x = q.y = q.z = q.w = 0.0;
    if (st == RES_OK) {
      if (frame == 0) { p = k.p; v = k.v; a = k.a; q = k.q; w = k.w_world; }
      else { q = qmul(k.q, s.q); p = qrot(k.q, s.p) + k.p; v = traj_sensor_velocity(k, s.p); w = k.w_world; }
    }
    put3(p3, i, p); put3(v3_, i, v); put3(a3, i, a); put3(w3, i, w);
    if (q4) { q4[4 * i] = q.x; q4[4 * i + 1] = q.y; q4[4 * i + 2] = q.z; q4[4 * i + 3] = q.w; }
  }
  return all;
}

extern "C" int th_predict_imu(const double* state, int N, double t0, double dt, int n, const double* t, double* gyro3, double* acc3, int* valid) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const ImuCal imu = traj_load_imu(state, N);
  int all = 0;
  for (int i = 0; i < n; ++i) {
    v3 g = mk(0, 0, 0), a = g;
    const int st = traj_predict_imu(sp, imu, t[i], &g, &a);
    all |= st;
    valid[i] = st == RES_OK;
    if (st != RES_OK) { g = mk(0, 0, 0); a = g; }
    put3(gyro3, i, g); put3(acc3, i, a);
  }
  return all;
}

// the pose-error pass over given trajectory poses (Tq x, y, z, w; Tp; valid) and reference poses, summed in index order: out = [n_valid | 4 x (rmse, mean, max, argmax, n)]
extern "C" void th_pose_errors(int n, const double* Tq, const double* Tp, const int* valid, const double* qr, const double* pr, int align, double* abs_t, double* abs_r, double* out) {
  auto pose = [](const double* q4, const double* p3, int i) { TrajPose T; T.q = load_q(q4 + 4 * i); T.p = load_v3(p3 + 3 * i); return T; };
  auto ref = [&](int i) { TrajPose R = pose(qr, pr, i); R.q = qnormalized(R.q); return R; };
  int a = 0;
  while (a < n && !valid[a]) ++a;
  TrajPose A; A.q = mkq(1, 0, 0, 0); A.p = mk(0, 0, 0);
  const bool al = align == 1 && a < n;
  if (al) A = traj_align_first(pose(Tq, Tp, a), ref(a));
  TrajSum acc[4] = {trajsum_zero(), trajsum_zero(), trajsum_zero(), trajsum_zero()};
  for (int i = 0; i < n; ++i) {
    abs_t[i] = 0.0; abs_r[i] = 0.0;
    if (!valid[i]) continue;
    const TrajPose Ti = pose(Tq, Tp, i), Ri = ref(i);
    double et, er;
    traj_pose_error(Ti, al ? pose_mul(A, Ri) : Ri, &et, &er);
    abs_t[i] = et; abs_r[i] = er;
    trajsum_add(&acc[0], et, i); trajsum_add(&acc[1], er, i);
    int j = i + 1;
    while (j < n && !valid[j]) ++j;
    if (j < n) { traj_rel_error(Ti, pose(Tq, Tp, j), Ri, ref(j), &et, &er); trajsum_add(&acc[2], et, i); trajsum_add(&acc[3], er, i); }
  }
  out[0] = (double)acc[0].n;
  for (int k = 0; k < 4; ++k) {
    double* o = out + 1 + 5 * k; const TrajSum& r = acc[k];
    o[0] = r.n ? sqrt(r.sumsq / r.n) : 0.0; o[1] = r.n ? r.sum / r.n : 0.0; o[2] = r.max; o[3] = r.argmax; o[4] = r.n;
  }
}
