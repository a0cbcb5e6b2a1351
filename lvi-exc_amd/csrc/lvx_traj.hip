// lvx_traj.hip — trajectory queries on the device: TrajectoryView::Evaluate(t, flags) in the spline's or a sensor's frame (k_traj_sample), the readings the IMU model
// predicts (k_predict_imu) and the absolute / relative pose errors against reference poses such as LOAM's (k_pose_errors; LIinitializer::PublishTrajectory,
// src/lvi_exc/test/lvi_initialize_surfel_orb.cpp:834-902).  Per-sample math: lvx_traj.h (shared with the host check); sensor poses: lvx_pose.h.  Built without FP
// contraction, so a sensor pose is the same bits as lvx_evaluate_lidar_pose / lvx_evaluate_camera_pose return.  A pass of its own: it reads a state and writes only its
// own buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lvx_ctx.h"
#include "lvx_pose.h"
#include "lvx_traj.h"

namespace lvx {

#define LVX_TRAJ_BLOCK 256
struct TrajOut { double *p, *v, *a, *q, *w; int32_t* valid; };

__device__ __forceinline__ void store3(double* base, long long i, v3 x) { double* o = base + 3 * (size_t)i; o[0] = x.x; o[1] = x.y; o[2] = x.z; }

// One lane per sample, grid-stride.  No LDS, no atomics: a lane that meets a non-unit control quaternion stores the constant RES_NONUNIT into *flag (every such store
// writes the same value).  The requested fields select one of four instantiations, so that a query holds only the registers of what it asks for (the pose-only sensor
// query is lidar_pose_dev and nothing else, as k_lidar_pose); within one, the output pointers are wave-uniform and the branches on them do not diverge.  The results do
// not depend on the instantiation: the file is built without FP contraction.
enum { TRAJ_K_SPLINE = 0, TRAJ_K_SPLINE_W = 1, TRAJ_K_SENSOR_POSE = 2, TRAJ_K_SENSOR_KIN = 3 };   // spline frame without / with angular velocity; sensor frame pose only / with velocities
template <int MODE>
__global__ __launch_bounds__(LVX_TRAJ_BLOCK) void k_traj_sample(const double* __restrict__ state, int N, double t0, double dt, int frame, long long n, const double* __restrict__ t,
                                                                TrajOut o, int* flag) {
  constexpr bool SENSOR = MODE == TRAJ_K_SENSOR_POSE || MODE == TRAJ_K_SENSOR_KIN, WITH_W = MODE == TRAJ_K_SPLINE_W || MODE == TRAJ_K_SENSOR_KIN;
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const bool want_pose = o.p || o.q;
  const double* ss = state + 7 * (size_t)N + (frame == LVX_FRAME_CAMERA ? 24 : 16);
  const long long stride = (long long)gridDim.x * LVX_TRAJ_BLOCK;
  for (long long i = (long long)blockIdx.x * LVX_TRAJ_BLOCK + threadIdx.x; i < n; i += stride) {
    const double ti = t[i];
    const double tt = SENSOR ? ti + ss[7] : ti;
    v3 p = mk(0, 0, 0), v = mk(0, 0, 0), a = mk(0, 0, 0), w = mk(0, 0, 0);
    quat q; q.x = 0; q.y = 0; q.z = 0; q.w = 0;
    int st = RES_RANGE;
    if (traj_time_valid(t0, dt, N, tt)) {
      st = RES_OK;
      if (MODE != TRAJ_K_SENSOR_POSE) {
        TrajKin k;
        st = traj_kinematics<WITH_W>(sp, tt, &k);
        if (st == RES_OK) {
          if (!SENSOR) { p = k.p; v = k.v; a = k.a; q = k.q; }
          if (WITH_W) w = k.w_world;
          if (MODE == TRAJ_K_SENSOR_KIN) v = traj_sensor_velocity(k, load_v3(ss + 4));
        }
      }
      if (SENSOR && st == RES_OK && (MODE == TRAJ_K_SENSOR_POSE || want_pose)) {   // the one definition of a sensor pose (lvx_pose.h); inside the range it fails only on a non-unit control quaternion
        const bool ok = frame == LVX_FRAME_LIDAR ? lidar_pose_dev(state, N, t0, dt, ti, &q, &p) : camera_pose_dev(state, N, t0, dt, ti, &q, &p);
        if (!ok) st = RES_NONUNIT;
      }
      if (st == RES_NONUNIT) *flag = RES_NONUNIT;
      if (st != RES_OK) { p = mk(0, 0, 0); v = p; a = p; w = p; q.x = 0; q.y = 0; q.z = 0; q.w = 0; }
    }
    if (o.p) store3(o.p, i, p);
    if (MODE != TRAJ_K_SENSOR_POSE && o.v) store3(o.v, i, v);
    if (!SENSOR && o.a) store3(o.a, i, a);
    if (o.q) { double* d = o.q + 4 * (size_t)i; d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; }
    if (WITH_W && o.w) store3(o.w, i, w);
    o.valid[i] = st == RES_OK ? 1 : 0;
  }
}

__global__ __launch_bounds__(LVX_TRAJ_BLOCK) void k_predict_imu(const double* __restrict__ state, int N, double t0, double dt, long long n, const double* __restrict__ t,
                                                                double* __restrict__ gyro3, double* __restrict__ acc3, int32_t* __restrict__ valid, int* flag) {
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const ImuCal imu = traj_load_imu(state, N);
  const long long stride = (long long)gridDim.x * LVX_TRAJ_BLOCK;
  for (long long i = (long long)blockIdx.x * LVX_TRAJ_BLOCK + threadIdx.x; i < n; i += stride) {
    v3 g = mk(0, 0, 0), a = mk(0, 0, 0);
    const int st = traj_predict_imu(sp, imu, t[i], &g, &a);
    if (st == RES_NONUNIT) *flag = RES_NONUNIT;
    if (st != RES_OK) { g = mk(0, 0, 0); a = g; }
    if (gyro3) store3(gyro3, i, g);
    if (acc3) store3(acc3, i, a);
    valid[i] = st == RES_OK ? 1 : 0;
  }
}

// Pose errors: ONE workgroup, three phases separated by barriers.  (1) lane k evaluates the trajectory pose of samples k, k + 256, ... in `frame` into the work arrays
// and the lowest valid index is found (integer minimum in LDS); (2) every lane forms the alignment from that sample, then the absolute errors of its samples and the
// relative error of the step to the next valid sample, adding each to its own summaries in index order; (3) the 256 summaries of each series are merged by a fixed tree.
// No floating-point atomic: two calls return the same bits.  out: [n_valid | 4 x (rmse, mean, max, argmax, n)].
struct PoseErrArgs {
  const double* state; int N; double t0, dt; int frame, n, align;
  const double* t; const double* qr; const double* pr;   // reference poses [n][4] (x, y, z, w), [n][3]
  double* Tq; double* Tp; int32_t* valid; double* abs_t; double* abs_r; double* out; int* flag;
};
__device__ __forceinline__ TrajPose load_pose(const double* q4, const double* p3, int i) { TrajPose T; T.q = load_q(q4 + 4 * (size_t)i); T.p = load_v3(p3 + 3 * (size_t)i); return T; }
__global__ __launch_bounds__(LVX_TRAJ_BLOCK) void k_pose_errors(PoseErrArgs g) {
  __shared__ int s_first;
  __shared__ TrajSum s_red[LVX_TRAJ_BLOCK];
  const int tid = threadIdx.x;
  if (tid == 0) s_first = g.n;
  __syncthreads();
  const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
  const double* ss = g.state + 7 * (size_t)g.N + (g.frame == LVX_FRAME_CAMERA ? 24 : 16);
  int first = g.n;
  for (int i = tid; i < g.n; i += LVX_TRAJ_BLOCK) {
    const double ti = g.t[i];
    const double tt = g.frame == LVX_FRAME_TRAJECTORY ? ti : ti + ss[7];
    quat q; q.x = 0; q.y = 0; q.z = 0; q.w = 0; v3 p = mk(0, 0, 0);
    bool ok = false;
    if (traj_time_valid(g.t0, g.dt, g.N, tt)) {
      if (g.frame == LVX_FRAME_TRAJECTORY) { TrajKin k; ok = traj_kinematics<false>(sp, tt, &k) == RES_OK; if (ok) { q = k.q; p = k.p; } }
      else ok = g.frame == LVX_FRAME_LIDAR ? lidar_pose_dev(g.state, g.N, g.t0, g.dt, ti, &q, &p) : camera_pose_dev(g.state, g.N, g.t0, g.dt, ti, &q, &p);
      if (!ok) { *g.flag = RES_NONUNIT; q.x = 0; q.y = 0; q.z = 0; q.w = 0; p = mk(0, 0, 0); }
    }
    double* dq = g.Tq + 4 * (size_t)i; dq[0] = q.x; dq[1] = q.y; dq[2] = q.z; dq[3] = q.w;
    store3(g.Tp, i, p);
    g.valid[i] = ok ? 1 : 0;
    if (ok && i < first) first = i;
  }
  if (first < g.n) atomicMin(&s_first, first);
  __syncthreads();
  const int a = s_first;
  TrajPose A; A.q = mkq(1, 0, 0, 0); A.p = mk(0, 0, 0);
  const bool align = g.align == LVX_ALIGN_FIRST && a < g.n;
  if (align) { TrajPose Ra = load_pose(g.qr, g.pr, a); Ra.q = qnormalized(Ra.q); A = traj_align_first(load_pose(g.Tq, g.Tp, a), Ra); }
  TrajSum acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = trajsum_zero();
  for (int i = tid; i < g.n; i += LVX_TRAJ_BLOCK) {
    if (!g.valid[i]) { g.abs_t[i] = 0.0; g.abs_r[i] = 0.0; continue; }
    const TrajPose Ti = load_pose(g.Tq, g.Tp, i);
    TrajPose Ri = load_pose(g.qr, g.pr, i); Ri.q = qnormalized(Ri.q);
    double et, er;
    traj_pose_error(Ti, align ? pose_mul(A, Ri) : Ri, &et, &er);
    g.abs_t[i] = et; g.abs_r[i] = er;
    trajsum_add(&acc[0], et, i); trajsum_add(&acc[1], er, i);
    int j = i + 1;
    while (j < g.n && !g.valid[j]) ++j;
    if (j < g.n) {
      TrajPose Rj = load_pose(g.qr, g.pr, j); Rj.q = qnormalized(Rj.q);
      traj_rel_error(Ti, load_pose(g.Tq, g.Tp, j), Ri, Rj, &et, &er);
      trajsum_add(&acc[2], et, i); trajsum_add(&acc[3], er, i);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    __syncthreads();
    s_red[tid] = acc[k];
    __syncthreads();
    for (int s = LVX_TRAJ_BLOCK / 2; s > 0; s >>= 1) {
      if (tid < s) s_red[tid] = trajsum_merge(s_red[tid], s_red[tid + s]);
      __syncthreads();
    }
    if (tid == 0) {
      const TrajSum r = s_red[0];
      double* o = g.out + 1 + 5 * k;
      if (k == 0) g.out[0] = (double)r.n;
      o[0] = r.n ? sqrt(r.sumsq / (double)r.n) : 0.0; o[1] = r.n ? r.sum / (double)r.n : 0.0; o[2] = r.max; o[3] = (double)r.argmax; o[4] = (double)r.n;
    }
  }
}

void traj_destroy(lvx_ctx* c) {
  for (auto& b : c->d_tj) if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
  if (c->h_tj) { (void)hipHostFree(c->h_tj); c->h_tj = nullptr; }
}

// lvx_synchronize: the flag word of the _d queries enqueued since the last look (the stream has been waited for)
int traj_check_d(lvx_ctx* c) {
  if ((!c->tj_d_unchecked && !c->tcov_d_unchecked) || !c->d_tj[3].p) return LVX_OK;
  c->tj_d_unchecked = false; c->tcov_d_unchecked = false;
  int w[2] = {0, 0};   // [1] a non-unit control quaternion in a _d query, [2] a lost pivot in lvx_trajectory_covariance_d / lvx_landmark_covariance_d / lvx_map_point_covariance_d (2: the latter's t_map window off the border)
  int* flag = (int*)c->d_tj[3].p + 1;
  LVX_HIP(c, hipMemcpy(w, flag, 8, hipMemcpyDeviceToHost));
  if (!w[0] && !w[1]) return LVX_OK;
  LVX_HIP(c, hipMemset(flag, 0, 8));
  if (w[1] == 2) return fail(c, LVX_E_STATE, "lvx_map_point_covariance_d / lvx_projection_covariance_d: a free scalar of the pose at t_map is a band position (nothing was written)");
  if (w[1]) return fail(c, LVX_E_NOTPD, "lvx_trajectory_covariance_d / lvx_landmark_covariance_d / lvx_projection_covariance_d: damped normal equations not positive definite (nothing was written)");
  return fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions");
}

// flag words (d_tj[3]), created on first use: [0] the host-array calls (cleared per call), [1 .. 2] the _d calls (kept until lvx_synchronize looks)
int traj_flag_words(lvx_ctx* c) {
  if (c->d_tj[3].p) return LVX_OK;
  int rc = dev_alloc(c, c->d_tj[3], 16);
  if (rc) return rc;
  LVX_HIP(c, hipMemsetAsync(c->d_tj[3].p, 0, 16, c->stream));
  return LVX_OK;
}

}  // namespace lvx

using namespace lvx;

namespace {

enum { TJ_STATE = 0, TJ_IN = 1, TJ_OUT = 2, TJ_FLAG = 3, TJ_WORK = 4 };

// the flag words and the pinned mirror of the small results
int traj_prepare(lvx_ctx* c) {
  LVX_HIP(c, hipSetDevice(c->device));
  int rc = traj_flag_words(c);
  if (rc) return rc;
  if (!c->h_tj) { LVX_HIP(c, hipHostMalloc((void**)&c->h_tj, 32 * 8, hipHostMallocDefault)); std::memset(c->h_tj, 0, 32 * 8); }
  return LVX_OK;
}
unsigned traj_blocks(const lvx_ctx* c, long long n) {   // 8 workgroups of 4 waves per CU, the loop takes the rest
  return (unsigned)std::min<long long>((n + LVX_TRAJ_BLOCK - 1) / LVX_TRAJ_BLOCK, (long long)c->n_cu * 8);
}
int sample_args(lvx_ctx* c, int frame, int n, const double* t, const lvx_traj_samples* out) {
  if (!c) return LVX_E_ARG;
  if (!out || !out->valid || !t || n <= 0) return fail(c, LVX_E_ARG, "lvx_sample_trajectory: n <= 0 or a required pointer is NULL");
  if (frame != LVX_FRAME_TRAJECTORY && frame != LVX_FRAME_LIDAR && frame != LVX_FRAME_CAMERA) return fail(c, LVX_E_ARG, "lvx_sample_trajectory: unknown frame");
  if (frame != LVX_FRAME_TRAJECTORY && out->acceleration3) return fail(c, LVX_E_ARG, "lvx_sample_trajectory: the acceleration of a sensor frame needs the angular acceleration, which is not offered");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  return LVX_OK;
}
int resident_state(lvx_ctx* c, const double** state_d) {
  if (*state_d) return LVX_OK;
  int rc = ensure_layout(c);
  if (rc) return rc;
  *state_d = (const double*)c->d_state.p;
  return LVX_OK;
}
int launch_sample(lvx_ctx* c, const double* state_d, int frame, int n, const double* t_d, const TrajOut& o, int* flag) {
  const bool sensor = frame != LVX_FRAME_TRAJECTORY, with_w = o.w != nullptr || (sensor && o.v != nullptr);   // (a sensor's velocity needs omega)
  const dim3 grid(traj_blocks(c, n)), block(LVX_TRAJ_BLOCK);
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    if (!sensor && !with_w) hipLaunchKernelGGL(k_traj_sample<TRAJ_K_SPLINE>, grid, block, 0, c->stream, state_d, c->N, c->t0, c->dt, frame, (long long)n, t_d, o, flag);
    else if (!sensor) hipLaunchKernelGGL(k_traj_sample<TRAJ_K_SPLINE_W>, grid, block, 0, c->stream, state_d, c->N, c->t0, c->dt, frame, (long long)n, t_d, o, flag);
    else if (with_w || !(o.p || o.q)) hipLaunchKernelGGL(k_traj_sample<TRAJ_K_SENSOR_KIN>, grid, block, 0, c->stream, state_d, c->N, c->t0, c->dt, frame, (long long)n, t_d, o, flag);
    else hipLaunchKernelGGL(k_traj_sample<TRAJ_K_SENSOR_POSE>, grid, block, 0, c->stream, state_d, c->N, c->t0, c->dt, frame, (long long)n, t_d, o, flag); }
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
int flag_code(lvx_ctx* c, int w) { return w ? fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions") : LVX_OK; }

}  // namespace

extern "C" {

int lvx_sample_trajectory_d(lvx_ctx* c, const double* state_d, int frame, int n, const double* t_d, const lvx_traj_samples* out_d) {
  int rc = sample_args(c, frame, n, t_d, out_d);
  if (rc) return rc;
  if ((rc = traj_prepare(c))) return rc;
  if ((rc = resident_state(c, &state_d))) return rc;
  const TrajOut o{out_d->position3, out_d->velocity3, out_d->acceleration3, out_d->orientation_xyzw4, out_d->angular_velocity3, out_d->valid};
  c->tj_d_unchecked = true;
  return launch_sample(c, state_d, frame, n, t_d, o, (int*)c->d_tj[TJ_FLAG].p + 1);
}

int lvx_sample_trajectory(lvx_ctx* c, const double* state, int frame, int n, const double* t, const lvx_traj_samples* out) {
  int rc = sample_args(c, frame, n, t, out);
  if (rc) return rc;
  if (!state) return fail(c, LVX_E_ARG, "lvx_sample_trajectory: n <= 0 or a required pointer is NULL");
  if ((rc = traj_prepare(c))) return rc;
  hipStream_t st = c->stream;
  const size_t nn = (size_t)n;
  if ((rc = upload(c, c->d_tj[TJ_STATE], state, (size_t)lvx_state_size(c) * 8))) return rc;
  if ((rc = upload(c, c->d_tj[TJ_IN], t, nn * 8))) return rc;
  double* host[5] = {out->position3, out->velocity3, out->acceleration3, out->orientation_xyzw4, out->angular_velocity3};
  const size_t width[5] = {3, 3, 3, 4, 3};
  if ((rc = dev_alloc(c, c->d_tj[TJ_OUT], nn * (16 * 8 + 4)))) return rc;
  double* dev[5]; double* cur = (double*)c->d_tj[TJ_OUT].p;
  for (int k = 0; k < 5; ++k) { dev[k] = host[k] ? cur : nullptr; cur += width[k] * nn; }
  int32_t* dvalid = (int32_t*)cur;
  int* flag = (int*)c->d_tj[TJ_FLAG].p;
  LVX_HIP(c, hipMemsetAsync(flag, 0, 4, st));
  if ((rc = launch_sample(c, (const double*)c->d_tj[TJ_STATE].p, frame, n, (const double*)c->d_tj[TJ_IN].p, TrajOut{dev[0], dev[1], dev[2], dev[3], dev[4], dvalid}, flag))) return rc;
  for (int k = 0; k < 5; ++k) if (host[k]) LVX_HIP(c, hipMemcpyAsync(host[k], dev[k], nn * width[k] * 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(out->valid, dvalid, nn * 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(c->h_tj, flag, 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  int w; std::memcpy(&w, c->h_tj, 4);
  return flag_code(c, w);
}

int lvx_predict_imu_d(lvx_ctx* c, const double* state_d, int n, const double* t_d, double* gyro3_d, double* acc3_d, int32_t* valid_d) {
  if (!c) return LVX_E_ARG;
  if (!valid_d || !t_d || n <= 0) return fail(c, LVX_E_ARG, "lvx_predict_imu: n <= 0 or a required pointer is NULL");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  int rc = traj_prepare(c);
  if (rc) return rc;
  if ((rc = resident_state(c, &state_d))) return rc;
  c->tj_d_unchecked = true;
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_predict_imu, dim3(traj_blocks(c, n)), dim3(LVX_TRAJ_BLOCK), 0, c->stream, state_d, c->N, c->t0, c->dt, (long long)n, t_d, gyro3_d, acc3_d, valid_d,
                       (int*)c->d_tj[TJ_FLAG].p + 1); }
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}

int lvx_predict_imu(lvx_ctx* c, const double* state, int n, const double* t, double* gyro3, double* acc3, int32_t* valid) {
  if (!c) return LVX_E_ARG;
  if (!state || !valid || !t || n <= 0) return fail(c, LVX_E_ARG, "lvx_predict_imu: n <= 0 or a required pointer is NULL");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  int rc = traj_prepare(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const size_t nn = (size_t)n;
  if ((rc = upload(c, c->d_tj[TJ_STATE], state, (size_t)lvx_state_size(c) * 8))) return rc;
  if ((rc = upload(c, c->d_tj[TJ_IN], t, nn * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_tj[TJ_OUT], nn * (6 * 8 + 4)))) return rc;
  double* dg = (double*)c->d_tj[TJ_OUT].p; double* da = dg + 3 * nn; int32_t* dv = (int32_t*)(da + 3 * nn);
  int* flag = (int*)c->d_tj[TJ_FLAG].p;
  LVX_HIP(c, hipMemsetAsync(flag, 0, 4, st));
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_predict_imu, dim3(traj_blocks(c, n)), dim3(LVX_TRAJ_BLOCK), 0, st, (const double*)c->d_tj[TJ_STATE].p, c->N, c->t0, c->dt, (long long)n,
                       (const double*)c->d_tj[TJ_IN].p, gyro3 ? dg : nullptr, acc3 ? da : nullptr, dv, flag); }
  LVX_HIP(c, hipGetLastError());
  if (gyro3) LVX_HIP(c, hipMemcpyAsync(gyro3, dg, nn * 24, hipMemcpyDeviceToHost, st));
  if (acc3) LVX_HIP(c, hipMemcpyAsync(acc3, da, nn * 24, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(valid, dv, nn * 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(c->h_tj, flag, 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  int w; std::memcpy(&w, c->h_tj, 4);
  return flag_code(c, w);
}

int lvx_compare_poses(lvx_ctx* c, const double* state, int frame, int n, const double* t, const double* q_xyzw4, const double* p3, int align, lvx_pose_errors* out,
                      double* abs_trans_n, double* abs_rot_n) {
  if (!c) return LVX_E_ARG;
  if (!state || !out || !t || !q_xyzw4 || !p3 || n <= 0) return fail(c, LVX_E_ARG, "lvx_compare_poses: n <= 0 or a required pointer is NULL");
  if (frame != LVX_FRAME_TRAJECTORY && frame != LVX_FRAME_LIDAR && frame != LVX_FRAME_CAMERA) return fail(c, LVX_E_ARG, "lvx_compare_poses: unknown frame");
  if (align != LVX_ALIGN_NONE && align != LVX_ALIGN_FIRST) return fail(c, LVX_E_ARG, "lvx_compare_poses: unknown alignment");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  int rc = traj_prepare(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const size_t nn = (size_t)n;
  if ((rc = upload(c, c->d_tj[TJ_STATE], state, (size_t)lvx_state_size(c) * 8))) return rc;
  // inputs [t | q | p]; work [Tq | Tp | abs_t | abs_r | out (32) | valid]
  if ((rc = dev_alloc(c, c->d_tj[TJ_IN], nn * 8 * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_tj[TJ_WORK], nn * (9 * 8 + 4) + 32 * 8))) return rc;
  double* in = (double*)c->d_tj[TJ_IN].p; double* wk = (double*)c->d_tj[TJ_WORK].p;
  LVX_HIP(c, hipMemcpyAsync(in, t, nn * 8, hipMemcpyHostToDevice, st));
  LVX_HIP(c, hipMemcpyAsync(in + nn, q_xyzw4, nn * 32, hipMemcpyHostToDevice, st));
  LVX_HIP(c, hipMemcpyAsync(in + 5 * nn, p3, nn * 24, hipMemcpyHostToDevice, st));
  int* flag = (int*)c->d_tj[TJ_FLAG].p;
  LVX_HIP(c, hipMemsetAsync(flag, 0, 4, st));
  PoseErrArgs g{};
  g.state = (const double*)c->d_tj[TJ_STATE].p; g.N = c->N; g.t0 = c->t0; g.dt = c->dt; g.frame = frame; g.n = n; g.align = align;
  g.t = in; g.qr = in + nn; g.pr = in + 5 * nn;
  g.Tq = wk; g.Tp = wk + 4 * nn; g.abs_t = wk + 7 * nn; g.abs_r = wk + 8 * nn; g.out = wk + 9 * nn; g.valid = (int32_t*)(g.out + 32); g.flag = flag;
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_pose_errors, dim3(1), dim3(LVX_TRAJ_BLOCK), 0, st, g); }
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(c->h_tj + 1, g.out, 21 * 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(c->h_tj, flag, 4, hipMemcpyDeviceToHost, st));
  if (abs_trans_n) LVX_HIP(c, hipMemcpyAsync(abs_trans_n, g.abs_t, nn * 8, hipMemcpyDeviceToHost, st));
  if (abs_rot_n) LVX_HIP(c, hipMemcpyAsync(abs_rot_n, g.abs_r, nn * 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));   // the one host stop
  const double* r = c->h_tj + 1;
  std::memset(out, 0, sizeof(*out));
  out->n = n; out->n_valid = (int32_t)r[0];
  lvx_err_summary* s[4] = {&out->abs_trans, &out->abs_rot, &out->rel_trans, &out->rel_rot};
  for (int k = 0; k < 4; ++k) { const double* o = r + 1 + 5 * k; s[k]->rmse = o[0]; s[k]->mean = o[1]; s[k]->max = o[2]; s[k]->argmax = (int32_t)o[3]; s[k]->n = (int32_t)o[4]; }
  int w; std::memcpy(&w, c->h_tj, 4);
  return flag_code(c, w);
}

}  // extern "C"
