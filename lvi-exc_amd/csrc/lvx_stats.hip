// lvx_stats.hip — error statistics on the device (include/lvx.h: lvx_error_statistics*, lvx_get_plane_stats, lvx_get_landmark_stats).
//
// What the reference prints around every optimisation stage (printErrorStatistics, trajectory_manager_lvi.cpp:621-697) plus what a user needs to prune a map: per
// family counts, cost share, Huber outliers and the sums of the raw (unweighted, unrobustified) error; per surfel plane and per landmark the error of its blocks.
// One launch per family and one reduction on the context's stream, nothing of the evaluation pass is read or written:
//   k_stats_eval    one thread per residual block, one instantiation per family (each holds its own registers only).  Value-only residuals (lvx_stats.h): no Jacobian, no
//                   LDS tile, no accumulators.  A workgroup reduces its 256 blocks to one 16-double record — wavefront butterfly, then the four wavefronts in order —
//                   and stores it; the per-row raw errors the segment statistics need go to a row array.
//   k_stats_reduce  a wavefront per plane / landmark walks the segment's row list in list order; one workgroup per family adds the family's records in a fixed order.
// Every sum has one fixed order of additions (no floating-point atomic anywhere): two calls on the same state return the same bits.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lvx_ctx.h"
#include "lvx_stats.h"

namespace lvx {

struct StatsArgs {
  SplineRef sp; CamIntr cam; uint32_t locks; double mto, t_map;
  int n_imu; const double* imu_t; const double* gyro; const double* acc; double w_gyro, w_acc;
  double prior_t; quat prior_q; double prior_w;
  int n_surf; const double* surf_t; const double* surf_pt; const double* surf_pl; const int* surf_perm; double surf_w, surf_huber;
  int n_rep; const int* rep_lm; const double* rep_uv; const double* rep_t0; double rep_w, rep_huber;
  int n_cs; const int* cs_lm; const int* cs_plane; double cs_w, cs_huber;
  const double* planes; const double* lm_uv; const double* lm_t0; int L;
  int blk0[LVX_NUM_FAM + 1];   // first workgroup of every family
  double* part;                // [workgroups][ST_W]
  double* surf_val;            // [n_surf] |raw error| of the surfel row at its INPUT position, -1: not evaluated
  double* rep_val;             // [n_rep] squared raw error of the reprojection block at its DEVICE position, -1: not evaluated
  int* err;                    // RES_RANGE | RES_NONUNIT of the blocks that were not evaluated
};

__device__ __forceinline__ double wave_add(double v) {   // butterfly: every lane ends with the same sum, formed in the same order every time
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// a workgroup's 256 records -> one, in thread 0 .. ST_W - 1 of the workgroup (slot = thread)
__device__ __forceinline__ void block_reduce(double acc[ST_W], double (*sh)[ST_W], double* dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < ST_W - 1; ++s) acc[s] = s >= ST_MAX ? wave_max(acc[s]) : wave_add(acc[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < ST_W; ++s) sh[wave][s] = acc[s];
  }
  __syncthreads();
  if (threadIdx.x < ST_W) {
    const int s = threadIdx.x;
    double v = sh[0][s];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v = s >= ST_MAX ? fmax(v, sh[w][s]) : v + sh[w][s];
    dst[s] = v;
  }
}

template <int FAM>
__global__ __launch_bounds__(256) void k_stats_eval(StatsArgs q) {
  __shared__ StatHub hub;
  __shared__ double sh[4][ST_W];
  constexpr int fam = FAM;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const SplineRef sp = q.sp;
  const double* s = sp.r3 + 7 * (size_t)sp.n;   // calibration block of the state (sp.r3 = the state's first double)
  double acc[ST_W];
#pragma unroll
  for (int k = 0; k < ST_W; ++k) acc[k] = 0.0;
  int status = RES_OK;
  if constexpr (fam == LVX_FAM_GYRO || fam == LVX_FAM_ACCEL) {
    if (i < q.n_imu) {
      ImuCal imu; imu.tau = s[7]; imu.roll = s[8]; imu.pitch = s[9]; imu.ba = load_v3(s + 10); imu.bg = load_v3(s + 13);
      double r[3];
      if (fam == LVX_FAM_GYRO) { status = stat_gyro(sp, imu, q.imu_t[i], load_v3(q.gyro + 3 * (size_t)i), q.w_gyro, r); if (status == RES_OK) stat_block<3>(r, q.w_gyro, 0.0, acc); }
      else { status = stat_accel(sp, imu, q.imu_t[i], load_v3(q.acc + 3 * (size_t)i), q.w_acc, r); if (status == RES_OK) stat_block<3>(r, q.w_acc, 0.0, acc); }
    }
  } else if constexpr (fam == LVX_FAM_PRIOR) {
    if (i == 0) {
      double r[1];
      status = stat_prior(sp, q.prior_t, q.prior_q, q.prior_w, r);
      if (status == RES_OK) stat_block<1>(r, q.prior_w, 0.0, acc);
    }
  } else if constexpr (fam == LVX_FAM_SURFEL || fam == LVX_FAM_CAMSURF) {
    SensorCal lidar, cam;
    lidar.q = load_q(s + 16); lidar.p = load_v3(s + 20); lidar.tau = s[23];
    cam.q = load_q(s + 24); cam.p = load_v3(s + 28); cam.tau = s[31];
    const bool surf = fam == LVX_FAM_SURFEL;
    const bool tl = (q.locks & (surf ? LVX_LOCK_LIDAR_TAU : LVX_LOCK_CAM_TAU)) != 0;
    if (threadIdx.x == 0) stat_hub(sp, q.t_map, tl, q.mto, surf ? lidar.tau : cam.tau, &hub);   // the map-time pose, once per workgroup
    __syncthreads();
    double r[1];
    if (surf) {
      if (i < q.n_surf) {
        status = stat_surfel(sp, hub, lidar, tl, q.mto, q.t_map, q.surf_t[i], load_v3(q.surf_pt + 3 * (size_t)i), load_v3(q.surf_pl + 3 * (size_t)i), q.surf_w, r);
        if (status == RES_OK) stat_block<1>(r, q.surf_w, q.surf_huber, acc);
        q.surf_val[q.surf_perm[i]] = status == RES_OK ? fabs(r[0] / q.surf_w) : -1.0;
      }
    } else if (i < q.n_cs) {
      const int l = q.cs_lm[i];
      status = stat_camsurf(sp, hub, q.cam, cam, lidar, tl, q.mto, q.t_map, q.lm_uv[2 * (size_t)l], q.lm_uv[2 * (size_t)l + 1], q.lm_t0[l], s[32 + l],
                            load_v3(q.planes + 3 * (size_t)q.cs_plane[i]), q.cs_w, r);
      if (status == RES_OK) stat_block<1>(r, q.cs_w, q.cs_huber, acc);
    }
  } else if (i < q.n_rep) {
    SensorCal cam; cam.q = load_q(s + 24); cam.p = load_v3(s + 28); cam.tau = s[31];
    const int l = q.rep_lm[i];
    double r[2] = {0.0, 0.0};
    if (l < 0 || l >= q.L) status = RES_RANGE;   // (lvx_set_reproj does not see the landmark table)
    else status = stat_reproj(sp, q.cam, cam, (q.locks & LVX_LOCK_CAM_TAU) != 0, q.mto, q.lm_uv[2 * (size_t)l], q.lm_uv[2 * (size_t)l + 1], q.lm_t0[l],
                              q.rep_uv[2 * (size_t)i], q.rep_uv[2 * (size_t)i + 1], q.rep_t0[i], s[32 + l], q.rep_w, r);
    if (status == RES_OK) stat_block<2>(r, q.rep_w, q.rep_huber, acc);
    const double e0 = r[0] / q.rep_w, e1 = r[1] / q.rep_w;
    q.rep_val[i] = status == RES_OK ? e0 * e0 + e1 * e1 : -1.0;
  }
  if (status != RES_OK) atomicOr(q.err, status);   // (an integer flag word)
  block_reduce(acc, sh, q.part + ((size_t)q.blk0[fam] + blockIdx.x) * ST_W);
}

// plane -> surfel rows and landmark -> reprojection blocks: rows[ptr[g] .. ptr[g + 1]) index the row arrays of k_stats_eval
struct StatsSeg { int n_seg; const int* ptr; const int* rows; const double* val; long long* n; double* sum; double* mx; int root; };   // root: mx = sqrt(max) (values are squared norms)
struct StatsReduce {
  StatsSeg seg[2]; int seg_blk[3];   // workgroups [seg_blk[k], seg_blk[k + 1]) walk the segments of set k, four per workgroup
  const double* part; int blk0[LVX_NUM_FAM + 1]; double* fam_out; const int* err;   // fam_out: [LVX_NUM_FAM][ST_W] then the error word
};
__global__ __launch_bounds__(256) void k_stats_reduce(StatsReduce q) {
  __shared__ double sh[4][ST_W];
  const int b = (int)blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (b < q.seg_blk[2]) {
    const int k = b < q.seg_blk[1] ? 0 : 1;
    const StatsSeg& sg = q.seg[k];
    const int g = (b - q.seg_blk[k]) * 4 + wave;
    if (g >= sg.n_seg) return;
    const int e0 = sg.ptr[g], e1 = sg.ptr[g + 1];
    double cnt = 0.0, sum = 0.0, mx = 0.0;
    for (int e = e0 + lane; e < e1; e += 64) {   // a lane takes every 64th entry of the list, in list order
      const double v = sg.val[sg.rows[e]];
      if (v >= 0.0) { cnt += 1.0; sum += v; mx = fmax(mx, v); }
    }
    cnt = wave_add(cnt); sum = wave_add(sum); mx = wave_max(mx);
    if (lane == 0) { sg.n[g] = (long long)cnt; sg.sum[g] = sum; sg.mx[g] = sg.root ? sqrt(mx) : mx; }
    return;
  }
  const int fam = b - q.seg_blk[2];
  double acc[ST_W];
#pragma unroll
  for (int s = 0; s < ST_W; ++s) acc[s] = 0.0;
  for (int p = q.blk0[fam] + (int)threadIdx.x; p < q.blk0[fam + 1]; p += 256) {   // a thread takes every 256th record of the family, in order
    const double* rec = q.part + (size_t)p * ST_W;
#pragma unroll
    for (int s = 0; s < ST_W - 1; ++s) acc[s] = s >= ST_MAX ? fmax(acc[s], rec[s]) : acc[s] + rec[s];
  }
  block_reduce(acc, sh, q.fam_out + (size_t)fam * ST_W);
  if (fam == 0 && threadIdx.x == 0) q.fam_out[LVX_NUM_FAM * ST_W] = (double)*q.err;
}

// LiDAR odometry position blocks (lvx_set_lidar_poses): one thread per block, a workgroup's 256 blocks to one record, then one workgroup adds the records in order
struct LpStatsArgs { SplineRef sp; uint32_t locks; double mto, t_start; int n; const double* t; const double* pm; double w, huber; double* part; int nblk; double* out; int* err; };
__global__ __launch_bounds__(256) void k_stats_lidarpos(LpStatsArgs q) {
  __shared__ StatHub hub;
  __shared__ double sh[4][ST_W];
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const SplineRef sp = q.sp;
  const double* s = sp.r3 + 7 * (size_t)sp.n;
  SensorCal lidar; lidar.q = load_q(s + 16); lidar.p = load_v3(s + 20); lidar.tau = s[23];
  const bool tl = (q.locks & LVX_LOCK_LIDAR_TAU) != 0;
  if (threadIdx.x == 0) stat_hub(sp, q.t_start, tl, q.mto, lidar.tau, &hub);
  __syncthreads();
  double acc[ST_W];
#pragma unroll
  for (int k = 0; k < ST_W; ++k) acc[k] = 0.0;
  if (i < q.n) {
    double r[3];
    const int status = stat_lidarpos(sp, hub, lidar, tl, q.mto, q.t_start, q.t[i], load_v3(q.pm + 3 * (size_t)i), q.w, r);
    if (status == RES_OK) stat_block<3>(r, q.w, q.huber, acc); else atomicOr(q.err, status);   // (an integer flag word)
  }
  block_reduce(acc, sh, q.part + (size_t)blockIdx.x * ST_W);
}
__global__ __launch_bounds__(256) void k_stats_lidarpos_reduce(LpStatsArgs q) {
  __shared__ double sh[4][ST_W];
  double acc[ST_W];
#pragma unroll
  for (int s = 0; s < ST_W; ++s) acc[s] = 0.0;
  for (int p = (int)threadIdx.x; p < q.nblk; p += 256) {   // a thread takes every 256th record, in order
    const double* rec = q.part + (size_t)p * ST_W;
#pragma unroll
    for (int s = 0; s < ST_W - 1; ++s) acc[s] = s >= ST_MAX ? fmax(acc[s], rec[s]) : acc[s] + rec[s];
  }
  block_reduce(acc, sh, q.out);
  if (threadIdx.x == 0) q.out[ST_W] = (double)*q.err;
}
static int run_lidarpos_stats(lvx_ctx* c, const double* state_d, lvx_family_stats* out) {
  int rc = ensure_layout(c);
  if (rc) return rc;
  std::memset(out, 0, sizeof(*out));
  const Family& f = c->lp;
  out->n_blocks = f.n;
  if (f.n <= 0) return LVX_OK;
  hipStream_t st = c->stream;
  LpStatsArgs a{};
  a.sp = SplineRef{c->t0, c->dt, c->N, state_d, state_d + 3 * (size_t)c->N};
  a.locks = c->locks; a.mto = c->sensor_mto; a.t_start = c->lp_t_start; a.n = f.n; a.t = (const double*)f.d_t.p; a.pm = (const double*)f.d_a3.p; a.w = f.weight; a.huber = f.huber;
  a.nblk = (f.n + 255) / 256;
  if ((rc = dev_alloc(c, c->d_lp_part, (size_t)a.nblk * ST_W * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_lp_out, (ST_W + 2) * 8))) return rc;
  if (!c->h_lp) LVX_HIP(c, hipHostMalloc((void**)&c->h_lp, (ST_W + 2) * 8, hipHostMallocDefault));
  a.part = (double*)c->d_lp_part.p; a.out = (double*)c->d_lp_out.p; a.err = (int*)(a.out + ST_W + 1);
  LVX_HIP(c, hipMemsetAsync(a.err, 0, 8, st));
  hipLaunchKernelGGL(k_stats_lidarpos, dim3((unsigned)a.nblk), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_stats_lidarpos_reduce, dim3(1), dim3(256), 0, st, a);
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(c->h_lp, a.out, (ST_W + 1) * 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));   // the one host stop
  const double* rec = c->h_lp;
  out->n_evaluated = (int64_t)rec[ST_EVAL]; out->n_outliers = (int64_t)rec[ST_OUT]; out->cost = rec[ST_COST];
  for (int k = 0; k < 3; ++k) { out->sum[k] = rec[ST_SUM + k]; out->sum_abs[k] = rec[ST_ABS + k]; out->sum_sq[k] = rec[ST_SQ + k]; out->max_abs[k] = rec[ST_MAX + k]; }
  const int err = (int)rec[ST_W];
  if (err & RES_RANGE) return fail(c, LVX_E_RANGE, "time span out of range for trajectory");
  if (err & RES_NONUNIT) return fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions");
  return LVX_OK;
}

void stats_destroy(lvx_ctx* c) {
  for (DevBuf* b : {&c->d_st_state, &c->d_st_part, &c->d_st_val, &c->d_st_out, &c->d_st_plist}) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->bytes = 0; }
  if (c->h_st) { (void)hipHostFree(c->h_st); c->h_st = nullptr; c->h_st_cap = 0; }
}

// layout of d_st_out / h_st in 8-byte words: [family records LVX_NUM_FAM * ST_W | error word (+ 1 pad) | plane n, sum, max (3 P) | landmark n, sum, max (3 L)]
static size_t st_off_planes() { return (size_t)LVX_NUM_FAM * ST_W + 2; }

static int run_stats(lvx_ctx* c, const double* state_d, lvx_error_stats* out) {
  int rc = ensure_layout(c);
  if (rc) return rc;
  c->st_valid = false;
  hipStream_t st = c->stream;
  const int P = (int)(c->planes.size() / 3), L = c->L;
  const bool has_acc = !(c->locks & LVX_LOCK_R3);
  const int cnt[LVX_NUM_FAM] = {c->imu.n, has_acc ? c->imu.n : 0, c->has_prior ? 1 : 0, c->surf.n, c->rep.n, c->cs.n};
  // plane -> surfel rows (input positions, input order): built on the first statistics call after the problem changed, never by lvx_set_surfel
  if (!c->st_plist_valid || c->st_plist_cfg != c->cfg_version) {
    if ((rc = handoff_fetch_ids(c))) return rc;   // (a device-origin surfel family keeps its plane ids on the device until somebody asks)
    std::vector<int> tab((size_t)P + 1 + (size_t)std::max(c->surf.n, 1), 0);
    for (int i = 0; i < c->surf.n; ++i) tab[(size_t)c->surf.id0[i] + 1]++;
    for (int p = 0; p < P; ++p) tab[(size_t)p + 1] += tab[p];
    std::vector<int> fill(tab.begin(), tab.begin() + P);
    for (int i = 0; i < c->surf.n; ++i) tab[(size_t)P + 1 + fill[c->surf.id0[i]]++] = i;
    if ((rc = upload_tmp(c, c->d_st_plist, tab.data(), tab.size() * 4))) return rc;
    c->st_plist_valid = true; c->st_plist_cfg = c->cfg_version;
  }
  StatsArgs a{};
  a.sp = SplineRef{c->t0, c->dt, c->N, state_d, state_d + 3 * (size_t)c->N};
  a.cam = c->cam; a.locks = c->locks; a.mto = c->sensor_mto; a.t_map = c->t_map;
  a.n_imu = c->imu.n; a.imu_t = (const double*)c->imu.d_t.p; a.gyro = (const double*)c->imu.d_a3.p; a.acc = (const double*)c->imu.d_b3.p; a.w_gyro = c->imu.weight; a.w_acc = c->imu.huber;
  a.prior_t = c->prior_t; a.prior_q = mkq(c->prior_q[0], c->prior_q[1], c->prior_q[2], c->prior_q[3]); a.prior_w = c->prior_w;
  a.n_surf = c->surf.n; a.surf_t = (const double*)c->surf.d_t.p; a.surf_pt = (const double*)c->surf.d_a3.p; a.surf_pl = (const double*)c->surf.d_b3.p; a.surf_perm = (const int*)c->surf.d_perm.p;
  a.surf_w = c->surf.weight; a.surf_huber = c->surf.huber;
  a.n_rep = c->rep.n; a.rep_lm = (const int*)c->rep.d_id0.p; a.rep_uv = (const double*)c->rep.d_a3.p; a.rep_t0 = (const double*)c->rep.d_t.p; a.rep_w = c->rep.weight; a.rep_huber = c->rep.huber;
  a.n_cs = c->cs.n; a.cs_lm = (const int*)c->cs.d_id0.p; a.cs_plane = (const int*)c->cs.d_id1.p; a.cs_w = c->cs.weight; a.cs_huber = c->cs.huber;
  a.planes = (const double*)c->d_planes.p; a.lm_uv = (const double*)c->d_lm_uv.p; a.lm_t0 = (const double*)c->d_lm_t0.p; a.L = L;
  a.blk0[0] = 0;
  for (int f = 0; f < LVX_NUM_FAM; ++f) a.blk0[f + 1] = a.blk0[f] + (cnt[f] + 255) / 256;
  const int nblk = a.blk0[LVX_NUM_FAM];
  const size_t n_out = st_off_planes() + 3 * (size_t)P + 3 * (size_t)L;
  if ((rc = dev_alloc(c, c->d_st_part, (size_t)std::max(nblk, 1) * ST_W * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_st_val, ((size_t)c->surf.n + (size_t)c->rep.n + 2) * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_st_out, (n_out + 2) * 8))) return rc;
  if (c->h_st_cap < n_out) {
    if (c->h_st) { (void)hipHostFree(c->h_st); c->h_st = nullptr; c->h_st_cap = 0; }
    LVX_HIP(c, hipHostMalloc((void**)&c->h_st, n_out * 8, hipHostMallocDefault)); c->h_st_cap = n_out;
  }
  double* o = (double*)c->d_st_out.p;
  int* err_d = (int*)(o + n_out);   // the kernels' flag word, behind the results
  a.part = (double*)c->d_st_part.p; a.surf_val = (double*)c->d_st_val.p; a.rep_val = a.surf_val + c->surf.n; a.err = err_d;
  LVX_HIP(c, hipMemsetAsync(err_d, 0, 8, st));
  auto nb = [&](int f) { return dim3((unsigned)(a.blk0[f + 1] - a.blk0[f])); };   // one launch per family with blocks: each kernel holds only its family's registers
  if (cnt[0]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_GYRO>, nb(0), dim3(256), 0, st, a);
  if (cnt[1]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_ACCEL>, nb(1), dim3(256), 0, st, a);
  if (cnt[2]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_PRIOR>, nb(2), dim3(256), 0, st, a);
  if (cnt[3]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_SURFEL>, nb(3), dim3(256), 0, st, a);
  if (cnt[4]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_REPROJ>, nb(4), dim3(256), 0, st, a);
  if (cnt[5]) hipLaunchKernelGGL(k_stats_eval<LVX_FAM_CAMSURF>, nb(5), dim3(256), 0, st, a);
  StatsReduce r{};
  const int* pl = (const int*)c->d_st_plist.p;
  const int* lp = (const int*)c->d_repB[3].p;   // ensure_layout: [ptr (L + 1) | device positions of every landmark's blocks]
  double* po = o + st_off_planes(); double* lo = po + 3 * (size_t)P;
  r.seg[0] = StatsSeg{c->surf.n > 0 ? P : 0, pl, pl + P + 1, a.surf_val, (long long*)po, po + P, po + 2 * (size_t)P, 0};
  r.seg[1] = StatsSeg{c->rep.n > 0 ? L : 0, lp, lp + L + 1, a.rep_val, (long long*)lo, lo + L, lo + 2 * (size_t)L, 1};
  r.seg_blk[0] = 0; r.seg_blk[1] = (r.seg[0].n_seg + 3) / 4; r.seg_blk[2] = r.seg_blk[1] + (r.seg[1].n_seg + 3) / 4;
  r.part = a.part; for (int f = 0; f <= LVX_NUM_FAM; ++f) r.blk0[f] = a.blk0[f];
  r.fam_out = o; r.err = err_d;
  if (r.seg[0].n_seg == 0 && P > 0) LVX_HIP(c, hipMemsetAsync(po, 0, 3 * (size_t)P * 8, st));   // no rows at all: every segment reports n = 0 and zeros
  if (r.seg[1].n_seg == 0 && L > 0) LVX_HIP(c, hipMemsetAsync(lo, 0, 3 * (size_t)L * 8, st));
  hipLaunchKernelGGL(k_stats_reduce, dim3((unsigned)(r.seg_blk[2] + LVX_NUM_FAM)), dim3(256), 0, st, r);
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(c->h_st, o, n_out * 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));   // the one host stop
  c->st_P = P; c->st_L = L; c->st_cfg = c->cfg_version; c->st_valid = true;
  if (out) {
    std::memset(out, 0, sizeof(*out));
    for (int f = 0; f < LVX_NUM_FAM; ++f) {
      const double* rec = c->h_st + (size_t)f * ST_W;
      lvx_family_stats& fs = out->fam[f];
      fs.n_blocks = cnt[f]; fs.n_evaluated = (int64_t)rec[ST_EVAL]; fs.n_outliers = (int64_t)rec[ST_OUT]; fs.cost = rec[ST_COST];
      for (int k = 0; k < 3; ++k) { fs.sum[k] = rec[ST_SUM + k]; fs.sum_abs[k] = rec[ST_ABS + k]; fs.sum_sq[k] = rec[ST_SQ + k]; fs.max_abs[k] = rec[ST_MAX + k]; }
      out->cost += fs.cost;   // LVX_FAM_* order
    }
  }
  const int err = (int)c->h_st[(size_t)LVX_NUM_FAM * ST_W];
  if (err & RES_RANGE) return fail(c, LVX_E_RANGE, "time span out of range for trajectory");
  if (err & RES_NONUNIT) return fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions");
  return LVX_OK;
}

}  // namespace lvx

using namespace lvx;

extern "C" {

int lvx_error_statistics_d(lvx_ctx* c, const double* state_d, lvx_error_stats* out) {
  if (!c || !out) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  if (!state_d) { int rc = ensure_layout(c); if (rc) return rc; state_d = (const double*)c->d_state.p; }
  return run_stats(c, state_d, out);
}

int lvx_error_statistics(lvx_ctx* c, const double* state, lvx_error_stats* out) {
  if (!c || !state || !out) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  int rc = ensure_layout(c); if (rc) return rc;
  const size_t bytes = (size_t)lvx_state_size(c) * 8;   // a buffer of its own: the resident state of lvx_set_state / lvx_evaluate stays what it is
  if ((rc = dev_alloc(c, c->d_st_state, bytes))) return rc;
  LVX_HIP(c, hipMemcpyAsync(c->d_st_state.p, state, bytes, hipMemcpyHostToDevice, c->stream));
  return run_stats(c, (const double*)c->d_st_state.p, out);
}

int lvx_lidar_pose_statistics_d(lvx_ctx* c, const double* state_d, lvx_family_stats* out) {
  if (!c || !out) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  if (!state_d) { int rc = ensure_layout(c); if (rc) return rc; state_d = (const double*)c->d_state.p; }
  return run_lidarpos_stats(c, state_d, out);
}
int lvx_lidar_pose_statistics(lvx_ctx* c, const double* state, lvx_family_stats* out) {
  if (!c || !state || !out) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  int rc = ensure_layout(c); if (rc) return rc;
  const size_t bytes = (size_t)lvx_state_size(c) * 8;
  if ((rc = dev_alloc(c, c->d_st_state, bytes))) return rc;
  LVX_HIP(c, hipMemcpyAsync(c->d_st_state.p, state, bytes, hipMemcpyHostToDevice, c->stream));
  return run_lidarpos_stats(c, (const double*)c->d_st_state.p, out);
}

static int stats_ready(lvx_ctx* c) {
  if (!c->st_valid || c->layout_dirty || c->st_cfg != c->cfg_version) return fail(c, LVX_E_STATE, "no error statistics of the current problem: call lvx_error_statistics first");
  return LVX_OK;
}
int lvx_get_plane_stats(lvx_ctx* c, int n_planes, int64_t* n, double* sum_abs, double* max_abs) {
  if (!c) return LVX_E_ARG;
  int rc = stats_ready(c); if (rc) return rc;
  if (n_planes != c->st_P) return fail(c, LVX_E_ARG, "n_planes differs from the plane table of lvx_set_planes");
  const double* p = c->h_st + st_off_planes();
  const size_t P = (size_t)c->st_P;
  if (n) std::memcpy(n, p, P * 8);
  if (sum_abs) std::memcpy(sum_abs, p + P, P * 8);
  if (max_abs) std::memcpy(max_abs, p + 2 * P, P * 8);
  return LVX_OK;
}
int lvx_get_landmark_stats(lvx_ctx* c, int n_landmarks, int64_t* n, double* sum_sq, double* max_norm) {
  if (!c) return LVX_E_ARG;
  int rc = stats_ready(c); if (rc) return rc;
  if (n_landmarks != c->st_L) return fail(c, LVX_E_ARG, "n_landmarks differs from the landmark table of lvx_set_landmarks");
  const double* p = c->h_st + st_off_planes() + 3 * (size_t)c->st_P;
  const size_t L = (size_t)c->st_L;
  if (n) std::memcpy(n, p, L * 8);
  if (sum_sq) std::memcpy(sum_sq, p + L, L * 8);
  if (max_norm) std::memcpy(max_norm, p + 2 * L, L * 8);
  return LVX_OK;
}

}  // extern "C"
