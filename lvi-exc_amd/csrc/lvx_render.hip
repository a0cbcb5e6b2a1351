// lvx_render.hip — what LCIoptimize produces after the last solve: the map coloured from camera images through the calibrated LiDAR -> camera chain
// (LIinitializer::RenderMap, src/lvi_exc/test/lvi_initialize_surfel_orb.cpp:711-811) and the scans drawn into their images (ReprojectPointCloudToImage, :1307-1363);
// the batched evaluateCameraPose (trajectory_manager_lvi.cpp:430-440).  Per-point math: lvx_render.h (shared with the host check).  Built without FP contraction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "lvx_ctx.h"
#include "lvx_pose.h"
#include "lvx_projcov.h"
#include "lvx_render.h"

namespace lvx {

static_assert(sizeof(lvx_point_xyzrgb) == 16, "pcl::PointXYZRGB record");
static_assert(sizeof(RenderTable) % 8 == 0, "table layout");

__global__ void k_camera_pose(const double* state, int N, double t0, double dt, int n, const double* t, double* q4, double* p3, int* valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  quat q; v3 p;
  const bool ok = camera_pose_dev(state, N, t0, dt, t[i], &q, &p);
  valid[i] = ok ? 1 : 0;
  if (ok) { q4[4 * (size_t)i] = q.x; q4[4 * (size_t)i + 1] = q.y; q4[4 * (size_t)i + 2] = q.z; q4[4 * (size_t)i + 3] = q.w; p3[3 * (size_t)i] = p.x; p3[3 * (size_t)i + 1] = p.y; p3[3 * (size_t)i + 2] = p.z; }
}

// The pose table of one k_render_map launch, built on the device: lane i < n_images evaluates the camera pose at image_t[i], lane n_images the LiDAR pose at the map
// time; the coloured-point counter is cleared.  One workgroup of 64.
__global__ __launch_bounds__(64) void k_render_poses(const double* state, int N, double t0, double dt, const double* times /* [n_images] image_t | map_time */, int n_images,
                                                     RenderTable* tab, unsigned long long* count) {
  const int i = threadIdx.x;
  quat q; v3 p;
  if (i < n_images) {
    const bool ok = camera_pose_dev(state, N, t0, dt, times[i], &q, &p);
    tab->valid[i] = ok ? 1 : 0;
    if (ok) tab->cam[i] = render_pose(q, p);
  } else if (i == n_images) {
    const bool ok = lidar_pose_dev(state, N, t0, dt, times[n_images], &q, &p);
    tab->map_valid = ok ? 1 : 0; tab->n_images = n_images;
    if (ok) tab->L0 = render_pose(q, p);
    *count = 0ull;
  }
}

// RenderMap: one lane per point, grid-stride.  Per point one 16-byte load (float4 xyzi) and one 16-byte store (the record) — 32 B of HBM traffic; the grey value is one
// byte gathered from an image that stays in L2.  The table is read at wave-uniform addresses (scalar loads).  Coloured points: per-lane count, wave reduction, one LDS word
// per wave, one 64-bit atomic add per workgroup (integer adds: the sum does not depend on the order).
#define LVX_RENDER_BLOCK 256
__global__ __launch_bounds__(LVX_RENDER_BLOCK) void k_render_map(const float4* __restrict__ pts, long long n, const RenderTable* __restrict__ tab, lvx_pinhole cam,
                                                                  const uint8_t* __restrict__ images, int pitch, double z_min, double z_max, uint4* __restrict__ out,
                                                                  unsigned long long* __restrict__ count) {
  __shared__ int wsum[LVX_RENDER_BLOCK / 64];
  int mine = 0;
  const long long stride = (long long)gridDim.x * LVX_RENDER_BLOCK;
  for (long long i = (long long)blockIdx.x * LVX_RENDER_BLOCK + threadIdx.x; i < n; i += stride) {
    const float4 p = pts[i];
    const float xyz[3] = {p.x, p.y, p.z};
    lvx_point_xyzrgb rec;
    const int st = render_point_images(xyz, *tab, cam, images, pitch, z_min, z_max, &rec);
    mine += st == RENDER_COLORED ? 1 : 0;
    uint4 w;
    w.x = __float_as_uint(rec.x); w.y = __float_as_uint(rec.y); w.z = __float_as_uint(rec.z);
    w.w = (unsigned)rec.b | ((unsigned)rec.g << 8) | ((unsigned)rec.r << 16) | ((unsigned)rec.a << 24);
    out[i] = w;
  }
  for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < LVX_RENDER_BLOCK / 64; ++k) tot += wsum[k];
    if (tot) atomicAdd(count, (unsigned long long)tot);
  }
}

// ReprojectPointCloudToImage: per (scan, image) pair the chain of :1333-1336, evaluated on the device
struct OverlayPair { quat q_LtoC; v3 p_LinC; quat q_GtoScan; int32_t scan, valid; };
__global__ void k_overlay_poses(const double* state, int N, double t0, double dt, int n_pairs, const int* scan_index, const double* scan_t, const double* image_t, OverlayPair* pairs, int* valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  quat qL, qC; v3 pL, pC;
  OverlayPair o;
  o.scan = scan_index[i];
  o.valid = (lidar_pose_dev(state, N, t0, dt, scan_t[i], &qL, &pL) && camera_pose_dev(state, N, t0, dt, image_t[i], &qC, &pC)) ? 1 : 0;
  if (o.valid) { overlay_chain(qL, pL, qC, pC, &o.q_LtoC, &o.p_LinC); o.q_GtoScan = quat{-qL.x, -qL.y, -qL.z, qL.w}; }
  else { o.q_LtoC = quat{0, 0, 0, 1}; o.p_LinC = mk(0, 0, 0); o.q_GtoScan = quat{0, 0, 0, 1}; }
  pairs[i] = o; valid[i] = o.valid;
}
struct RawPoint { float x, y, z, pad; float intensity; float pad2; double timestamp; };   // lvx_point_xyzit
static_assert(sizeof(RawPoint) == 32, "PointXYZIT layout (pcl_utils.h:39-44)");
// blockIdx.y = pair, one lane per point of its scan.  The point is de-skewed rotation-only into the scan's frame at the scan time exactly as lvx_undistort_scan with
// correct_position = 0 does (ScanUndistortion::undistortScan: a NaN return stays NaN, a stamp outside the spline keeps the resize()'d zeros), rounded to float — the
// reference's VPoint — and projected.  Every store writes the same value 1: the mask does not depend on the order.
__global__ __launch_bounds__(256) void k_overlay(const double* state, int N, double t0, double dt, const RawPoint* __restrict__ raw, int HW, const OverlayPair* __restrict__ pairs, lvx_pinhole cam,
                                                 uint8_t* __restrict__ mask) {
  const OverlayPair pr = pairs[blockIdx.y];
  if (!pr.valid) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  const RawPoint r = raw[(size_t)pr.scan * HW + i];
  if (isnan(r.x)) return;
  float xyz[3] = {0.f, 0.f, 0.f};
  quat q; v3 p;
  if (lidar_pose_dev(state, N, t0, dt, r.timestamp, &q, &p)) {
    const v3 po = qrot(qmul(pr.q_GtoScan, q), mk((double)r.x, (double)r.y, (double)r.z));
    xyz[0] = (float)po.x; xyz[1] = (float)po.y; xyz[2] = (float)po.z;
  }
  const int px = overlay_point(xyz, pr.q_LtoC, pr.p_LinC, cam);
  if (px >= 0) mask[(size_t)blockIdx.y * (size_t)cam.rows * (size_t)cam.cols + (size_t)px] = 1;
}


// lvx_projection_covariance, the launches around k_proj_hub (lvx_selinv.h).  They stand here because this translation unit is built without FP contraction: the
// poses are k_render_poses' bits and uv, the depth test and the bounds test round as k_render_map's, so a point's status IS lvx_render_map_d's decision.
// k_proj_poses: lane i < n_images the camera pose at image_t[i], lane n_images the LiDAR pose at t_map.  One workgroup of 64.
static_assert(sizeof(ProjTable) % 8 == 0 && sizeof(ProjImage) % 8 == 0 && offsetof(ProjTable, img) % 8 == 0, "table layout");
__global__ __launch_bounds__(64) void k_proj_poses(const double* state, int N, double t0, double dt, double t_map, int n_images, const double* __restrict__ image_t, ProjTable* tab) {
  const int i = threadIdx.x;
  quat q; v3 p;
  if (i < n_images) {
    const bool ok = camera_pose_dev(state, N, t0, dt, image_t[i], &q, &p);
    tab->img[i].valid = ok ? 1 : 0; tab->img[i].pad = 0;
    if (ok) tab->img[i].C = render_pose(q, p);
  } else if (i == n_images) {
    const bool ok = lidar_pose_dev(state, N, t0, dt, t_map, &q, &p);
    tab->map_valid = ok ? 1 : 0; tab->n_images = n_images; tab->status = 0; tab->pad = 0;
    if (ok) tab->L0 = render_pose(q, p);
  }
}
// A lane per point, 256 per workgroup, grid-stride.  The table (the LiDAR pose and per image the camera pose and the 78 entries of pose_cov: 112 + 728 n_images
// bytes) is staged in LDS once per workgroup; neighbouring lanes almost always stop at the same image, so its reads are broadcasts.  Per point one 16-byte load and
// 77 bytes of plain vector stores (uv 16, cov 32, sigma 16, sigma_max 8, image 4: 76, and the status byte), each array only where it was asked for.  A failed call (status 1 / 2 of
// k_proj_hub) writes nothing.
#define LVX_PROJ_BLOCK 256
struct ProjOut { double* uv; double* cov; double* sigma; double* sigma_max; int32_t* image; uint8_t* status; };
__global__ __launch_bounds__(LVX_PROJ_BLOCK) void k_proj_cov(const float4* __restrict__ pts, long long n, const ProjTable* __restrict__ tab_g, lvx_pinhole cam, double z_min, double z_max, ProjOut o) {
  __shared__ ProjTable tab;
  const int st = tab_g->status;
  if (st == 1 || st == 2) return;
  const int nw = (int)((offsetof(ProjTable, img) + (size_t)tab_g->n_images * sizeof(ProjImage)) / 8);
  for (int e = threadIdx.x; e < nw; e += LVX_PROJ_BLOCK) ((double*)&tab)[e] = ((const double*)tab_g)[e];
  __syncthreads();
  const long long stride = (long long)gridDim.x * LVX_PROJ_BLOCK;
  for (long long i = (long long)blockIdx.x * LVX_PROJ_BLOCK + threadIdx.x; i < n; i += stride) {
    const float4 p = pts[i];
    const float xyz[3] = {p.x, p.y, p.z};
    ProjRecord r;
    proj_point_images(xyz, tab, cam, z_min, z_max, &r);
    if (o.uv) { o.uv[2 * i] = r.uv[0]; o.uv[2 * i + 1] = r.uv[1]; }   // (8-byte stores: the caller's arrays need no more than a double's alignment)
    if (o.cov) { o.cov[4 * i] = r.cov[0]; o.cov[4 * i + 1] = r.cov[1]; o.cov[4 * i + 2] = r.cov[2]; o.cov[4 * i + 3] = r.cov[3]; }
    if (o.sigma) { o.sigma[2 * i] = r.sigma[0]; o.sigma[2 * i + 1] = r.sigma[1]; }
    if (o.sigma_max) o.sigma_max[i] = r.sigma_max;
    if (o.image) o.image[i] = r.image;
    o.status[i] = (uint8_t)r.status;
  }
}

int proj_poses_enqueue(lvx_ctx* c, const double* state_d, double t_map, int n_images, const double* image_t_d, void* tab) {
  hipLaunchKernelGGL(k_proj_poses, dim3(1), dim3(64), 0, c->stream, state_d, c->N, c->t0, c->dt, t_map, n_images, image_t_d, (ProjTable*)tab);
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}

}  // namespace lvx

using namespace lvx;

namespace {

lvx_pinhole pinhole_of(const CamIntr& k) {
  lvx_pinhole p;
  p.rows = k.rows; p.cols = k.cols; p.readout = k.readout; p.fx = k.fx; p.fy = k.fy; p.cx = k.cx; p.cy = k.cy; p.k1 = k.k1; p.k2 = k.k2; p.p1 = k.p1; p.p2 = k.p2; p.k3 = k.k3;
  return p;
}

// state, times -> table and counter in d_rn[0]; the launch over the cloud; image_valid / n_colored back (one host stop)
int render_run(lvx_ctx* c, const double* state, double map_time, long long n, const float4* pts_d, int n_images, const uint8_t* images_d, int pitch, const double* image_t,
               const lvx_render_options* opt_in, lvx_point_xyzrgb* out_d, int32_t* image_valid, int64_t* n_colored) {
  lvx_render_options o; lvx_render_default_options(&o); if (opt_in) o = *opt_in;
  hipStream_t st = c->stream;
  int rc;
  if ((rc = upload(c, c->d_rn[1], state, (size_t)lvx_state_size(c) * 8))) return rc;
  double times[LVX_RENDER_MAX_IMAGES + 1];
  for (int i = 0; i < n_images; ++i) times[i] = image_t[i];
  times[n_images] = map_time;
  const size_t tab_off = sizeof(times), cnt_off = tab_off + sizeof(RenderTable);
  if ((rc = dev_alloc(c, c->d_rn[0], cnt_off + 8))) return rc;
  char* base = (char*)c->d_rn[0].p;
  LVX_HIP(c, hipMemcpyAsync(base, times, sizeof(times), hipMemcpyHostToDevice, st));
  RenderTable* tab = (RenderTable*)(base + tab_off); unsigned long long* cnt = (unsigned long long*)(base + cnt_off);
  int dev_cus = 256;
  (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c->device);
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_render_poses, dim3(1), dim3(64), 0, st, (const double*)c->d_rn[1].p, c->N, c->t0, c->dt, (const double*)base, n_images, tab, cnt);
    const long long blocks = std::min<long long>((n + LVX_RENDER_BLOCK - 1) / LVX_RENDER_BLOCK, (long long)dev_cus * 8);   // 8 workgroups of 4 waves per CU: full occupancy, the loop takes the rest
    hipLaunchKernelGGL(k_render_map, dim3((unsigned)blocks), dim3(LVX_RENDER_BLOCK), 0, st, pts_d, n, (const RenderTable*)tab, pinhole_of(c->cam), images_d, pitch, o.z_min, o.z_max,
                       (uint4*)out_d, cnt); }
  LVX_HIP(c, hipGetLastError());
  struct { int32_t map_valid; int32_t valid[LVX_RENDER_MAX_IMAGES]; unsigned long long count; } back;
  LVX_HIP(c, hipMemcpyAsync(&back.map_valid, &tab->map_valid, 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(back.valid, tab->valid, sizeof(back.valid), hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(&back.count, cnt, 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  if (!back.map_valid) {   // (the kernel wrote zero records)
    for (int i = 0; i < n_images; ++i) image_valid[i] = 0;
    *n_colored = 0;
    return fail(c, LVX_E_RANGE, "map time outside the trajectory");
  }
  for (int i = 0; i < n_images; ++i) image_valid[i] = back.valid[i];
  *n_colored = (int64_t)back.count;
  return LVX_OK;
}

}  // namespace

int lvx::proj_cov_enqueue(lvx_ctx* c, long long n, const float* xyzi4_d, const void* tab, double z_min, double z_max, double* uv, double* cov, double* sigma, double* sigma_max,
                          int32_t* image, uint8_t* status) {
  const long long blocks = std::min<long long>((n + LVX_PROJ_BLOCK - 1) / LVX_PROJ_BLOCK, (long long)c->n_cu * 8);   // the loop takes the rest, the table is staged once per workgroup
  hipLaunchKernelGGL(k_proj_cov, dim3((unsigned)blocks), dim3(LVX_PROJ_BLOCK), 0, c->stream, (const float4*)xyzi4_d, n, (const ProjTable*)tab, pinhole_of(c->cam), z_min, z_max,
                     ProjOut{uv, cov, sigma, sigma_max, image, status});
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}

namespace {

int render_args(lvx_ctx* c, const double* state, int n, int n_images, const uint8_t* images, int pitch, const double* image_t, const void* out, const int32_t* image_valid, const int64_t* n_colored) {
  if (!c) return LVX_E_ARG;
  if (!state || n < 0 || !images || !image_t || !image_valid || !n_colored || (n > 0 && !out)) return fail(c, LVX_E_ARG, "lvx_render_map: a required pointer is NULL");
  if (n_images < 1 || n_images > LVX_RENDER_MAX_IMAGES) return fail(c, LVX_E_ARG, "lvx_render_map: 1 .. 32 images per call");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  if (c->cam.rows <= 0 || c->cam.cols <= 0) return fail(c, LVX_E_STATE, "lvx_set_camera has not been called");
  if (pitch < c->cam.cols) return fail(c, LVX_E_ARG, "lvx_render_map: pitch < cols");
  return LVX_OK;
}

}  // namespace

extern "C" {

int lvx_evaluate_camera_pose(lvx_ctx* c, const double* state, int n, const double* t, double* q4, double* p3, int32_t* valid) {
  if (!c || !state || n < 0 || (n > 0 && (!t || !q4 || !p3 || !valid))) return LVX_E_ARG;
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  if (n == 0) return LVX_OK;
  LVX_HIP(c, hipSetDevice(c->device));
  int rc;
  if ((rc = upload(c, c->d_rn[1], state, (size_t)lvx_state_size(c) * 8))) return rc;
  if ((rc = upload(c, c->d_rn[2], t, (size_t)n * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_rn[3], (size_t)n * (32 + 24 + 4)))) return rc;
  double* dq = (double*)c->d_rn[3].p; double* dp = dq + 4 * (size_t)n; int* dv = (int*)(dp + 3 * (size_t)n);
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_camera_pose, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const double*)c->d_rn[1].p, c->N, c->t0, c->dt, n, (const double*)c->d_rn[2].p, dq, dp, dv); }
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(q4, dq, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
  LVX_HIP(c, hipMemcpyAsync(p3, dp, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  LVX_HIP(c, hipMemcpyAsync(valid, dv, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  LVX_HIP(c, hipStreamSynchronize(c->stream));
  return LVX_OK;
}

int lvx_render_default_options(lvx_render_options* o) {
  if (!o) return LVX_E_ARG;
  o->z_min = 0.1; o->z_max = 15.0; o->reserved[0] = o->reserved[1] = 0;   // lvi_initialize_surfel_orb.cpp:757
  return LVX_OK;
}

int lvx_render_map(lvx_ctx* c, const double* state, double map_time, int n, const float* map_xyzi4, int n_images, const uint8_t* images, int pitch, const double* image_t,
                   const lvx_render_options* opt, lvx_point_xyzrgb* out, int32_t* image_valid, int64_t* n_colored) {
  int rc = render_args(c, state, map_xyzi4 ? n : 0, n_images, images, pitch, image_t, out, image_valid, n_colored);
  if (rc) return rc;
  const float4* pts_d = nullptr;
  if (!map_xyzi4) {   // the cloud the last association left on the device: nothing to upload
    const long long np = (long long)c->da_S * c->da_H * c->da_W;
    if (np == 0 || !c->d_da[4].p || c->d_da[4].bytes < (size_t)np * 16) return fail(c, LVX_E_STATE, "lvx_data_association has not been called");
    if (!out) return fail(c, LVX_E_ARG, "lvx_render_map: a required pointer is NULL");
    n = (int)np; pts_d = (const float4*)c->d_da[4].p;
  }
  if (n == 0) return LVX_OK;
  LVX_HIP(c, hipSetDevice(c->device));
  const size_t image_bytes = (size_t)c->cam.rows * (size_t)pitch * (size_t)n_images;
  if (!pts_d) { if ((rc = upload(c, c->d_rn[2], map_xyzi4, (size_t)n * 16))) return rc; pts_d = (const float4*)c->d_rn[2].p; }
  if ((rc = upload(c, c->d_rn[3], images, image_bytes))) return rc;
  if ((rc = dev_alloc(c, c->d_rn[4], (size_t)n * 16))) return rc;
  rc = render_run(c, state, map_time, n, pts_d, n_images, (const uint8_t*)c->d_rn[3].p, pitch, image_t, opt, (lvx_point_xyzrgb*)c->d_rn[4].p, image_valid, n_colored);
  if (rc != LVX_OK && rc != LVX_E_RANGE) return rc;
  LVX_HIP(c, hipMemcpyAsync(out, c->d_rn[4].p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));   // (LVX_E_RANGE: zero records)
  LVX_HIP(c, hipStreamSynchronize(c->stream));
  return rc;
}

int lvx_render_map_d(lvx_ctx* c, const double* state, double map_time, int n, const float* map_xyzi4_d, int n_images, const uint8_t* images_d, int pitch, const double* image_t,
                     const lvx_render_options* opt, lvx_point_xyzrgb* out_d, int32_t* image_valid, int64_t* n_colored) {
  int rc = render_args(c, state, map_xyzi4_d ? n : 0, n_images, images_d, pitch, image_t, out_d, image_valid, n_colored);
  if (rc) return rc;
  long long np = n;
  if (!map_xyzi4_d) {
    np = (long long)c->da_S * c->da_H * c->da_W;
    if (np == 0 || !c->d_da[4].p || c->d_da[4].bytes < (size_t)np * 16) return fail(c, LVX_E_STATE, "lvx_data_association has not been called");
    if (!out_d) return fail(c, LVX_E_ARG, "lvx_render_map: a required pointer is NULL");
    map_xyzi4_d = (const float*)c->d_da[4].p;
  }
  if (np == 0) return LVX_OK;
  LVX_HIP(c, hipSetDevice(c->device));
  return render_run(c, state, map_time, np, (const float4*)map_xyzi4_d, n_images, images_d, pitch, image_t, opt, out_d, image_valid, n_colored);
}

int lvx_overlay_scans(lvx_ctx* c, const double* state, int n_pairs, const int32_t* scan_index, const double* scan_t, const double* image_t, uint8_t* mask, int32_t* valid) {
  if (!c) return LVX_E_ARG;
  if (!state || n_pairs < 0 || (n_pairs > 0 && (!scan_index || !scan_t || !image_t || !mask || !valid))) return fail(c, LVX_E_ARG, "lvx_overlay_scans: a required pointer is NULL");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  if (c->cam.rows <= 0 || c->cam.cols <= 0) return fail(c, LVX_E_STATE, "lvx_set_camera has not been called");
  const int HW = c->da_H * c->da_W;
  if (c->da_S <= 0 || HW <= 0 || !c->d_da[0].p) return fail(c, LVX_E_STATE, "lvx_set_scans has not been called");
  for (int i = 0; i < n_pairs; ++i) if (scan_index[i] < 0 || scan_index[i] >= c->da_S) return fail(c, LVX_E_ARG, "lvx_overlay_scans: scan index outside the scans");
  if (n_pairs == 0) return LVX_OK;
  LVX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  int rc;
  if ((rc = upload(c, c->d_rn[1], state, (size_t)lvx_state_size(c) * 8))) return rc;
  // [scan_t | image_t | pairs | scan_index | valid]
  const size_t np = (size_t)n_pairs, off_pairs = np * 16, off_idx = off_pairs + np * sizeof(OverlayPair), off_valid = off_idx + np * 4;
  if ((rc = dev_alloc(c, c->d_rn[2], off_valid + np * 4))) return rc;
  char* base = (char*)c->d_rn[2].p;
  LVX_HIP(c, hipMemcpyAsync(base, scan_t, np * 8, hipMemcpyHostToDevice, st));
  LVX_HIP(c, hipMemcpyAsync(base + np * 8, image_t, np * 8, hipMemcpyHostToDevice, st));
  LVX_HIP(c, hipMemcpyAsync(base + off_idx, scan_index, np * 4, hipMemcpyHostToDevice, st));
  const size_t mask_bytes = np * (size_t)c->cam.rows * (size_t)c->cam.cols;
  if ((rc = dev_alloc(c, c->d_rn[4], mask_bytes))) return rc;
  LVX_HIP(c, hipMemsetAsync(c->d_rn[4].p, 0, mask_bytes, st));
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_overlay_poses, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, st, (const double*)c->d_rn[1].p, c->N, c->t0, c->dt, n_pairs, (const int*)(base + off_idx),
                       (const double*)base, (const double*)(base + np * 8), (OverlayPair*)(base + off_pairs), (int*)(base + off_valid));
    for (int p0 = 0; p0 < n_pairs; p0 += 32768) {   // (grid.y limit)
      const int m = std::min(32768, n_pairs - p0);
      hipLaunchKernelGGL(k_overlay, dim3((unsigned)((HW + 255) / 256), (unsigned)m), dim3(256), 0, st, (const double*)c->d_rn[1].p, c->N, c->t0, c->dt, (const RawPoint*)c->d_da[0].p, HW,
                         (const OverlayPair*)(base + off_pairs) + p0, pinhole_of(c->cam), (uint8_t*)c->d_rn[4].p + (size_t)p0 * c->cam.rows * c->cam.cols);
    } }
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(mask, c->d_rn[4].p, mask_bytes, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(valid, base + off_valid, np * 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  return LVX_OK;
}

}  // extern "C"
