// lvx_handoff.hip — the surfel family and its plane table from DEVICE arrays (include/lvx.h: lvx_set_planes_d, lvx_set_surfel_d; lvx_set_surfel_from_association in
// lvx_upstream.hip ends here too), and the surfel block of ensure_layout as kernels: ordered selection, key per row, stable sort by key, gather, row-ordered plane
// copy, permutation, per-interval histogram.  What the host needs of it is the row count, the extremes of the plane ids and the histogram (<= N + 1 integers): the
// sorted key vector of upload_chunks / upload_chunks_rows is rebuilt from the histogram, so chunk tables and the deterministic colouring are the host route's.
//
// Kernels of one hand-off talk to each other only through stream order (one launch per phase): nothing here waits on another workgroup of its own launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "lvx_ctx.h"

namespace lvx {
namespace {

constexpr int HO_TB = 256;   // threads per workgroup = candidates per compaction tile (4 wavefronts)
constexpr int HO_HDR = 4;    // d_work: [0] rows selected, [1] plane id min, [2] plane id max, [3] unused | tile offsets [tiles + 1] | histogram

__device__ __forceinline__ bool ho_take(const double* t, int j, int cap, int step, bool use_tmap, double t_map) {
  if (j >= cap) return false;
  return !use_tmap || t[(size_t)j * (size_t)step] >= t_map;   // (a NaN time is dropped, as `t >= t_map` drops it on the host)
}
// rows a tile of HO_TB candidates keeps
__global__ __launch_bounds__(HO_TB) void k_ho_count(const double* t, int cap, int step, int use_tmap, double t_map, int* tile) {
  __shared__ int s_w[HO_TB / 64];
  const int j = blockIdx.x * HO_TB + threadIdx.x;
  const unsigned long long m = __ballot(ho_take(t, j, cap, step, use_tmap != 0, t_map));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) { int s = 0; for (int w = 0; w < HO_TB / 64; ++w) s += s_w[w]; tile[blockIdx.x] = s; }
}
// exclusive scan of the tile counts in place (one workgroup: thread i owns a contiguous run of tiles), total -> hdr[0]; resets the id extremes
__global__ __launch_bounds__(HO_TB) void k_ho_scan(int* tile, int n_tiles, int* hdr) {
  __shared__ int s[HO_TB];
  const int per = (n_tiles + HO_TB - 1) / HO_TB, a = min(n_tiles, (int)threadIdx.x * per), b = min(n_tiles, a + per);
  int sum = 0;
  for (int i = a; i < b; ++i) sum += tile[i];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < HO_TB; o <<= 1) {
    const int v = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  int run = s[threadIdx.x] - sum;
  for (int i = a; i < b; ++i) { const int v = tile[i]; tile[i] = run; run += v; }
  if (threadIdx.x == HO_TB - 1) { hdr[0] = s[HO_TB - 1]; hdr[1] = INT_MAX; hdr[2] = INT_MIN; hdr[3] = 0; }
}
// stable compaction: the kept rows of tile b go to [tile[b], tile[b] + count) in candidate order; extremes of their plane ids
__global__ __launch_bounds__(HO_TB) void k_ho_compact(const double* pt, const double* t, const int* pl, int cap, int step, int use_tmap, double t_map, const int* tile,
                                                      double* o_pt, double* o_t, int* o_pl, int* hdr) {
  __shared__ int s_w[HO_TB / 64];
  const int j = blockIdx.x * HO_TB + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool take = ho_take(t, j, cap, step, use_tmap != 0, t_map);
  const unsigned long long m = __ballot(take);
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int base = tile[blockIdx.x];
  for (int k = 0; k < w; ++k) base += s_w[k];
  int lo = INT_MAX, hi = INT_MIN;
  if (take) {
    const size_t i = (size_t)j * (size_t)step, d = (size_t)(base + __popcll(m & ((1ull << lane) - 1ull)));
    const int id = pl[i];
    o_t[d] = t[i]; o_pl[d] = id;
    o_pt[3 * d] = pt[3 * i]; o_pt[3 * d + 1] = pt[3 * i + 1]; o_pt[3 * d + 2] = pt[3 * i + 2];
    lo = hi = id;
  }
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  if (lane == 0 && m) { atomicMin(hdr + 1, lo); atomicMax(hdr + 2, hi); }
}
// knot interval of every row (host_i0: the same knot_lookup, -1 out of range) as the sort key `interval + 1`, the identity permutation, rows per key.  n_d: the row
// count is still on the device (the call that selected the rows has not stopped yet).  Lanes of a wavefront with equal keys add to the histogram once.
__global__ __launch_bounds__(HO_TB) void k_ho_keys(const double* t, int n_fixed, const int* n_d, double t0, double dt, int N, unsigned* ukey, int* iota, int* hist) {
  const int n = n_d ? *n_d : n_fixed;
  const int i = blockIdx.x * HO_TB + threadIdx.x, lane = threadIdx.x & 63;
  const bool on = i < n;
  int u = 0;
  if (on) {
    KnotRef k;
    const double ti = t[i];
    u = knot_lookup(t0, dt, N, ti, ti, &k) ? k.i0 + 1 : 0;
    ukey[i] = (unsigned)u; iota[i] = i;
  }
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int ku = __shfl(u, leader);
    const unsigned long long same = __ballot(on && u == ku);
    if (lane == leader) atomicAdd(hist + ku, __popcll(same));
    todo &= ~same;
  }
}
// device order: row r is input row perm[r]; its plane's closest point beside it (zero for an id outside the table: the layout reports it before any pass runs)
__global__ __launch_bounds__(HO_TB) void k_ho_gather(int n, const int* perm, const double* in_t, const double* in_pt, const int* in_pl, const double* planes, int n_planes,
                                                     double* o_t, double* o_pt, int* o_pl, double* o_rowpl) {
  const int r = blockIdx.x * HO_TB + threadIdx.x;
  if (r >= n) return;
  const size_t i = (size_t)perm[r], d = (size_t)r;
  const int id = in_pl[i];
  o_t[d] = in_t[i]; o_pl[d] = id;
  const bool ok = id >= 0 && id < n_planes;
  for (int c = 0; c < 3; ++c) { o_pt[3 * d + c] = in_pt[3 * i + c]; o_rowpl[3 * d + c] = ok ? planes[3 * (size_t)id + c] : 0.0; }
}
// Pi (closest point) of P plane records [p4 4 | Pi 3 | box 6 | 4 ints] = 15 doubles each
__global__ void k_ho_planes(int P, const double* recs, double* pi3) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < 3 * P) pi3[e] = recs[(size_t)(e / 3) * 15 + 4 + e % 3];
}

unsigned blocks_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + HO_TB - 1) / HO_TB); }

int pin_reserve(lvx_ctx* c, size_t ints) {
  lvx_ctx::Handoff& h = c->ho;
  if (h.pin && h.pin_cap >= ints) return LVX_OK;
  if (h.pin) { LVX_HIP(c, hipStreamSynchronize(c->stream)); (void)hipHostFree(h.pin); h.pin = nullptr; h.pin_cap = 0; }
  LVX_HIP(c, hipHostMalloc((void**)&h.pin, ints * 4, hipHostMallocDefault));
  h.pin_cap = ints;
  return LVX_OK;
}
int* work_hist(lvx_ctx* c, size_t tiles) { return (int*)c->ho.d_work.p + HO_HDR + tiles + 1; }
// keys + histogram of `rows` candidates of in_t[set] for the current spline, histogram -> pinned words [4 ..]; the caller waits for the stream
int keys_enqueue(lvx_ctx* c, int set, int rows, const int* n_d, size_t tiles) {
  lvx_ctx::Handoff& h = c->ho;
  hipStream_t st = c->stream;
  const int N = c->N;
  int* hist = work_hist(c, tiles);
  LVX_HIP(c, hipMemsetAsync(hist, 0, (size_t)(N + 1) * 4, st));
  hipLaunchKernelGGL(k_ho_keys, dim3(blocks_of((size_t)rows)), dim3(HO_TB), 0, st, (const double*)h.in_t[set].p, rows, n_d, c->t0, c->dt, N, (unsigned*)h.d_key.p, (int*)h.d_iota.p, hist);
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(h.pin + HO_HDR, hist, (size_t)(N + 1) * 4, hipMemcpyDeviceToHost, st));
  return LVX_OK;
}
void keep_hist(lvx_ctx* c) {
  lvx_ctx::Handoff& h = c->ho;
  h.hist.assign(h.pin + HO_HDR, h.pin + HO_HDR + c->N + 1);
  h.hist_valid = true; h.hist_t0 = c->t0; h.hist_dt = c->dt; h.hist_N = c->N;
}
void clear_surfel(lvx_ctx* c, double t_map, double huber, double weight) {   // lvx_set_surfel(n = 0)
  Family& f = c->surf;
  f.n = 0; f.t.clear(); f.a3.clear(); f.id0.clear();
  f.huber = huber; f.weight = weight; c->t_map = t_map; c->layout_dirty = true;
  c->ho.surf_dev = false; c->ho.hist_valid = false;
}

}  // namespace

void handoff_destroy(lvx_ctx* c) {
  lvx_ctx::Handoff& h = c->ho;
  for (DevBuf* b : {&h.d_planes_in, &h.in_t[0], &h.in_t[1], &h.in_pt[0], &h.in_pt[1], &h.in_pl[0], &h.in_pl[1], &h.d_key, &h.d_iota, &h.d_skey, &h.d_work, &h.d_tmp})
    if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->bytes = 0; }
  if (h.pin) { (void)hipHostFree(h.pin); h.pin = nullptr; h.pin_cap = 0; }
}

int handoff_planes_from_records(lvx_ctx* c, int P, const void* records_d) {
  lvx_ctx::Handoff& h = c->ho;
  int rc;
  if ((rc = dev_alloc(c, h.d_planes_in, (size_t)P * 24))) return rc;
  if (P > 0) {
    hipLaunchKernelGGL(k_ho_planes, dim3(blocks_of((size_t)3 * P)), dim3(HO_TB), 0, c->stream, P, (const double*)records_d, (double*)h.d_planes_in.p);
    LVX_HIP(c, hipGetLastError());
  }
  c->planes.assign((size_t)P * 3, 0.0);
  h.planes_dev = true; h.planes_stale = P > 0; c->layout_dirty = true;
  return LVX_OK;
}

int handoff_set_surfel(lvx_ctx* c, int total, int step, bool use_tmap, const double* pt3_d, const double* t_d, const int32_t* plane_d, double t_map, double huber, double weight, int32_t* n_used) {
  lvx_ctx::Handoff& h = c->ho;
  hipStream_t st = c->stream;
  if (n_used) *n_used = 0;
  if (step <= 0) step = 1;
  const int cap = total > 0 ? (int)(((long long)total + step - 1) / step) : 0;
  if (cap == 0) { clear_surfel(c, t_map, huber, weight); return LVX_OK; }
  int rc;
  const int set = h.sel ^ 1;
  const size_t tiles = blocks_of((size_t)cap);
  const bool keys = c->have_spline;
  if ((rc = dev_alloc(c, h.in_t[set], (size_t)cap * 8)) || (rc = dev_alloc(c, h.in_pt[set], (size_t)cap * 24)) || (rc = dev_alloc(c, h.in_pl[set], (size_t)cap * 4))) return rc;
  if ((rc = dev_alloc(c, h.d_key, (size_t)cap * 4)) || (rc = dev_alloc(c, h.d_iota, (size_t)cap * 4))) return rc;
  if ((rc = dev_alloc(c, h.d_work, (HO_HDR + tiles + 1 + (size_t)(keys ? c->N + 1 : 0)) * 4))) return rc;
  if ((rc = pin_reserve(c, HO_HDR + (size_t)(keys ? c->N + 1 : 0)))) return rc;
  h.hist_valid = false;   // (d_key / d_iota are overwritten below: a family this call does not replace computes its keys again at the layout)
  int* hdr = (int*)h.d_work.p; int* tile = hdr + HO_HDR;
  hipLaunchKernelGGL(k_ho_count, dim3((unsigned)tiles), dim3(HO_TB), 0, st, t_d, cap, step, use_tmap ? 1 : 0, t_map, tile);
  hipLaunchKernelGGL(k_ho_scan, dim3(1), dim3(HO_TB), 0, st, tile, (int)tiles, hdr);
  hipLaunchKernelGGL(k_ho_compact, dim3((unsigned)tiles), dim3(HO_TB), 0, st, pt3_d, t_d, (const int*)plane_d, cap, step, use_tmap ? 1 : 0, t_map, (const int*)tile,
                     (double*)h.in_pt[set].p, (double*)h.in_t[set].p, (int*)h.in_pl[set].p, hdr);
  LVX_HIP(c, hipGetLastError());
  LVX_HIP(c, hipMemcpyAsync(h.pin, hdr, HO_HDR * 4, hipMemcpyDeviceToHost, st));
  if (keys && (rc = keys_enqueue(c, set, cap, hdr, tiles))) return rc;
  LVX_HIP(c, hipStreamSynchronize(st));   // THE host stop of the hand-off: rows kept, plane id extremes, rows per knot interval
  const int n = h.pin[0];
  if (n < 0 || n > cap) return fail(c, LVX_E_STATE, "surfel hand-off: the device reported an impossible row count");
  if (n == 0) { clear_surfel(c, t_map, huber, weight); return LVX_OK; }
  if (h.pin[1] < 0 || (size_t)h.pin[2] * 3 >= c->planes.size()) return fail(c, LVX_E_ARG, "plane id out of range (call lvx_set_planes first)");
  Family& f = c->surf;
  f.n = n; f.t.clear(); f.a3.clear(); f.id0.clear();
  f.huber = huber; f.weight = weight; c->t_map = t_map; c->layout_dirty = true;
  h.sel = set; h.surf_dev = true; h.id_min = h.pin[1]; h.id_max = h.pin[2];
  if (keys) keep_hist(c);
  if (n_used) *n_used = n;
  return LVX_OK;
}

int handoff_planes_to_device(lvx_ctx* c) {
  lvx_ctx::Handoff& h = c->ho;
  if (!h.planes_dev) return upload_tmp(c, c->d_planes, c->planes.data(), c->planes.size() * 8);
  const size_t bytes = c->planes.size() * 8;
  if (h.planes_stale && c->surf.n > 0 && !h.surf_dev) {   // a host-origin surfel family builds its row-ordered plane copy on the host
    LVX_HIP(c, hipMemcpyAsync(c->planes.data(), h.d_planes_in.p, bytes, hipMemcpyDeviceToHost, c->stream));
    LVX_HIP(c, hipStreamSynchronize(c->stream));
    h.planes_stale = false;
  }
  const int rc = dev_alloc(c, c->d_planes, bytes); if (rc) return rc;
  if (bytes) LVX_HIP(c, hipMemcpyAsync(c->d_planes.p, h.d_planes_in.p, bytes, hipMemcpyDeviceToDevice, c->stream));
  return LVX_OK;
}

int handoff_layout_surfel(lvx_ctx* c, std::vector<int>& sk) {
  lvx_ctx::Handoff& h = c->ho;
  Family& f = c->surf;
  hipStream_t st = c->stream;
  const int n = f.n, N = c->N, set = h.sel;
  int rc;
  if (!(h.hist_valid && h.hist_N == N && !std::memcmp(&h.hist_t0, &c->t0, 8) && !std::memcmp(&h.hist_dt, &c->dt, 8))) {   // the spline changed since the call (or was not set yet)
    const size_t tiles = blocks_of((size_t)n);
    if ((rc = dev_alloc(c, h.d_work, (HO_HDR + tiles + 1 + (size_t)N + 1) * 4)) || (rc = pin_reserve(c, HO_HDR + (size_t)N + 1))) return rc;
    if ((rc = keys_enqueue(c, set, n, nullptr, tiles))) return rc;
    LVX_HIP(c, hipStreamSynchronize(st));
    keep_hist(c);
  }
  sk.resize((size_t)n);
  { size_t at = 0;
    for (int u = 0; u <= N && at < (size_t)n; ++u) { const size_t e = std::min((size_t)n, at + (size_t)std::max(h.hist[u], 0)); std::fill(sk.begin() + at, sk.begin() + e, u - 1); at = e; }
    if (at != (size_t)n) return fail(c, LVX_E_STATE, "surfel hand-off: the interval histogram does not add up to the row count"); }
  // stable sort of (interval + 1, input row) by key: the permutation of stable_perm_by_key
  int bits = 1; while (bits < 31 && (1ll << bits) <= (long long)N) ++bits;
  if ((rc = dev_alloc(c, h.d_skey, (size_t)n * 4)) || (rc = dev_alloc(c, f.d_perm, (size_t)n * 4))) return rc;
  if ((rc = sort_pairs_u32(c, h.d_tmp, (unsigned*)h.d_key.p, (unsigned*)h.d_skey.p, (int*)h.d_iota.p, (int*)f.d_perm.p, (size_t)n, bits))) return rc;
  if ((rc = dev_alloc(c, f.d_t, (size_t)n * 8)) || (rc = dev_alloc(c, f.d_a3, (size_t)n * 24)) || (rc = dev_alloc(c, f.d_id0, (size_t)n * 4)) || (rc = dev_alloc(c, f.d_b3, (size_t)n * 24))) return rc;
  hipLaunchKernelGGL(k_ho_gather, dim3(blocks_of((size_t)n)), dim3(HO_TB), 0, st, n, (const int*)f.d_perm.p, (const double*)h.in_t[set].p, (const double*)h.in_pt[set].p, (const int*)h.in_pl[set].p,
                     (const double*)c->d_planes.p, (int)(c->planes.size() / 3), (double*)f.d_t.p, (double*)f.d_a3.p, (int*)f.d_id0.p, (double*)f.d_b3.p);
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}

int handoff_fetch_ids(lvx_ctx* c) {
  lvx_ctx::Handoff& h = c->ho;
  Family& f = c->surf;
  if (!h.surf_dev || f.id0.size() == (size_t)f.n) return LVX_OK;
  f.id0.assign((size_t)f.n, 0);
  LVX_HIP(c, hipMemcpyAsync(f.id0.data(), h.in_pl[h.sel].p, (size_t)f.n * 4, hipMemcpyDeviceToHost, c->stream));
  LVX_HIP(c, hipStreamSynchronize(c->stream));
  return LVX_OK;
}

}  // namespace lvx

using namespace lvx;

extern "C" {

int lvx_set_planes_d(lvx_ctx* c, int n, const double* pi3_d) { if (c) c->cfg_version++;
  if (!c || n < 0 || (n > 0 && !pi3_d)) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  lvx_ctx::Handoff& h = c->ho;
  const int rc = dev_alloc(c, h.d_planes_in, (size_t)n * 24); if (rc) return rc;
  if (n > 0) LVX_HIP(c, hipMemcpyAsync(h.d_planes_in.p, pi3_d, (size_t)n * 24, hipMemcpyDeviceToDevice, c->stream));
  c->planes.assign((size_t)n * 3, 0.0);
  h.planes_dev = true; h.planes_stale = n > 0; c->layout_dirty = true;
  return LVX_OK;
}

int lvx_set_surfel_d(lvx_ctx* c, int n, const double* pt3_d, const double* t_d, const int32_t* plane_id_d, double t_map, double huber, double weight) { if (c) c->cfg_version++;
  if (!c || n < 0 || (n > 0 && (!pt3_d || !t_d || !plane_id_d))) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  return handoff_set_surfel(c, n, 1, false, pt3_d, t_d, plane_id_d, t_map, huber, weight, nullptr);
}

}  // extern "C"
