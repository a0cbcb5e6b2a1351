// lvx_rotinit.hip — sensor-to-IMU rotation from odometry on the device: InertialInitializer::EstimateRotation (src/lvi_exc/src/core/inertial_initializer.cpp:26-81) for every
// prefix of a list and every time shift of a list in two launches.  Per-pair math, the order of the sums and the 4 x 4 eigen-solver: lvx_rotinit.h (shared with the host
// check, tests/native/rotinit_host_check.cpp).  Built without FP contraction, so the records are the bits the g++ build of the header gives.  A pass of its own: it reads
// a state and writes only its own buffers.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "lvx_ctx.h"
#include "lvx_rotinit.h"

namespace lvx {

static_assert(sizeof(RotOptions) == sizeof(lvx_rotinit_options) && sizeof(RotOptions) == 24, "lvx_rotinit_options");
static_assert(sizeof(RotResult) == sizeof(lvx_rotinit_result) && sizeof(RotResult) == 80, "lvx_rotinit_result");

#define LVX_ROT_BLOCK 256   // four tiles of 64 pairs, one wavefront each
struct RotArgs {
  const double* state; int N; double t0, dt;
  int n; const double* t; const double* q;         // odometry stamps [n], quaternions [n][4] (x, y, z, w)
  RotPrefixes P; int n_tau; const double* tau;       // tau NULL: one shift of 0
  RotOptions opt;
  double* pieces; int32_t* tile_drop;               // [n_tau][slots][ROT_REC], [n_tau][tiles]
  RotResult* results; int32_t* first_ok; int* flag;
};

// Pass 1.  Lanes over (pair, shift): blockIdx.y is the shift, a wavefront is one tile of 64 consecutive pairs.  No LDS and no barrier: the first dropped pair of the tile
// is the lowest set bit of a ballot, a piece's twelve sums go down the halving tree of rot_tile_sum by lane shuffles (lane l adds lane l + 32, + 16, ... + 1; the lanes
// at and above the stride compute values nobody reads), lane 0 stores the record.  A tile meets more than one segment only where a prefix ends inside it.
__global__ __launch_bounds__(LVX_ROT_BLOCK) void k_rot_pairs(RotArgs g) {
  const int lane = threadIdx.x & (LVX_ROT_TILE - 1);
  const int n_tiles = rot_num_tiles(g.n), n_seg = rot_num_prefixes(g.P), n_pairs = g.n - 1;
  const int tile = blockIdx.x * (LVX_ROT_BLOCK / LVX_ROT_TILE) + (threadIdx.x / LVX_ROT_TILE);
  if (tile >= n_tiles) return;   // whole wavefronts
  const int s = blockIdx.y;
  const double tau = g.tau ? g.tau[s] : 0.0;
  const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
  const int p = tile * LVX_ROT_TILE + lane;
  double a10[ROT_NSUM];
#pragma unroll
  for (int e = 0; e < ROT_NSUM; ++e) a10[e] = 0.0;
  int status = -1, seg = n_seg;
  if (p < n_pairs) {
    status = rot_pair(sp, g.t[p], g.t[p + 1], tau, load_q(g.q + 4 * (size_t)p), load_q(g.q + 4 * (size_t)(p + 1)), g.opt.huber_deg, a10);
    seg = rot_segment_of(g.P, p);
    if (status == ROT_NONUNIT) *g.flag = RES_NONUNIT;   // every such store writes the same value
  }
  const unsigned long long dropped = __ballot(status == ROT_DROPPED);
  const int drop = dropped ? __ffsll((long long)dropped) - 1 : LVX_ROT_TILE;
  if (lane == 0) g.tile_drop[(size_t)s * n_tiles + tile] = drop;
  const bool live = lane < drop;
  const bool counted = live && status == ROT_COUNTED, skipped = live && (status == ROT_SKIPPED || status == ROT_NONUNIT);
  const int seg_lo = __shfl(seg, 0);
  int seg_hi = __shfl(seg, LVX_ROT_TILE - 1);
  if (seg_hi > n_seg - 1) seg_hi = n_seg - 1;
  double* out = g.pieces + (size_t)s * rot_num_slots(g.P) * ROT_REC;
  for (int k = seg_lo; k <= seg_hi; ++k) {
    const bool in = seg == k;
    if (!__ballot(in)) continue;   // an empty segment
    double v[ROT_REC];
#pragma unroll
    for (int e = 0; e < ROT_NSUM; ++e) v[e] = in && counted ? a10[e] : 0.0;
    v[ROT_NSUM] = in && counted ? 1.0 : 0.0; v[ROT_NSUM + 1] = in && skipped ? 1.0 : 0.0;
#pragma unroll
    for (int off = LVX_ROT_TILE / 2; off > 0; off >>= 1)
#pragma unroll
      for (int e = 0; e < ROT_REC; ++e) v[e] = v[e] + __shfl_down(v[e], off);
    if (lane == 0) {
      double* r = out + (size_t)ROT_REC * rot_slot(tile, k);
#pragma unroll
      for (int e = 0; e < ROT_REC; ++e) r[e] = v[e];
    }
  }
}

// Pass 2.  One workgroup per shift, one lane per prefix: the pieces of the segments 0 .. k in order, the Jacobi solve, the record; the lowest prefix with ok is an integer
// minimum in LDS.
__global__ __launch_bounds__(LVX_ROT_BLOCK) void k_rot_solve(RotArgs g) {
  __shared__ int s_first;
  const int n_tiles = rot_num_tiles(g.n), n_seg = rot_num_prefixes(g.P);
  const int s = blockIdx.x;
  if (threadIdx.x == 0) s_first = n_seg;
  __syncthreads();
  const double* pieces = g.pieces + (size_t)s * rot_num_slots(g.P) * ROT_REC;
  const int32_t* tile_drop = g.tile_drop + (size_t)s * n_tiles;
  int first = n_seg;
  for (int k = threadIdx.x; k < n_seg; k += LVX_ROT_BLOCK) {
    double sum[ROT_REC];
    rot_prefix_sum(g.P, k, pieces, tile_drop, sum);
    RotResult r;
    rot_solve(sum, rot_prefix_len(g.P, k), g.opt, &r);
    g.results[(size_t)s * n_seg + k] = r;
    if (r.ok && k < first) first = k;
  }
  if (first < n_seg) atomicMin(&s_first, first);
  __syncthreads();
  if (threadIdx.x == 0) g.first_ok[s] = s_first < n_seg ? s_first : -1;
}

void rotinit_destroy(lvx_ctx* c) {
  for (auto& b : c->d_ri) if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
}

}  // namespace lvx

using namespace lvx;

namespace {

enum { RI_STATE = 0, RI_IN = 1, RI_WORK = 2 };
enum { TJ_FLAG = 3 };   // the flag words of the trajectory queries (lvx_traj.hip): [0] the host-array calls, [1] the _d calls, looked at by lvx_synchronize

int rot_prepare(lvx_ctx* c) {
  LVX_HIP(c, hipSetDevice(c->device));
  if (!c->d_tj[TJ_FLAG].p) {
    int rc = dev_alloc(c, c->d_tj[TJ_FLAG], 16);
    if (rc) return rc;
    LVX_HIP(c, hipMemsetAsync(c->d_tj[TJ_FLAG].p, 0, 16, c->stream));
  }
  if (!c->h_tj) { LVX_HIP(c, hipHostMalloc((void**)&c->h_tj, 32 * 8, hipHostMallocDefault)); std::memset(c->h_tj, 0, 32 * 8); }
  return LVX_OK;
}
size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }
// the two launches; work: [pieces | tile_drop]
int rot_launch(lvx_ctx* c, RotArgs g) {
  const int n_tau = g.tau ? g.n_tau : 1, n_tiles = rot_num_tiles(g.n);
  const size_t piece_bytes = (size_t)n_tau * rot_num_slots(g.P) * ROT_REC * 8;
  int rc = dev_alloc(c, c->d_ri[RI_WORK], piece_bytes + align8((size_t)n_tau * n_tiles * 4));
  if (rc) return rc;
  g.pieces = (double*)c->d_ri[RI_WORK].p; g.tile_drop = (int32_t*)((char*)c->d_ri[RI_WORK].p + piece_bytes);
  { ProfScope ps(c, LVX_KERNEL_UPSTREAM);
    hipLaunchKernelGGL(k_rot_pairs, dim3((n_tiles + 3) / 4, n_tau), dim3(LVX_ROT_BLOCK), 0, c->stream, g);
    hipLaunchKernelGGL(k_rot_solve, dim3(n_tau), dim3(LVX_ROT_BLOCK), 0, c->stream, g); }
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
int rot_args(lvx_ctx* c, int n, const double* t, const double* q, int n_prefix, int n_tau, const void* results, const void* first_ok) {
  if (!c) return LVX_E_ARG;
  if (!t || !q || !results || !first_ok || n <= 0 || n_prefix < 0 || n_tau < 0 || n_tau > 65535) return fail(c, LVX_E_ARG, "lvx_estimate_rotation: n <= 0, a negative count or a required pointer is NULL");
  if (!c->have_spline) return fail(c, LVX_E_STATE, "lvx_set_spline has not been called");
  return LVX_OK;
}
RotOptions rot_options(const lvx_rotinit_options* opt) {
  lvx_rotinit_options d; lvx_rotinit_default_options(&d);
  if (opt) d = *opt;
  return RotOptions{d.huber_deg, d.min_pairs, 0, d.min_sigma};
}

}  // namespace

extern "C" {

int lvx_rotinit_default_options(lvx_rotinit_options* opt) {
  if (!opt) return LVX_E_ARG;
  opt->huber_deg = 1.0; opt->min_pairs = 15; opt->reserved = 0; opt->min_sigma = 0.25;
  return LVX_OK;
}

int lvx_estimate_rotation_d(lvx_ctx* c, const double* state_d, int n, const double* t_d, const double* q_xyzw4_d, int n_prefix, const int32_t* prefix_len_d, int n_tau,
                            const double* tau_d, const lvx_rotinit_options* opt, lvx_rotinit_result* results_d, int32_t* first_ok_d) {
  int rc = rot_args(c, n, t_d, q_xyzw4_d, n_prefix, n_tau, results_d, first_ok_d);
  if (rc) return rc;
  if ((rc = rot_prepare(c))) return rc;
  if (!state_d) {
    if ((rc = ensure_layout(c))) return rc;
    state_d = (const double*)c->d_state.p;
  }
  if (!prefix_len_d || n_prefix == 0) { prefix_len_d = nullptr; n_prefix = 0; }
  if (!tau_d || n_tau == 0) { tau_d = nullptr; n_tau = 0; }
  RotArgs g{};
  g.state = state_d; g.N = c->N; g.t0 = c->t0; g.dt = c->dt; g.n = n; g.t = t_d; g.q = q_xyzw4_d;
  g.P = RotPrefixes{prefix_len_d, n_prefix, n}; g.n_tau = n_tau; g.tau = tau_d; g.opt = rot_options(opt);
  g.results = (RotResult*)results_d; g.first_ok = first_ok_d; g.flag = (int*)c->d_tj[TJ_FLAG].p + 1;
  c->tj_d_unchecked = true;
  return rot_launch(c, g);
}

int lvx_estimate_rotation(lvx_ctx* c, const double* state, int n, const double* t, const double* q_xyzw4, int n_prefix, const int32_t* prefix_len, int n_tau, const double* tau,
                          const lvx_rotinit_options* opt, lvx_rotinit_result* results, int32_t* first_ok) {
  int rc = rot_args(c, n, t, q_xyzw4, n_prefix, n_tau, results, first_ok);
  if (rc) return rc;
  if (!state) return fail(c, LVX_E_ARG, "lvx_estimate_rotation: n <= 0, a negative count or a required pointer is NULL");
  if (!prefix_len || n_prefix == 0) { prefix_len = nullptr; n_prefix = 0; }
  if (!tau || n_tau == 0) { tau = nullptr; n_tau = 0; }
  for (int k = 0; k < n_prefix; ++k)
    if (prefix_len[k] < 1 || prefix_len[k] > n || (k > 0 && prefix_len[k] < prefix_len[k - 1]))
      return fail(c, LVX_E_ARG, "lvx_estimate_rotation: prefix_len must be non-decreasing with every entry in [1, n]");
  if ((rc = rot_prepare(c))) return rc;
  hipStream_t st = c->stream;
  const size_t nn = (size_t)n, np = (size_t)(n_prefix ? n_prefix : 1), nt = (size_t)(n_tau ? n_tau : 1);
  if ((rc = upload(c, c->d_ri[RI_STATE], state, (size_t)lvx_state_size(c) * 8))) return rc;
  // inputs [t | q | tau | results | first_ok | prefix_len]
  const size_t o_tau = 5 * nn * 8, o_res = o_tau + nt * 8, o_first = o_res + nt * np * sizeof(RotResult), o_len = o_first + align8(nt * 4);
  if ((rc = dev_alloc(c, c->d_ri[RI_IN], o_len + align8(np * 4)))) return rc;
  char* in = (char*)c->d_ri[RI_IN].p;
  LVX_HIP(c, hipMemcpyAsync(in, t, nn * 8, hipMemcpyHostToDevice, st));
  LVX_HIP(c, hipMemcpyAsync(in + nn * 8, q_xyzw4, nn * 32, hipMemcpyHostToDevice, st));
  if (tau) LVX_HIP(c, hipMemcpyAsync(in + o_tau, tau, nt * 8, hipMemcpyHostToDevice, st));
  if (prefix_len) LVX_HIP(c, hipMemcpyAsync(in + o_len, prefix_len, np * 4, hipMemcpyHostToDevice, st));
  int* flag = (int*)c->d_tj[TJ_FLAG].p;
  LVX_HIP(c, hipMemsetAsync(flag, 0, 4, st));
  RotArgs g{};
  g.state = (const double*)c->d_ri[RI_STATE].p; g.N = c->N; g.t0 = c->t0; g.dt = c->dt; g.n = n; g.t = (const double*)in; g.q = (const double*)(in + nn * 8);
  g.P = RotPrefixes{prefix_len ? (const int32_t*)(in + o_len) : nullptr, n_prefix, n}; g.n_tau = n_tau; g.tau = tau ? (const double*)(in + o_tau) : nullptr; g.opt = rot_options(opt);
  g.results = (RotResult*)(in + o_res); g.first_ok = (int32_t*)(in + o_first); g.flag = flag;
  if ((rc = rot_launch(c, g))) return rc;
  LVX_HIP(c, hipMemcpyAsync(results, g.results, nt * np * sizeof(RotResult), hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(first_ok, g.first_ok, nt * 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(c->h_tj, flag, 4, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));   // the one host stop
  int w; std::memcpy(&w, c->h_tj, 4);
  return w ? fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions") : LVX_OK;
}

}  // extern "C"
