// lvx_selinv.h — selected inverse of the damped LM system from its sequential factor, and the three queries that read it.  In file order: the selected inverse
// (k_border_inv, k_band_selinv); what the queries share (SigmaView and its accessors, the window of a pose's scalars, J W J^T); then what each adds — pose covariances
// (lvx_trajectory_covariance: nothing but the pose Jacobian), landmark covariances (lvx_landmark_covariance: the eliminated landmark's row) and LiDAR map point
// covariances (lvx_map_point_covariance: a lane per point, two pose windows and their cross block); last, the pixel covariance of map points in the images
// (lvx_projection_covariance: k_proj_hub, one wavefront per image, the camera's and the LiDAR's pose windows with their cross block).
// Included by lvx_solver.hip (its translation unit holds the factor's kernels).
//
// reduce_to_border(force_seq) leaves   Lb[j (bw + 1) + d] = L(j + d, j)   (band Cholesky),   Z[r ldz + j] = (L^-1 A_bc)(j, r)   and   S = A_cc - Zc^T Zc (unfactored),
// so A over (band, border) has the factor G = [[L, 0], [Zc^T, L_S]].  The entries of Sigma = A^-1 on the pattern of G + G^T follow back to front (Takahashi):
//   Sigma_cc = S^-1                                                                                   k_border_inv
//   Sigma(i, j) = -(1 / G_jj) sum_{k in N(j)} G(k, j) Sigma(k, i),   N(j) = band rows below j + border   k_band_selinv
//   Sigma(j, j) = 1 / G_jj^2 - (1 / G_jj) sum_{k in N(j)} G(k, j) Sigma(k, j)
// k_band_selinv takes 16 columns J at a time against the trailing set T = (TB band rows below the panel, the border), TB = max(bw, 23) rounded up to 16 — a
// superset of the profile, structural zeros in G, on which the recurrence is as valid as on the profile itself.  In block form
//   W = G_TJ^T Sigma_TT (16 x m)          the product: v_mfma_f64_16x16x4_f64, one 16 x 16 accumulator tile of W per wavefront, Sigma_TT read from global memory
//   Sigma_TJ^T = -Linv^T W,   Sigma_JJ = Linv^T (I + W G_TJ) Linv,   Linv = G_JJ^-1 (16 x 16 triangle, by substitution)
// which is the 16-step recurrence inside the panel written once.  Sigma_TT lives in a RING: a dense symmetric (R + nbd') x (R + nbd') array, R = TB + 16, band position
// p at slot p mod R — the panel's own 16 slots are those of the positions that just left the window.  512 KB at bw = 180, nbd = 46: resident in L2.  One workgroup,
// no atomics, no waiting on another workgroup; what a query reads afterwards is stored apart: SigB[j][d] = Sigma(j + d, j), d <= 23, and Sigma(border r, j) over Z's
// border rows in place.  For the landmark call the same values also go to SigW[j][d], d <= TB (every d the panel's columns reach lies on the block pattern).
#pragma once
#include "lvx_chol16.h"
#include "lvx_lmcov.h"
#include "lvx_projcov.h"
#include "lvx_ptcov.h"

namespace lvx {

#define SI_NT 1024
#define SI_BD 24          // stored band entries per column of the selected inverse: d = 0 .. 23, the reach of four knots

__host__ __device__ inline int si_up16(int x) { return (x + 15) & ~15; }
__host__ __device__ inline int si_tb(int bw) { return si_up16(bw > 23 ? bw : 23); }

// Sigma_cc = S^-1 (n <= 128, as k_dense_partial): Cholesky in LDS, the factor's inverse by substitution (one thread per column), Linv^T Linv.  S (lower triangle in)
// becomes the full symmetric inverse in place; a pivot <= 0 goes to info[1] / (double) info[2..3] as k_dense_partial reports it.
__global__ __launch_bounds__(SI_NT) void k_border_inv(double* S, int n, int* info) {
  extern __shared__ double ds[];   // T [n][n + 1] | V [n][n + 1]
  const int tid = threadIdx.x, ld = n + 1;
  double* T = ds; double* V = ds + (size_t)n * ld;
  for (int e = tid; e < n * n; e += SI_NT) T[(e / n) * ld + e % n] = S[e];
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    if (tid == 0) { const double d = T[k * ld + k]; if (!(d > 0.0)) { if (info[1] == 0) { info[1] = k + 1; ((double*)(info + 2))[0] = d; } T[k * ld + k] = 1.0; } else T[k * ld + k] = sqrt(d); }
    __syncthreads();
    const double inv = 1.0 / T[k * ld + k];
    for (int rr = k + 1 + tid; rr < n; rr += SI_NT) T[rr * ld + k] *= inv;
    __syncthreads();
    for (int c0 = k + 1; c0 < n; c0 += 64) {
      const int cc = c0 + (tid & 63);
      const double lc = cc < n ? T[cc * ld + k] : 0.0;
      for (int rr = k + 1 + (tid >> 6); rr < n; rr += SI_NT / 64) if (cc < n && rr >= cc) T[rr * ld + cc] -= T[rr * ld + k] * lc;
    }
    __syncthreads();
  }
  if (tid < n) {   // column tid of L^-1
    const int c = tid;
    for (int r = 0; r < c; ++r) V[r * ld + c] = 0.0;
    V[c * ld + c] = 1.0 / T[c * ld + c];
    for (int r = c + 1; r < n; ++r) {
      double s = 0.0;
      for (int q = c; q < r; ++q) s += T[r * ld + q] * V[q * ld + c];
      V[r * ld + c] = -s / T[r * ld + r];
    }
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += SI_NT) {
    const int a = e / n, b = e % n;
    if (b > a) continue;
    double s = 0.0;
    for (int q = a; q < n; ++q) s += V[q * ld + a] * V[q * ld + b];
    S[a * n + b] = s; S[b * n + a] = s;
  }
}

// lowest band position any query's window holds -> *lowest (the caller starts it at nb); one thread per query
__global__ void k_tc_lowest(const double* __restrict__ state, int N, double t0, double dt, int frame, int n, const double* __restrict__ t, const int* __restrict__ ord, int* lowest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double tau = frame == LVX_FRAME_TRAJECTORY ? 0.0 : state[7 * (size_t)N + (frame == LVX_FRAME_CAMERA ? 31 : 23)];
  KnotRef k;
  if (!traj_knot(t0, dt, N, t[i] + tau, &k)) return;
  int lo = 0x7fffffff;
  for (int c = 0; c < 24; ++c) { const int o = ord[6 * k.i0 + c]; if (o >= 0 && o < lo) lo = o; }
  if (lo != 0x7fffffff) atomicMin(lowest, lo);
}

struct SelInv {
  const double* Lb; int nb, bw; double* Z; int ldz, nbd;
  const double* Scc;      // Sigma_cc, full symmetric [nbd][nbd] (k_border_inv)
  double* D; int M;       // the ring, zero on entry: [M][M], M = R + up16(nbd)
  double* SigB;           // [nb][SI_BD]
  const int* lowest; const int* info;
  double* SigW;           // [nb][TB + 1], or null: SigW[j][d] = Sigma(j + d, j), d <= TB (lvx_landmark_covariance)
};
__global__ __launch_bounds__(SI_NT) void k_band_selinv(SelInv g) {
  extern __shared__ double ds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fk = lane >> 4, fi = lane & 15;
  const int nb = g.nb, bw = g.bw, nbd = g.nbd, TB = si_tb(bw), R = TB + 16, nbp = si_up16(nbd), mT = TB + nbp, M = g.M;
  const int ldg = 17, ldw = mT + 1;
  double* Gp = ds;                              // [16 + mT][17]: rows 0..15 the panel's triangle, then G_TJ
  double* Wt = Gp + (size_t)(16 + mT) * ldg;    // [16][mT + 1]
  double* Xt = Wt + 16 * (size_t)ldw;           // [16][mT + 1]: Sigma_TJ^T
  double* Li = Xt + 16 * (size_t)ldw;           // [16][17] Linv
  double* Q = Li + 16 * ldg;                    // [16][17] W G_TJ, then (I + Q) Linv
  double* P = Q + 16 * ldg;                     // [16][17] Sigma_JJ
  if (g.info[0] != 0 || g.info[1] != 0) return;   // a lost pivot: the caller reports it, nothing is read from here
  const int lowest = *g.lowest;
  if (lowest >= nb) return;
  double* D = g.D;
  for (int e = tid; e < nbd * nbd; e += SI_NT) D[(size_t)(R + e / nbd) * M + R + e % nbd] = g.Scc[e];
  __threadfence();
  __syncthreads();
  for (int j0 = ((nb - 1) >> 4) << 4; j0 >= 0 && j0 + 15 >= lowest; j0 -= 16) {
    const int nk = min(16, nb - j0);
    const int sJ = j0 % R, sT0 = (j0 + 16) % R;   // ring slots of the panel and of the first trailing row (both multiples of 16; the trailing rows wrap at R)
    for (int e = tid; e < (16 + mT) * 16; e += SI_NT) {
      const int r = e >> 4, c = e & 15, j = j0 + c;
      double v = 0.0;
      if (c < nk) {
        if (r < 16 + TB) { const int i = j0 + r, d = i - j; if (i < nb && d >= 0 && d <= bw) v = g.Lb[(size_t)j * (bw + 1) + d]; }
        else { const int b = r - 16 - TB; if (b < nbd) v = g.Z[(size_t)b * g.ldz + j]; }
      } else if (r == c) v = 1.0;
      Gp[r * ldg + c] = v;
    }
    __syncthreads();
    // W = G_TJ^T Sigma_TT: A[c][k] = G(T_k, j0 + c) from LDS, B[k][i] = Sigma(T_k, T_i) from the ring
    for (int tile = wave; tile < mT / 16; tile += SI_NT / 64) {
      const int i0 = tile * 16;
      int cs = i0 < TB ? sT0 + i0 : R + (i0 - TB); if (i0 < TB && cs >= R) cs -= R;
      d4c acc = d4c{0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < mT; k0 += 16) {
        int rs = k0 < TB ? sT0 + k0 : R + (k0 - TB); if (k0 < TB && rs >= R) rs -= R;
        const double* Dk = D + (size_t)(rs + fk) * M + cs + fi;
        const double b0 = Dk[0], b1 = Dk[(size_t)4 * M], b2 = Dk[(size_t)8 * M], b3 = Dk[(size_t)12 * M];
        const double* Gk = Gp + (16 + k0 + fk) * ldg + fi;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Gk[0], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Gk[4 * ldg], b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Gk[8 * ldg], b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Gk[12 * ldg], b3, acc, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) Wt[(fk + 4 * v) * ldw + i0 + fi] = acc[v];
    }
    __syncthreads();
    // Linv by substitution (one thread per column) beside Q = W G_TJ (256 threads)
    if (tid < 16) {
      const int c = tid;
      for (int r = 0; r < c; ++r) Li[r * ldg + c] = 0.0;
      Li[c * ldg + c] = 1.0 / Gp[c * ldg + c];
      for (int r = c + 1; r < 16; ++r) {
        double s = 0.0;
        for (int q = c; q < r; ++q) s += Gp[r * ldg + q] * Li[q * ldg + c];
        Li[r * ldg + c] = -s / Gp[r * ldg + r];
      }
    } else if (tid >= 64 && tid < 64 + 256) {
      const int a = (tid - 64) >> 4, b = (tid - 64) & 15;
      double s = 0.0;
      for (int k = 0; k < mT; ++k) s += Wt[a * ldw + k] * Gp[(16 + k) * ldg + b];
      Q[a * ldg + b] = s;
    }
    __syncthreads();
    // Sigma_TJ^T = -Linv^T W; U = (I + Q) Linv (held in registers across the barrier)
    for (int e = tid; e < 16 * mT; e += SI_NT) {
      const int c = e / mT, i = e % mT;
      double s = 0.0;
      for (int q = c; q < 16; ++q) s += Li[q * ldg + c] * Wt[q * ldw + i];
      Xt[c * ldw + i] = -s;
    }
    double u = 0.0;
    if (tid < 256) {
      const int a = tid >> 4, b = tid & 15;
      u = a >= b ? Li[a * ldg + b] : 0.0;
      for (int q = b; q < 16; ++q) u += Q[a * ldg + q] * Li[q * ldg + b];
    }
    __syncthreads();
    if (tid < 256) Q[(tid >> 4) * ldg + (tid & 15)] = u;
    __syncthreads();
    if (tid < 256) {
      const int a = tid >> 4, b = tid & 15;
      if (a >= b) {
        double s = 0.0;
        for (int q = a; q < 16; ++q) s += Li[q * ldg + a] * Q[q * ldg + b];
        P[a * ldg + b] = s; P[b * ldg + a] = s;
      }
    }
    __syncthreads();
    // into the ring (both triangles), the band store and Z's border rows; the columns beyond nb of the last panel are zero
    for (int e = tid; e < 16 * mT; e += SI_NT) {
      const int c = e / mT, i = e % mT;
      const double v = c < nk ? Xt[c * ldw + i] : 0.0;
      int s = i < TB ? sT0 + i : R + (i - TB); if (i < TB && s >= R) s -= R;
      D[(size_t)s * M + sJ + c] = v;
      D[(size_t)(sJ + c) * M + s] = v;
      if (c < nk) {
        if (i < TB) {
          const int d = 16 + i - c;
          if (d < SI_BD && j0 + 16 + i < nb) g.SigB[(size_t)(j0 + c) * SI_BD + d] = v;
          if (g.SigW && d <= TB && j0 + 16 + i < nb) g.SigW[(size_t)(j0 + c) * (TB + 1) + d] = v;
        }
        else if (i - TB < nbd) g.Z[(size_t)(i - TB) * g.ldz + j0 + c] = v;
      }
    }
    if (tid < 256) {
      const int a = tid >> 4, b = tid & 15;
      const double v = (a < nk && b < nk) ? P[a * ldg + b] : 0.0;
      D[(size_t)(sJ + a) * M + sJ + b] = v;
      if (a >= b && a < nk) { g.SigB[(size_t)(j0 + b) * SI_BD + (a - b)] = v; if (g.SigW) g.SigW[(size_t)(j0 + b) * (TB + 1) + (a - b)] = v; }
    }
    __threadfence();
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------
// What every query reads from the factored step, written once.
//   SigmaView       ord[] and the stores of Sigma' (the SCALED system's selected inverse): a band store with its row stride (SigB, stride SI_BD, or SigW, stride
//                   TB + 1), Z's border rows, Sigma_cc, the Jacobi scale and the pivot words.
//   sigma_at        Sigma' between two positions: >= 0 a band position, < 0 border slot -1 - o.  scale_at: the Jacobi scale of a position, 0 for LVX_DEAD.
//   window_scalars  a window's tangent indices -> pos[] (through ord[]; LVX_DEAD constant or absent), sc[] and the index written out (-1 where dead).
//   window_gather   W[a][b] = Sigma'(pos a, pos b) sc[a] sc[b] (unscaled), element e = lane, lane + 64, ...; zero where either scalar is dead.
//   window_sandwich T = J W over a ascending, C = T J^T for r >= s over b ascending, mirrored: every sum in index order.
// The helpers work on the calling kernel's __shared__ arrays, one wavefront per window; the bit identity between the queries (a landmark's pose window against
// lvx_trajectory_covariance's, a point's t_map window likewise) is that of one piece of code.
// ---------------------------------------------------------------------------------------------------------
struct SigmaView {
  const int* ord;
  const double* band; int stride;   // band[j stride + d] = Sigma'(j + d, j), d < stride
  const double* Z; int ldz, nb, nbd; const double* Scc; const double* scale;
  const int* info; int force_bad;   // the factor's pivot codes; the tests' switch TEST_BAD_PIVOT
};
__device__ __forceinline__ bool sigma_lost(const SigmaView& v) { return v.force_bad || v.info[0] != 0 || v.info[1] != 0; }
__device__ __forceinline__ double sigma_at(const SigmaView& v, int pa, int pb) {
  if (pa >= 0 && pb >= 0) { const int lo = min(pa, pb), d = max(pa, pb) - lo; return d < v.stride ? v.band[(size_t)lo * v.stride + d] : 0.0; }
  if (pa >= 0) return v.Z[(size_t)(-1 - pb) * v.ldz + pa];
  if (pb >= 0) return v.Z[(size_t)(-1 - pa) * v.ldz + pb];
  const int ra = -1 - pa, rb = -1 - pb;
  return v.Scc[(size_t)max(ra, rb) * v.nbd + min(ra, rb)];
}
__device__ __forceinline__ double scale_at(const SigmaView& v, int o) { return o == LVX_DEAD ? 0.0 : v.scale[o >= 0 ? o : v.nb + (-1 - o)]; }
// lanes first .. W - 1, one window scalar each (idx < 0: absent); widx null: not asked for
template <int W>
__device__ __forceinline__ void window_scalars(const SigmaView& v, const int* idx, int first, int lane, int* pos, double* sc, int32_t* widx) {
  if (lane < first || lane >= W) return;
  int o = LVX_DEAD, id = -1;
  if (idx[lane] >= 0) { o = v.ord[idx[lane]]; if (o != LVX_DEAD) id = idx[lane]; }
  pos[lane] = o; sc[lane] = scale_at(v, o);
  if (widx) widx[lane] = id;
}
// out null: not asked for; otherwise the window as [W][W], dense
template <int W>
__device__ __forceinline__ void window_gather(const SigmaView& v, const int* pos, const double* sc, int lane, double (*Wm)[W + 1], double* out) {
  for (int e = lane; e < W * W; e += 64) {
    const int a = e / W, b = e % W, pa = pos[a], pb = pos[b];
    double s = 0.0;
    if (pa != LVX_DEAD && pb != LVX_DEAD) s = sigma_at(v, pa, pb) * (sc[a] * sc[b]);
    Wm[a][b] = s;
    if (out) out[e] = s;
  }
}
// (W complete before the call; C complete after it)
template <int R, int W>
__device__ __forceinline__ void window_sandwich(const double (*J)[W], const double (*Wm)[W + 1], int lane, double (*T)[W], double (*C)[R]) {
  for (int e = lane; e < R * W; e += 64) {
    const int r = e / W, b = e % W;
    double s = 0.0;
    for (int a = 0; a < W; ++a) s += J[r][a] * Wm[a][b];
    T[r][b] = s;
  }
  __syncthreads();
  for (int e = lane; e < R * R; e += 64) {   // (one pass for R * R <= 64; lvx_projection_covariance has R = 12)
    const int r = e / R, s2 = e % R;
    if (r >= s2) {
      double s = 0.0;
      for (int b = 0; b < W; ++b) s += T[r][b] * J[s2][b];
      C[r][s2] = s; C[s2][r] = s;
    }
  }
  __syncthreads();
}

// lvx_trajectory_covariance.  One wavefront per query: lane 0 evaluates the pose and its 6 x 31 Jacobian (lvx_trajcov.h) into LDS; the shared pieces do the rest.
// An invalid query (outside the trajectory, a non-unit control quaternion) holds zeros and indices of -1.
struct PoseCov {
  const double* state; int N; double t0, dt; int frame, n; const double* t; SigmaView v;
  double* cov; double* sigma; double* wcov; int32_t* widx; uint8_t* valid; int* flag; int* bad;
};
__global__ __launch_bounds__(64) void k_pose_cov(PoseCov g) {
  __shared__ double J[6][TCOV_W], W[TCOV_W][TCOV_W + 1], T[6][TCOV_W], sc[TCOV_W], Cv[6][6];
  __shared__ int idx[TCOV_W], pos[TCOV_W], status;
  const int lane = threadIdx.x, i = blockIdx.x;
  if (sigma_lost(g.v)) { if (lane == 0 && i == 0) *g.bad = 1; return; }   // a lost pivot: nothing is written
  if (lane == 0) {
    const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
    SensorCal ext; ext.q = mkq(1, 0, 0, 0); ext.p = mk(0, 0, 0); ext.tau = 0.0;
    if (g.frame != LVX_FRAME_TRAJECTORY) {
      const double* ss = g.state + 7 * (size_t)g.N + (g.frame == LVX_FRAME_CAMERA ? 24 : 16);
      ext.q = load_q(ss); ext.p = load_v3(ss + 4); ext.tau = ss[7];
    }
    const int st = traj_pose_jacobian(sp, g.frame == LVX_FRAME_TRAJECTORY ? 0 : (g.frame == LVX_FRAME_LIDAR ? 1 : 2), ext, g.t[i] + ext.tau, J, idx);
    if (st == RES_NONUNIT) *g.flag = RES_NONUNIT;
    status = st;
  }
  __syncthreads();
  const size_t W2 = (size_t)TCOV_W * TCOV_W;
  if (status != RES_OK) {
    if (lane == 0) g.valid[i] = 0;
    if (lane < TCOV_W && g.widx) g.widx[(size_t)i * TCOV_W + lane] = -1;
    if (g.wcov) for (int e = lane; e < (int)W2; e += 64) g.wcov[(size_t)i * W2 + e] = 0.0;
    if (lane < 36 && g.cov) g.cov[(size_t)i * 36 + lane] = 0.0;
    if (lane < 6 && g.sigma) g.sigma[(size_t)i * 6 + lane] = 0.0;
    return;
  }
  window_scalars<TCOV_W>(g.v, idx, 0, lane, pos, sc, g.widx ? g.widx + (size_t)i * TCOV_W : nullptr);
  if (lane == 0) g.valid[i] = 1;
  __syncthreads();
  window_gather<TCOV_W>(g.v, pos, sc, lane, W, g.wcov ? g.wcov + (size_t)i * W2 : nullptr);
  __syncthreads();
  window_sandwich<6, TCOV_W>(J, W, lane, T, Cv);
  if (lane < 36 && g.cov) g.cov[(size_t)i * 36 + lane] = Cv[lane / 6][lane % 6];
  if (lane < 6 && g.sigma) g.sigma[(size_t)i * 6 + lane] = sqrt(Cv[lane][lane]);
}

// ---------------------------------------------------------------------------------------------------------
// lvx_landmark_covariance.  The landmarks were eliminated before the band (k_lm_schur): with E_l the landmark's row of DevCommon::lmH over its band window and the
// border, d_l = s_l^2 H_ll + lmd_l / radius, w_l = s_l^2 / d_l and Sigma_xx the UNSCALED covariance of the reduced system (the selected inverse above),
//   Sigma_ll = w_l + w_l^2 E_l Sigma_xx E_l^T,      Sigma_lx = -w_l E_l Sigma_xx
// Every entry of Sigma_xx that E_l or the reference pose's window touches lies on the factor's pattern: the elimination wrote E_l^T E_l into the band, so the reach of
// a landmark's row is <= bw <= TB.  Those entries are read from SigW[j][d] = Sigma(j + d, j), d <= TB, which k_band_selinv stores beside SigB when asked to: the
// query's SigmaView has SigW as its band store.  On top of the shared pieces the query adds the landmark's row (E_l Sigma_xx E_l^T and the 31 cross terms).
// ---------------------------------------------------------------------------------------------------------
struct LmQuery {
  const double* state; int N; double t0, dt; CamIntr cam; const double* lm_uv; const double* lm_t0; int L; const int* ord;
  const double* lmH; const int* p0s; int wl, nbd_ext, ls;   // lmH null: no landmark rows were formed (no reprojection block): every free landmark is unobserved
  int n; const int* ids;                                     // ids null: 0 .. n - 1
};
// the query's landmark (-1: outside [0, L) or constant under the lock mask) and the knot interval of its reference pose
__device__ __forceinline__ int lc_landmark(const LmQuery& q, int i, KnotRef* k, bool* pose) {
  const int l = q.ids ? q.ids[i] : i;
  if (l < 0 || l >= q.L || q.ord[6 * (size_t)q.N + 22 + l] != LVX_LM_BASE + l) return -1;
  const double tau = q.state[7 * (size_t)q.N + 31];
  *pose = traj_knot(q.t0, q.dt, q.N, landmark_ref_time(q.cam, tau, q.lm_uv[2 * (size_t)l + 1], q.lm_t0[l]), k);
  return l;
}
// lowest band position any query needs -> *lowest (the caller starts it at nb): the reference pose's window and, where rows reached the landmark, its first coupling
__global__ void k_lc_lowest(LmQuery q, int* lowest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  KnotRef k; bool pose = false;
  const int l = lc_landmark(q, i, &k, &pose);
  if (l < 0 || !pose) return;
  int lo = 0x7fffffff;
  for (int c = 0; c < 24; ++c) { const int o = q.ord[6 * k.i0 + c]; if (o >= 0 && o < lo) lo = o; }
  if (q.lmH && q.lmH[(size_t)l * q.ls + q.wl + q.nbd_ext] > 0.0 && q.p0s[l] < lo) lo = q.p0s[l];
  if (lo != 0x7fffffff) atomicMin(lowest, lo);
}

struct LmCov {
  LmQuery q;
  SigmaView v;                                   // the band store is SigW: the couplings of a landmark's row reach up to TB
  const double* lmd; double inv_radius;          // lmd and v.scale: SolveWork's, [band | border | landmarks]
  double* var; double* sigma; double* point; double* pcov; double* wcov; int32_t* widx; uint8_t* valid; int* flag; int* bad;
};
// One wavefront per queried landmark.  Lane 0 evaluates the map point and its 3 x 32 Jacobian (lvx_lmcov.h); the non-zeros of the landmark's row are compacted by
// ballot in index order (value times the Jacobi scale of its column, position); E Sigma E^T runs over the pairs a <= b with the lanes along b — the entries of one row
// of SigW, consecutive where the couplings are — each lane adding its terms in (a, b) order, the lanes joined by a butterfly (every lane ends with the same bits); the 31
// cross terms take a lane pair per window scalar.  Window scalar 0 is the landmark itself: dead to the shared gather, its row and column of W are written afterwards.
// Dynamic LDS: ev [ne] doubles | epos [ne] ints, ne = wl + nbd.
__global__ __launch_bounds__(64) void k_landmark_cov(LmCov g) {
  extern __shared__ double lds_e[];
  __shared__ double Jp[6][TCOV_W], J[3][LCOV_W], W[LCOV_W][LCOV_W + 1], T[3][LCOV_W], sc[LCOV_W], Cv[3][3], Pw[3];
  __shared__ int idx[LCOV_W], pos[LCOV_W], status, lm_s;
  const LmQuery& q = g.q;
  const int lane = threadIdx.x, i = blockIdx.x, ne = q.wl + g.v.nbd;
  double* ev = lds_e; int* epos = (int*)(lds_e + ne);
  if (sigma_lost(g.v)) { if (lane == 0 && i == 0) *g.bad = 1; return; }   // a lost pivot: nothing is written
  if (lane == 0) {
    KnotRef k; bool pose = false;
    const int l = lc_landmark(q, i, &k, &pose);
    int st = RES_RANGE;
    if (l >= 0 && pose) {
      const SplineRef sp{q.t0, q.dt, q.N, q.state, q.state + 3 * (size_t)q.N};
      const double* ss = q.state + 7 * (size_t)q.N + 24;
      SensorCal cam; cam.q = load_q(ss); cam.p = load_v3(ss + 4); cam.tau = ss[7];
      st = landmark_point_jacobian(sp, q.cam, cam, l, q.lm_uv[2 * (size_t)l], q.lm_uv[2 * (size_t)l + 1], q.lm_t0[l], q.state[7 * (size_t)q.N + 32 + l], Jp, J, idx, Pw);
      if (st == RES_NONUNIT) *g.flag = RES_NONUNIT;
    }
    status = st; lm_s = l;
  }
  __syncthreads();
  const size_t W2 = (size_t)LCOV_W * LCOV_W;
  if (status != RES_OK) {   // constant under the lock mask, or no reference pose: zeros
    if (lane == 0) { g.valid[i] = 0; if (g.var) g.var[i] = 0.0; if (g.sigma) g.sigma[i] = 0.0; }
    if (lane < 3 && g.point) g.point[(size_t)i * 3 + lane] = 0.0;
    if (lane < 9 && g.pcov) g.pcov[(size_t)i * 9 + lane] = 0.0;
    if (lane < LCOV_W && g.widx) g.widx[(size_t)i * LCOV_W + lane] = -1;
    if (g.wcov) for (int e = lane; e < (int)W2; e += 64) g.wcov[(size_t)i * W2 + e] = 0.0;
    return;
  }
  const int l = lm_s;
  window_scalars<LCOV_W>(g.v, idx, 1, lane, pos, sc, g.widx ? g.widx + (size_t)i * LCOV_W : nullptr);
  if (lane == 0) { pos[0] = LVX_DEAD; sc[0] = 0.0; if (g.widx) g.widx[(size_t)i * LCOV_W] = idx[0]; }
  // the landmark's row: non-zeros in index order
  const double* row = q.lmH ? q.lmH + (size_t)l * q.ls : nullptr;
  const double Hll = row ? row[q.wl + q.nbd_ext] : 0.0;
  int nn = 0;
  if (Hll > 0.0) {   // (k_lm_schur's test: a landmark no row reached was not eliminated, and its row is zero)
    const int p0 = q.p0s[l];
    for (int k0 = 0; k0 < ne; k0 += 64) {
      const int k = k0 + lane;
      double e = 0.0; int p = 0;
      if (k < ne) { p = k < q.wl ? p0 + k : -1 - (k - q.wl); if (k >= q.wl || p < g.v.nb) e = row[k]; }
      const bool nz = e != 0.0;
      const unsigned long long mask = __ballot(nz);
      if (nz) { const int at = nn + __popcll(mask & ((1ull << lane) - 1ull)); ev[at] = e * scale_at(g.v, p); epos[at] = p; }
      nn += __popcll(mask);
    }
  }
  __syncthreads();
  double acc = 0.0;
  for (int a = 0; a < nn; ++a) {
    const int pa = epos[a]; const double ea = ev[a];
    for (int b = a + lane; b < nn; b += 64) { const double t = ea * ev[b] * sigma_at(g.v, pa, epos[b]); acc += b == a ? t : 2.0 * t; }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  const int m = lane & 31, pm = pos[m];
  double cm = 0.0;
  if (pm != LVX_DEAD) for (int a = lane >> 5; a < nn; a += 2) cm += ev[a] * sigma_at(g.v, epos[a], pm);
  cm += __shfl_xor(cm, 32);
  double s = 1.0, dmp = 1e-6;   // no landmark rows: the solver holds no diagonal for the landmarks; an unobserved one has scale 1 and the floor of the damping
  if (row) { s = g.v.scale[g.v.nb + g.v.nbd + l]; dmp = g.lmd[g.v.nb + g.v.nbd + l]; }
  const double w = s * s / (s * s * Hll + dmp * g.inv_radius);
  window_gather<LCOV_W>(g.v, pos, sc, lane, W, nullptr);
  __syncthreads();
  if (lane == 0) W[0][0] = w + w * w * acc;
  else if (lane < LCOV_W) { const double v = pm != LVX_DEAD ? -w * cm * sc[lane] : 0.0; W[0][lane] = v; W[lane][0] = v; }
  __syncthreads();
  if (g.wcov) for (int e = lane; e < (int)W2; e += 64) g.wcov[(size_t)i * W2 + e] = W[e / LCOV_W][e % LCOV_W];
  window_sandwich<3, LCOV_W>(J, W, lane, T, Cv);
  if (lane < 9 && g.pcov) g.pcov[(size_t)i * 9 + lane] = Cv[lane / 3][lane % 3];
  if (lane < 3 && g.point) g.point[(size_t)i * 3 + lane] = Pw[lane];
  if (lane == 0) { g.valid[i] = 1; if (g.var) g.var[i] = W[0][0]; if (g.sigma) g.sigma[i] = sqrt(W[0][0]); }
}

// ---------------------------------------------------------------------------------------------------------
// lvx_map_point_covariance (lvx_ptcov.h has the algebra).  A map is 1e5 .. 1e6 points per call, so a LANE owns a point here, not a wavefront.
//   k_pt_hub     once per call, one wavefront: the pose Jacobian J0 at t_map + tau_L, its window W00 (hub knots and the LiDAR's scalars: border x border) and
//                C00 = J0 W00 J0^T, by the shared pieces.  It also decides what makes the whole call fail: a lost pivot (status 1), a scalar of the t_map
//                window that is a BAND position — its cross terms with a point's knots would be off the factor's pattern (status 2).
//   k_point_cov  256 points per workgroup.  Every lane evaluates its own pose Jacobian and Gk = A_k Jk (3 x 31, registers).  The windows depend on the knot interval
//                only: the workgroup walks the DISTINCT intervals of its points in ascending order (an integer minimum in LDS — times may arrive in any order), stages
//                Wkk (32 x 32 padded), Wk0 and B0 = Wk0 J0^T (32 x 16 padded) once per interval, and the lanes of that interval take their turn: per wavefront and
//                group of 16 lanes, T = Gk [Wkk | B0] is 3 row tiles x 3 column tiles x 8 steps of v_mfma_f64_16x16x4_f64 (tile row = point, one tile per row of
//                Gk), staged through a 16-point tile in LDS that first holds Gk and then T; pt_cov_assemble finishes in registers.
// A point's bits depend on its own inputs and on its interval's windows only — every sum has a fixed order and an MFMA row never sees another row — so they are the
// same alone, in any batch and at any position.  No atomics on floating-point data.  512 registers (one wavefront per SIMD); the compiler spills 718 of them to
// scratch (780 bytes per lane) around the pose evaluation in front of the loop.
// ---------------------------------------------------------------------------------------------------------
#define PC_NT 256
#define PC_TS 115        // doubles per point of a wavefront's tile: Gk as [3][32] (96), then T as [3][PCOV_TW] (114); odd, so 16 points spread over the banks
struct PtHub {   // what k_pt_hub leaves for k_point_cov
  double J0[6][32];                 // column 31 zero
  double W00[TCOV_W][TCOV_W];
  double C00[36], q0[4], p0[3], sc[TCOV_W];
  int pos[TCOV_W], idx[TCOV_W];     // ord[] of the window's scalars; their tangent indices, -1 constant
  int status;                       // 0 ok, 1 a lost pivot, 2 the window of t_map is off the border, 3 a non-unit control quaternion at t_map (every point is invalid)
};
struct PtCov {
  const double* state; int N; double t0, dt, t_map; int n;
  const double* pt; const float* xyzi; const double* t; const double* dir;   // pt [n][3] or xyzi [n][4] (the scan buffers' layout)
  SigmaView v; PtHub* hub;
  double* point; double* cov; double* sigma; double* sigma_max; double* var_dir; double* wcov; int32_t* widx; uint8_t* valid; int* flag; int* bad;
};
__device__ __forceinline__ SensorCal pc_lidar(const PtCov& g) {
  const double* ss = g.state + 7 * (size_t)g.N + 16;
  SensorCal ext; ext.q = load_q(ss); ext.p = load_v3(ss + 4); ext.tau = ss[7];
  return ext;
}
// The pose window of ONE query — the LiDAR frame at t_map — as k_pose_cov forms it, stored to PtHub; what is its own are the status decisions.
__global__ __launch_bounds__(64) void k_pt_hub(PtCov g) {
  __shared__ double J[6][TCOV_W], W[TCOV_W][TCOV_W + 1], T[6][TCOV_W], sc[TCOV_W], Cv[6][6];
  __shared__ int idx[TCOV_W], pos[TCOV_W], status;
  const int lane = threadIdx.x;
  PtHub* h = g.hub;
  if (sigma_lost(g.v)) { if (lane == 0) { h->status = 1; *g.bad = 1; } return; }   // a lost pivot: nothing is written
  if (lane == 0) {
    const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
    const SensorCal ext = pc_lidar(g);
    int st = traj_pose_jacobian(sp, 1, ext, g.t_map + ext.tau, J, idx);
    quat q0; v3 p0;
    if (st == RES_OK && pt_lidar_pose(sp, ext, g.t_map + ext.tau, &q0, &p0) != RES_OK) st = RES_NONUNIT;
    if (st == RES_OK) { h->q0[0] = q0.x; h->q0[1] = q0.y; h->q0[2] = q0.z; h->q0[3] = q0.w; h->p0[0] = p0.x; h->p0[1] = p0.y; h->p0[2] = p0.z; }
    status = st;
  }
  __syncthreads();
  if (status == RES_RANGE) { if (lane == 0) { h->status = 2; *g.bad = 2; } return; }   // t_map + tau_L has left the trajectory
  if (status == RES_NONUNIT) { if (lane == 0) { h->status = 3; *g.flag = RES_NONUNIT; } return; }
  window_scalars<TCOV_W>(g.v, idx, 0, lane, pos, sc, h->idx);
  if (lane < TCOV_W) { h->pos[lane] = pos[lane]; h->sc[lane] = sc[lane]; }
  if (__any(lane < 24 && pos[lane] != LVX_DEAD && pos[lane] >= 0)) { if (lane == 0) { h->status = 2; *g.bad = 2; } return; }   // a free knot scalar of the t_map window in the band
  __syncthreads();
  window_gather<TCOV_W>(g.v, pos, sc, lane, W, &h->W00[0][0]);
  for (int e = lane; e < 6 * 32; e += 64) h->J0[e >> 5][e & 31] = (e & 31) < TCOV_W ? J[e >> 5][e & 31] : 0.0;
  __syncthreads();
  window_sandwich<6, TCOV_W>(J, W, lane, T, Cv);
  if (lane < 36) h->C00[lane] = Cv[lane / 6][lane % 6];
  if (lane == 0) h->status = 0;
}

// the 55 x 55 window and its indices of one point (tests and small n): k-window column a stands at a (a < 24) or 24 + a, 0-window column b at 24 + b
__device__ __forceinline__ void pc_write_window(const PtCov& g, size_t i, const double (*Wkk)[33], const double (*Wk0)[32], const PtHub* h, const int* idxk, const int* idx0) {
  if (g.widx) for (int c = 0; c < PCOV_W; ++c) g.widx[i * PCOV_W + c] = (c >= 24 && c < 48) ? idx0[c - 24] : idxk[c < 24 ? c : c - 24];
  if (!g.wcov) return;
  const size_t W2 = (size_t)PCOV_W * PCOV_W;
  for (int e = 0; e < (int)W2; ++e) {
    const int A = e / PCOV_W, B = e % PCOV_W;
    const bool Ak = A < 24 || A >= 48, Bk = B < 24 || B >= 48;
    double v;
    if (Ak && Bk) v = Wkk[A < 24 ? A : A - 24][B < 24 ? B : B - 24];
    else if (Ak) v = Wk0[A < 24 ? A : A - 24][B - 24];
    else if (Bk) v = Wk0[B < 24 ? B : B - 24][A - 24];
    else v = h->W00[A - 24][B - 24];
    g.wcov[i * W2 + e] = v;
  }
}
// MFMA = false (switch PTCOV_VALU): the plain formulation for comparison — every lane multiplies its own Gk against the staged window, read from LDS as a broadcast
template <bool MFMA>
__global__ __launch_bounds__(PC_NT) void k_point_cov(PtCov g) {
  extern __shared__ double pc_tiles[];   // [PC_NT / 64][16][PC_TS]
  __shared__ double Wkk[32][33], Bk[32][17], Wk0[TCOV_W][32], J0s[6][32], C00s[36], sck[32], sc0[32];
  __shared__ int posk[32], idxk[32], pos0[32], idx0[32], s_key;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fk = lane >> 4;
  const size_t i = (size_t)blockIdx.x * PC_NT + tid;
  const PtHub* h = g.hub;
  const int hs = h->status;
  if (hs == 1 || hs == 2) return;   // the call fails as a whole: nothing is written
  const bool in = i < (size_t)g.n;
  for (int e = tid; e < 6 * 32; e += PC_NT) J0s[e >> 5][e & 31] = h->J0[e >> 5][e & 31];
  if (tid < 36) C00s[tid] = h->C00[tid];
  if (tid < 32) { const bool w = tid < TCOV_W; pos0[tid] = w ? h->pos[tid] : LVX_DEAD; idx0[tid] = w ? h->idx[tid] : -1; sc0[tid] = w ? h->sc[tid] : 0.0; }
  // the lane's point: geometry and Gk = A_k Jk
  v3 pL = mk(0, 0, 0), vv = mk(0, 0, 0), pm = mk(0, 0, 0);
  double tk = 0.0;
  if (in) {
    if (g.xyzi) { const float4 f = ((const float4*)g.xyzi)[i]; pL = mk((double)f.x, (double)f.y, (double)f.z); }
    else pL = load_v3(g.pt + 3 * i);
    tk = g.t[i];
  }
  const quat q0 = mkq(h->q0[3], h->q0[0], h->q0[1], h->q0[2]);
  const v3 p0 = mk(h->p0[0], h->p0[1], h->p0[2]);
  int key = -1;
  double Gk[3][TCOV_W];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < TCOV_W; ++c) Gk[r][c] = 0.0;
  if (in && hs == 0 && isfinite(pL.x) && isfinite(pL.y) && isfinite(pL.z)) {
    const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
    const SensorCal ext = pc_lidar(g);
    KnotRef kr;
    if (traj_knot(g.t0, g.dt, g.N, tk + ext.tau, &kr)) {
      double Jk[6][TCOV_W]; int ik[TCOV_W];
      int st = traj_pose_jacobian(sp, 1, ext, tk + ext.tau, Jk, ik);
      quat qk; v3 pk;
      if (st == RES_OK && pt_lidar_pose(sp, ext, tk + ext.tau, &qk, &pk) != RES_OK) st = RES_NONUNIT;
      if (st == RES_OK) {
        v3 r;
        pt_chain(qk, pk, q0, p0, pL, &r, &vv, &pm);
        pt_lever(Jk, r, Gk);
        key = kr.i0;
      } else if (st == RES_NONUNIT) *g.flag = RES_NONUNIT;
    }
  }
  const bool valid = key >= 0;
  double cov[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) cov[e] = 0.0;
  double* tile = pc_tiles + (size_t)wave * 16 * PC_TS;
  const size_t W2 = (size_t)PCOV_W * PCOV_W;
  for (;;) {
    __syncthreads();
    if (tid == 0) s_key = 0x7fffffff;
    __syncthreads();
    if (key >= 0) atomicMin(&s_key, key);
    __syncthreads();
    const int cur = s_key;
    if (cur == 0x7fffffff) break;
    // the interval's windows, once for the workgroup
    if (tid < 32) {
      int o = LVX_DEAD, id = -1;
      if (tid < TCOV_W) { const int gi = tid < 24 ? 6 * cur + tid : 6 * g.N + 8 + (tid - 24); o = g.v.ord[gi]; if (o != LVX_DEAD) id = gi; }
      posk[tid] = o; idxk[tid] = id; sck[tid] = scale_at(g.v, o);
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += PC_NT) {
      const int a = e >> 5, b = e & 31;
      const int pa = posk[a];
      double vk = 0.0, v0 = 0.0;
      if (pa != LVX_DEAD) {
        const int pb = posk[b], qb = pos0[b];
        if (pb != LVX_DEAD) { vk = sigma_at(g.v, pa, pb); vk *= sck[a] * sck[b]; }
        if (qb != LVX_DEAD) { v0 = sigma_at(g.v, pa, qb); v0 *= sck[a] * sc0[b]; }
      }
      Wkk[a][b] = vk;
      if (a < TCOV_W) Wk0[a][b] = v0;
    }
    __syncthreads();
    for (int e = tid; e < 32 * 16; e += PC_NT) {
      const int a = e >> 4, m = e & 15;
      double s = 0.0;
      if (a < TCOV_W && m < 6) for (int b = 0; b < TCOV_W; ++b) s += Wk0[a][b] * J0s[m][b];
      Bk[a][m] = s;
    }
    __syncthreads();
    const bool mine = key == cur;
    const unsigned long long act = __ballot(mine);
    if (!MFMA) {
      if (mine) {
        double Tl[3 * PCOV_TW];
#pragma unroll
        for (int b = 0; b < PCOV_TW; ++b) {
          double t0 = 0.0, t1 = 0.0, t2 = 0.0;
          if (b != 31) {
#pragma unroll
            for (int a = 0; a < TCOV_W; ++a) { const double w = b < 31 ? Wkk[a][b] : Bk[a][b - 32]; t0 += Gk[0][a] * w; t1 += Gk[1][a] * w; t2 += Gk[2][a] * w; }
          }
          Tl[b] = t0; Tl[PCOV_TW + b] = t1; Tl[2 * PCOV_TW + b] = t2;
        }
        pt_cov_assemble(Gk, Tl, PCOV_TW, C00s, vv, rotmat(q0), cov);
        pc_write_window(g, i, Wkk, Wk0, h, idxk, idx0);
      }
    } else
    for (int grp = 0; grp < 4; ++grp) {
      const bool any = ((act >> (16 * grp)) & 0xffffull) != 0;   // uniform over the wavefront; the barriers below are reached by every wavefront all the same
      if (any && fk == grp) {
        double* Gp = tile + fi * PC_TS;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < TCOV_W; ++c) Gp[32 * r + c] = mine ? Gk[r][c] : 0.0;
          Gp[32 * r + 31] = 0.0;
        }
      }
      __syncthreads();
      d4c acc[3][3];
      if (any) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int nt = 0; nt < 3; ++nt) acc[r][nt] = d4c{0.0, 0.0, 0.0, 0.0};
        // A[i = fi][k = fk] = Gk of point fi, B[k = fk][j = fi] = the window's row 4 s + fk
        for (int s = 0; s < 8; ++s) {
          const int k = 4 * s + fk;
          const double b0 = Wkk[k][fi], b1 = Wkk[k][16 + fi], b2 = Bk[k][fi];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double a = tile[fi * PC_TS + 32 * r + k];
            acc[r][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[r][0], 0, 0, 0);
            acc[r][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[r][1], 0, 0, 0);
            acc[r][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, acc[r][2], 0, 0, 0);
          }
        }
      }
      __syncthreads();   // every read of Gk is done: the tile now takes T (C/D: column = lane & 15, row = (lane >> 4) + 4 v)
      if (any) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int nt = 0; nt < 3; ++nt) {
            const int col = 16 * nt + fi;
            if (col < PCOV_TW) {
#pragma unroll
              for (int v = 0; v < 4; ++v) tile[(fk + 4 * v) * PC_TS + PCOV_TW * r + col] = acc[r][nt][v];
            }
          }
      }
      __syncthreads();
      if (mine && fk == grp) {
        pt_cov_assemble(Gk, tile + fi * PC_TS, PCOV_TW, C00s, vv, rotmat(q0), cov);
        pc_write_window(g, i, Wkk, Wk0, h, idxk, idx0);
      }
      __syncthreads();
    }
    if (mine) key = -1;
  }
  if (!in) return;
  g.valid[i] = valid ? 1 : 0;
  if (g.point) { g.point[3 * i] = pm.x; g.point[3 * i + 1] = pm.y; g.point[3 * i + 2] = pm.z; }
  if (g.cov) for (int e = 0; e < 9; ++e) g.cov[9 * i + e] = cov[e];
  // (a point measured at t_map itself does not move at all: the four terms cancel to rounding, a diagonal entry of -1e-21 counts as zero)
  if (g.sigma) { g.sigma[3 * i] = sqrt(cov[0] < 0.0 ? 0.0 : cov[0]); g.sigma[3 * i + 1] = sqrt(cov[4] < 0.0 ? 0.0 : cov[4]); g.sigma[3 * i + 2] = sqrt(cov[8] < 0.0 ? 0.0 : cov[8]); }
  if (g.sigma_max) g.sigma_max[i] = valid ? pt_sigma_max(cov) : 0.0;
  if (g.var_dir && g.dir) g.var_dir[i] = valid ? pt_var_dir(cov, load_v3(g.dir + 3 * i)) : 0.0;
  if (!valid) {
    if (g.widx) for (int c = 0; c < PCOV_W; ++c) g.widx[i * PCOV_W + c] = -1;
    if (g.wcov) for (int e = 0; e < (int)W2; ++e) g.wcov[i * W2 + e] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------
// lvx_projection_covariance (lvx_projcov.h has the algebra): the pixel covariance of map points in the images.  Three launches behind the selected inverse:
//   k_proj_poses  (lvx_render.hip) the table's poses: the camera pose of every image and the LiDAR pose at t_map, by the functions and in the translation unit of
//                 k_render_poses — the same bits, so that the decisions below are lvx_render_map_d's.
//   k_proj_hub    here: one wavefront per image.  Lane 0 evaluates the two 6 x 31 pose Jacobians (camera frame at image_t + tau_C, LiDAR frame at t_map + tau_L); the
//                 shared pieces gather the 62 x 62 window — the image's band window, band x border (the knots at t_map are hub slots) and border x border — and
//                 form pose_cov = J12 W J12^T (12 x 12, J12 block-diagonal).  It makes k_pt_hub's status decisions (every workgroup reaches the same ones; the
//                 first writes them) and leaves validity and the 78 unique entries of pose_cov in the image's record.
//   k_proj_cov    (lvx_render.hip, built without FP contraction as k_render_map is: uv and the depth / bounds tests round as there) a lane per point.
// ---------------------------------------------------------------------------------------------------------
struct ProjHub {
  const double* state; int N; double t0, dt, t_map; int n_images; const double* image_t; SigmaView v; ProjTable* tab;
  double* pose_cov; double* wcov; int32_t* widx; int32_t* valid; int* flag; int* bad;
};
__global__ __launch_bounds__(64) void k_proj_hub(ProjHub g) {
  __shared__ double JC[6][TCOV_W], JL[6][TCOV_W], J[12][PJ_W], W[PJ_W][PJ_W + 1], T[12][PJ_W], sc[PJ_W], Cv[12][12];
  __shared__ int idxc[TCOV_W], idxl[TCOV_W], idx[PJ_W], pos[PJ_W], st_map, st_cam;
  const int lane = threadIdx.x, i = blockIdx.x;
  ProjTable* tab = g.tab;
  if (sigma_lost(g.v)) { if (lane == 0 && i == 0) { tab->status = 1; *g.bad = 1; } return; }   // a lost pivot: nothing is written
  if (lane == 0) {
    const SplineRef sp{g.t0, g.dt, g.N, g.state, g.state + 3 * (size_t)g.N};
    const double* ss = g.state + 7 * (size_t)g.N + 16;
    SensorCal lid, cam;
    lid.q = load_q(ss); lid.p = load_v3(ss + 4); lid.tau = ss[7];
    cam.q = load_q(ss + 8); cam.p = load_v3(ss + 12); cam.tau = ss[15];
    int sm = traj_pose_jacobian(sp, 1, lid, g.t_map + lid.tau, JL, idxl);
    if (sm == RES_OK && !tab->map_valid) sm = RES_NONUNIT;   // (k_proj_poses' verdict on the same pose)
    st_map = sm;
    int sk = RES_RANGE;
    if (sm == RES_OK) {
      sk = traj_pose_jacobian(sp, 2, cam, g.image_t[i] + cam.tau, JC, idxc);
      if (sk == RES_NONUNIT) *g.flag = RES_NONUNIT;
      if (sk == RES_OK && !tab->img[i].valid) sk = RES_RANGE;
    }
    st_cam = sk;
  }
  __syncthreads();
  if (st_map == RES_RANGE) { if (lane == 0 && i == 0) { tab->status = 2; *g.bad = 2; } return; }   // t_map + tau_L has left the trajectory
  const size_t W2 = (size_t)PJ_W * PJ_W;
  bool ok = st_map == RES_OK && st_cam == RES_OK;
  if (st_map == RES_OK) {
    // the LiDAR half of the window decides the call: a free knot scalar of the t_map window in the band is off the factor's pattern
    if (lane < TCOV_W) idx[31 + lane] = idxl[lane];
    if (lane < TCOV_W) idx[lane] = ok ? idxc[lane] : -1;
    __syncthreads();
    window_scalars<PJ_W>(g.v, idx, 0, lane, pos, sc, nullptr);
    __syncthreads();
    if (__any(lane >= 31 && lane < 55 && pos[lane] != LVX_DEAD && pos[lane] >= 0)) { if (lane == 0 && i == 0) { tab->status = 2; *g.bad = 2; } return; }
  } else if (lane == 0 && i == 0) *g.flag = RES_NONUNIT;   // a non-unit control quaternion at t_map: every image is invalid, every point skipped
  if (lane == 0 && i == 0) tab->status = st_map == RES_OK ? 0 : 3;
  if (!ok) {   // image_t outside the spline (not an error), or a non-unit quaternion: zeros, indices -1
    if (lane == 0) { g.valid[i] = 0; tab->img[i].valid = 0; }
    if (lane < PJ_W && g.widx) g.widx[(size_t)i * PJ_W + lane] = -1;
    if (g.wcov) for (int e = lane; e < (int)W2; e += 64) g.wcov[(size_t)i * W2 + e] = 0.0;
    if (g.pose_cov) for (int e = lane; e < 144; e += 64) g.pose_cov[(size_t)i * 144 + e] = 0.0;
    return;
  }
  if (lane < PJ_W && g.widx) g.widx[(size_t)i * PJ_W + lane] = pos[lane] != LVX_DEAD ? idx[lane] : -1;
  for (int e = lane; e < 12 * PJ_W; e += 64) {
    const int r = e / PJ_W, c = e % PJ_W;
    J[r][c] = (r < 6 && c < 31) ? JC[r][c] : ((r >= 6 && c >= 31) ? JL[r - 6][c - 31] : 0.0);
  }
  window_gather<PJ_W>(g.v, pos, sc, lane, W, g.wcov ? g.wcov + (size_t)i * W2 : nullptr);
  __syncthreads();
  window_sandwich<12, PJ_W>(J, W, lane, T, Cv);
  if (g.pose_cov) for (int e = lane; e < 144; e += 64) g.pose_cov[(size_t)i * 144 + e] = Cv[e / 12][e % 12];
  for (int e = lane; e < 144; e += 64) { const int r = e / 12, c = e % 12; if (r >= c) tab->img[i].pc[r * (r + 1) / 2 + c] = Cv[r][c]; }
  if (lane == 0) g.valid[i] = 1;
}

}  // namespace lvx
