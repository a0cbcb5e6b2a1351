// lvx_selinv.h — selected inverse of the damped LM system from its sequential factor, and what is read from it: pose covariances (lvx_trajectory_covariance) and
// landmark covariances (lvx_landmark_covariance, at the end of the file).
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

// One wavefront per query: lane 0 evaluates the pose and its Jacobian (lvx_trajcov.h) into LDS, the 31 scalars go through ord[] (>= 0 a band position, < 0 border
// slot -1 - o, LVX_DEAD constant), the window of Sigma is gathered and unscaled, cov = J W J^T with every sum in index order (lower triangle computed, mirrored).
struct PoseCov {
  const double* state; int N; double t0, dt; int frame, n; const double* t; const int* ord;
  const double* SigB; const double* Z; int ldz, nb, nbd; const double* Scc; const double* scale;
  const int* info; int force_bad;
  double* cov; double* sigma; double* wcov; int32_t* widx; uint8_t* valid; int* flag; int* bad;
};
__global__ __launch_bounds__(64) void k_pose_cov(PoseCov g) {
  __shared__ double J[6][TCOV_W], W[TCOV_W][TCOV_W + 1], T[6][TCOV_W], sc[TCOV_W], Cv[6][6];
  __shared__ int idx[TCOV_W], pos[TCOV_W], status;
  const int lane = threadIdx.x, i = blockIdx.x;
  if (g.force_bad || g.info[0] != 0 || g.info[1] != 0) { if (lane == 0 && i == 0) *g.bad = 1; return; }   // a lost pivot: nothing is written
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
  const bool ok = status == RES_OK;
  if (lane < TCOV_W) {
    int o = LVX_DEAD, id = -1;
    if (ok && idx[lane] >= 0) { o = g.ord[idx[lane]]; if (o != LVX_DEAD) id = idx[lane]; }
    pos[lane] = o;
    sc[lane] = o == LVX_DEAD ? 0.0 : g.scale[o >= 0 ? o : g.nb + (-1 - o)];
    if (g.widx) g.widx[(size_t)i * TCOV_W + lane] = id;
  }
  if (lane == 0) g.valid[i] = ok ? 1 : 0;
  __syncthreads();
  for (int e = lane; e < TCOV_W * TCOV_W; e += 64) {
    const int a = e / TCOV_W, b = e % TCOV_W;
    const int pa = pos[a], pb = pos[b];
    double v = 0.0;
    if (pa != LVX_DEAD && pb != LVX_DEAD) {
      if (pa >= 0 && pb >= 0) { const int lo = min(pa, pb), d = max(pa, pb) - lo; v = d < SI_BD ? g.SigB[(size_t)lo * SI_BD + d] : 0.0; }
      else if (pa >= 0) v = g.Z[(size_t)(-1 - pb) * g.ldz + pa];
      else if (pb >= 0) v = g.Z[(size_t)(-1 - pa) * g.ldz + pb];
      else { const int ra = -1 - pa, rb = -1 - pb; v = g.Scc[(size_t)max(ra, rb) * g.nbd + min(ra, rb)]; }
      v *= sc[a] * sc[b];
    }
    W[a][b] = v;
    if (g.wcov) g.wcov[(size_t)i * TCOV_W * TCOV_W + e] = v;
  }
  __syncthreads();
  for (int e = lane; e < 6 * TCOV_W; e += 64) {
    const int r = e / TCOV_W, b = e % TCOV_W;
    double s = 0.0;
    if (ok) for (int a = 0; a < TCOV_W; ++a) s += J[r][a] * W[a][b];
    T[r][b] = s;
  }
  __syncthreads();
  if (lane < 36) {
    const int r = lane / 6, s2 = lane % 6;
    if (r >= s2) {
      double s = 0.0;
      if (ok) for (int b = 0; b < TCOV_W; ++b) s += T[r][b] * J[s2][b];
      Cv[r][s2] = s; Cv[s2][r] = s;
    }
  }
  __syncthreads();
  if (lane < 36 && g.cov) g.cov[(size_t)i * 36 + lane] = Cv[lane / 6][lane % 6];
  if (lane < 6 && g.sigma) g.sigma[(size_t)i * 6 + lane] = sqrt(Cv[lane][lane]);
}

// ---------------------------------------------------------------------------------------------------------
// lvx_landmark_covariance.  The landmarks were eliminated before the band (k_lm_schur): with E_l the landmark's row of DevCommon::lmH over its band window and the
// border, d_l = s_l^2 H_ll + lmd_l / radius, w_l = s_l^2 / d_l and Sigma_xx the UNSCALED covariance of the reduced system (the selected inverse above),
//   Sigma_ll = w_l + w_l^2 E_l Sigma_xx E_l^T,      Sigma_lx = -w_l E_l Sigma_xx
// Every entry of Sigma_xx that E_l or the reference pose's window touches lies on the factor's pattern: the elimination wrote E_l^T E_l into the band, so the reach of
// a landmark's row is <= bw <= TB.  Those entries are read from SigW[j][d] = Sigma(j + d, j), d <= TB, which k_band_selinv stores beside SigB when asked to.
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
  const double* SigW; int TB; const double* Z; int ldz, nb, nbd; const double* Scc;
  const double* scale; const double* lmd; double inv_radius;   // scale / lmd: SolveWork's, [band | border | landmarks]
  const int* info; int force_bad;
  double* var; double* sigma; double* point; double* pcov; double* wcov; int32_t* widx; uint8_t* valid; int* flag; int* bad;
};
// Sigma' (scaled) between two positions: >= 0 a band position, < 0 border slot -1 - o
__device__ __forceinline__ double lc_sigma(const LmCov& g, int pa, int pb) {
  if (pa >= 0 && pb >= 0) { const int lo = min(pa, pb), d = max(pa, pb) - lo; return d <= g.TB ? g.SigW[(size_t)lo * (g.TB + 1) + d] : 0.0; }
  if (pa >= 0) return g.Z[(size_t)(-1 - pb) * g.ldz + pa];
  if (pb >= 0) return g.Z[(size_t)(-1 - pa) * g.ldz + pb];
  const int ra = -1 - pa, rb = -1 - pb;
  return g.Scc[(size_t)max(ra, rb) * g.nbd + min(ra, rb)];
}
// One wavefront per queried landmark.  Lane 0 evaluates the map point and its 3 x 32 Jacobian (lvx_lmcov.h); the non-zeros of the landmark's row are compacted by
// ballot in index order (value times the Jacobi scale of its column, position); E Sigma E^T runs over the pairs a <= b with the lanes along b — the entries of one row
// of SigW, consecutive where the couplings are — each lane adding its terms in (a, b) order, the lanes joined by a butterfly (every lane ends with the same bits); the 31
// cross terms take a lane pair per window scalar.  The window, J W J^T and the stores follow k_pose_cov.  Dynamic LDS: ev [ne] doubles | epos [ne] ints, ne = wl + nbd.
__global__ __launch_bounds__(64) void k_landmark_cov(LmCov g) {
  extern __shared__ double lds_e[];
  __shared__ double Jp[6][TCOV_W], J[3][LCOV_W], W[LCOV_W][LCOV_W + 1], T[3][LCOV_W], sc[LCOV_W], Cv[3][3], Pw[3];
  __shared__ int idx[LCOV_W], pos[LCOV_W], status, lm_s;
  const LmQuery& q = g.q;
  const int lane = threadIdx.x, i = blockIdx.x, ne = q.wl + g.nbd;
  double* ev = lds_e; int* epos = (int*)(lds_e + ne);
  if (g.force_bad || g.info[0] != 0 || g.info[1] != 0) { if (lane == 0 && i == 0) *g.bad = 1; return; }   // a lost pivot: nothing is written
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
  if (lane < LCOV_W) {
    int o = LVX_DEAD, id = -1;
    if (lane == 0) { o = LVX_LM_BASE; id = idx[0]; }
    else if (idx[lane] >= 0) { o = q.ord[idx[lane]]; if (o != LVX_DEAD) id = idx[lane]; }
    pos[lane] = o;
    sc[lane] = (lane == 0 || o == LVX_DEAD) ? 0.0 : g.scale[o >= 0 ? o : g.nb + (-1 - o)];
    if (g.widx) g.widx[(size_t)i * LCOV_W + lane] = id;
  }
  // the landmark's row: non-zeros in index order
  const double* row = q.lmH ? q.lmH + (size_t)l * q.ls : nullptr;
  const double Hll = row ? row[q.wl + q.nbd_ext] : 0.0;
  int nn = 0;
  if (Hll > 0.0) {   // (k_lm_schur's test: a landmark no row reached was not eliminated, and its row is zero)
    const int p0 = q.p0s[l];
    for (int k0 = 0; k0 < ne; k0 += 64) {
      const int k = k0 + lane;
      double e = 0.0; int p = 0;
      if (k < ne) { p = k < q.wl ? p0 + k : -1 - (k - q.wl); if (k >= q.wl || p < g.nb) e = row[k]; }
      const bool nz = e != 0.0;
      const unsigned long long mask = __ballot(nz);
      if (nz) { const int at = nn + __popcll(mask & ((1ull << lane) - 1ull)); ev[at] = e * g.scale[p >= 0 ? p : g.nb + (-1 - p)]; epos[at] = p; }
      nn += __popcll(mask);
    }
  }
  __syncthreads();
  double acc = 0.0;
  for (int a = 0; a < nn; ++a) {
    const int pa = epos[a]; const double ea = ev[a];
    for (int b = a + lane; b < nn; b += 64) { const double t = ea * ev[b] * lc_sigma(g, pa, epos[b]); acc += b == a ? t : 2.0 * t; }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  const int m = lane & 31, pm = pos[m];
  double cm = 0.0;
  if (m > 0 && pm != LVX_DEAD) for (int a = lane >> 5; a < nn; a += 2) cm += ev[a] * lc_sigma(g, epos[a], pm);
  cm += __shfl_xor(cm, 32);
  double s = 1.0, dmp = 1e-6;   // no landmark rows: the solver holds no diagonal for the landmarks; an unobserved one has scale 1 and the floor of the damping
  if (row) { s = g.scale[g.nb + g.nbd + l]; dmp = g.lmd[g.nb + g.nbd + l]; }
  const double w = s * s / (s * s * Hll + dmp * g.inv_radius);
  for (int e = lane; e < (int)W2; e += 64) {
    const int a = e / LCOV_W, b = e % LCOV_W;
    double v = 0.0;
    if (a > 0 && b > 0) { const int pa = pos[a], pb = pos[b]; if (pa != LVX_DEAD && pb != LVX_DEAD) v = lc_sigma(g, pa, pb) * (sc[a] * sc[b]); }
    W[a][b] = v;
  }
  __syncthreads();
  if (lane == 0) W[0][0] = w + w * w * acc;
  else if (lane < LCOV_W) { const double v = pm != LVX_DEAD ? -w * cm * sc[lane] : 0.0; W[0][lane] = v; W[lane][0] = v; }
  __syncthreads();
  if (g.wcov) for (int e = lane; e < (int)W2; e += 64) g.wcov[(size_t)i * W2 + e] = W[e / LCOV_W][e % LCOV_W];
  for (int e = lane; e < 3 * LCOV_W; e += 64) {
    const int r = e / LCOV_W, b = e % LCOV_W;
    double t = 0.0;
    for (int a = 0; a < LCOV_W; ++a) t += J[r][a] * W[a][b];
    T[r][b] = t;
  }
  __syncthreads();
  if (lane < 9) {
    const int r = lane / 3, s2 = lane % 3;
    if (r >= s2) {
      double t = 0.0;
      for (int b = 0; b < LCOV_W; ++b) t += T[r][b] * J[s2][b];
      Cv[r][s2] = t; Cv[s2][r] = t;
    }
  }
  __syncthreads();
  if (lane < 9 && g.pcov) g.pcov[(size_t)i * 9 + lane] = Cv[lane / 3][lane % 3];
  if (lane < 3 && g.point) g.point[(size_t)i * 3 + lane] = Pw[lane];
  if (lane == 0) { g.valid[i] = 1; if (g.var) g.var[i] = W[0][0]; if (g.sigma) g.sigma[i] = sqrt(W[0][0]); }
}

}  // namespace lvx
