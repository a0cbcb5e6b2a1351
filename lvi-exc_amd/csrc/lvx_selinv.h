// lvx_selinv.h — selected inverse of the damped LM system from its sequential factor, and the pose covariances read from it (lvx_trajectory_covariance).
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
// border rows in place.
#pragma once
#include "lvx_chol16.h"
#include "lvx_trajcov.h"

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
        if (i < TB) { const int d = 16 + i - c; if (d < SI_BD && j0 + 16 + i < nb) g.SigB[(size_t)(j0 + c) * SI_BD + d] = v; }
        else if (i - TB < nbd) g.Z[(size_t)(i - TB) * g.ldz + j0 + c] = v;
      }
    }
    if (tid < 256) {
      const int a = tid >> 4, b = tid & 15;
      const double v = (a < nk && b < nk) ? P[a * ldg + b] : 0.0;
      D[(size_t)(sJ + a) * M + sJ + b] = v;
      if (a >= b && a < nk) g.SigB[(size_t)(j0 + b) * SI_BD + (a - b)] = v;
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

}  // namespace lvx
