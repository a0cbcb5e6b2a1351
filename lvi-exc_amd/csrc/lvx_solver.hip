// lvx_solver.hip — Levenberg-Marquardt step and loop on the structured normal equations (gfx950, FP64).
//
// What this replaces: ceres::Solve with TRUST_REGION / LEVENBERG_MARQUARDT / SPARSE_SCHUR as configured at
// kontiki/trajectory_estimator.h:38-68 (Ceres itself is out-of-tree; its trust-region loop, LM strategy and
// Jacobi scaling are RESTATED from public semantics — PARITY UNPINNED).
//
// System (tangent coordinates, constant scalars removed):
//     [ A  B^T ] [y_b]   [f_b]      A: banded SPD (non-hub knots interleaved with landmarks), half-bandwidth bw
//     [ B  C   ] [y_c] = [f_c]      B: n_border x n_band dense rows (hub knots + calibration),  C: dense
// with A = S (J^T J) S + D^2 etc., S = Jacobi scaling, D^2 = clamp(diag)/radius, f = -S J^T r.
//   1. band Cholesky A = L L^T                (one persistent workgroup, NB-column panels in LDS)
//   2. Z = L^-1 [B^T, f_b]                    (one wavefront per 4 right-hand sides, active window in LDS)
//   3. S_c = C - Z_B^T Z_B, rhs = f_c - Z_B^T z; dense Cholesky solve for y_c (one workgroup)
//   4. y_b = L^-T (z - Z_B y_c)               (one wavefront)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <vector>

#include <chrono>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the entry points are resolved with dlsym (rccl_api)

#include <functional>
#include "lvx_ctx.h"
#include "lvx_lm_policy.h"
#include "lvx_symeig.h"
#include "lvx_selinv.h"

namespace lvx {
// dense border of a single sequence on 16 x 16 tiles (lvx_nd.h, in lvx_bcr.hip's translation unit)
bool dense_tiles_ok(const lvx_ctx* c, int n);
int dense_tiles_factor(lvx_ctx* c, const double* S, double* rhs, int n, int* info);
int dense_tiles_back(lvx_ctx* c, double* rhs, int n);

// ---------------------------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------------------------
// diag[0..nb) from the band, diag[nb..nb+nbd) from C
// Jacobi scaling 1/(1+sqrt(diag)) (ceres TrustRegionMinimizer, jacobi_scaling = true; computed at the first iterate only)
__global__ void k_scale_from_diag(const double* diag, int n, double* scale, int use_scaling) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) scale[i] = use_scaling ? 1.0 / (1.0 + sqrt(fmax(diag[i], 0.0))) : 1.0;
}
// LM diagonal (LevenbergMarquardtStrategy::ComputeStep): clamp(scale^2 diag, min, max)
__global__ void k_lm_diag(const double* diag, const double* scale, int n, double mn, double mx, double* lmd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lmd[i] = fmin(fmax(scale[i] * scale[i] * diag[i], mn), mx);
}
// A = S Hb S + lmd/radius on the diagonal
__global__ void k_build_band(const double* Hb, const double* scale, const double* lmd, double inv_radius, int nb, int bw, double* Lb) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t tot = (size_t)nb * (bw + 1);
  if (idx >= tot) return;
  const int j = (int)(idx / (bw + 1)), d = (int)(idx % (bw + 1));
  double v = 0.0;
  if (j + d < nb) { v = Hb[idx] * scale[j] * scale[j + d]; if (d == 0) v += lmd[j] * inv_radius; }
  else if (d == 0) v = 1.0;
  Lb[idx] = v;
}
// Z rows 0..nbd-1 = S_c B S_b ; row nbd = -S_b g_b
__global__ void k_build_rhs(const double* Bd, const double* gb, const double* scale, int nb, int nbd, int ldz, double* Z) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t tot = (size_t)(nbd + 1) * ldz;
  if (idx >= tot) return;
  const int r = (int)(idx / ldz), j = (int)(idx % ldz);
  double v = 0.0;
  if (j < nb) v = r < nbd ? Bd[(size_t)r * nb + j] * scale[nb + r] * scale[j] : -gb[j] * scale[j];
  Z[idx] = v;
}

// ---------------------------------------------------------------------------------------------------------
// banded Cholesky, lower band storage Lb[j*(bw+1) + d] = A(j+d, j).  One workgroup, NB-column panels.
// ---------------------------------------------------------------------------------------------------------
#define CH_NB 16
#define CH_T 1024
__global__ __launch_bounds__(CH_T) void k_band_chol(double* Lb, int nb, int bw, int* info) {
  extern __shared__ double P[];   // (bw + NB) rows x NB (+1 pad)
  const int ld = CH_NB + 1;
  const int tid = threadIdx.x;
  __shared__ int bad;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int j0 = 0; j0 < nb; j0 += CH_NB) {
    const int nk = min(CH_NB, nb - j0);
    const int rows = min(bw + nk, nb - j0);
    // load panel: P[r][k] = A(j0 + r, j0 + k) for k <= r <= k + bw
    for (int e = tid; e < rows * CH_NB; e += CH_T) {
      const int r = e / CH_NB, k = e % CH_NB;
      double v = 0.0;
      if (k < nk && r >= k && r - k <= bw) v = Lb[(size_t)(j0 + k) * (bw + 1) + (r - k)];
      P[r * ld + k] = v;
    }
    __syncthreads();
    // right-looking factorisation of the panel
    for (int k = 0; k < nk; ++k) {
      if (tid == 0) { const double dkk = P[k * ld + k]; if (!(dkk > 0.0)) { bad = j0 + k + 1; P[k * ld + k] = 1.0; } else P[k * ld + k] = sqrt(dkk); }
      __syncthreads();
      const double inv = 1.0 / P[k * ld + k];
      for (int r = k + 1 + tid; r < rows; r += CH_T) P[r * ld + k] *= inv;
      __syncthreads();
      const int ncol = nk - k - 1;
      for (int e = tid; e < (rows - k - 1) * ncol; e += CH_T) {
        const int r = k + 1 + e / ncol, c = k + 1 + e % ncol;
        if (r >= c) P[r * ld + c] -= P[r * ld + k] * P[c * ld + k];
      }
      __syncthreads();
    }
    // write the factored panel back
    for (int e = tid; e < rows * CH_NB; e += CH_T) {
      const int r = e / CH_NB, k = e % CH_NB;
      if (k < nk && r >= k && r - k <= bw) Lb[(size_t)(j0 + k) * (bw + 1) + (r - k)] = P[r * ld + k];
    }
    // trailing update of the window: W(i, c) -= sum_k P[i][k] P[c][k], nk <= c <= i < rows, 4x4 register tiles
    const int w = rows - nk;
    if (w > 0) {
      const int nt = (w + 3) / 4;
      const int ntiles = nt * (nt + 1) / 2;
      for (int t = tid; t < ntiles; t += CH_T) {
        // tile (ti >= tc) from the linear index
        int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        while (ti * (ti + 1) / 2 > t) --ti;
        const int tc = t - ti * (ti + 1) / 2;
        const int i0 = nk + 4 * ti, c0 = nk + 4 * tc;
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        for (int k = 0; k < nk; ++k) {
          double pi[4], pc[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) { pi[a] = (i0 + a < rows) ? P[(i0 + a) * ld + k] : 0.0; pc[a] = (c0 + a < rows) ? P[(c0 + a) * ld + k] : 0.0; }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] += pi[a] * pc[b];
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int c = c0 + b;
          if (c >= rows) continue;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const int i = i0 + a;
            if (i >= rows || i < c || i - c > bw) continue;
            Lb[(size_t)(j0 + c) * (bw + 1) + (i - c)] -= acc[a][b];
          }
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0 && bad) atomicMax(info, bad);
}

// forward substitution Z[r][:] <- L^-1 Z[r][:] for FW_R right-hand sides per wavefront; window of bw+1 entries in LDS
#define FW_R 4
__global__ __launch_bounds__(64) void k_band_fwd(const double* __restrict__ Lb, int nb, int bw, double* Z, int nrhs, int ldz) {
  extern __shared__ double W[];   // [FW_R][bw + 1] ring buffers
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * FW_R;
  const int nr = min(FW_R, nrhs - r0);
  const int wl = bw + 1;
  for (int r = 0; r < nr; ++r)
    for (int d = lane; d < wl; d += 64) W[r * wl + d] = d < nb ? Z[(size_t)(r0 + r) * ldz + d] : 0.0;
  __syncthreads();
  int head = 0;   // ring position of row j
  for (int j = 0; j < nb; ++j) {
    const double* col = Lb + (size_t)j * (bw + 1);
    const double inv = 1.0 / col[0];
    double zj[FW_R];
#pragma unroll
    for (int r = 0; r < FW_R; ++r) zj[r] = r < nr ? W[r * wl + head] * inv : 0.0;
    __syncthreads();
    for (int d = 1 + lane; d <= bw; d += 64) {
      const double l = col[d];
      int pos = head + d; if (pos >= wl) pos -= wl;
#pragma unroll
      for (int r = 0; r < FW_R; ++r) if (r < nr) W[r * wl + pos] -= l * zj[r];
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < FW_R; ++r) if (r < nr) {
        Z[(size_t)(r0 + r) * ldz + j] = zj[r];
        const int jn = j + wl;   // row entering the window takes the slot just vacated
        W[r * wl + head] = jn < nb ? Z[(size_t)(r0 + r) * ldz + jn] : 0.0;
      }
    }
    head += 1; if (head == wl) head = 0;
    __syncthreads();
  }
}
// backward substitution x <- L^-T x (single right-hand side, one wavefront)
__global__ __launch_bounds__(64) void k_band_bwd(const double* __restrict__ Lb, int nb, int bw, double* x) {
  extern __shared__ double W[];   // ring of the bw most recent solutions x_{j+1..j+bw}
  const int lane = threadIdx.x;
  for (int d = lane; d < bw + 1; d += 64) W[d] = 0.0;
  __syncthreads();
  const int wl = bw + 1;
  int head = 0;   // W[(head + d) % wl] = x_{j + d} for d = 1..bw ; slot head is free for x_j
  for (int j = nb - 1; j >= 0; --j) {
    const double* col = Lb + (size_t)j * (bw + 1);
    double s = 0.0;
    for (int d = 1 + lane; d <= bw; d += 64) {
      int pos = head + d; if (pos >= wl) pos -= wl;
      s += col[d] * W[pos];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const double xj = (x[j] - s) / col[0];
    __syncthreads();
    if (lane == 0) { x[j] = xj; W[head] = xj; }
    head -= 1; if (head < 0) head = wl - 1;
    __syncthreads();
  }
}

// S = Cs - Z_B Z_B^T (lower), rhs = f_c - Z_B z : one workgroup per (row a); dot products over nb
__global__ __launch_bounds__(256) void k_schur(const double* __restrict__ Z, const double* C, const double* gc, const double* scale, int nb, int nbd, int ldc, int ldz,
                                               const double* lmd, double inv_radius, double* S, double* rhs) {
  const int a = blockIdx.x;
  __shared__ double red[256];
  for (int b = 0; b <= nbd; ++b) {   // b == nbd: the right-hand side column z
    if (b < nbd && b > a) continue;
    double s = 0.0;
    const double* za = Z + (size_t)a * ldz;
    const double* zb = Z + (size_t)b * ldz;
    for (int j = threadIdx.x; j < nb; j += 256) s += za[j] * zb[j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
      if (b < nbd) {
        double c = C[(size_t)a * ldc + b] * scale[nb + a] * scale[nb + b];
        if (a == b) c += lmd[nb + a] * inv_radius;
        S[(size_t)a * nbd + b] = c - red[0];
      } else {
        rhs[a] = -gc[a] * scale[nb + a] - red[0];
      }
    }
    __syncthreads();
  }
}
// S and rhs from the Gram matrix M = [Z_B, z]^T [Z_B, z] ((nbd+1) x (nbd+1), column-major)
__global__ void k_schur_from_gram(const double* M, const double* C, const double* gc, const double* scale, int nb, int nbd, int ldc,
                                  const double* lmd, double inv_radius, double* S, double* rhs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int n1 = nbd + 1;
  if (e >= nbd * n1) return;
  const int a = e / n1, b = e % n1;
  if (b < nbd) {
    if (b > a) return;
    double cv = C[(size_t)a * ldc + b] * scale[nb + a] * scale[nb + b];
    if (a == b) cv += lmd[nb + a] * inv_radius;
    S[(size_t)a * nbd + b] = cv - M[(size_t)b * n1 + a];
  } else {
    rhs[a] = -gc[a] * scale[nb + a] - M[(size_t)nbd * n1 + a];
  }
}
// dense Cholesky of the border system (n <= 128), one workgroup; unused border slots have S_aa = lmd/radius > 0.
// Columns 0..np-1 are eliminated (right-looking, so the trailing (n-np) x (n-np) block ends up holding the Schur complement onto the
// SHARED variables) and the right-hand side is forward-substituted: rhs[0..np) = L_pp^-1 b_p, rhs[np..n) = b_s - L_sp z_p.
// np == n is the plain factorisation + forward substitution.
// (the border block and its right-hand side live in LDS for the whole factorisation: in global memory every one of the ~3 n steps was a round trip
// to HBM / L2 and the forward substitution a chain of n^2 / 2 dependent loads on one thread — 180 us for n = 52)
#define DENSE_NT 1024   // (measured, n = 64: 128 threads 95 us, 256: 68, 1024: 50 — the trailing updates, not the barriers)
__global__ __launch_bounds__(DENSE_NT) void k_dense_partial(double* S, double* rhs, int n, int np, int* info) {
  extern __shared__ double ds[];           // T [n][n + 1] | r [n]
  const int tid = threadIdx.x, ld = n + 1;
  double* T = ds; double* r = ds + (size_t)n * ld;
  for (int e = tid; e < n * n; e += DENSE_NT) T[(e / n) * ld + e % n] = S[e];
  for (int e = tid; e < n; e += DENSE_NT) r[e] = rhs[e];
  __syncthreads();
  for (int k = 0; k < np; ++k) {
    if (tid == 0) { const double d = T[k * ld + k]; if (!(d > 0.0)) { if (info[1] == 0) { info[1] = k + 1; ((double*)(info + 2))[0] = d; } T[k * ld + k] = 1.0; } else T[k * ld + k] = sqrt(d); }
    __syncthreads();
    const double inv = 1.0 / T[k * ld + k];
    for (int rr = k + 1 + tid; rr < n; rr += DENSE_NT) T[rr * ld + k] *= inv;
    __syncthreads();
    for (int c0 = k + 1; c0 < n; c0 += 64) {   // lane = column, wavefront = row (no integer divisions: e / m, e % m per entry were most of this kernel)
      const int cc = c0 + (tid & 63);
      const double lc = cc < n ? T[cc * ld + k] : 0.0;
      for (int rr = k + 1 + (tid >> 6); rr < n; rr += DENSE_NT / 64) if (cc < n && rr >= cc) T[rr * ld + cc] -= T[rr * ld + k] * lc;
    }
    __syncthreads();
  }
  // forward substitution, column by column: y_k = r_k / L_kk, then r_i -= L_ik y_k for every i > k (also the rows of the trailing block)
  for (int k = 0; k < np; ++k) {
    if (tid == 0) r[k] = r[k] / T[k * ld + k];
    __syncthreads();
    const double yk = r[k];
    for (int i = k + 1 + tid; i < n; i += DENSE_NT) r[i] -= T[i * ld + k] * yk;
    __syncthreads();
  }
  for (int e = tid; e < n * n; e += DENSE_NT) S[e] = T[(e / n) * ld + e % n];
  for (int e = tid; e < n; e += DENSE_NT) rhs[e] = r[e];
}
// backward substitution of the eliminated part given the solution of the trailing (shared) variables in rhs[np..n)
__global__ __launch_bounds__(DENSE_NT) void k_dense_back(const double* S, double* rhs, int n, int np) {
  extern __shared__ double ds[];           // T [n][n + 1] | r [n]
  const int tid = threadIdx.x, ld = n + 1;
  double* T = ds; double* r = ds + (size_t)n * ld;
  for (int e = tid; e < n * n; e += DENSE_NT) T[(e / n) * ld + e % n] = S[e];
  for (int e = tid; e < n; e += DENSE_NT) r[e] = rhs[e];
  __syncthreads();
  // the trailing variables are known: r_i -= sum_{k >= np} L_ki x_k for i < np, then L^T x = r column by column from the bottom
  for (int i = tid; i < np; i += DENSE_NT) { double s = r[i]; for (int k = np; k < n; ++k) s -= T[k * ld + i] * r[k]; r[i] = s; }
  __syncthreads();
  for (int i = np - 1; i >= 0; --i) {
    if (tid == 0) r[i] = r[i] / T[i * ld + i];
    __syncthreads();
    const double xi = r[i];
    for (int k = tid; k < i; k += DENSE_NT) r[k] -= T[i * ld + k] * xi;
    __syncthreads();
  }
  for (int e = tid; e < np; e += DENSE_NT) rhs[e] = r[e];
}
// z <- z - Z_B^T y_c
// Reductions to a single address: a same-address atomic per WAVEFRONT (2 400 of them for 155 k scalars) serialises at the memory side — 25 ns each, 60 us for a
// kernel that moves 3 MB.  These kernels walk their range with a grid-stride loop of at most RED_BLOCKS workgroups and issue ONE atomic per workgroup.
#define RED_BLOCKS 256
// DETERMINISTIC mode (LVX_DETERMINISTIC): whatever the workgroups of a launch ADD to global memory they add in blockIdx order — a ticket (*tk, one int
// per reduction, self-resetting) is passed from workgroup to workgroup; everything inside a workgroup already has a fixed order.  Workgroups are dispatched in index
// order, so the one a workgroup waits for is resident or done.  tk == nullptr: the default (atomics in timing order).
__device__ __forceinline__ void det_enter(int* tk) {
  if (!tk) return;
  if (threadIdx.x == 0) while (__hip_atomic_load(tk, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != (int)blockIdx.x) __builtin_amdgcn_s_sleep(2);
  __syncthreads();
}
__device__ __forceinline__ void det_leave(int* tk) {
  if (!tk) return;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(tk, blockIdx.x + 1 == gridDim.x ? 0 : (int)blockIdx.x + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void block_atomic_add(double v, double* dst, int* tk = nullptr) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __shared__ double part_[16];
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part_[w] = v;
  __syncthreads();
  det_enter(tk);
  if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < nw; ++k) t += part_[k]; if (t != 0.0 || tk) atomicAdd(dst, t); }
  det_leave(tk);
}
__device__ __forceinline__ void block_atomic_max_nonneg(double v, double* dst) {   // non-negative doubles order like their bit patterns
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __shared__ double part_[16];
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part_[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < nw; ++k) t = fmax(t, part_[k]); atomicMax((unsigned long long*)dst, (unsigned long long)__double_as_longlong(t)); }
}
// the same on the ROW-major right-hand sides of the leaves + separators elimination (lvx_nd.h): Z [ldz][nz], the band's own column is column nbd; 16 lanes per row
__global__ __launch_bounds__(256) void k_sub_border_rm(const double* Z, const double* yc, int nb, int nbd, int nz, double* z) {
  const int j = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  double s = 0.0;
  if (j < nb) {
    const double* row = Z + (size_t)j * nz;
    for (int b = l; b < nbd; b += 16) s -= row[b] * yc[b];
    if (l == 0) s += row[nbd];
  }
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (j < nb && l == 0) z[j] = s;
}
__global__ void k_sub_border(const double* Z, const double* yc, int nb, int nbd, int ldz, double* z) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb) return;
  double s = z[j];
  for (int b = 0; b < nbd; ++b) s -= Z[(size_t)b * ldz + j] * yc[b];
  z[j] = s;
}
// delta (tangent layout) from the scaled solution; also accumulates g_s.y and y^T D^2 y for the model cost change
__global__ void k_unscale(const int* ord, int nt, const double* yb, const double* yc, const double* scale, const double* lmd, double inv_radius,
                          const double* gb, const double* gc, int nb, double* delta, double* sums, int* tk) {
  double gy = 0.0, ydy = 0.0;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nt; v += gridDim.x * blockDim.x) {
    const int o = ord[v];
    double d = 0.0;
    if (o != LVX_DEAD && o < LVX_LM_BASE) {   // landmark entries: k_lm_back
      const int i = o >= 0 ? o : nb + (-1 - o);
      const double y = o >= 0 ? yb[o] : yc[-1 - o];
      const double g = o >= 0 ? gb[o] : gc[-1 - o];
      d = y * scale[i];
      gy += g * scale[i] * y;
      ydy += y * y * lmd[i] * inv_radius;
    }
    delta[v] = d;
  }
  block_atomic_add(gy, &sums[0], tk);
  block_atomic_add(ydy, &sums[1], tk ? tk + 1 : nullptr);
}
// sums[5] += delta^T H delta for the UNSCALED step (H = J^T J in band / border storage): the model cost change is then
// -(g.delta + 1/2 delta^T H delta), what ceres computes from J * step — valid for any (also inexact) step
__global__ void k_quad(const double* __restrict__ Hb, const double* __restrict__ Bd, const double* __restrict__ C, int ldc, const double* yb, const double* yc,
                       const double* scale, int nb, int bw, int nbd, double* sums, int* tk) {
  double q = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb + nbd; i += gridDim.x * blockDim.x) {
    if (i < nb) {
      const double di = yb[i] * scale[i];   // the band part of delta^T H delta is k_quad_band's
      double u = 0.0;
      for (int b = 0; b < nbd; ++b) u += Bd[(size_t)b * nb + i] * (yc[b] * scale[nb + b]);
      q += di * 2.0 * u;
    } else {
      const int a = i - nb;
      const double da = yc[a] * scale[nb + a];
      double t = 0.0;
      for (int b = 0; b < nbd; ++b) t += (a >= b ? C[(size_t)a * ldc + b] : C[(size_t)b * ldc + a]) * (yc[b] * scale[nb + b]);
      q += da * t;
    }
  }
  block_atomic_add(q, &sums[5], tk);
}
// band part: sum_i delta_i (H_ii delta_i + 2 sum_{d >= 1} H(i+d, i) delta_{i+d}) — every stored entry once, a wavefront per band column so
// that its bw + 1 entries are read as contiguous 512-byte pieces (a thread per column read them 1568 bytes apart: 0.5 ms for 243 MB)
__global__ __launch_bounds__(256) void k_quad_band(const double* __restrict__ Hb, const double* __restrict__ yb, const double* __restrict__ scale, int nb, int bw, double* sums, int* tk) {
  const int lane = threadIdx.x & 63;
  double q = 0.0;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nb; i += gridDim.x * 4) {
    const double* col = Hb + (size_t)i * (bw + 1);
    double t = 0.0;
    for (int d = lane; d <= bw && i + d < nb; d += 64) { const double v = col[d] * (yb[i + d] * scale[i + d]); t += d == 0 ? v : 2.0 * v; }
    q += (yb[i] * scale[i]) * t;
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  __shared__ double part[4];   // one atomic per workgroup: thousands of same-address atomics serialise in L2
  if (lane == 0) part[threadIdx.x >> 6] = q;
  __syncthreads();
  det_enter(tk);
  if (threadIdx.x == 0) { const double t = part[0] + part[1] + part[2] + part[3]; if (t != 0.0) atomicAdd(&sums[5], t); }
  det_leave(tk);
}
__device__ __forceinline__ void qplus_dev(const double* x, const double* d, double* o) {   // EigenQuaternionParameterization::Plus
  const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (nd > 0.0) {
    const double sd = sin(nd) / nd;
    const quat r = qmul(mkq(cos(nd), sd * d[0], sd * d[1], sd * d[2]), load_q(x));
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
  } else { o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = x[3]; }
}
// x_out = x (+) delta ; sums[2] += |x_out - x|^2, sums[3] += |x|^2 over the free parameter blocks (ambient); the lidar / camera
// blocks (shared between sequences in the joint solve) go to sums[6], sums[7] instead when split_shared
// Box constraints (inverse depth >= 0: static_rscamera_measurement.h:185, camera_surfel_landmark.h:232; |free time offset| <= mto: sensors.h:161-162)
// are enforced by projection of the candidate, as ceres::ParameterBlock::Plus does.
__global__ void k_plus(const double* x, const double* delta, int N, int L, uint32_t locks, double* xo, double* sums, int split_shared, double mto, int* tk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double dn = 0.0, xn = 0.0;
  if (i < N) {
    const bool r3_free = !tangent_locked(6 * i, N, L, locks), so3_free = !tangent_locked(6 * i + 3, N, L, locks);
    for (int j = 0; j < 3; ++j) { const double a = x[3 * i + j], b = a + delta[6 * i + j]; xo[3 * i + j] = b; if (r3_free) { dn += (b - a) * (b - a); xn += a * a; } }
    double q[4]; qplus_dev(x + 3 * (size_t)N + 4 * i, delta + 6 * i + 3, q);
    for (int j = 0; j < 4; ++j) { const double a = x[3 * (size_t)N + 4 * i + j]; xo[3 * (size_t)N + 4 * i + j] = q[j]; if (so3_free) { dn += (q[j] - a) * (q[j] - a); xn += a * a; } }
  } else if (i == N) {
    const double* s = x + 7 * (size_t)N; double* o = xo + 7 * (size_t)N; const double* d = delta + 6 * (size_t)N;
    const int cb = 6 * N;
    for (int j = 0; j < 8; ++j) o[j] = s[j];
    auto addv = [&](int so, int to, int n, double bound = 0.0) { const bool fr = !tangent_locked(cb + to, N, L, locks); for (int j = 0; j < n; ++j) { const double a = s[so + j]; double b = a + d[to + j]; if (fr && bound > 0.0) b = fmin(fmax(b, -bound), bound); o[so + j] = b; if (fr) { dn += (b - a) * (b - a); xn += a * a; } } };
    auto addq = [&](int so, int to) { const bool fr = !tangent_locked(cb + to, N, L, locks); double q[4]; qplus_dev(s + so, d + to, q); for (int j = 0; j < 4; ++j) { const double a = s[so + j]; o[so + j] = q[j]; if (fr) { dn += (q[j] - a) * (q[j] - a); xn += a * a; } } };
    addv(8, 0, 1); addv(9, 1, 1); addv(10, 2, 3); addv(13, 5, 3);
    const double dn_p = dn, xn_p = xn;
    addq(16, 8); addv(20, 11, 3); addv(23, 14, 1, mto);
    addq(24, 15); addv(28, 18, 3); addv(31, 21, 1, mto);
    if (split_shared) { atomicAdd(&sums[6], dn - dn_p); atomicAdd(&sums[7], xn - xn_p); dn = dn_p; xn = xn_p; }
  } else if (i < N + 1 + L) {
    const int l = i - N - 1;
    const bool fr = !tangent_locked(6 * N + 22 + l, N, L, locks);
    const double a = x[7 * (size_t)N + 32 + l];
    double b = a + delta[6 * (size_t)N + 22 + l];
    if (fr) b = fmax(b, 0.0);
    xo[7 * (size_t)N + 32 + l] = b;
    if (fr) { dn += (b - a) * (b - a); xn += a * a; }
  }
  if (tk) { block_atomic_add(dn, &sums[2], tk); block_atomic_add(xn, &sums[3], tk + 1); return; }
  for (int o = 32; o > 0; o >>= 1) { dn += __shfl_xor(dn, o); xn += __shfl_xor(xn, o); }
  if ((threadIdx.x & 63) == 0 && (dn != 0.0 || xn != 0.0)) { atomicAdd(&sums[2], dn); atomicAdd(&sums[3], xn); }
}
// ---------------------------------------------------------------------------------------------------------
// Landmark elimination.  Every landmark (inverse depth) is a 1 x 1 diagonal block of J^T J coupled to the knots its views touch and to the
// camera extrinsics (DevCommon::lmH); ceres' SPARSE_SCHUR eliminates exactly these e-blocks first.  With Jacobi scaling s and LM damping,
//   d_l = s_l^2 H_ll + lmd_l / radius,  w_l = s_l^2 / d_l :   A' = A - sum_l w_l E_l^T E_l,   g' = g - sum_l w_l E_l^T g_l
// on the UNSCALED band / border rows / dense border / gradients (copies: a rejected step solves the same normal equations again with another
// radius), and after the reduced solve  delta_l = -w_l (g_l + E_l . delta).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lm_schur(const double* __restrict__ lmH, const int* __restrict__ p0s, int wl, int nbd, int ls, const double* __restrict__ scale_l,
                                                  const double* __restrict__ lmd_l, double inv_radius, double* Hr, int bw, double* Br, int nb, double* Cr, int ldc, double* gbr, double* gcr, int* tk) {
  extern __shared__ double e[];            // the landmark's row, then the indices of its non-zero couplings
  const int l = blockIdx.x, ne = wl + nbd;
  int* idx = (int*)(e + ne + 2);
  __shared__ int nn_s;
  const double* row = lmH + (size_t)l * ls;
  if (threadIdx.x == 0) nn_s = 0;
  for (int k = threadIdx.x; k < ne + 2; k += 256) e[k] = row[k];
  __syncthreads();
  const double Hll = e[ne], gl = e[ne + 1];
  if (!(Hll > 0.0)) { det_enter(tk); det_leave(tk); return; }   // no observation reached this landmark: nothing to eliminate
  for (int k = threadIdx.x; k < ne; k += 256) if (e[k] != 0.0) idx[atomicAdd(&nn_s, 1)] = k;   // (any order: every pair of couplings reaches its own address once)
  __syncthreads();
  det_enter(tk);
  const int nn = nn_s, p0 = p0s[l];
  const double s = scale_l[l], w = s * s / (s * s * Hll + lmd_l[l] * inv_radius);
  for (int t = threadIdx.x; t < nn * nn; t += 256) {
    const int ia = t / nn, ib = t - ia * nn;
    if (ib > ia) continue;
    const int ka = idx[ia], kb = idx[ib];
    const double val = -w * e[ka] * e[kb];
    const int lo = ka < kb ? ka : kb, hi = ka < kb ? kb : ka;
    if (hi < wl) atomicAdd(&Hr[(size_t)(p0 + lo) * (bw + 1) + (hi - lo)], val);
    else if (lo < wl) atomicAdd(&Br[(size_t)(hi - wl) * nb + p0 + lo], val);
    else atomicAdd(&Cr[(size_t)(hi - wl) * ldc + (lo - wl)], val);
  }
  for (int t = threadIdx.x; t < nn; t += 256) {
    const int k = idx[t];
    const double val = -w * e[k] * gl;
    if (k < wl) atomicAdd(&gbr[p0 + k], val); else atomicAdd(&gcr[k - wl], val);
  }
  det_leave(tk);
}
typedef double d4s __attribute__((ext_vector_type(4)));
// Landmark elimination by GROUPS (the default).  A workgroup owns up to 32 landmarks whose rows start within 24 band positions of each other —
// the landmarks of one reference frame: same first knot, same co-visible frames — and forms  -sum_l w_l E_l^T E_l  over the union of their
// non-zero columns in LDS before anything reaches HBM: one atomic per non-zero entry of the union block per GROUP instead of per landmark
// (k_lm_schur: 42 M atomics at config 4, most of them on the same addresses, 2.5 ms; here 5 M, 0.1 ms).
__global__ __launch_bounds__(256) void k_lm_schur_grp(const double* __restrict__ lmH, const int* __restrict__ p0s, const int* __restrict__ grp, int ngrp, int wl, int nbd, int ls,
                                                      const double* __restrict__ scale_l, const double* __restrict__ lmd_l, double inv_radius, int ne_max, double* Hr, int bw, double* Br, int nb,
                                                      double* Cr, int ldc, double* gbr, double* gcr, int* tk) {
  extern __shared__ double sm[];   // E[32][nn | 1] (rows scaled by sqrt(w_l), zero rows behind the group's last landmark) | glw[32] | cpos[ne_max] | cols[ne_max]
  const int g = blockIdx.x, j0 = grp[g], j1 = grp[g + 1], G = j1 - j0;
  const int* lms = grp + ngrp + 1;
  const int pmin = p0s[lms[j0]];
  const int U = wl + (p0s[lms[j1 - 1]] - pmin), ne = U + nbd;
  double* glw = sm + (size_t)32 * (ne_max + 1);
  int* cpos = (int*)(glw + 32);
  int* cols = cpos + ne_max;
  __shared__ int nn_s;
  __shared__ double sw[32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int c = tid; c < ne; c += 256) cpos[c] = 0;
  if (tid < 32) {
    double w = 0.0, gl = 0.0;
    if (tid < G) {
      const int l = lms[j0 + tid];
      const double Hll = lmH[(size_t)l * ls + wl + nbd];
      if (Hll > 0.0) { const double s = scale_l[l]; w = s * s / (s * s * Hll + lmd_l[l] * inv_radius); gl = lmH[(size_t)l * ls + wl + nbd + 1]; }
    }
    sw[tid] = sqrt(w); glw[tid] = sqrt(w) * gl;
  }
  __syncthreads();
  // which columns of the union carry a non-zero coupling
  for (int gi = wv; gi < G; gi += 4) {
    if (sw[gi] == 0.0) continue;
    const int l = lms[j0 + gi], sh = p0s[l] - pmin;
    const double* row = lmH + (size_t)l * ls;
    for (int k = lane; k < wl + nbd; k += 64) if (row[k] != 0.0) cpos[k < wl ? k + sh : U + (k - wl)] = 1;
  }
  __syncthreads();
  if (wv == 0) {   // ordered compaction
    int base = 0;
    for (int c0 = 0; c0 < ne; c0 += 64) {
      const int c = c0 + lane;
      const bool on = c < ne && cpos[c] != 0;
      const unsigned long long m = __ballot(on);
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (c < ne) cpos[c] = on ? pos : -1;
      if (on) cols[pos] = c;
      base += __popcll(m);
    }
    if (lane == 0) nn_s = base;
  }
  __syncthreads();
  const int nn = nn_s;
  if (nn == 0) { det_enter(tk); det_leave(tk); return; }
  const int es = nn | 1;   // odd row stride: the four rows of a k-step land in different banks
  for (int e = tid; e < 32 * es; e += 256) sm[e] = 0.0;
  __syncthreads();
  for (int gi = wv; gi < G; gi += 4) {
    const double q = sw[gi];
    if (q == 0.0) continue;
    const int l = lms[j0 + gi], sh = p0s[l] - pmin;
    const double* row = lmH + (size_t)l * ls;
    for (int k = lane; k < wl + nbd; k += 64) { const double v = row[k]; if (v != 0.0) sm[(size_t)gi * es + cpos[k < wl ? k + sh : U + (k - wl)]] = q * v; }
  }
  __syncthreads();
  det_enter(tk);
  // gradient: - sum_l w_l E_l^T g_l
  for (int ia = tid; ia < nn; ia += 256) {
    const int c = cols[ia];
    double acc = 0.0;
    for (int gi = 0; gi < G; ++gi) acc += sm[(size_t)gi * es + ia] * glw[gi];
    if (acc != 0.0) { if (c < U) atomicAdd(&gbr[pmin + c], -acc); else atomicAdd(&gcr[c - U], -acc); }
  }
  // E^T E on the matrix cores: E is [32 landmarks][nn columns] in LDS, i.e. already the [k][column] panel whose 16-column fragments are both operands of a tile pair
  // (lane l: E[4 ks + (l >> 4)][16 c + (l & 15)]); 8 k-steps per pair, the upper tile pairs dealt to the four wavefronts.  A thread per entry walking the 32 landmarks
  // with two LDS reads per product took 161 us per solve at config 4.
  const int nt = (nn + 15) >> 4, npair = nt * (nt + 1) / 2;
  for (int t = wv; t < npair; t += 4) {
    int ci = 0, r = t;
    while (r >= nt - ci) { r -= nt - ci; ++ci; }
    const int cj = ci + r;
    const int ca = 16 * ci + (lane & 15), cb = 16 * cj + (lane & 15);
    d4s D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const double* src = sm + (size_t)(4 * ks + (lane >> 4)) * es;
      const double fa = ca < nn ? src[ca] : 0.0, fb = cb < nn ? src[cb] : 0.0;
      D = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, D, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int ia = 16 * ci + (lane >> 4) + 4 * v, ib = 16 * cj + (lane & 15);   // ia <= ib except inside a diagonal tile
      const double acc = D[v];
      if (ia >= nn || ib >= nn || acc == 0.0 || (ci == cj && ia > ib)) continue;
      const int lo = cols[ia], hi = cols[ib];   // cols is ascending: hi >= lo
      if (hi < U) { if (hi - lo <= bw) atomicAdd(&Hr[(size_t)(pmin + lo) * (bw + 1) + (hi - lo)], -acc); }
      else if (lo < U) atomicAdd(&Br[(size_t)(hi - U) * nb + pmin + lo], -acc);
      else atomicAdd(&Cr[(size_t)(hi - U) * ldc + (lo - U)], -acc);
    }
  }
  det_leave(tk);
}
// delta_l = -w_l (g_l + E_l . delta) and the landmark's terms of g.delta (sums[0]), y^T D^2 y (sums[1]) and delta^T H delta (sums[5]); a wavefront per landmark
__global__ __launch_bounds__(256) void k_lm_back(const double* __restrict__ lmH, const int* __restrict__ p0s, int L, int wl, int nbd_solve, int nbd, int ls, const double* __restrict__ scale_l,
                                                 const double* __restrict__ lmd_l, double inv_radius, const double* __restrict__ yb, const double* __restrict__ yc, const double* __restrict__ scale,
                                                 int nb, double* delta_l, double* sums, int* tk) {
  const int wvi = threadIdx.x >> 6, l = blockIdx.x * 4 + wvi, lane = threadIdx.x & 63;
  __shared__ double red[4][3];   // the workgroup's four landmarks are summed before they reach the three global sums (15 k same-address atomics took 190 us)
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  if (l < L) {
    const double* row = lmH + (size_t)l * ls;
    const int p0 = p0s[l];
    double dot = 0.0;
    for (int k = lane; k < wl; k += 64) { const double ev = row[k]; if (ev != 0.0) dot += ev * yb[p0 + k] * scale[p0 + k]; }
    for (int b = lane; b < nbd_solve; b += 64) { const double ev = row[wl + b]; if (ev != 0.0) dot += ev * yc[b] * scale[nb + b]; }
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
    if (lane == 0) {
      const double Hll = row[wl + nbd], gl = row[wl + nbd + 1];
      double d = 0.0;
      if (Hll > 0.0) {
        const double s = scale_l[l], dmp = lmd_l[l] * inv_radius, w = s * s / (s * s * Hll + dmp);
        d = -w * (gl + dot);
        const double y = d / s;
        t0 = gl * d; t1 = y * y * dmp; t2 = d * (Hll * d + 2.0 * dot);
      }
      delta_l[l] = d;
    }
  }
  if (lane == 0) { red[wvi][0] = t0; red[wvi][1] = t1; red[wvi][2] = t2; }
  __syncthreads();
  det_enter(tk);
  if (threadIdx.x < 3) {
    const double v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (v != 0.0) atomicAdd(&sums[threadIdx.x == 2 ? 5 : threadIdx.x], v);
  }
  det_leave(tk);
}
// rho != null: the PROJECTED gradient of the bounded inverse depths, rho - max(rho - g, 0) (TrustRegionMinimizer::ComputeGradientNorms for a constrained problem)
// out[0] += g . delta with the gradient of the accumulators (band, border, landmark rows) and a step in the tangent layout
__global__ void k_gdot(const int* ord, int nt, const double* gb, const double* gc, const double* lmH, int ls, int goff, const double* delta, double* out, int* tk) {
  double s = 0.0;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nt; v += gridDim.x * blockDim.x) {
    const int o = ord[v];
    if (o == LVX_DEAD) continue;
    const double g = o >= LVX_LM_BASE ? (lmH ? lmH[(size_t)(o - LVX_LM_BASE) * ls + goff] : 0.0) : (o >= 0 ? gb[o] : gc[-1 - o]);
    s += g * delta[v];
  }
  block_atomic_add(s, out, tk);
}

// max |g| over free scalars; bounded border scalars (a free sensor time offset: border index tb[k], value tx[k], |.| <= bound) enter projected
struct TauBox { int idx[2]; const double* x[2]; double bound; };
// One launch for what four did until round 6 (diagonal of the band / border, of the landmarks, gradient max norm of band + border, of the landmarks — each ~5 us of launch
// for microseconds of work, between the pass and the solve of every LM iteration):
// the diagonal of J^T J (band, border, landmarks behind them) and the max norm of the (projected) gradient over band, private border and landmarks
struct PostEval { const double *Hb, *C, *lmH, *gb, *gc, *rho; double* diag; double* sums; int nb, bw, nbd, ldc, nl, ls, off_d, off_g, nbd_g; TauBox tb; };
__global__ __launch_bounds__(256) void k_post_eval(PostEval q) {
  double v = 0.0;
  const int n = q.nb + q.nbd, tot = n + q.nl;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x) {
    if (i < q.nb) { q.diag[i] = q.Hb[(size_t)i * (q.bw + 1)]; v = fmax(v, fabs(q.gb[i])); }
    else if (i < n) {
      const int b = i - q.nb;
      q.diag[i] = q.C[(size_t)b * q.ldc + b];
      if (b < q.nbd_g) {
        double g = q.gc[b];
        for (int k = 0; k < 2; ++k) if (b == q.tb.idx[k] && q.tb.idx[k] >= 0) { const double x = *q.tb.x[k]; g = x - fmin(fmax(x - g, -q.tb.bound), q.tb.bound); }
        v = fmax(v, fabs(g));
      }
    } else {
      const int l = i - n;
      const double* row = q.lmH + (size_t)l * q.ls;
      q.diag[i] = row[q.off_d];
      const double g = row[q.off_g];
      v = fmax(v, q.rho ? fabs(q.rho[l] - fmax(q.rho[l] - g, 0.0)) : fabs(g));
    }
  }
  block_atomic_max_nonneg(v, &q.sums[4]);
}
// what the solve reads of the normal equations beside the band and the border rows — g_b, C, g_c — copied for the landmark elimination to work on, and the solver's
// sums / pivot codes / tickets cleared: one launch for a fill and three copies
__global__ __launch_bounds__(256) void k_pre_solve(const double* gb, double* gbs, int nb, const double* C, double* Cs, int nc2, const double* gc, double* gcs, int ldc, double* sums) {
  const int tot = nb + nc2 + ldc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x) {
    if (i < nb) gbs[i] = gb[i];
    else if (i < nb + nc2) Cs[i - nb] = C[i - nb];
    else gcs[i - nb - nc2] = gc[i - nb - nc2];
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) sums[threadIdx.x] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------
// Marginal covariance of the calibration scalars (lvx_calibration_covariance).  One workgroup, everything in LDS (n <= 128 as k_dense_partial).
// S: the reduced border system (lower triangle), hub knots first, the 22 calibration slots last.  The nh hub columns are eliminated right-looking (L D L^T: no
// right-hand side, nothing is kept of the factor), which leaves the scaled marginal information T of the calibration slots in the trailing block.  A locked slot is an
// inert lmd / radius diagonal: only the free slots are compacted into M.  M = V diag(w) V^T by cyclic Jacobi (lvx_symeig.h; the pairs of a round over the lanes), then
// cov = D V diag(1 / w) V^T D with D = the Jacobi scale.
// out (LVX_CCOV_N doubles): cov [22][22] | sigma [22] | w ascending [22] | V [22][22] (column k <-> w[k]) | scale [22] | off, sweeps, status, band pivot code,
// first hub pivot (1-based, 0 = none), its value.  status: 0 ok, 1 the sweep cap was reached, 2 an eigenvalue is not positive.
// ---------------------------------------------------------------------------------------------------------
#define LVX_NCAL 22
#define LVX_CCOV_N (2 * LVX_NCAL * LVX_NCAL + 3 * LVX_NCAL + 6)
#define CCOV_NT 256
struct SymeigBlockSync { __device__ void operator()() const { __syncthreads(); } };
// Columns 0 .. ne - 1 of T (lower triangle, [n][ld] in LDS) eliminated in place by the CCOV_NT threads of the workgroup: afterwards T[k][k] = d_k and, below it, column k
// holds l_ik d_k of the L D L^T factor; the trailing block is the Schur complement.  A pivot that is not positive is replaced by 1 and the first one is noted in piv
// (1-based column, value).  The caller has a barrier behind its loads; the last step's barrier is the exit.
__device__ __forceinline__ void border_eliminate(double* T, int ld, int n, int ne, double* piv, int tid) {
  for (int k = 0; k < ne; ++k) {
    if (tid == 0) { const double d = T[k * ld + k]; if (!(d > 0.0)) { if (piv[0] == 0.0) { piv[0] = (double)(k + 1); piv[1] = d; } T[k * ld + k] = 1.0; } }
    __syncthreads();
    const double inv = 1.0 / T[k * ld + k];
    for (int c0 = k + 1; c0 < n; c0 += 64) {   // lane = column, wavefront = row (as k_dense_partial); column k is read, never written, in this step
      const int cc = c0 + (tid & 63);
      const double lc = cc < n ? T[cc * ld + k] * inv : 0.0;
      for (int rr = k + 1 + (tid >> 6); rr < n; rr += CCOV_NT / 64) if (cc < n && rr >= cc) T[rr * ld + cc] -= T[rr * ld + k] * lc;
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(CCOV_NT) void k_calib_cov(const double* __restrict__ S, int n, int nh, const double* __restrict__ scale_c, uint32_t free_mask, int max_sweeps, const int* info, double* out) {
  extern __shared__ double ds[];           // T [n][n + 1]
  __shared__ double M[LVX_NCAL * (LVX_NCAL + 1)], V[LVX_NCAL * (LVX_NCAL + 1)], cs[LVX_SYMEIG_CS], piv[2];
  __shared__ int order[LVX_NCAL], fr[LVX_NCAL], slot[LVX_NCAL];
  const int tid = threadIdx.x, ld = n + 1, ldm = LVX_NCAL + 1;
  double* T = ds;
  for (int r = tid >> 6; r < n; r += CCOV_NT / 64) for (int cc = tid & 63; cc <= r; cc += 64) T[r * ld + cc] = S[(size_t)r * n + cc];
  if (tid == 0) {
    piv[0] = 0.0; piv[1] = 0.0;
    int nf0 = 0;
    for (int c = 0; c < LVX_NCAL; ++c) { slot[c] = -1; if (free_mask >> c & 1u) { slot[c] = nf0; fr[nf0++] = c; } }
  }
  __syncthreads();
  int nf = 0;
  for (int c = 0; c < LVX_NCAL; ++c) nf += (int)(free_mask >> c & 1u);
  border_eliminate(T, ld, n, nh, piv, tid);
  for (int e = tid; e < nf * nf; e += CCOV_NT) {
    const int i = e / nf, j = e % nf, a = nh + fr[i > j ? i : j], b = nh + fr[i > j ? j : i];
    M[i * ldm + j] = T[a * ld + b];
  }
  __syncthreads();
  int sweeps = 0; double off = 0.0;
  const int capped = symeig_jacobi(M, ldm, nf, V, ldm, cs, max_sweeps, tid, CCOV_NT, SymeigBlockSync(), &sweeps, &off);
  if (tid == 0) symeig_order(M, ldm + 1, nf, order);
  __syncthreads();
  int status = capped ? 1 : 0;
  for (int k = 0; k < nf; ++k) if (!status && !(M[k * (ldm + 1)] > 0.0)) status = 2;
  double* o_cov = out, *o_sig = out + LVX_NCAL * LVX_NCAL, *o_w = o_sig + LVX_NCAL, *o_v = o_w + LVX_NCAL, *o_sc = o_v + LVX_NCAL * LVX_NCAL, *o_tail = o_sc + LVX_NCAL;
  for (int e = tid; e < LVX_NCAL * LVX_NCAL; e += CCOV_NT) {
    const int ci = e / LVX_NCAL, cj = e % LVX_NCAL, i = slot[ci], j = slot[cj];
    double s = 0.0;
    if (i >= 0 && j >= 0 && status == 0) { for (int k = 0; k < nf; ++k) { const int q = order[k]; s += V[i * ldm + q] * V[j * ldm + q] / M[q * (ldm + 1)]; } s *= scale_c[ci] * scale_c[cj]; }
    o_cov[e] = s;
    if (ci == cj) o_sig[ci] = sqrt(s);
    o_v[e] = (ci < nf && cj < nf) ? V[ci * ldm + order[cj]] : 0.0;
  }
  if (tid < LVX_NCAL) { o_w[tid] = tid < nf ? M[order[tid] * (ldm + 1)] : 0.0; o_sc[tid] = scale_c[tid]; }
  if (tid == 0) { o_tail[0] = off; o_tail[1] = (double)sweeps; o_tail[2] = (double)status; o_tail[3] = (double)info[0]; o_tail[4] = piv[0]; o_tail[5] = piv[1]; }
}

// ---------------------------------------------------------------------------------------------------------
// lvx_calibration_covariance_shared: the calibration covariance of the JOINT problem (private scalars per rank, the 14 extrinsic scalars shared).  Two one-workgroup
// kernels around ONE sum over the ranks.  Border order: [nh hub | 8 private calibration slots | 14 shared slots]; the shared damping is not in S (apply_diag).
//   k_joint_cov_local   eliminates hub and private columns (a locked slot is an inert lmd / R diagonal), keeps P^-1 (8 x 8, P the private block behind the hub
//                       elimination) and G = P^-1 X (8 x 14, X the coupling) from the L D L^T factor, and packs this rank's term T_r of the shared block.
//   k_joint_cov_shared  the same instructions on the same reduced message on every rank: M = sum_r T_r + lmd_shared / R over the free shared slots, M = V w V^T,
//                       cov_ss = D M^-1 D, cov_pp = D_p (P^-1 + G M^-1 G^T) D_p, cov_ps = -D_p G M^-1 D_s.
// Message (LVX_JC_N doubles, summed): T_r [14][14] canonical slots | slot free (14) | 1 (ranks) | not-PD votes | error votes | ranks whose elimination ran on the
// reduction route (a sequential redo can help) | one-hot of min(max_sweeps, 64): the smallest cap over the ranks applies on all of them.
// Record (LVX_JREC_N): cov [22][22] | sigma [22] | w [14] | V [14][14] | own T_r [14][14] | scale [22] | off, sweeps, status, band pivot code, first pivot, its value,
// ranks, not-PD votes, error votes, redo votes.  status: 0 ok, 1 sweep cap, 2 eigenvalue not positive, 3 a shared slot is free on some ranks only, 4 / 5 votes.
// ---------------------------------------------------------------------------------------------------------
#define LVX_NPRIV (LVX_NCAL - LVX_N_SHARED)
#define LVX_JC_FREE (LVX_N_SHARED * LVX_N_SHARED)
#define LVX_JC_WORLD (LVX_JC_FREE + LVX_N_SHARED)
#define LVX_JC_NOTPD (LVX_JC_WORLD + 1)
#define LVX_JC_ERR (LVX_JC_WORLD + 2)
#define LVX_JC_REDO (LVX_JC_WORLD + 3)
#define LVX_JC_SWEEPS (LVX_JC_WORLD + 4)
#define LVX_JC_SWEEP_SLOTS 64
#define LVX_JC_N (LVX_JC_SWEEPS + LVX_JC_SWEEP_SLOTS)
#define LVX_JKEEP_N (LVX_NPRIV * LVX_NPRIV + LVX_NPRIV * LVX_N_SHARED)
#define LVX_JREC_COV 0
#define LVX_JREC_SIG (LVX_NCAL * LVX_NCAL)
#define LVX_JREC_W (LVX_JREC_SIG + LVX_NCAL)
#define LVX_JREC_V (LVX_JREC_W + LVX_N_SHARED)
#define LVX_JREC_OWN (LVX_JREC_V + LVX_N_SHARED * LVX_N_SHARED)
#define LVX_JREC_SCALE (LVX_JREC_OWN + LVX_N_SHARED * LVX_N_SHARED)
#define LVX_JREC_TAIL (LVX_JREC_SCALE + LVX_NCAL)
#define LVX_JREC_N (LVX_JREC_TAIL + 10)
// S == nullptr: this rank failed before its border system existed — the message carries its votes only
__global__ __launch_bounds__(CCOV_NT) void k_joint_cov_local(const double* __restrict__ S, int n, int nh, uint32_t free_mask, int sweep_slot, double err, double force_notpd, double redo,
                                                            const int* info, double* msg, double* keep, double* rec) {
  extern __shared__ double ds[];           // T [n][n + 1]
  __shared__ double piv[2], d[LVX_NPRIV], Li[LVX_NPRIV * LVX_NPRIV], W[LVX_N_SHARED * LVX_NPRIV];
  const int tid = threadIdx.x, ld = n + 1, np = nh + LVX_NPRIV;
  double* T = ds;
  for (int e = tid; e < LVX_JC_N; e += CCOV_NT) msg[e] = 0.0;
  if (tid == 0) { piv[0] = 0.0; piv[1] = 0.0; }
  __syncthreads();
  if (S != nullptr) {
    for (int r = tid >> 6; r < n; r += CCOV_NT / 64) for (int cc = tid & 63; cc <= r; cc += 64) T[r * ld + cc] = S[(size_t)r * n + cc];
    __syncthreads();
    border_eliminate(T, ld, n, np, piv, tid);
    if (tid < LVX_NPRIV) d[tid] = T[(nh + tid) * ld + nh + tid];
    __syncthreads();
    for (int e = tid; e < LVX_N_SHARED * LVX_NPRIV; e += CCOV_NT) W[e] = T[(np + e / LVX_NPRIV) * ld + nh + e % LVX_NPRIV] / d[e % LVX_NPRIV];   // W = X^T L^-T D^-1
    if (tid < LVX_NPRIV) {   // column tid of L^-1 (unit lower triangular): L x = e_tid
      for (int i = 0; i < LVX_NPRIV; ++i) {
        double t = i == tid ? 1.0 : 0.0;
        for (int k = tid; k < i; ++k) t -= T[(nh + i) * ld + nh + k] / d[k] * Li[k * LVX_NPRIV + tid];
        Li[i * LVX_NPRIV + tid] = i < tid ? 0.0 : t;
      }
    }
    __syncthreads();
    for (int e = tid; e < LVX_NPRIV * LVX_NPRIV; e += CCOV_NT) {   // P^-1 = L^-T D^-1 L^-1
      const int i = e / LVX_NPRIV, j = e % LVX_NPRIV;
      double s = 0.0;
      for (int k = i > j ? i : j; k < LVX_NPRIV; ++k) s += Li[k * LVX_NPRIV + i] * Li[k * LVX_NPRIV + j] / d[k];
      keep[e] = s;
    }
    for (int e = tid; e < LVX_NPRIV * LVX_N_SHARED; e += CCOV_NT) {   // G = L^-T W^T
      const int i = e / LVX_N_SHARED, a = e % LVX_N_SHARED;
      double g = 0.0;
      for (int k = i; k < LVX_NPRIV; ++k) g += Li[k * LVX_NPRIV + i] * W[a * LVX_NPRIV + k];
      keep[LVX_NPRIV * LVX_NPRIV + e] = g;
    }
    for (int e = tid; e < LVX_N_SHARED * LVX_N_SHARED; e += CCOV_NT) {
      const int a = e / LVX_N_SHARED, b = e % LVX_N_SHARED, hi = a > b ? a : b, lo = a > b ? b : a;
      const bool fr = (free_mask >> (LVX_NPRIV + a) & 1u) && (free_mask >> (LVX_NPRIV + b) & 1u);
      const double v = fr ? T[(np + hi) * ld + np + lo] : 0.0;
      msg[e] = v; rec[LVX_JREC_OWN + e] = v;
    }
    if (tid < LVX_N_SHARED) msg[LVX_JC_FREE + tid] = (free_mask >> (LVX_NPRIV + tid) & 1u) ? 1.0 : 0.0;
  }
  if (tid == 0) {
    const int code = (S != nullptr && info != nullptr) ? info[0] : 0;
    msg[LVX_JC_WORLD] = 1.0;
    msg[LVX_JC_NOTPD] = (piv[0] != 0.0 || code != 0 || force_notpd != 0.0) ? 1.0 : 0.0;
    msg[LVX_JC_ERR] = err; msg[LVX_JC_REDO] = redo;
    msg[LVX_JC_SWEEPS + sweep_slot] = 1.0;
    rec[LVX_JREC_TAIL + 3] = (double)code; rec[LVX_JREC_TAIL + 4] = piv[0]; rec[LVX_JREC_TAIL + 5] = piv[1];
  }
}
struct JointLmd { double v[LVX_N_SHARED]; };
__global__ __launch_bounds__(CCOV_NT) void k_joint_cov_shared(const double* __restrict__ msg, const double* __restrict__ keep, JointLmd lmd, double inv_radius, const double* __restrict__ scale_c,
                                                             uint32_t free_mask, double* rec) {
  __shared__ double M[LVX_N_SHARED * (LVX_N_SHARED + 1)], V[LVX_N_SHARED * (LVX_N_SHARED + 1)], Mi[LVX_N_SHARED * LVX_N_SHARED], GM[LVX_NPRIV * LVX_N_SHARED], cs[LVX_SYMEIG_CS];
  __shared__ int order[LVX_N_SHARED], fr[LVX_N_SHARED], slot[LVX_N_SHARED], hdr[3];   // hdr: free shared slots, status, sweep cap
  const int tid = threadIdx.x, ldm = LVX_N_SHARED + 1;
  const double* Pi = keep, *G = keep + LVX_NPRIV * LVX_NPRIV;
  if (tid == 0) {
    const double world = msg[LVX_JC_WORLD];
    int st = msg[LVX_JC_ERR] > 0.0 ? 5 : msg[LVX_JC_NOTPD] > 0.0 ? 4 : 0, nf0 = 0, cap = LVX_JC_SWEEP_SLOTS;
    for (int a = 0; a < LVX_N_SHARED; ++a) {
      const double f = msg[LVX_JC_FREE + a];
      slot[a] = -1;
      if (f == world) { slot[a] = nf0; fr[nf0++] = a; }
      else if (f != 0.0 && st == 0) st = 3;
    }
    for (int k = LVX_JC_SWEEP_SLOTS - 1; k >= 0; --k) if (msg[LVX_JC_SWEEPS + k] > 0.0) cap = k + 1;
    hdr[0] = nf0; hdr[1] = st; hdr[2] = cap;
  }
  __syncthreads();
  const int nf = hdr[0];
  int status = hdr[1], sweeps = 0;
  double off = 0.0;
  if (status == 0) {
    for (int e = tid; e < nf * nf; e += CCOV_NT) {
      const int i = e / nf, j = e % nf;
      M[i * ldm + j] = msg[fr[i] * LVX_N_SHARED + fr[j]] + (i == j ? lmd.v[fr[i]] * inv_radius : 0.0);
    }
    __syncthreads();
    if (symeig_jacobi(M, ldm, nf, V, ldm, cs, hdr[2], tid, CCOV_NT, SymeigBlockSync(), &sweeps, &off)) status = 1;
    if (tid == 0) symeig_order(M, ldm + 1, nf, order);
    __syncthreads();
    for (int k = 0; k < nf; ++k) if (!status && !(M[k * (ldm + 1)] > 0.0)) status = 2;
  }
  if (status == 0) {
    for (int e = tid; e < nf * nf; e += CCOV_NT) {   // M^-1 over the free shared slots
      const int i = e / nf, j = e % nf;
      double s = 0.0;
      for (int k = 0; k < nf; ++k) { const int q = order[k]; s += V[i * ldm + q] * V[j * ldm + q] / M[q * (ldm + 1)]; }
      Mi[i * LVX_N_SHARED + j] = s;
    }
    __syncthreads();
    for (int e = tid; e < LVX_NPRIV * nf; e += CCOV_NT) {   // G M^-1
      const int p = e / nf, j = e % nf;
      double s = 0.0;
      for (int i = 0; i < nf; ++i) s += G[p * LVX_N_SHARED + fr[i]] * Mi[i * LVX_N_SHARED + j];
      GM[p * LVX_N_SHARED + j] = s;
    }
    __syncthreads();
  }
  for (int e = tid; e < LVX_NCAL * LVX_NCAL; e += CCOV_NT) {
    const int ci = e / LVX_NCAL, cj = e % LVX_NCAL, a = ci > cj ? ci : cj, b = ci > cj ? cj : ci;   // one expression per unordered pair: the record is symmetric to the bit
    const int sa = a >= LVX_NPRIV ? slot[a - LVX_NPRIV] : -1, sb = b >= LVX_NPRIV ? slot[b - LVX_NPRIV] : -1;
    const bool fa = a >= LVX_NPRIV ? sa >= 0 : (free_mask >> a & 1u) != 0, fb = b >= LVX_NPRIV ? sb >= 0 : (free_mask >> b & 1u) != 0;
    double s = 0.0;
    if (status == 0 && fa && fb) {
      if (b >= LVX_NPRIV) s = Mi[sa * LVX_N_SHARED + sb];
      else if (a >= LVX_NPRIV) s = -GM[b * LVX_N_SHARED + sa];
      else { s = Pi[a * LVX_NPRIV + b]; for (int j = 0; j < nf; ++j) s += GM[a * LVX_N_SHARED + j] * G[b * LVX_N_SHARED + fr[j]]; }
      s *= scale_c[a] * scale_c[b];
    }
    rec[LVX_JREC_COV + e] = s;
    if (ci == cj) rec[LVX_JREC_SIG + ci] = sqrt(s);
  }
  for (int e = tid; e < LVX_N_SHARED * LVX_N_SHARED; e += CCOV_NT) {
    const int i = e / LVX_N_SHARED, j = e % LVX_N_SHARED;
    rec[LVX_JREC_V + e] = (hdr[1] == 0 && i < nf && j < nf) ? V[i * ldm + order[j]] : 0.0;   // (hdr[1] == 0: the decomposition ran, V and order exist)
  }
  if (tid < LVX_N_SHARED) rec[LVX_JREC_W + tid] = (hdr[1] == 0 && tid < nf) ? M[order[tid] * (ldm + 1)] : 0.0;
  if (tid < LVX_NCAL) rec[LVX_JREC_SCALE + tid] = scale_c[tid];
  if (tid == 0) {
    double* t = rec + LVX_JREC_TAIL;
    t[0] = off; t[1] = (double)sweeps; t[2] = (double)status; t[6] = msg[LVX_JC_WORLD]; t[7] = msg[LVX_JC_NOTPD]; t[8] = msg[LVX_JC_ERR]; t[9] = msg[LVX_JC_REDO];
  }
}

}  // namespace lvx

using namespace lvx;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct SolveWork { double *L, *Z, *S, *rhs, *delta, *diag, *scale, *lmd, *sums, *Z2, *gram; int* info; int ldz; bool use_bcr;
                   bool lm;                                   // landmarks are eliminated first (k_lm_schur)
                   const double *Hs, *Bs, *Cs, *gbs, *gcs;     // what the band / border solve reads: the normal equations, or their copies after the landmark elimination
                   bool inplace = false, lm_done = false, constrained = false;
                   int* tk = nullptr; };                      // deterministic mode: the reductions' tickets (det_enter / det_leave), null otherwise   // inplace (LM loop, single sequence): the landmark elimination works on the band / border rows THEMSELVES — no 290 MB copy per
                                                               // solve; the accumulators no longer hold J^T J afterwards (the loop re-evaluates before it needs them).  lm_done: this step's elimination has run

// ---------------------------------------------------------------------------------------------------------
// Reductions of the joint (sequence-per-GPU) solve.  Two transports: RCCL on the context's stream (lvx_rccl_init: librccl is loaded with dlopen, so the
// library carries no link-time dependency and shares the RCCL a host process may already have loaded, e.g. torch's), or a host callback over host
// buffers (lvx_allreduce_fn: MPI, torch.distributed, a test harness).  Identity for a single sequence.
// ---------------------------------------------------------------------------------------------------------
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi* rccl_api(lvx_ctx* c) {
  static RcclApi api;
  if (api.lib) return &api;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) { fail(c, LVX_E_COMM, std::string("cannot load librccl: ") + dlerror()); return nullptr; }
  api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank))dlsym(lib, "ncclCommInitRank");
  api.CommDestroy = (decltype(api.CommDestroy))dlsym(lib, "ncclCommDestroy");
  api.AllReduce = (decltype(api.AllReduce))dlsym(lib, "ncclAllReduce");
  api.GetErrorString = (decltype(api.GetErrorString))dlsym(lib, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce) { fail(c, LVX_E_COMM, "librccl lacks the expected entry points"); return nullptr; }
  api.lib = lib;
  return &api;
}
#define LVX_COMM_BUF 512   // doubles of the device staging buffer of the reductions (the largest message is LVX_JC_N = 278)
static bool is_joint(const lvx_ctx* c) { return c->ar_fn != nullptr || c->rccl_comm != nullptr; }
// in place over all ranks on the DEVICE buffer d_comm[0..n), queued on the context's stream
static int reduce_device(lvx_ctx* c, int n, int op) {
  RcclApi* api = rccl_api(c); if (!api) return LVX_E_COMM;
  double* d = (double*)c->d_comm.p;
  const ncclResult_t r = api->AllReduce(d, d, (size_t)n, ncclDouble, op == LVX_REDUCE_SUM ? ncclSum : ncclMax, (ncclComm_t)c->rccl_comm, c->stream);
  c->n_collectives++;
  if (r != ncclSuccess) return fail(c, LVX_E_COMM, std::string("ncclAllReduce: ") + (api->GetErrorString ? api->GetErrorString(r) : "error"));
  return LVX_OK;
}
// in place over all ranks on a HOST buffer
static int reduce(lvx_ctx* c, double* buf, int n, int op) {
  if (c->rccl_comm) {
    if (n > LVX_COMM_BUF) return fail(c, LVX_E_ARG, "reduction larger than the staging buffer");
    LVX_HIP(c, hipMemcpyAsync(c->d_comm.p, buf, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    int rc = reduce_device(c, n, op); if (rc) return rc;
    LVX_HIP(c, hipMemcpyAsync(buf, c->d_comm.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    LVX_HIP(c, hipStreamSynchronize(c->stream));
    return LVX_OK;
  }
  if (!c->ar_fn) return LVX_OK;
  c->n_collectives++;
  if (c->ar_fn(c->ar_user, buf, n, op) != 0) return fail(c, LVX_E_COMM, "all-reduce callback failed");
  return LVX_OK;
}
// a rank that failed locally keeps meeting the scheduled collectives with its vote set; at the first collective that carries a vote EVERY rank leaves:
// the failing rank with its own code, the others with LVX_E_COMM — nobody is left waiting inside a reduction
static int leave_together(lvx_ctx* c, double votes, int lerr) {
  if (!(votes > 0.0)) return LVX_OK;
  return lerr ? lerr : fail(c, LVX_E_COMM, "another rank of the joint solve failed");
}

// will_inplace: the caller is going to run the landmark elimination on the band / border rows themselves (LM loop of a single sequence): no reduced copies needed (290 MB at config 4)
static int solver_alloc(lvx_ctx* c, SolveWork& w, bool will_inplace = false) {
  int rc;
  const size_t nb = (size_t)std::max(c->nb, 1), nbd = c->nbd, nt = (size_t)lvx_tangent_size(c);
  // the block chain's batched triangular solves stop at blocks of 256 (trsv_batched): a wider band — a free landmark tracked over more than ~42 knots writes fill across
  // its whole reach — goes to the sequential band Cholesky, whose panel holds half-bandwidths up to ~1 100.  (Until the landmark-track tests such a problem ended in LVX_E_ARG.)
  const bool use_bcr = !c->sw.solver_seq && ((c->bw + 3) / 4) * 4 <= 256;
  size_t ldz = nb;
  if (use_bcr && c->nb > 0) {
    if ((rc = nd_plan(c, (int)nbd + 1))) return rc;      // leaves + separators elimination when the band's column profile allows it (lvx_nd.h), the uniform chain otherwise
    if (nd_active(c)) ldz = (size_t)nd_ldz(c);
    else { if ((rc = bcr_plan(c))) return rc; ldz = (size_t)c->bcr_nblk * c->bcr_b; }
  }
  w.ldz = (int)ldz; w.use_bcr = use_bcr && c->nb > 0;
  if ((rc = dev_alloc(c, c->d_Y, std::max((nbd + 1) * ldz, nd_active(c) ? ((size_t)nd_nz(c) + 1) * ldz : (size_t)0) * 8))) return rc;   // (row-major [ldz][nd_nz] + the band's vector on the leaves + separators path)
  if (w.use_bcr) { if ((rc = dev_alloc(c, c->d_gram, (nbd + 1) * (nbd + 1) * 8))) return rc; }
  w.Z2 = (double*)c->d_Y2.p; w.gram = (double*)c->d_gram.p;
  if ((rc = dev_alloc(c, c->d_S, (nbd * nbd + nbd + 16) * 8))) return rc;
  if ((rc = dev_alloc(c, c->d_delta, nt * 8))) return rc;
  const size_t nall = nb + nbd + (size_t)std::max(c->L, 0);
  if ((rc = dev_alloc(c, c->d_diag, 3 * nall * 8))) return rc;
  w.lm = c->L > 0 && c->rep.n > 0 && !(c->locks & LVX_LOCK_LANDMARKS);
  if (!w.lm) c->lm_elim_kernel = 0;
  w.Hs = (const double*)c->d_Hb.p; w.Bs = (const double*)c->d_Bd.p; w.Cs = (const double*)c->d_C.p; w.gbs = (const double*)c->d_gb.p; w.gcs = (const double*)c->d_gc.p;
  if (w.lm) {
    const size_t ldc = c->nbd_ext;
    if (!will_inplace) {
      if ((rc = dev_alloc(c, c->d_Hr, c->d_Hb.bytes))) return rc;
      if ((rc = dev_alloc(c, c->d_Br, (size_t)nbd * nb * 8))) return rc;
    }
    if ((rc = dev_alloc(c, c->d_red, (nb + ldc * ldc + ldc) * 8))) return rc;
    w.Hs = will_inplace ? (const double*)c->d_Hb.p : (const double*)c->d_Hr.p; w.Bs = will_inplace ? (const double*)c->d_Bd.p : (const double*)c->d_Br.p; w.gbs = (const double*)c->d_red.p; w.Cs = w.gbs + nb; w.gcs = w.Cs + ldc * ldc;
  }
  c->p_Hs = w.Hs;
  if ((rc = dev_alloc(c, c->d_scal, 64 * 8))) return rc;
  // sums, error words and (deterministic mode) tickets start from zero: the IterationZero projection of a constrained solve takes a ticket before the first solve_local cleared them
  LVX_HIP(c, hipMemsetAsync(c->d_scal.p, 0, 64 * 8, c->stream));
  if ((rc = dev_alloc(c, c->d_state_try, (size_t)lvx_state_size(c) * 8))) return rc;
  w.L = (double*)c->d_L.p; w.Z = (double*)c->d_Y.p; w.S = (double*)c->d_S.p; w.rhs = w.S + nbd * nbd; w.delta = (double*)c->d_delta.p;
  w.diag = (double*)c->d_diag.p; w.scale = w.diag + nall; w.lmd = w.scale + nall;
  w.sums = (double*)c->d_scal.p; w.info = (int*)(w.sums + 32);
  w.tk = c->sw.deterministic ? (int*)(w.sums + 48) : nullptr;   // (zero = start state; the buffer is cleared at the head of every solve and every ticket resets itself)
  // shared extrinsics of the joint solve: tangent 6N+8 .. 6N+21 own the LAST 14 border slots (ensure_layout gives every calibration
  // scalar a fixed slot after the hub knots; a locked one keeps an inert slot with S_aa = lmd / radius)
  c->ns = 0;
  if (is_joint(c)) {   // either transport: host callback or RCCL communicator
    c->ns = LVX_N_SHARED;
    for (int k = 0; k < LVX_N_SHARED; ++k) {
      c->sh_slot[k] = k;
      const int o = c->ord[6 * (size_t)c->N + 8 + k];
      if (o != LVX_DEAD && -1 - o != c->nbd - LVX_N_SHARED + k) return fail(c, LVX_E_STATE, "shared extrinsics are not the tail of the border");
    }
  }
  c->last_ns = c->ns;
  return LVX_OK;
}

// Local half of one damped solve: factor the band, eliminate it and the private border variables.  On return the trailing ns x ns block
// of w.S / w.rhs holds this sequence's contribution to the reduced system of the shared variables (all of the border system when ns = 0).
struct StageTimer {   // LVX_SOLVER_TIMING=1: host wall time per stage (enqueue cost) and at the synchronisation points
  bool on; std::chrono::steady_clock::time_point t;
  explicit StageTimer(const lvx_ctx* c) : on(c->sw.solver_timing != 0), t(std::chrono::steady_clock::now()) {}
  void lap(const char* what) { if (!on) return; const auto n = std::chrono::steady_clock::now(); fprintf(stderr, "[lvx solver] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count()); t = n; }
};

// First half of solve_local, and all that lvx_calibration_covariance needs of it: landmarks and band are eliminated (on whichever route the plan and force_seq select) and
// w.S (lower triangle) / w.rhs hold the reduced border system, unfactored.  Everything is queued; the band's pivot code is in w.info[0].
static int reduce_to_border(lvx_ctx* c, SolveWork& w, double radius, bool force_seq, bool* bcr_used, StageTimer& tm) {
  hipStream_t st = c->stream;
  const int nb = c->nb, bw = c->bw, nbd = c->nbd;
  const double ir = 1.0 / radius;
  bool sums_cleared = false;   // (k_pre_solve clears them with its copies; otherwise the fill below)
  const bool use_bcr = w.use_bcr && !force_seq;
  *bcr_used = use_bcr;
  if (!use_bcr && nb > 0) { int rca = dev_alloc(c, c->d_L, (size_t)nb * (bw + 1) * 8); if (rca) return rca; w.L = (double*)c->d_L.p; }
  const int ldz = w.ldz;
  if (w.lm && !(w.inplace && w.lm_done)) {   // copies of the normal equations, then A' = A - sum_l w_l E_l^T E_l, g' = g - sum_l w_l E_l^T g_l   (second call of a step = the sequential fallback: everything is eliminated already)
    const size_t nb1 = (size_t)std::max(nb, 1), ldc = c->nbd_ext;
    w.lm_done = true;
    if (!w.inplace) {
      LVX_HIP(c, hipMemcpyAsync((void*)w.Hs, c->d_Hb.p, nb1 * (bw + 1) * 8, hipMemcpyDeviceToDevice, st));
      LVX_HIP(c, hipMemcpyAsync((void*)w.Bs, c->d_Bd.p, (size_t)nbd * nb1 * 8, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_pre_solve, dim3((unsigned)std::min<size_t>(RED_BLOCKS, (nb1 + ldc * ldc + ldc + 255) / 256)), dim3(256), 0, st, (const double*)c->d_gb.p, (double*)w.gbs, (int)nb1,
                       (const double*)c->d_C.p, (double*)w.Cs, (int)(ldc * ldc), (const double*)c->d_gc.p, (double*)w.gcs, (int)ldc, w.sums);
    sums_cleared = true;
    const int ne_max = c->lm_wl + c->lm_gspread + c->nbd_ext;
    const size_t lds_g = (size_t)32 * (ne_max + 1) * 8 + 32 * 8 + (size_t)2 * ne_max * 4 + 16;
    if (c->lm_ngrp > 0 && lds_g <= 160 * 1024 && !c->sw.test_lm_schur_one) {   // (switch TEST_LM_SCHUR_ONE: the tests' way into the per-landmark kernel on small problems)
      c->lm_elim_kernel = 1;
      LVX_HIP(c, hipFuncSetAttribute((const void*)k_lm_schur_grp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
      hipLaunchKernelGGL(k_lm_schur_grp, dim3((unsigned)c->lm_ngrp), dim3(256), lds_g, st, (const double*)c->d_lmH.p, (const int*)c->d_lm_p0.p, (const int*)c->d_lm_grp.p, c->lm_ngrp, c->lm_wl, c->nbd_ext, c->lm_ls,
                         w.scale + (nb + nbd), w.lmd + (nb + nbd), ir, ne_max, (double*)w.Hs, bw, (double*)w.Bs, nb, (double*)w.Cs, c->nbd_ext, (double*)w.gbs, (double*)w.gcs, w.tk ? w.tk + 5 : nullptr);
    } else {
    c->lm_elim_kernel = 2;
    const size_t lds = (size_t)(c->lm_wl + c->nbd_ext + 2) * 8 + (size_t)(c->lm_wl + c->nbd_ext) * 4 + 16;
    LVX_HIP(c, hipFuncSetAttribute((const void*)k_lm_schur, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_lm_schur, dim3((unsigned)c->L), dim3(256), lds, st, (const double*)c->d_lmH.p, (const int*)c->d_lm_p0.p, c->lm_wl, c->nbd_ext, c->lm_ls, w.scale + (nb + nbd), w.lmd + (nb + nbd), ir,
                       (double*)w.Hs, bw, (double*)w.Bs, nb, (double*)w.Cs, c->nbd_ext, (double*)w.gbs, (double*)w.gcs, w.tk ? w.tk + 5 : nullptr);
    }
  }
  if (!sums_cleared) LVX_HIP(c, hipMemsetAsync(w.sums, 0, 64 * 8, st));
  if (nb > 0) {
    const size_t tr = (size_t)(nbd + 1) * ldz;
    // leaves + separators elimination: no array of right-hand sides is built — its kernels form [B^T | -g_b] S from the border rows where they load them (lvx_nd.h: nd_rhs)
    if (use_bcr && nd_active(c)) { const int rcd = nd_dense_start(c, w.scale, w.lmd, ir, w.Bs, w.gbs, w.Z, ldz); if (rcd) return rcd; }
    else hipLaunchKernelGGL(k_build_rhs, dim3((unsigned)((tr + 255) / 256)), dim3(256), 0, st, w.Bs, w.gbs, w.scale, nb, nbd, ldz, w.Z);
    if (use_bcr) {
      int rc2;
      tm.lap("enqueue build_rhs");
      if (nd_active(c)) { if ((rc2 = nd_factor(c, w.scale, w.lmd, ir, w.info, w.Bs, w.gbs, w.Z, ldz, nbd + 1))) return rc2; }
      else if ((rc2 = bcr_factor(c, w.scale, w.lmd, ir, w.info, w.Z, ldz, nbd + 1))) return rc2;   // factor, and Z <- L^-1 [B^T, f_b] (in place) level by level with it
      tm.lap("enqueue bcr_factor + forward");
    } else {
      const size_t tot = (size_t)nb * (bw + 1);
      hipLaunchKernelGGL(k_build_band, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, w.Hs, w.scale, w.lmd, ir, nb, bw, w.L);
      const size_t lds_ch = (size_t)(bw + CH_NB) * (CH_NB + 1) * 8;
      if (lds_ch > 150 * 1024) return fail(c, LVX_E_ARG, "bandwidth too large for the single-workgroup band Cholesky panel");
      LVX_HIP(c, hipFuncSetAttribute((const void*)k_band_chol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ch));
      hipLaunchKernelGGL(k_band_chol, dim3(1), dim3(CH_T), lds_ch, st, w.L, nb, bw, w.info);
      const size_t lds_fw = (size_t)FW_R * (bw + 1) * 8;
      LVX_HIP(c, hipFuncSetAttribute((const void*)k_band_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fw));
      hipLaunchKernelGGL(k_band_fwd, dim3((unsigned)((nbd + 1 + FW_R - 1) / FW_R)), dim3(64), lds_fw, st, (const double*)w.L, nb, bw, w.Z, nbd + 1, ldz);
    }
  }
  double* Zf = w.Z;   // forward-substituted right-hand sides
  if (use_bcr && nb > 0) {
    int rc2;
    if ((rc2 = bcr_gram(c, Zf, ldz, nbd + 1, w.gram, nd_active(c) ? nd_nz(c) : 0))) return rc2;
    hipLaunchKernelGGL(k_schur_from_gram, dim3((unsigned)((nbd * (nbd + 1) + 255) / 256)), dim3(256), 0, st, (const double*)w.gram, w.Cs, w.gcs,
                       (const double*)w.scale, nb, nbd, c->nbd_ext, (const double*)w.lmd, ir, w.S, w.rhs);
  } else {
    hipLaunchKernelGGL(k_schur, dim3(nbd), dim3(256), 0, st, (const double*)Zf, w.Cs, w.gcs, (const double*)w.scale,
                       nb > 0 ? nb : 0, nbd, c->nbd_ext, ldz, (const double*)w.lmd, ir, w.S, w.rhs);
  }
  return LVX_OK;
}

static int solve_local(lvx_ctx* c, SolveWork& w, double radius, bool force_seq, bool* bcr_used, bool defer_check = false) {   // defer_check: the caller reads the pivot codes with the step's sums
  hipStream_t st = c->stream;
  StageTimer tm(c);
  const int nbd = c->nbd;
  { const int rcb = reduce_to_border(c, w, radius, force_seq, bcr_used, tm); if (rcb) return rcb; }
  if (dense_tiles_ok(c, nbd)) { const int rcd = dense_tiles_factor(c, w.S, w.rhs, nbd, w.info); if (rcd) return rcd; }   // single sequence: one wavefront on 16 x 16 tiles (10 us against 50)
  else {
  const size_t lds_dense = ((size_t)nbd * (nbd + 1) + nbd) * 8;
  LVX_HIP(c, hipFuncSetAttribute((const void*)k_dense_partial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dense));
  hipLaunchKernelGGL(k_dense_partial, dim3(1), dim3(DENSE_NT), lds_dense, st, w.S, w.rhs, nbd, nbd - c->ns, w.info);
  }
  LVX_HIP(c, hipGetLastError());
  int info[4] = {0, 0, 0, 0};
  tm.lap("enqueue gram+schur+dense");
  if (defer_check) return LVX_OK;
  LVX_HIP(c, hipMemcpyAsync(info, w.info, 16, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  tm.lap("sync (GPU drain)");
  if (info[0] || info[1]) { double dv; memcpy(&dv, info + 2, 8); return fail(c, LVX_E_NOTPD, "damped normal equations not positive definite (band pivot code " + std::to_string(info[0]) + ", first border pivot " + std::to_string(info[1]) + " value " + std::to_string(dv) + ")"); }
  return LVX_OK;
}

// ---- the ONE per-step collective on the device: [S (14 x 14, canonical slots) | rhs (14) | not-PD votes | error votes] ----
struct SharedMap { int ns, np, nbd; int slot[LVX_N_SHARED]; double lmd[LVX_N_SHARED]; };
#define LVX_R1_N (LVX_N_SHARED * LVX_N_SHARED + LVX_N_SHARED + 2)
__global__ void k_pack_shared(const double* S, const double* rhs, SharedMap m, double notpd, double err, double* out) {
  const int e = threadIdx.x;
  if (e < LVX_R1_N) out[e] = 0.0;
  __syncthreads();
  if (notpd == 0.0 && err == 0.0) {
    for (int k = e; k < m.ns * m.ns; k += blockDim.x) { const int a = k / m.ns, b = k % m.ns; if (b <= a) out[m.slot[a] * LVX_N_SHARED + m.slot[b]] = S[(size_t)(m.np + a) * m.nbd + m.np + b]; }
    if (e < m.ns) out[LVX_N_SHARED * LVX_N_SHARED + m.slot[e]] = rhs[m.np + e];
  }
  if (e == 0) { out[LVX_R1_N - 2] = notpd; out[LVX_R1_N - 1] = err; }
}
// the same ns x ns Cholesky on every rank (identical inputs after the sum); shared damping is added once, here.  buf[LVX_R1_N - 2] > 0 afterwards: not positive definite
__global__ void k_solve_shared(double* buf, SharedMap m, double inv_radius, double* rhs) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (buf[LVX_R1_N - 2] > 0.0 || buf[LVX_R1_N - 1] > 0.0 || m.ns == 0) return;
  double A[LVX_N_SHARED][LVX_N_SHARED], y[LVX_N_SHARED];
  for (int a = 0; a < m.ns; ++a) { for (int b = 0; b <= a; ++b) A[a][b] = buf[m.slot[a] * LVX_N_SHARED + m.slot[b]]; A[a][a] += m.lmd[a] * inv_radius; y[a] = buf[LVX_N_SHARED * LVX_N_SHARED + m.slot[a]]; }
  for (int k = 0; k < m.ns; ++k) {
    if (!(A[k][k] > 0.0)) { buf[LVX_R1_N - 2] = 1.0; return; }
    A[k][k] = sqrt(A[k][k]);
    for (int r = k + 1; r < m.ns; ++r) A[r][k] /= A[k][k];
    for (int r = k + 1; r < m.ns; ++r) for (int q = k + 1; q <= r; ++q) A[r][q] -= A[r][k] * A[q][k];
  }
  for (int i = 0; i < m.ns; ++i) { double t = y[i]; for (int k = 0; k < i; ++k) t -= A[i][k] * y[k]; y[i] = t / A[i][i]; }
  for (int i = m.ns - 1; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < m.ns; ++k) t -= A[k][i] * y[k]; y[i] = t / A[i][i]; }
  for (int i = 0; i < m.ns; ++i) rhs[m.np + i] = y[i];
}

// Solve the damped, scaled system for the normal equations of the last evaluation.  Leaves delta (tangent layout) on the device.
// m[0] = g.delta, m[1] = delta^T H delta, m[2] = y^T D^2 y of THIS rank (the caller reduces them together with what else it has to reduce);
// *notpd: the (joint) system was not positive definite.  lerr: a local error of the caller's that has not met a collective yet.
// Returns != LVX_OK only when every rank returns (an error vote travelled with the collective) or for a purely local failure of a single sequence.
static int solve_step_device(lvx_ctx* c, SolveWork& w, double radius, double m[3], bool* notpd_out, int lerr) {
  hipStream_t st = c->stream;
  const int nb = c->nb, bw = c->bw, nbd = c->nbd, nt = lvx_tangent_size(c), ns = c->ns, np = nbd - ns;
  const double ir = 1.0 / radius;
  ProfScope ps(c, LVX_KERNEL_SOLVE);
  bool bcr_used = false;
  m[0] = m[1] = m[2] = 0.0; *notpd_out = false;
  w.lm_done = false;
  // Single sequence: the pivot codes of the factorisations travel to the host WITH the step's sums — the back substitution is queued right behind the elimination and the
  // solve stops the host once, not twice (a failed pivot voids the step, which is then redone by the sequential solver as before).  The joint solve votes on the
  // pivots in its collective, in the middle: it keeps the early check.
  const bool defer = !is_joint(c) && !lerr && w.use_bcr;
  int rc = lerr ? lerr : solve_local(c, w, radius, false, &bcr_used, defer);
  if (rc == LVX_E_NOTPD && w.use_bcr) {
    // the cyclic-reduction elimination order can lose positive definiteness in floating point on nearly singular systems
    // (huge trust radius at convergence); the sequential band Cholesky is the exact fallback.  Purely local: no collective yet.
    rc = solve_local(c, w, radius, true, &bcr_used);
    ++c->solver_fallbacks;
  }
  bool notpd = rc == LVX_E_NOTPD;
  int lrc = (rc != LVX_OK && rc != LVX_E_NOTPD) ? rc : LVX_OK;   // a local failure other than "not positive definite": voted, everybody leaves
  if (!is_joint(c) && lrc) return lrc;
  if (is_joint(c)) {
    SharedMap sm{}; sm.ns = ns; sm.np = np; sm.nbd = nbd;
    for (int a = 0; a < ns; ++a) { sm.slot[a] = c->sh_slot[a]; sm.lmd[a] = c->sh_lmd[a]; }
    double* dbuf = (double*)c->d_comm.p;
    if (c->rccl_comm) {   // pack -> ncclAllReduce -> 14 x 14 solve, all queued on the stream: no host round trip for the collective
      hipLaunchKernelGGL(k_pack_shared, dim3(1), dim3(256), 0, st, (const double*)w.S, (const double*)w.rhs, sm, notpd ? 1.0 : 0.0, lrc ? 1.0 : 0.0, dbuf);
      int r2 = reduce_device(c, LVX_R1_N, LVX_REDUCE_SUM); if (r2) return r2;
      hipLaunchKernelGGL(k_solve_shared, dim3(1), dim3(64), 0, st, dbuf, sm, ir, w.rhs);
      double votes[2];
      LVX_HIP(c, hipMemcpyAsync(votes, dbuf + LVX_R1_N - 2, 16, hipMemcpyDeviceToHost, st));
      LVX_HIP(c, hipStreamSynchronize(st));
      if ((r2 = leave_together(c, votes[1], lrc))) return r2;
      notpd = votes[0] > 0.0;
    } else {   // host callback: stage the block through the host
      double buf[LVX_R1_N] = {0};
      double hs[LVX_N_SHARED * LVX_N_SHARED], hr[LVX_N_SHARED];
      if (ns > 0 && !notpd && !lrc) {
        LVX_HIP(c, hipMemcpy2DAsync(hs, (size_t)ns * 8, w.S + (size_t)np * nbd + np, (size_t)nbd * 8, (size_t)ns * 8, ns, hipMemcpyDeviceToHost, st));
        LVX_HIP(c, hipMemcpyAsync(hr, w.rhs + np, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
        LVX_HIP(c, hipStreamSynchronize(st));
        for (int a = 0; a < ns; ++a) {
          for (int b = 0; b <= a; ++b) buf[c->sh_slot[a] * LVX_N_SHARED + c->sh_slot[b]] = hs[a * ns + b];
          buf[LVX_N_SHARED * LVX_N_SHARED + c->sh_slot[a]] = hr[a];
        }
      }
      buf[LVX_R1_N - 2] = notpd ? 1.0 : 0.0; buf[LVX_R1_N - 1] = lrc ? 1.0 : 0.0;
      int r2 = reduce(c, buf, LVX_R1_N, LVX_REDUCE_SUM); if (r2) return r2;
      if ((r2 = leave_together(c, buf[LVX_R1_N - 1], lrc))) return r2;
      if (buf[LVX_R1_N - 2] > 0.0) notpd = true;
      if (!notpd && ns > 0) {
        double A[LVX_N_SHARED][LVX_N_SHARED], y[LVX_N_SHARED];
        for (int a = 0; a < ns; ++a) { for (int b = 0; b <= a; ++b) A[a][b] = buf[c->sh_slot[a] * LVX_N_SHARED + c->sh_slot[b]]; A[a][a] += c->sh_lmd[a] * ir; y[a] = buf[LVX_N_SHARED * LVX_N_SHARED + c->sh_slot[a]]; }
        for (int k = 0; k < ns && !notpd; ++k) {
          if (!(A[k][k] > 0.0)) { notpd = true; break; }
          A[k][k] = std::sqrt(A[k][k]);
          for (int r = k + 1; r < ns; ++r) A[r][k] /= A[k][k];
          for (int r = k + 1; r < ns; ++r) for (int q = k + 1; q <= r; ++q) A[r][q] -= A[r][k] * A[q][k];
        }
        if (!notpd) {
          for (int i = 0; i < ns; ++i) { double t = y[i]; for (int k = 0; k < i; ++k) t -= A[i][k] * y[k]; y[i] = t / A[i][i]; }
          for (int i = ns - 1; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < ns; ++k) t -= A[k][i] * y[k]; y[i] = t / A[i][i]; }
          LVX_HIP(c, hipMemcpyAsync(w.rhs + np, y, (size_t)ns * 8, hipMemcpyHostToDevice, st));
          LVX_HIP(c, hipStreamSynchronize(st));   // y lives on this stack frame
        }
      }
    }
  }
  *notpd_out = notpd;
  if (notpd) { fail(c, LVX_E_NOTPD, "damped normal equations not positive definite"); return LVX_OK; }
  double h[8]; int info4[4] = {0, 0, 0, 0};
  const bool quad_explicit = is_joint(c);   // (see the tail)
  auto tail = [&]() -> int {
  if (dense_tiles_ok(c, nbd)) { const int rcd = dense_tiles_back(c, w.rhs, nbd); if (rcd) return rcd; }
  else { const size_t lds_dense = ((size_t)nbd * (nbd + 1) + nbd) * 8;
    LVX_HIP(c, hipFuncSetAttribute((const void*)k_dense_back, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dense));
    hipLaunchKernelGGL(k_dense_back, dim3(1), dim3(DENSE_NT), lds_dense, st, (const double*)w.S, w.rhs, nbd, np); }
  const int ldz = w.ldz;
  double* Zf = w.Z;
  const bool zrm = bcr_used && nd_active(c);   // row-major right-hand sides; the band's vector lives behind them
  double* zb = zrm ? Zf + (size_t)nd_nz(c) * ldz : Zf + (size_t)nbd * std::max(ldz, 1);
  if (nb > 0) {
    if (zrm) hipLaunchKernelGGL(k_sub_border_rm, dim3((unsigned)((nb + 15) / 16)), dim3(256), 0, st, (const double*)Zf, (const double*)w.rhs, nb, nbd, nd_nz(c), zb);
    else hipLaunchKernelGGL(k_sub_border, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const double*)Zf, (const double*)w.rhs, nb, nbd, ldz, zb);
    if (bcr_used) {
      int rc2;
      if (nd_active(c)) { if ((rc2 = nd_backward(c, zb))) return rc2; }
      else if ((rc2 = bcr_backward(c, zb, zb, ldz, 1))) return rc2;
    } else {
      const size_t lds_bw = (size_t)(bw + 1) * 8;
      hipLaunchKernelGGL(k_band_bwd, dim3(1), dim3(64), lds_bw, st, (const double*)w.L, nb, bw, zb);
    }
  }
  hipLaunchKernelGGL(k_unscale, dim3((unsigned)std::min(RED_BLOCKS, (nt + 255) / 256)), dim3(256), 0, st, (const int*)c->d_ord.p, nt, (const double*)zb, (const double*)w.rhs, (const double*)w.scale,
                     (const double*)w.lmd, ir, (const double*)c->d_gb.p, (const double*)c->d_gc.p, nb, w.delta, w.sums, w.tk);
  if (w.lm) hipLaunchKernelGGL(k_lm_back, dim3((unsigned)((c->L + 3) / 4)), dim3(256), 0, st, (const double*)c->d_lmH.p, (const int*)c->d_lm_p0.p, c->L, c->lm_wl, nbd, c->nbd_ext, c->lm_ls,
                               (const double*)(w.scale + (nb + nbd)), (const double*)(w.lmd + (nb + nbd)), ir, (const double*)zb, (const double*)w.rhs, (const double*)w.scale, nb,
                               w.delta + 6 * (size_t)c->N + 22, w.sums, w.tk ? w.tk + 4 : nullptr);
  // delta^T H delta.  Single sequence: the step solves (H + D) delta = -g EXACTLY (SPARSE_SCHUR semantics; residual 1e-15 of the scale, tests/test_gpu_fullsize_oracle.py),
  // so delta^T H delta = -g.delta - delta^T D delta comes with the sums k_unscale / k_lm_back form anyway — the explicit product streams the whole band again (216 MB, 0.16 ms).
  // Joint problem: the identity holds for the SUM over the ranks only and the shared damping is counted once, after the reduction — the explicit product stays.
  if (quad_explicit) {
    if (nb > 0) hipLaunchKernelGGL(k_quad_band, dim3((unsigned)std::min(2048, (nb + 3) / 4)), dim3(256), 0, st, (const double*)c->d_Hb.p, (const double*)zb, (const double*)w.scale, nb, bw, w.sums, w.tk ? w.tk + 2 : nullptr);
    hipLaunchKernelGGL(k_quad, dim3((unsigned)std::min(2 * RED_BLOCKS, (nb + nbd + 255) / 256)), dim3(256), 0, st, (const double*)c->d_Hb.p, (const double*)c->d_Bd.p, (const double*)c->d_C.p, c->nbd_ext,
                       (const double*)zb, (const double*)w.rhs, (const double*)w.scale, nb, bw, nbd, w.sums, w.tk ? w.tk + 3 : nullptr);
  }
  LVX_HIP(c, hipGetLastError());
  if (!c->pin) { LVX_HIP(c, hipHostMalloc((void**)&c->pin, 128 * 8, hipHostMallocDefault)); std::memset(c->pin, 0, 128 * 8); }
  LVX_HIP(c, hipMemcpyAsync(c->pin + 40, w.sums, 8 * 8, hipMemcpyDeviceToHost, st));
  if (defer) LVX_HIP(c, hipMemcpyAsync(c->pin + 48, w.info, 16, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  for (int q = 0; q < 8; ++q) h[q] = c->pin[40 + q];
  if (defer) std::memcpy(info4, c->pin + 48, 16);
  return LVX_OK;
  };
  { const int rt = tail(); if (rt) return rt; }
  // (switch TEST_BAD_PIVOT: the tests' way into this branch — a pivot failure is declared where there was none)
  if (defer && (info4[0] || info4[1] || c->sw.test_bad_pivot)) {   // a pivot failed in the elimination this step came from: redo it with the sequential band Cholesky (checked at once)
    ++c->solver_fallbacks;
    rc = solve_local(c, w, radius, true, &bcr_used, false);
    if (rc == LVX_E_NOTPD) { *notpd_out = true; return LVX_OK; }
    if (rc) return rc;
    const int rt = tail(); if (rt) return rt;
  }
  // model_cost_change = -(g.delta + 1/2 delta^T H delta)   (TrustRegionMinimizer: -model_residuals.(residuals + model_residuals / 2));
  // joint problem: H = sum_r H_r, g = sum_r g_r with delta_r = [private_r | shared]  =>  both terms are sums over the ranks
  m[0] = h[0]; m[1] = quad_explicit ? h[5] : -h[0] - h[1]; m[2] = h[1];
  return LVX_OK;
}

// What a LVX_EVAL_NORMAL_EQ evaluation leaves on the host (local_after_eval): this rank's private gradient max norm, the shared entries of diagonal / gradient
struct EvalLocal { double gm = 0.0; double hd[LVX_N_SHARED] = {0}, hg[LVX_N_SHARED] = {0}; double tau[2] = {0, 0}; bool have_tau = false; };   // tau: the (shared) sensor time offsets of a constrained joint solve
// max |g| over this rank's private free scalars (band, private border, landmarks) and the shared entries of g_c, queued into the pinned words
static int local_gmax(lvx_ctx* c, SolveWork& w) {   // (with the diagonal of J^T J, which the same launch fetches: k_post_eval)
  hipStream_t st = c->stream;
  LVX_HIP(c, hipMemsetAsync(w.sums + 4, 0, 8, st));
  // box constraints of a single sequence (w.constrained): the gradient norm is the projected one, at the state of the last evaluation
  const double* xs = (w.constrained && c->last_state_d) ? c->last_state_d : nullptr;
  TauBox tb{{-1, -1}, {nullptr, nullptr}, c->sensor_mto};
  if (xs) {
    const int oL = c->ord[6 * c->N + 14], oC = c->ord[6 * c->N + 21];
    if (oL != LVX_DEAD && oL < 0) { tb.idx[0] = -1 - oL; tb.x[0] = xs + 7 * (size_t)c->N + 23; }
    if (oC != LVX_DEAD && oC < 0) { tb.idx[1] = -1 - oC; tb.x[1] = xs + 7 * (size_t)c->N + 31; }
  }
  PostEval q{};
  q.Hb = (const double*)c->d_Hb.p; q.C = (const double*)c->d_C.p; q.lmH = (const double*)c->d_lmH.p; q.gb = (const double*)c->d_gb.p; q.gc = (const double*)c->d_gc.p;
  q.rho = xs ? xs + 7 * (size_t)c->N + 32 : nullptr; q.diag = w.diag; q.sums = w.sums;
  q.nb = c->nb; q.bw = c->bw; q.nbd = c->nbd; q.ldc = c->nbd_ext; q.nl = w.lm ? c->L : 0; q.ls = c->lm_ls; q.off_d = c->lm_wl + c->nbd_ext; q.off_g = c->lm_wl + c->nbd_ext + 1;
  q.nbd_g = c->nbd - c->ns; q.tb = tb;
  const int tot = c->nb + c->nbd + q.nl;
  hipLaunchKernelGGL(k_post_eval, dim3((unsigned)std::min(RED_BLOCKS, (tot + 255) / 256)), dim3(256), 0, st, q);
  // into the pinned words (lvx_ctx::pin); local_collect moves them to EvalLocal::gm / hg after the host stop
  if (!c->pin) { LVX_HIP(c, hipHostMalloc((void**)&c->pin, 128 * 8, hipHostMallocDefault)); std::memset(c->pin, 0, 128 * 8); }
  LVX_HIP(c, hipMemcpyAsync(c->pin + 24, w.sums + 4, 8, hipMemcpyDeviceToHost, st));
  if (c->ns > 0) LVX_HIP(c, hipMemcpyAsync(c->pin + 25, (const double*)c->d_gc.p + (c->nbd - c->ns), (size_t)c->ns * 8, hipMemcpyDeviceToHost, st));
  return LVX_OK;
}
// What follows a LVX_EVAL_NORMAL_EQ evaluation, in two halves so that the loop can put ONE collective between them.
// local_after_eval: the diagonal of J^T J into w.diag (the LM damping in w.lmd — what the solver reads — is untouched until apply_diag), this rank's private
// gradient max norm, and the shared entries of diagonal / gradient on the host.
// after the host stop behind local_after_eval's copies: the pinned words into *e
static void local_collect(const lvx_ctx* c, EvalLocal* e) {
  e->gm = c->pin[24];
  for (int i = 0; i < c->ns && i < LVX_N_SHARED; ++i) { e->hg[i] = c->pin[25 + i]; e->hd[i] = c->pin[50 + i]; }
  if (e->have_tau) { e->tau[0] = c->pin[70]; e->tau[1] = c->pin[71]; }
}
static int local_after_eval(lvx_ctx* c, SolveWork& w, EvalLocal* e, bool sync = true) {   // sync = false: queued only (the caller's next host stop completes the copies into *e)
  const int n = c->nb + c->nbd, ns = c->ns;
  hipStream_t st = c->stream;
  int rc = local_gmax(c, w); if (rc) return rc;   // k_post_eval: the diagonal (band, border, landmarks behind them) and the gradient norm in one launch
  if (is_joint(c) && ns > 0) LVX_HIP(c, hipMemcpyAsync(c->pin + 50, w.diag + (n - ns), (size_t)ns * 8, hipMemcpyDeviceToHost, st));
  // (keyed on the LOCKS, which every rank shares — a rank whose own sequence has no block that makes it constrained must project the summed shared gradient
  // exactly as its peers do, or they disagree on gradient_tolerance convergence and part ways before the next collective)
  const bool tau_free = !(c->locks & LVX_LOCK_LIDAR_TAU) || !(c->locks & LVX_LOCK_CAM_TAU);
  if (is_joint(c) && (w.constrained || tau_free) && c->last_state_d) {   // the shared time offsets' box enters the projected gradient of the SUMMED shared gradient (apply_diag)
    LVX_HIP(c, hipMemcpyAsync(c->pin + 70, c->last_state_d + 7 * (size_t)c->N + 23, 8, hipMemcpyDeviceToHost, st));
    LVX_HIP(c, hipMemcpyAsync(c->pin + 71, c->last_state_d + 7 * (size_t)c->N + 31, 8, hipMemcpyDeviceToHost, st));
    e->have_tau = true;
  }
  if (sync) { LVX_HIP(c, hipStreamSynchronize(st)); local_collect(c, e); }
  return LVX_OK;
}
// Joint quantities of an evaluation as ONE sum block: [shared diagonal (14, canonical slots) | shared gradient (14) | ranks whose private gradient max norm exceeds the
// tolerance] — the termination test max|g| <= tol needs no MAX reduction: it holds iff no rank reports a violation and the summed shared gradient passes.
#define LVX_JB_N (2 * LVX_N_SHARED + 1)
static void joint_block_pack(const lvx_ctx* c, const EvalLocal& e, double grad_tol, double* buf) {
  for (int i = 0; i < LVX_JB_N; ++i) buf[i] = 0.0;
  for (int i = 0; i < c->ns; ++i) { buf[c->sh_slot[i]] = e.hd[i]; buf[LVX_N_SHARED + c->sh_slot[i]] = e.hg[i]; }
  buf[2 * LVX_N_SHARED] = e.gm > grad_tol ? 1.0 : 0.0;
}
// apply_diag: Jacobi scaling (first iterate), LM damping from w.diag — with the JOINT diagonal at the shared scalars (buf: the reduced block, or null for a single
// sequence); *grad_converged: max|g| over the joint problem <= grad_tol
static int apply_diag(lvx_ctx* c, SolveWork& w, bool compute_scale, int use_scaling, double mn, double mx, const EvalLocal& e, const double* buf, double grad_tol, bool* grad_converged) {
  const int n = c->nb + c->nbd, ns = c->ns;
  hipStream_t st = c->stream;
  const int nl = w.lm ? c->L : 0;
  double hd[LVX_N_SHARED];
  bool conv = e.gm <= grad_tol;
  if (buf) {
    conv = !(buf[2 * LVX_N_SHARED] > 0.0);
    for (int i = 0; i < ns; ++i) {
      hd[i] = buf[c->sh_slot[i]];
      double gsh = buf[LVX_N_SHARED + c->sh_slot[i]];
      // a FREE shared time offset (canonical slots 6: lidar, 13: camera) is bounded: its entry of the projected gradient is x - clamp(x - g, -b, b)
      if (e.have_tau && (c->sh_slot[i] == 6 || c->sh_slot[i] == 13) && c->ord[6 * (size_t)c->N + (c->sh_slot[i] == 6 ? 14 : 21)] != LVX_DEAD) {
        const double x = e.tau[c->sh_slot[i] == 6 ? 0 : 1];
        gsh = x - std::min(std::max(x - gsh, -c->sensor_mto), c->sensor_mto);
      }
      if (std::fabs(gsh) > grad_tol) conv = false;
    }
    if (ns > 0) LVX_HIP(c, hipMemcpyAsync(w.diag + (n - ns), hd, (size_t)ns * 8, hipMemcpyHostToDevice, st));   // Jacobi scaling and LM damping use the JOINT diagonal at the shared scalars
  } else for (int i = 0; i < ns; ++i) if (std::fabs(e.hg[i]) > grad_tol) conv = false;
  *grad_converged = conv;
  if (compute_scale) hipLaunchKernelGGL(k_scale_from_diag, dim3((unsigned)((n + nl + 255) / 256)), dim3(256), 0, st, (const double*)w.diag, n + nl, w.scale, use_scaling);
  hipLaunchKernelGGL(k_lm_diag, dim3((unsigned)((n + nl + 255) / 256)), dim3(256), 0, st, (const double*)w.diag, (const double*)w.scale, n + nl, mn, mx, w.lmd);
  if (is_joint(c) && ns > 0) {   // shared damping is applied once to the reduced system (solve_step_device), not per rank
    LVX_HIP(c, hipMemcpyAsync(c->sh_lmd, w.lmd + (n - ns), (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    LVX_HIP(c, hipStreamSynchronize(st));   // (also keeps hd alive until the copy above has read it)
    LVX_HIP(c, hipMemsetAsync(w.lmd + (n - ns), 0, (size_t)ns * 8, st));
  } else if (buf) LVX_HIP(c, hipStreamSynchronize(st));
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
// The first evaluation of a solve (and lvx_solve_step_shared): both halves around one sum [cost | joint block | error votes].  lerr: error of the evaluation that
// has not met a collective yet.
static int post_eval(lvx_ctx* c, SolveWork& w, bool compute_scale, int use_scaling, double mn, double mx, double* cost, double grad_tol, bool* grad_converged, int lerr, double* votes = nullptr) {
  EvalLocal e;
  if (!lerr) lerr = local_after_eval(c, w, &e);
  if (is_joint(c)) {
    double buf[LVX_JB_N + 3] = {0};
    if (!lerr) { joint_block_pack(c, e, grad_tol, buf); buf[LVX_JB_N] = *cost; }
    buf[LVX_JB_N + 1] = lerr ? 1.0 : 0.0;
    buf[LVX_JB_N + 2] = votes ? *votes : 0.0;   // rides along: e.g. "this rank's problem is constrained" (summed over the ranks)
    int rc = reduce(c, buf, LVX_JB_N + 3, LVX_REDUCE_SUM); if (rc) return rc;
    if (votes) *votes = buf[LVX_JB_N + 2];
    if ((rc = leave_together(c, buf[LVX_JB_N + 1], lerr))) return rc;
    *cost = buf[LVX_JB_N];
    return apply_diag(c, w, compute_scale, use_scaling, mn, mx, e, buf, grad_tol, grad_converged);
  }
  if (lerr) return lerr;
  return apply_diag(c, w, compute_scale, use_scaling, mn, mx, e, nullptr, grad_tol, grad_converged);
}

// g . delta with the gradient the accumulators hold now
static int grad_dot(lvx_ctx* c, SolveWork& w, double* out) {
  hipStream_t st = c->stream;
  const int nt = lvx_tangent_size(c);
  LVX_HIP(c, hipMemsetAsync(w.sums + 8, 0, 8, st));
  hipLaunchKernelGGL(k_gdot, dim3((unsigned)std::min(RED_BLOCKS, (nt + 255) / 256)), dim3(256), 0, st, (const int*)c->d_ord.p, nt, (const double*)c->d_gb.p, (const double*)c->d_gc.p,
                     w.lm ? (const double*)c->d_lmH.p : (const double*)nullptr, c->lm_ls, c->lm_wl + c->nbd_ext + 1, (const double*)w.delta, w.sums + 8, w.tk ? w.tk + 6 : nullptr);
  LVX_HIP(c, hipMemcpyAsync(out, w.sums + 8, 8, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipStreamSynchronize(st));
  return LVX_OK;
}

struct HookScope {   // installs the all-reduce hook for the duration of one API call
  lvx_ctx* c;
  HookScope(lvx_ctx* ctx, lvx_allreduce_fn fn, void* user) : c(ctx) { c->ar_fn = fn; c->ar_user = user; }
  ~HookScope() { c->ar_fn = nullptr; c->ar_user = nullptr; c->ns = 0; }
};

// ---- shared by lvx_calibration_covariance and lvx_calibration_covariance_shared ----
// bit k: calibration scalar k is free
static uint32_t calib_free_mask(const lvx_ctx* c) {
  uint32_t m = 0;
  for (int k = 0; k < LVX_NCAL; ++k) if (c->ord[6 * (size_t)c->N + k] != LVX_DEAD) m |= 1u << k;
  return m;
}
template <class Rec> static void cov_free_index(uint32_t free_mask, Rec* out) {
  for (int k = 0; k < LVX_NCAL; ++k) if (free_mask >> k & 1u) out->free_index[out->n_free++] = k;
}
// the record's tail words as a status: tail[0] the Jacobi off-diagonal ratio, [1] sweeps, [2] the eigen-solver's code, [3] band pivot code, [4] first hub pivot, [5] its
// value; pivot_lost and min_eig are read where each call's record keeps them
static int cov_status(lvx_ctx* c, const double* tail, bool pivot_lost, double min_eig) {
  if (pivot_lost) return fail(c, LVX_E_NOTPD, "damped normal equations not positive definite (band pivot code " + std::to_string((int)tail[3]) + ", first hub pivot " + std::to_string((int)tail[4]) + " value " + std::to_string(tail[5]) + ")");
  if (tail[2] == 2.0) return fail(c, LVX_E_NOTPD, "marginal information of the calibration scalars has a non-positive eigenvalue " + std::to_string(min_eig));
  if (tail[2] != 0.0) { char buf[160]; snprintf(buf, sizeof buf, "Jacobi eigen-decomposition not converged after %d sweeps: max |t_pq| / sqrt(t_pp t_qq) = %.3e", (int)tail[1], tail[0]); return fail(c, LVX_E_NOTPD, buf); }
  return LVX_OK;
}

// ---- the Levenberg-Marquardt driver: what lvx_lm_solve_shared's loop carries out.  Every decision that needs no device is lvx_lm_policy.h's ----
struct LmRun {
  lvx_ctx* c; SolveWork& w; const lvx_lm_options& o;
  const bool joint;
  bool ls_on = false;     // the joint problem (or this single sequence) is constrained: every rank runs the line-search protocol
  double* x; double* xt;  // the iterate and the candidate (device)
  hipStream_t st; const int N, L;
  TrustRegion tr;
  double cost = 0;
  int it = 0;
  int pending = LVX_OK;   // a local failure (restoring the normal equations of x) that has not met a collective yet: voted in the next R1
  bool acc_is_x = true;   // the accumulators hold the normal equations of x (not of a candidate that was not accepted)
  bool restored = false;  // a restore ran since the last collective: if the loop ends now, its outcome has not been voted on yet
  lvx_lm_summary s{};
  LmRun(lvx_ctx* c_, SolveWork& w_, const lvx_lm_options& o_)
      : c(c_), w(w_), o(o_), joint(is_joint(c_)), x((double*)c_->d_state.p), xt((double*)c_->d_state_try.p), st(c_->stream), N(c_->N), L(c_->L), tr(o_) { s.termination = LVX_LM_NO_CONVERGENCE; }
  // one entry of the history lvx_lm_get_history returns: accepted (1) / rejected or not applied (0) / invalid (-1)
  void record(int flag) { c->lm_cost.push_back(cost); c->lm_radius.push_back(tr.radius); c->lm_accept.push_back(flag); }
  // the accumulators hold the candidate's normal equations: put those of x back (no reduction: every rank takes this branch together)
  void restore_x() { double cx = 0; const int re = lvx_evaluate_d(c, x, LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, &cx); if (re && !pending) pending = re; acc_is_x = re == 0; restored = true; }
};
// a sum over the ranks whose last slot v[n - 1] carries the error vote: when a rank failed, all leave together.  Single sequence: nothing to sum, the error itself
static int vote_sum(LmRun& r, double* v, int n, int err) {
  if (!r.joint) return err;
  v[n - 1] = err ? 1.0 : 0.0;
  int rc = reduce(r.c, v, n, LVX_REDUCE_SUM); if (rc) return rc;
  return leave_together(r.c, v[n - 1], err);
}
// x (+) w.delta -> dst, evaluated with cost (*f) AND normal equations: they replace those of x in the accumulators.  pre: an error the caller holds already (nothing is
// queued then).  Inside the joint protocol a local error must meet a collective, so every failure is RETURNED for the caller to vote, never acted on here.
//   h            the six sums k_plus leaves, cleared before and fetched after: step norm^2, x norm^2 over the free blocks, [4], [5] the shared blocks' halves of a joint
//                solve; fetched for a point that cannot be evaluated too (the parameter-tolerance test reads the candidate's norms whatever its cost).  Null: neither
//                cleared nor fetched (the start point's projection onto the box, whose norms nobody reads)
//   unevaluable  set when the point cannot be evaluated (*f = INFINITY: a rejected step, not an error); null: that is an error like any other
//   ev           the single sequence's hooked variant: what the loop wants on the host after the pass — its cost and error words, the sums, the candidate's diagonal and
//                gradient norm (local_after_eval: used if the step is accepted) — arrives with ONE host stop: the copies and the small kernels are queued from inside the
//                evaluation call, right before it waits (lvx_ctx::before_eval_sync).  *ev_done: they were.  The joint solve keeps its stops (its collectives sit between them)
static int try_step(LmRun& r, double* dst, int pre, double* f, double* h, bool* unevaluable = nullptr, EvalLocal* ev = nullptr, bool* ev_done = nullptr) {
  lvx_ctx* c = r.c; SolveWork& w = r.w;
  if (pre) return pre;
  if (h) LVX_HIP(c, hipMemsetAsync(w.sums + 2, 0, 48, r.st));
  hipLaunchKernelGGL(k_plus, dim3((unsigned)((r.N + 1 + r.L + 255) / 256)), dim3(256), 0, r.st, (const double*)r.x, (const double*)w.delta, r.N, r.L, c->locks, dst, w.sums, (h && r.joint) ? 1 : 0,
                     c->sensor_mto, w.tk ? w.tk + 7 : nullptr);
  bool hooked = false; int hook_rc = LVX_OK;
  if (ev) c->before_eval_sync = [&]() {
    hooked = true; hook_rc = LVX_OK;
    if (hipMemcpyAsync(c->pin + 16, w.sums + 2, 48, hipMemcpyDeviceToHost, r.st) != hipSuccess) hook_rc = LVX_E_HIP;
    if (!hook_rc) hook_rc = local_after_eval(c, w, ev, false);
  };
  int le = lvx_evaluate_d(c, dst, LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, f);
  c->before_eval_sync = nullptr;
  if (unevaluable) { *unevaluable = le == LVX_E_RANGE || le == LVX_E_NONUNIT_QUAT; if (*unevaluable) { *f = INFINITY; le = LVX_OK; } }
  if (!le && hooked && hook_rc) le = hook_rc;
  if (hooked && !hook_rc) { for (int q = 0; q < 6; ++q) h[q] = c->pin[16 + q]; local_collect(c, ev); }
  if (h && !le && !hooked && hipMemcpy(h, w.sums + 2, 48, hipMemcpyDeviceToHost) != hipSuccess) le = LVX_E_HIP;
  if (ev_done) *ev_done = hooked && !hook_rc;
  return le;
}
static int ls_hip(lvx_ctx* c, hipError_t e) { return e == hipSuccess ? LVX_OK : fail(c, LVX_E_HIP, std::string("line search: ") + hipGetErrorString(e)); }
// g . (the unscaled step dh) at the trial the accumulators hold: w.delta <- dh for the product, then back to the trial's scaled step dt
static int grad_dot_unscaled(LmRun& r, const std::vector<double>& dh, const std::vector<double>& dt, double* ga) {
  int le = ls_hip(r.c, hipMemcpyAsync(r.w.delta, dh.data(), dh.size() * 8, hipMemcpyHostToDevice, r.st));
  if (!le) le = grad_dot(r.c, r.w, ga);
  if (!le) le = ls_hip(r.c, hipMemcpyAsync(r.w.delta, dt.data(), dt.size() * 8, hipMemcpyHostToDevice, r.st));
  return le;
}
// Projected Armijo line search along the trust-region step of a constrained problem (ArmijoSearch decides, this evaluates).  In: the candidate of the full step — its
// cost *cand, its sums h, lerr its error so far — and g_delta = g . delta, the linear prediction.  Out: when a shorter step satisfies Armijo, w.delta (device) is that
// step, xt, the accumulators, *cand and h belong to it; otherwise the full step stays (Ceres leaves delta alone) and its candidate is put back.  *searched: a pass ran
// here, so what the candidate's own pass queued for local_after_eval is stale.
// Joint solve: every quantity the search decides on is the SUM over the ranks (costs, directional derivatives), so every rank contracts by the same factor; payloads
// {4, 2, 4 per trial, 1}, the last slot of each the error vote.  Inside the protocol a local HIP error is never returned: the peers would wait in the next reduction
// for ever.  It is kept, voted in the next collective, and every rank leaves together.  Returns non-zero when the solve ends here.
static int line_search(LmRun& r, double g_delta, int lerr, double* cand, double* h, bool* searched) {
  lvx_ctx* c = r.c; SolveWork& w = r.w;
  int rc;
  double cand_g = *cand, m0_g = g_delta;
  if (r.joint) {   // decide together: the candidate's JOINT cost against the joint linear prediction
    double b4[4] = {std::isfinite(*cand) ? *cand : 0.0, g_delta, std::isfinite(*cand) ? 0.0 : 1.0, 0.0};
    if (lerr) { b4[0] = b4[1] = b4[2] = 0.0; }
    if ((rc = vote_sum(r, b4, 4, lerr))) return rc;
    cand_g = b4[2] > 0.0 ? INFINITY : b4[0]; m0_g = b4[1];
  } else if (lerr) return LVX_OK;   // (the caller returns it)
  if (!ArmijoSearch::needed(r.cost, cand_g, m0_g)) return LVX_OK;
  *searched = true;
  double g1 = 0.0;
  { int le = grad_dot(c, w, &g1); double b2[2] = {le ? 0.0 : g1, 0.0}; if ((rc = vote_sum(r, b2, 2, le))) return rc; g1 = b2[0]; }
  const int ntg = lvx_tangent_size(c);
  std::vector<double> dh((size_t)ntg), dt((size_t)ntg);   // the full step, the trial's step
  int hip_ls = ls_hip(c, hipMemcpyAsync(dh.data(), w.delta, (size_t)ntg * 8, hipMemcpyDeviceToHost, r.st));
  if (!hip_ls) hip_ls = ls_hip(c, hipStreamSynchronize(r.st));
  // ArmijoLineSearch measures the step against ||direction||_inf; joint: the norm of the JOINT step (max over the ranks; the second slot carries the vote of a rank that failed)
  double dinf = 0.0;
  for (int i = 0; i < ntg; ++i) dinf = std::max(dinf, std::fabs(dh[i]));
  if (r.joint) {
    double dv[2] = {dinf, hip_ls ? 1.0 : 0.0};
    if ((rc = reduce(c, dv, 2, LVX_REDUCE_MAX))) return rc;
    if ((rc = leave_together(c, dv[1], hip_ls))) return rc;
    dinf = dv[0];
  } else if (hip_ls) return hip_ls;
  ArmijoSearch ls(r.cost, m0_g, cand_g, g1, dinf);
  bool found = false;
  for (double a = 1.0;;) {
    const int fitted = ls.trial;
    const bool go = ls.next(&a);
    if (r.o.verbose && ls.trial != fitted) fprintf(stderr, "[lvx lm] it %3d line search trial %d: f0 %.12e g0 %.12e | last step %.6e f %.12e df %.12e -> step %.12e\n", r.it, ls.trial, ls.f0, ls.g0, ls.cur.x, ls.cur.f, ls.cur.df, a);
    if (!go) break;
    for (int i = 0; i < ntg; ++i) dt[i] = a * dh[i];
    double f = 0, ga = 0.0, htr[6] = {0, 0, 0, 0, 0, 0};
    bool bad = false;   // a trial that cannot be evaluated: contract again without a new sample
    int le = try_step(r, r.xt, ls_hip(c, hipMemcpyAsync(w.delta, dt.data(), (size_t)ntg * 8, hipMemcpyHostToDevice, r.st)), &f, htr, &bad);
    // the directional derivative along the UNSCALED step is needed only when the trial fails Armijo.  Joint: taken with every trial, its sum rides on the trial's one
    // reduction; single sequence: taken AFTER the test, by the trials that fail it — two copies of the step, a k_gdot launch and a stream sync less per accepted trial
    if (r.joint && !le && !bad) le = grad_dot_unscaled(r, dh, dt, &ga);
    double b4[4] = {(le || bad) ? 0.0 : f, (le || bad) ? 0.0 : ga, bad ? 1.0 : 0.0, 0.0};
    if ((rc = vote_sum(r, b4, 4, le))) return rc;
    if (r.joint) bad = b4[2] > 0.0;
    if (!r.joint && !bad && !ls.armijo(b4[0]) && (rc = grad_dot_unscaled(r, dh, dt, &b4[1]))) return rc;
    if (ls.report(b4[0], b4[1], bad)) { *cand = f; for (int q = 0; q < 6; ++q) h[q] = htr[q]; found = true; break; }
  }
  if (!found) {   // no step satisfies Armijo: the full step stays — put its candidate back
    const int re = try_step(r, r.xt, ls_hip(c, hipMemcpyAsync(w.delta, dh.data(), (size_t)ntg * 8, hipMemcpyHostToDevice, r.st)), cand, h);
    double b1[1] = {0.0};
    if ((rc = vote_sum(r, b1, 1, re))) return rc;
  }
  return LVX_OK;
}
// R2, the joint solve's one reduction behind the candidate: the private blocks' terms summed over the ranks, the shared blocks' norms (identical on every rank: h[4],
// h[5]) added once.  r2: [g.delta, delta^T H delta, y^T D^2 y, candidate cost, step norm^2, x norm^2, error votes | the candidate's joint block].  Single sequence: nothing
// to reduce, the error itself
static int reduce_candidate(LmRun& r, int lerr, const EvalLocal& ev, const double* h, double* r2) {
  if (!r.joint) return lerr;
  int rc;
  r2[6] = lerr ? 1.0 : 0.0;
  if (lerr) { r2[0] = r2[1] = r2[2] = r2[3] = r2[4] = r2[5] = 0.0; for (int i = 0; i < LVX_JB_N; ++i) r2[7 + i] = 0.0; }
  else joint_block_pack(r.c, ev, r.o.gradient_tolerance, r2 + 7);
  if ((rc = reduce(r.c, r2, 7 + LVX_JB_N, LVX_REDUCE_SUM))) return rc;
  if ((rc = leave_together(r.c, r2[6], lerr))) return rc;
  r2[4] += h[4]; r2[5] += h[5];
  return LVX_OK;
}
// the defaults of the three covariance queries on the selected inverse (a template: outside the C linkage block)
template <class Opt>
static int cov_default_options(Opt* o) {
  if (!o) return LVX_E_ARG;
  o->radius = 1e8; o->jacobi_scaling = 1; o->reserved = 0;
  return LVX_OK;
}

extern "C" {

int lvx_lm_default_options(lvx_lm_options* o) {
  if (!o) return LVX_E_ARG;
  o->max_iterations = 50; o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32; o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->jacobi_scaling = 1; o->verbose = 0;
  return LVX_OK;
}

int lvx_solve_step_shared(lvx_ctx* c, double radius, int jacobi_scaling, lvx_allreduce_fn fn, void* user, double* delta, double* model_cost_change) {
  if (!c || !(radius > 0)) return LVX_E_ARG;
  if (!(c->last_what & LVX_EVAL_NORMAL_EQ)) return fail(c, LVX_E_STATE, "lvx_solve_step needs a preceding LVX_EVAL_NORMAL_EQ evaluation");
  LVX_HIP(c, hipSetDevice(c->device));
  int lerr = check_last_eval(c);   // an evaluation queued without a cost pointer has not had its device error word read yet
  HookScope hook(c, fn, user);
  SolveWork w;
  if (!lerr) lerr = solver_alloc(c, w);
  if (lerr && !is_joint(c)) return lerr;
  double cost = 0; bool gconv = false;
  int rc = post_eval(c, w, true, jacobi_scaling, 1e-6, 1e32, &cost, 0.0, &gconv, lerr); if (rc) return rc;
  double m[3]; bool notpd = false;
  if ((rc = solve_step_device(c, w, radius, m, &notpd, LVX_OK))) return rc;
  if ((rc = reduce(c, m, 3, LVX_REDUCE_SUM))) return rc;
  if (notpd) return LVX_E_NOTPD;
  if (model_cost_change) *model_cost_change = -m[0] - 0.5 * m[1];
  if (delta) LVX_HIP(c, hipMemcpy(delta, w.delta, (size_t)lvx_tangent_size(c) * 8, hipMemcpyDeviceToHost));
  return LVX_OK;
}
int lvx_solve_step(lvx_ctx* c, double radius, int jacobi_scaling, double* delta, double* model_cost_change) {
  return lvx_solve_step_shared(c, radius, jacobi_scaling, nullptr, nullptr, delta, model_cost_change);
}

int lvx_calib_cov_default_options(lvx_calib_cov_options* o) {
  if (!o) return LVX_E_ARG;
  o->radius = 1e8; o->jacobi_scaling = 1; o->max_sweeps = 30;
  return LVX_OK;
}
// lvx_solve_step's front half (diagonal, scale, damping, elimination down to the border system — from copies, so the stored normal equations stay), then k_calib_cov
// in place of the border factorisation.  The record and every pivot code come back in ONE copy: the only host stop.
int lvx_calibration_covariance(lvx_ctx* c, const lvx_calib_cov_options* opt, lvx_calib_cov* out) {
  if (!c || !opt || !out || !(opt->radius > 0) || opt->max_sweeps < 1) return LVX_E_ARG;
  if (!(c->last_what & LVX_EVAL_NORMAL_EQ)) return fail(c, LVX_E_STATE, "lvx_calibration_covariance needs a preceding LVX_EVAL_NORMAL_EQ evaluation");
  if (is_joint(c)) return fail(c, LVX_E_STATE, "lvx_calibration_covariance: the context takes part in a joint solve (the covariance of the shared extrinsics over the ranks is not computed)");
  LVX_HIP(c, hipSetDevice(c->device));
  int rc = check_last_eval(c); if (rc) return rc;
  SolveWork w;
  if ((rc = solver_alloc(c, w))) return rc;
  const int nb = c->nb, nbd = c->nbd, nh = nbd - LVX_NCAL;
  if (nh < 0 || nbd > 128) return fail(c, LVX_E_ARG, "lvx_calibration_covariance: border of " + std::to_string(nbd) + " scalars (22 .. 128 fit the one-workgroup kernel)");
  if ((rc = dev_alloc(c, c->d_ccov, (size_t)LVX_CCOV_N * 8))) return rc;
  hipStream_t st = c->stream;
  EvalLocal e; bool gconv = false;
  if ((rc = local_after_eval(c, w, &e, false))) return rc;   // the diagonal of THIS evaluation (queued; nothing of *e is used)
  if ((rc = apply_diag(c, w, true, opt->jacobi_scaling, 1e-6, 1e32, e, nullptr, 0.0, &gconv))) return rc;
  const uint32_t free_mask = calib_free_mask(c);
  std::vector<double> h(LVX_CCOV_N);
  StageTimer tm(c);
  const size_t lds = (size_t)nbd * (nbd + 1) * 8;
  LVX_HIP(c, hipFuncSetAttribute((const void*)k_calib_cov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  auto run = [&](bool force_seq, bool* bcr_used) -> int {
    w.lm_done = false;
    const int r = reduce_to_border(c, w, opt->radius, force_seq, bcr_used, tm); if (r) return r;
    hipLaunchKernelGGL(k_calib_cov, dim3(1), dim3(CCOV_NT), lds, st, (const double*)w.S, nbd, nh, (const double*)(w.scale + (nb + nh)), free_mask, (int)opt->max_sweeps, (const int*)w.info, (double*)c->d_ccov.p);
    LVX_HIP(c, hipGetLastError());
    LVX_HIP(c, hipMemcpyAsync(h.data(), c->d_ccov.p, (size_t)LVX_CCOV_N * 8, hipMemcpyDeviceToHost, st));
    LVX_HIP(c, hipStreamSynchronize(st));
    return LVX_OK;
  };
  bool bcr_used = false;
  if ((rc = run(false, &bcr_used))) return rc;
  const double* tail = h.data() + LVX_CCOV_N - 6;
  // a pivot lost in the reduction's elimination order: once more with the sequential band Cholesky, as lvx_solve_step does (switch TEST_BAD_PIVOT: the tests' way in)
  if (bcr_used && (tail[3] != 0.0 || tail[4] != 0.0 || tail[2] == 2.0 || c->sw.test_bad_pivot)) {
    ++c->solver_fallbacks;
    if ((rc = run(true, &bcr_used))) return rc;
  }
  if ((rc = cov_status(c, tail, tail[3] != 0.0 || tail[4] != 0.0, h[LVX_NCAL * LVX_NCAL + LVX_NCAL]))) return rc;
  std::memset(out, 0, sizeof *out);
  cov_free_index(free_mask, out);
  const double* p = h.data();
  std::memcpy(out->cov, p, sizeof out->cov); p += LVX_NCAL * LVX_NCAL;
  std::memcpy(out->sigma, p, sizeof out->sigma); p += LVX_NCAL;
  std::memcpy(out->info_eig, p, sizeof out->info_eig); p += LVX_NCAL;
  std::memcpy(out->info_vec, p, sizeof out->info_vec); p += LVX_NCAL * LVX_NCAL;
  std::memcpy(out->scale, p, sizeof out->scale);
  out->radius = opt->radius; out->sweeps = (int32_t)tail[1]; out->n_hub_eliminated = nh;
  return LVX_OK;
}

// ---- the covariance queries on the selected inverse: lvx_trajectory_covariance, lvx_landmark_covariance, lvx_map_point_covariance ----
int lvx_traj_cov_default_options(lvx_traj_cov_options* o) { return cov_default_options(o); }
int lvx_landmark_cov_default_options(lvx_landmark_cov_options* o) { return cov_default_options(o); }
int lvx_point_cov_default_options(lvx_point_cov_options* o) { return cov_default_options(o); }
// lvx_calibration_covariance's front half with the sequential band Cholesky forced, then the selected inverse of that factor (lvx_selinv.h): what
// the three queries share.  lowest(head) queues the kernel that lowers *head (started at nb) to the lowest band position a query
// needs; wide: the band store SigW (d <= TB, lvx_ctx::d_lcov) is written beside SigB.  Everything is queued.
struct SelInvOut { double* SigB; double* SigW; int TB; };
static int selinv_enqueue(lvx_ctx* c, const std::string& who, double radius, int scaling, bool wide, SolveWork& w, SelInvOut* so, const std::function<void(int*)>& lowest) {
  int rc;
  if ((rc = solver_alloc(c, w))) return rc;
  const int nb = c->nb, bw = c->bw, nbd = c->nbd;
  if (nbd > 96) return fail(c, LVX_E_ARG, who + ": border of " + std::to_string(nbd) + " scalars (up to 96 fit the one-workgroup inverse)");
  const int TB = si_tb(bw), R = TB + 16, mT = TB + si_up16(nbd), M = R + si_up16(nbd);
  const size_t lds_si = ((size_t)(16 + mT) * 17 + (size_t)32 * (mT + 1) + 3 * 16 * 17) * 8;
  if (nb > 0 && lds_si > 160 * 1024) return fail(c, LVX_E_ARG, who + ": half-bandwidth " + std::to_string(bw) + " too wide for the panel of the selected inverse");
  const size_t nb1 = (size_t)std::max(nb, 1);
  if ((rc = dev_alloc(c, c->d_tcov, (8 + nb1 * SI_BD + (size_t)M * M) * 8))) return rc;
  if (wide && (rc = dev_alloc(c, c->d_lcov, nb1 * (size_t)(TB + 1) * 8))) return rc;
  int* head = (int*)c->d_tcov.p; double* SigB = (double*)c->d_tcov.p + 8; double* D = SigB + nb1 * SI_BD;
  so->SigB = SigB; so->SigW = wide ? (double*)c->d_lcov.p : nullptr; so->TB = TB;
  hipStream_t st = c->stream;
  EvalLocal e; bool gconv = false;
  if ((rc = local_after_eval(c, w, &e, false))) return rc;   // the diagonal of THIS evaluation (queued; nothing of *e is used)
  if ((rc = apply_diag(c, w, true, scaling, 1e-6, 1e32, e, nullptr, 0.0, &gconv))) return rc;
  StageTimer tm(c);
  bool bcr_used = false;
  w.lm_done = false;
  if ((rc = reduce_to_border(c, w, radius, true, &bcr_used, tm))) return rc;
  const size_t lds_b = (size_t)2 * nbd * (nbd + 1) * 8;
  LVX_HIP(c, hipFuncSetAttribute((const void*)k_border_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
  hipLaunchKernelGGL(k_border_inv, dim3(1), dim3(SI_NT), lds_b, st, w.S, nbd, w.info);
  LVX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)head, nb, 1, st));
  if (nb > 0) {
    lowest(head);
    LVX_HIP(c, hipMemsetAsync(D, 0, (size_t)M * M * 8, st));
    SelInv g{(const double*)w.L, nb, bw, w.Z, w.ldz, nbd, (const double*)w.S, D, M, SigB, (const int*)head, (const int*)w.info, so->SigW};
    LVX_HIP(c, hipFuncSetAttribute((const void*)k_band_selinv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_si));
    hipLaunchKernelGGL(k_band_selinv, dim3(1), dim3(SI_NT), lds_si, st, g);
  }
  return LVX_OK;
}
// what a query's kernels read of the factored step: the band store is SigB (stride SI_BD) or SigW (stride TB + 1)
static SigmaView sigma_view(lvx_ctx* c, const SolveWork& w, const double* band, int stride) {
  return SigmaView{(const int*)c->d_ord.p, band, stride, (const double*)w.Z, w.ldz, c->nb, c->nbd, (const double*)w.S, (const double*)w.scale, (const int*)w.info, c->sw.test_bad_pivot ? 1 : 0};
}
// The checks the three queries make alike, in the order each of them always made its own: the context; the arguments (required_ok: the query's required pointers;
// reserved null: lvx_trajectory_covariance has never looked at opt->reserved, and still does not); own_arg, the query's own argument condition (its message, null when
// met); the preceding evaluation; the joint solve; own_state likewise; the device and the evaluation's error word.
static int cov_common_args(lvx_ctx* c, const std::string& who, bool required_ok, double radius, const int32_t* reserved, int n, const char* own_arg, const char* own_state) {
  if (!c) return LVX_E_ARG;
  if (!required_ok || n <= 0 || !(radius > 0) || (reserved && *reserved != 0))
    return fail(c, LVX_E_ARG, who + ": n <= 0, radius <= 0" + (reserved ? ", reserved != 0" : "") + " or a required pointer is NULL");
  if (own_arg) return fail(c, LVX_E_ARG, who + ": " + own_arg);
  if (!(c->last_what & LVX_EVAL_NORMAL_EQ) || !c->last_state_d) return fail(c, LVX_E_STATE, who + " needs a preceding LVX_EVAL_NORMAL_EQ evaluation");
  if (is_joint(c)) return fail(c, LVX_E_STATE, who + ": the context takes part in a joint solve");
  if (own_state) return fail(c, LVX_E_STATE, who + ": " + own_state);
  LVX_HIP(c, hipSetDevice(c->device));
  return check_last_eval(c);
}
// The flag words of a _d form: those of the _d trajectory queries (lvx_traj.hip), kept until lvx_synchronize looks.
static int cov_d_flags(lvx_ctx* c, int** flags) {
  int rc = traj_flag_words(c);
  if (rc) return rc;
  c->tcov_d_unchecked = true;
  *flags = (int*)c->d_tj[3].p + 1;
  return LVX_OK;
}
// The staging of a host form (lvx_ctx::d_cov_io and its pinned mirror h_cov, shared by the three queries): [inputs | outputs | 2 flag words], every array on a 16-byte
// boundary.  An array the caller does not give (h null) takes no bytes, has no device address and is not computed.  cov_stage lays the arrays out, grows the two
// buffers, uploads the inputs in one copy and clears the flags; behind the query's enqueue cov_finish brings outputs, flags and pivot codes back — the one host stop —
// and turns the flags into the return code.
struct CovArr { void* h; size_t bytes; };
struct CovStage { enum { MAX = 12 }; int n, nin; void* h[MAX]; size_t bytes[MAX], off[MAX + 1], total; void* d[MAX]; int* flags; };
static int cov_stage(lvx_ctx* c, std::initializer_list<CovArr> in, std::initializer_list<CovArr> out, CovStage* s) {
  int rc;
  s->n = 0; s->nin = (int)in.size();
  size_t cur = 0;
  for (const auto* list : {&in, &out})
    for (const CovArr& a : *list) { const int k = s->n++; s->h[k] = a.h; s->bytes[k] = a.h ? a.bytes : 0; s->off[k] = cur; cur += (s->bytes[k] + 15) & ~(size_t)15; }
  s->off[s->n] = cur; s->total = cur + 16;
  if ((rc = dev_alloc(c, c->d_cov_io, s->total))) return rc;
  if (c->h_cov_cap < s->total) {
    if (c->h_cov) { (void)hipHostFree(c->h_cov); c->h_cov = nullptr; c->h_cov_cap = 0; }
    LVX_HIP(c, hipHostMalloc(&c->h_cov, s->total, hipHostMallocDefault));
    c->h_cov_cap = s->total;
  }
  char* d = (char*)c->d_cov_io.p; char* h = (char*)c->h_cov;
  for (int k = 0; k < s->n; ++k) s->d[k] = s->bytes[k] ? d + s->off[k] : nullptr;
  s->flags = (int*)(d + cur);
  for (int k = 0; k < s->nin; ++k) if (s->bytes[k]) std::memcpy(h + s->off[k], s->h[k], s->bytes[k]);
  if (s->off[s->nin]) LVX_HIP(c, hipMemcpyAsync(d, h, s->off[s->nin], hipMemcpyHostToDevice, c->stream));
  LVX_HIP(c, hipMemsetAsync(s->flags, 0, 16, c->stream));
  return LVX_OK;
}
// off_border: the message of flags[1] == 2 (lvx_map_point_covariance: the window of t_map is off the border), null for a query without that status
static int cov_finish(lvx_ctx* c, const CovStage& s, const char* off_border = nullptr) {
  hipStream_t st = c->stream;
  const size_t o0 = s.off[s.nin];
  char* d = (char*)c->d_cov_io.p; char* h = (char*)c->h_cov;
  LVX_HIP(c, hipMemcpyAsync(h + o0, d + o0, s.total - o0, hipMemcpyDeviceToHost, st));
  LVX_HIP(c, hipMemcpyAsync(c->pin + 48, (const double*)c->d_scal.p + 32, 16, hipMemcpyDeviceToHost, st));   // the pivot codes (SolveWork::info), for the message
  LVX_HIP(c, hipStreamSynchronize(st));   // the one host stop
  int fl[2]; std::memcpy(fl, h + s.off[s.n], 8);
  if (fl[1] == 2 && off_border) return fail(c, LVX_E_STATE, off_border);
  if (fl[1]) {
    int info[4]; std::memcpy(info, c->pin + 48, 16); double dv; std::memcpy(&dv, info + 2, 8);
    return fail(c, LVX_E_NOTPD, "damped normal equations not positive definite (band pivot code " + std::to_string(info[0]) + ", first border pivot " + std::to_string(info[1]) + " value " + std::to_string(dv) + ")");
  }
  for (int k = s.nin; k < s.n; ++k) if (s.bytes[k]) std::memcpy(s.h[k], h + s.off[k], s.bytes[k]);
  if (fl[0]) return fail(c, LVX_E_NONUNIT_QUAT, "logq: only implemented for unit quaternions");
  return LVX_OK;
}
// One wavefront per query behind the selected inverse: t_d and the arrays of o are device addresses; flags[0] takes RES_NONUNIT, flags[1] a lost pivot (nothing
// written then).
static int traj_cov_enqueue(lvx_ctx* c, const lvx_traj_cov_options* opt, int frame, int n, const double* t_d, const lvx_traj_cov& o, int* flags) {
  int rc;
  SolveWork w; SelInvOut so;
  hipStream_t st = c->stream;
  const double* state_d = c->last_state_d;
  if ((rc = selinv_enqueue(c, "lvx_trajectory_covariance", opt->radius, opt->jacobi_scaling, false, w, &so, [&](int* head) {
        hipLaunchKernelGGL(k_tc_lowest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, state_d, c->N, c->t0, c->dt, frame, n, t_d, (const int*)c->d_ord.p, head); }))) return rc;
  PoseCov p{state_d, c->N, c->t0, c->dt, frame, n, t_d, sigma_view(c, w, so.SigB, SI_BD), o.cov, o.sigma, o.window_cov, o.window_idx, o.valid, flags, flags + 1};
  { ProfScope ps(c, LVX_KERNEL_POSE_COV); hipLaunchKernelGGL(k_pose_cov, dim3((unsigned)n), dim3(64), 0, st, p); }
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
static int traj_cov_args(lvx_ctx* c, const lvx_traj_cov_options* opt, int frame, int n, const double* t, const lvx_traj_cov* out) {
  const bool known = frame == LVX_FRAME_TRAJECTORY || frame == LVX_FRAME_LIDAR || frame == LVX_FRAME_CAMERA;
  return cov_common_args(c, "lvx_trajectory_covariance", opt && t && out && out->valid, opt ? opt->radius : 0.0, nullptr, n, known ? nullptr : "unknown frame", nullptr);
}
int lvx_trajectory_covariance_d(lvx_ctx* c, const lvx_traj_cov_options* opt, int frame, int n, const double* t_d, const lvx_traj_cov* out_d) {
  int rc = traj_cov_args(c, opt, frame, n, t_d, out_d);
  int* flags;
  if (rc || (rc = cov_d_flags(c, &flags))) return rc;
  return traj_cov_enqueue(c, opt, frame, n, t_d, *out_d, flags);
}
int lvx_trajectory_covariance(lvx_ctx* c, const lvx_traj_cov_options* opt, int frame, int n, const double* t, lvx_traj_cov* out) {
  int rc = traj_cov_args(c, opt, frame, n, t, out);
  if (rc) return rc;
  const size_t nn = (size_t)n, W2 = (size_t)LVX_TRAJ_COV_W * LVX_TRAJ_COV_W;
  CovStage s;
  if ((rc = cov_stage(c, {{(void*)t, nn * 8}},
                      {{out->cov, nn * 36 * 8}, {out->sigma, nn * 6 * 8}, {out->window_cov, nn * W2 * 8}, {out->window_idx, nn * LVX_TRAJ_COV_W * 4}, {out->valid, nn}}, &s))) return rc;
  const lvx_traj_cov od{(double*)s.d[1], (double*)s.d[2], (double*)s.d[3], (int32_t*)s.d[4], (uint8_t*)s.d[5]};
  if ((rc = traj_cov_enqueue(c, opt, frame, n, (const double*)s.d[0], od, s.flags))) return rc;
  return cov_finish(c, s);
}

// The selected inverse with the wide band store, then one wavefront per queried landmark (k_landmark_cov).  ids_d (device, or null for 0 .. n - 1) and the arrays of o
// are device addresses; flags as traj_cov_enqueue's.
static int lm_cov_enqueue(lvx_ctx* c, const lvx_landmark_cov_options* opt, int n, const int32_t* ids_d, const lvx_landmark_cov& o, int* flags) {
  int rc;
  SolveWork w; SelInvOut so;
  hipStream_t st = c->stream;
  LmQuery q{};
  q.state = c->last_state_d; q.N = c->N; q.t0 = c->t0; q.dt = c->dt; q.cam = c->cam; q.lm_uv = (const double*)c->d_lm_uv.p; q.lm_t0 = (const double*)c->d_lm_t0.p; q.L = c->L;
  q.ord = (const int*)c->d_ord.p; q.p0s = (const int*)c->d_lm_p0.p; q.wl = c->lm_wl; q.nbd_ext = c->nbd_ext; q.ls = c->lm_ls; q.n = n; q.ids = ids_d;
  if ((rc = selinv_enqueue(c, "lvx_landmark_covariance", opt->radius, opt->jacobi_scaling, true, w, &so, [&](int* head) {
        q.lmH = w.lm ? (const double*)c->d_lmH.p : nullptr;
        hipLaunchKernelGGL(k_lc_lowest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, head); }))) return rc;
  q.lmH = w.lm ? (const double*)c->d_lmH.p : nullptr;
  LmCov g{q, sigma_view(c, w, so.SigW, so.TB + 1), (const double*)w.lmd, 1.0 / opt->radius, o.var_rho, o.sigma_rho, o.point, o.point_cov, o.window_cov, o.window_idx, o.valid, flags, flags + 1};
  const size_t lds = (size_t)(c->lm_wl + c->nbd) * 12 + 16;
  hipLaunchKernelGGL(k_landmark_cov, dim3((unsigned)n), dim3(64), lds, st, g);
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
static int lm_cov_args(lvx_ctx* c, const lvx_landmark_cov_options* opt, int n, const lvx_landmark_cov* out) {
  return cov_common_args(c, "lvx_landmark_covariance", opt && out && out->valid, opt ? opt->radius : 0.0, opt ? &opt->reserved : nullptr, n,
                         c && n > c->L ? "n exceeds the number of landmarks" : nullptr, nullptr);
}
int lvx_landmark_covariance_d(lvx_ctx* c, const lvx_landmark_cov_options* opt, int n, const int32_t* landmark_id_d, const lvx_landmark_cov* out_d) {
  int rc = lm_cov_args(c, opt, n, out_d);
  int* flags;
  if (rc || (rc = cov_d_flags(c, &flags))) return rc;
  return lm_cov_enqueue(c, opt, n, landmark_id_d, *out_d, flags);
}
int lvx_landmark_covariance(lvx_ctx* c, const lvx_landmark_cov_options* opt, int n, const int32_t* landmark_id, lvx_landmark_cov* out) {
  int rc = lm_cov_args(c, opt, n, out);
  if (rc) return rc;
  if (landmark_id) for (int i = 0; i < n; ++i) if (landmark_id[i] < 0 || landmark_id[i] >= c->L) return fail(c, LVX_E_ARG, "lvx_landmark_covariance: landmark id out of range");
  const size_t nn = (size_t)n, W2 = (size_t)LVX_LM_COV_W * LVX_LM_COV_W;
  CovStage s;
  if ((rc = cov_stage(c, {{(void*)landmark_id, nn * 4}},
                      {{out->var_rho, nn * 8}, {out->sigma_rho, nn * 8}, {out->point, nn * 24}, {out->point_cov, nn * 72}, {out->window_cov, nn * W2 * 8},
                       {out->window_idx, nn * LVX_LM_COV_W * 4}, {out->valid, nn}}, &s))) return rc;
  const lvx_landmark_cov od{(double*)s.d[1], (double*)s.d[2], (double*)s.d[3], (double*)s.d[4], (double*)s.d[5], (int32_t*)s.d[6], (uint8_t*)s.d[7]};
  if ((rc = lm_cov_enqueue(c, opt, n, (const int32_t*)s.d[0], od, s.flags))) return rc;
  return cov_finish(c, s);
}

// The selected inverse down to the lowest band position a point's window holds (k_tc_lowest in the LiDAR frame), k_pt_hub once, then k_point_cov with a lane per
// point.  pt_d [n][3] or xyzi_d [n][4] float, t_d, dir_d (or null) and the arrays of o are device addresses; flags as traj_cov_enqueue's, flags[1] = 2 when the window of
// t_map is off the border.
static int pt_cov_enqueue(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const double* pt_d, const float* xyzi_d, const double* t_d, const double* dir_d, const lvx_point_cov& o,
                          int* flags) {
  int rc;
  SolveWork w; SelInvOut so;
  hipStream_t st = c->stream;
  const double* state_d = c->last_state_d;
  if ((rc = dev_alloc(c, c->d_ptcov, sizeof(PtHub)))) return rc;
  if ((rc = selinv_enqueue(c, "lvx_map_point_covariance", opt->radius, opt->jacobi_scaling, false, w, &so, [&](int* head) {
        hipLaunchKernelGGL(k_tc_lowest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, state_d, c->N, c->t0, c->dt, (int)LVX_FRAME_LIDAR, n, t_d, (const int*)c->d_ord.p, head); }))) return rc;
  PtCov g{};
  g.state = state_d; g.N = c->N; g.t0 = c->t0; g.dt = c->dt; g.t_map = c->t_map; g.n = n; g.pt = pt_d; g.xyzi = xyzi_d; g.t = t_d; g.dir = dir_d;
  g.v = sigma_view(c, w, so.SigB, SI_BD); g.hub = (PtHub*)c->d_ptcov.p;
  g.point = o.point; g.cov = o.cov; g.sigma = o.sigma; g.sigma_max = o.sigma_max; g.var_dir = o.var_dir; g.wcov = o.window_cov; g.widx = o.window_idx; g.valid = o.valid;
  g.flag = flags; g.bad = flags + 1;
  const size_t lds = (size_t)(PC_NT / 64) * 16 * PC_TS * 8;   // the wavefronts' tiles of the MFMA product
  const dim3 grid((unsigned)(((size_t)n + PC_NT - 1) / PC_NT));
  LVX_HIP(c, hipFuncSetAttribute((const void*)k_point_cov<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  {
    ProfScope ps(c, LVX_KERNEL_POINT_COV);
    hipLaunchKernelGGL(k_pt_hub, dim3(1), dim3(64), 0, st, g);
    if (c->sw.ptcov_valu) hipLaunchKernelGGL(k_point_cov<false>, grid, dim3(PC_NT), 0, st, g);
    else hipLaunchKernelGGL(k_point_cov<true>, grid, dim3(PC_NT), lds, st, g);
  }
  LVX_HIP(c, hipGetLastError());
  return LVX_OK;
}
static int pt_cov_args(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const void* pt, const double* t, const lvx_point_cov* out) {
  const bool no_hub = c && ((c->surf.n <= 0 && c->cs.n <= 0) || c->n_hub <= 0);
  return cov_common_args(c, "lvx_map_point_covariance", opt && pt && t && out && out->valid, opt ? opt->radius : 0.0, opt ? &opt->reserved : nullptr, n,
                         nullptr, no_hub ? "no surfel / camera-surfel family has set t_map" : nullptr);
}
static int pt_cov_d(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const double* pt_d, const float* xyzi_d, const double* t_d, const double* dir_d, const lvx_point_cov* out_d) {
  int rc = pt_cov_args(c, opt, n, pt_d ? (const void*)pt_d : (const void*)xyzi_d, t_d, out_d);
  int* flags;
  if (rc || (rc = cov_d_flags(c, &flags))) return rc;
  return pt_cov_enqueue(c, opt, n, pt_d, xyzi_d, t_d, dir_d, *out_d, flags);
}
int lvx_map_point_covariance_d(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const double* pt3_d, const double* t_d, const double* dir3_d, const lvx_point_cov* out_d) {
  return pt_cov_d(c, opt, n, pt3_d, nullptr, t_d, dir3_d, out_d);
}
int lvx_map_point_covariance_xyzi_d(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const float* xyzi4_d, const double* t_d, const lvx_point_cov* out_d) {
  return pt_cov_d(c, opt, n, nullptr, xyzi4_d, t_d, nullptr, out_d);
}
int lvx_map_point_covariance(lvx_ctx* c, const lvx_point_cov_options* opt, int n, const double* pt_lidar3, const double* t, const double* dir3, lvx_point_cov* out) {
  int rc = pt_cov_args(c, opt, n, pt_lidar3, t, out);
  if (rc) return rc;
  const size_t nn = (size_t)n, W2 = (size_t)LVX_PT_COV_W * LVX_PT_COV_W;
  const bool vd = dir3 && out->var_dir;   // the directions travel only when their variances are asked for, and the reverse
  CovStage s;
  if ((rc = cov_stage(c, {{(void*)pt_lidar3, nn * 24}, {(void*)t, nn * 8}, {vd ? (void*)dir3 : nullptr, nn * 24}},
                      {{out->point, nn * 24}, {out->cov, nn * 72}, {out->sigma, nn * 24}, {out->sigma_max, nn * 8}, {vd ? out->var_dir : nullptr, nn * 8}, {out->window_cov, nn * W2 * 8},
                       {out->window_idx, nn * LVX_PT_COV_W * 4}, {out->valid, nn}}, &s))) return rc;
  const lvx_point_cov od{(double*)s.d[3], (double*)s.d[4], (double*)s.d[5], (double*)s.d[6], (double*)s.d[7], (double*)s.d[8], (int32_t*)s.d[9], (uint8_t*)s.d[10]};
  if ((rc = pt_cov_enqueue(c, opt, n, (const double*)s.d[0], nullptr, (const double*)s.d[1], (const double*)s.d[2], od, s.flags))) return rc;
  return cov_finish(c, s, "lvx_map_point_covariance: a free scalar of the pose at t_map is a band position of the factor (its cross terms are off the pattern)");
}

// lvx_projection_covariance.  The selected inverse down to the lowest band position an image's camera window holds (k_tc_lowest in the camera frame; the window of
// t_map stands in the border), the table's poses, k_proj_hub with a wavefront per image, then k_proj_cov with a lane per point.  xyzi_d [n][4] float, image_t_d and
// the arrays of img / o are device addresses; flags as pt_cov_enqueue's.
int lvx_proj_cov_default_options(lvx_proj_cov_options* o) {
  const int rc = cov_default_options(o);
  if (rc) return rc;
  o->z_min = 0.1; o->z_max = 15.0;   // lvx_render_default_options'
  return LVX_OK;
}
static int proj_cov_enqueue_all(lvx_ctx* c, const lvx_proj_cov_options* opt, long long n, const float* xyzi_d, int n_images, const double* image_t_d, const lvx_proj_cov_images& img,
                                const lvx_proj_cov& o, int* flags) {
  int rc;
  SolveWork w; SelInvOut so;
  hipStream_t st = c->stream;
  const double* state_d = c->last_state_d;
  if ((rc = dev_alloc(c, c->d_projcov, sizeof(ProjTable)))) return rc;
  if ((rc = selinv_enqueue(c, "lvx_projection_covariance", opt->radius, opt->jacobi_scaling, false, w, &so, [&](int* head) {
        hipLaunchKernelGGL(k_tc_lowest, dim3(1), dim3(64), 0, st, state_d, c->N, c->t0, c->dt, (int)LVX_FRAME_CAMERA, n_images, image_t_d, (const int*)c->d_ord.p, head); }))) return rc;
  ProjTable* tab = (ProjTable*)c->d_projcov.p;
  ProjHub g{state_d, c->N, c->t0, c->dt, c->t_map, n_images, image_t_d, sigma_view(c, w, so.SigB, SI_BD), tab, img.pose_cov, img.window_cov, img.window_idx, img.valid, flags, flags + 1};
  {
    ProfScope ps(c, LVX_KERNEL_PROJ_HUB);
    if ((rc = proj_poses_enqueue(c, state_d, c->t_map, n_images, image_t_d, tab))) return rc;
    hipLaunchKernelGGL(k_proj_hub, dim3((unsigned)n_images), dim3(64), 0, st, g);
  }
  LVX_HIP(c, hipGetLastError());
  ProfScope ps(c, LVX_KERNEL_PROJ_COV);
  return proj_cov_enqueue(c, n, xyzi_d, tab, opt->z_min, opt->z_max, o.uv, o.cov, o.sigma, o.sigma_max, o.image, o.status);
}
static int proj_cov_args(lvx_ctx* c, const lvx_proj_cov_options* opt, int n, bool cloud_ok, int n_images, const double* image_t, const lvx_proj_cov_images* img, const lvx_proj_cov* out) {
  const bool no_hub = c && ((c->surf.n <= 0 && c->cs.n <= 0) || c->n_hub <= 0);
  const bool no_cam = c && (c->cam.rows <= 0 || c->cam.cols <= 0);
  const char* own_arg = (n_images < 1 || n_images > LVX_RENDER_MAX_IMAGES) ? "1 .. 32 images per call" : (opt && opt->z_min > opt->z_max ? "z_min > z_max" : nullptr);
  return cov_common_args(c, "lvx_projection_covariance", opt && cloud_ok && image_t && img && img->valid && out && out->status, opt ? opt->radius : 0.0, opt ? &opt->reserved : nullptr, n,
                         own_arg, no_cam ? "lvx_set_camera has not been called" : (no_hub ? "no surfel / camera-surfel family has set t_map" : nullptr));
}
int lvx_projection_covariance_d(lvx_ctx* c, const lvx_proj_cov_options* opt, int n, const float* map_xyzi4_d, int n_images, const double* image_t_d, const lvx_proj_cov_images* img_d,
                                const lvx_proj_cov* out_d) {
  int rc = proj_cov_args(c, opt, map_xyzi4_d ? n : 1, true, n_images, image_t_d, img_d, out_d);
  if (rc) return rc;
  long long np = n;
  if (!map_xyzi4_d) {   // the cloud the last association left on the device, as lvx_render_map_d
    np = (long long)c->da_S * c->da_H * c->da_W;
    if (np == 0 || !c->d_da[4].p || c->d_da[4].bytes < (size_t)np * 16) return fail(c, LVX_E_STATE, "lvx_projection_covariance_d: lvx_data_association has not been called");
    map_xyzi4_d = (const float*)c->d_da[4].p;
  }
  int* flags;
  if ((rc = cov_d_flags(c, &flags))) return rc;
  return proj_cov_enqueue_all(c, opt, np, map_xyzi4_d, n_images, image_t_d, *img_d, *out_d, flags);
}
int lvx_projection_covariance(lvx_ctx* c, const lvx_proj_cov_options* opt, int n, const float* map_xyzi4, int n_images, const double* image_t, const lvx_proj_cov_images* img,
                              const lvx_proj_cov* out) {
  int rc = proj_cov_args(c, opt, n, map_xyzi4 != nullptr, n_images, image_t, img, out);
  if (rc) return rc;
  const size_t nn = (size_t)n, ni = (size_t)n_images, W2 = (size_t)LVX_PROJ_COV_W * LVX_PROJ_COV_W;
  CovStage s;
  if ((rc = cov_stage(c, {{(void*)map_xyzi4, nn * 16}, {(void*)image_t, ni * 8}},
                      {{img->pose_cov, ni * 144 * 8}, {img->window_cov, ni * W2 * 8}, {img->window_idx, ni * LVX_PROJ_COV_W * 4}, {img->valid, ni * 4},
                       {out->uv, nn * 16}, {out->cov, nn * 32}, {out->sigma, nn * 16}, {out->sigma_max, nn * 8}, {out->image, nn * 4}, {out->status, nn}}, &s))) return rc;
  const lvx_proj_cov_images id{(double*)s.d[2], (double*)s.d[3], (int32_t*)s.d[4], (int32_t*)s.d[5]};
  const lvx_proj_cov od{(double*)s.d[6], (double*)s.d[7], (double*)s.d[8], (double*)s.d[9], (int32_t*)s.d[10], (uint8_t*)s.d[11]};
  if ((rc = proj_cov_enqueue_all(c, opt, n, (const float*)s.d[0], n_images, (const double*)s.d[1], id, od, s.flags))) return rc;
  return cov_finish(c, s, "lvx_projection_covariance: a free scalar of the pose at t_map is a band position of the factor (its cross terms are off the pattern)");
}

// The covariance of the JOINT problem: lvx_solve_step_shared's front half (the diagonal collective puts the joint diagonal at the shared slots and withholds their
// damping), the elimination down to the border system from copies, then k_joint_cov_local -> ONE sum over the ranks -> k_joint_cov_shared.  Two collectives per call;
// every failure is voted in the collective that follows it, so all ranks leave together.  With RCCL everything behind the diagonal collective is queued on the stream
// and the record comes back in one copy: one host stop.  A pivot lost on the reduction route of ANY rank: every rank repeats the second half sequentially (a third
// collective, as rare as the fallback of lvx_solve_step).
static int identity_allreduce(void*, double*, int, int) { return 0; }
int lvx_calibration_covariance_shared(lvx_ctx* c, const lvx_calib_cov_options* opt, lvx_allreduce_fn fn, void* user, lvx_joint_calib_cov* out) {
  if (!c || !opt || !out || !(opt->radius > 0) || opt->max_sweeps < 1) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  HookScope hook(c, (fn || c->rccl_comm) ? fn : identity_allreduce, user);   // no transport: a joint problem of one rank
  int lerr = LVX_OK;
  double no_eval = 0.0;
  if (!(c->last_what & LVX_EVAL_NORMAL_EQ)) { lerr = fail(c, LVX_E_STATE, "lvx_calibration_covariance_shared needs a preceding LVX_EVAL_NORMAL_EQ evaluation"); no_eval = 1.0; }
  if (!lerr) lerr = check_last_eval(c);
  SolveWork w;
  if (!lerr) lerr = solver_alloc(c, w);
  const int nb = c->nb, nbd = c->nbd, nh = nbd - LVX_NCAL;
  if (!lerr && (nh < 0 || nbd > 128)) lerr = fail(c, LVX_E_ARG, "lvx_calibration_covariance_shared: border of " + std::to_string(nbd) + " scalars (22 .. 128 fit the one-workgroup kernel)");
  if (!lerr) lerr = dev_alloc(c, c->d_ccov, (size_t)(LVX_JREC_N + LVX_JKEEP_N + LVX_JC_N) * 8);
  double cost = 0.0; bool gconv = false;
  int rc = post_eval(c, w, true, opt->jacobi_scaling, 1e-6, 1e32, &cost, 0.0, &gconv, lerr, &no_eval);
  if (no_eval > 0.0) return lerr == LVX_E_STATE ? lerr : fail(c, LVX_E_STATE, "lvx_calibration_covariance_shared: a rank of the joint problem has no preceding LVX_EVAL_NORMAL_EQ evaluation");
  if (rc) return rc;
  hipStream_t st = c->stream;
  const uint32_t free_mask = calib_free_mask(c);
  double* rec = (double*)c->d_ccov.p, *keep = rec + LVX_JREC_N;
  double* msg = c->rccl_comm ? (double*)c->d_comm.p : keep + LVX_JKEEP_N;   // RCCL reduces in its staging buffer; the callback's message is staged through the host
  JointLmd lmd{};
  for (int a = 0; a < LVX_N_SHARED; ++a) lmd.v[a] = c->sh_lmd[a];
  const int sweep_slot = std::min((int)opt->max_sweeps, LVX_JC_SWEEP_SLOTS) - 1;
  std::vector<double> h(LVX_JREC_N), hm(LVX_JC_N);
  StageTimer tm(c);
  const size_t lds = (size_t)nbd * (nbd + 1) * 8;
  LVX_HIP(c, hipFuncSetAttribute((const void*)k_joint_cov_local, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const double* tail = h.data() + LVX_JREC_TAIL;
  auto run = [&](bool force_seq, bool* bcr_used) -> int {
    w.lm_done = false;
    const int lrc = reduce_to_border(c, w, opt->radius, force_seq, bcr_used, tm);   // a local failure is voted: nobody waits in the sum
    if (lrc) hipLaunchKernelGGL(k_joint_cov_local, dim3(1), dim3(CCOV_NT), 0, st, (const double*)nullptr, nbd, nh, free_mask, sweep_slot, 1.0, 0.0, 0.0, (const int*)nullptr, msg, keep, rec);
    else hipLaunchKernelGGL(k_joint_cov_local, dim3(1), dim3(CCOV_NT), lds, st, (const double*)w.S, nbd, nh, free_mask, sweep_slot, 0.0, (*bcr_used && c->sw.test_bad_pivot) ? 1.0 : 0.0,
                            *bcr_used ? 1.0 : 0.0, (const int*)w.info, msg, keep, rec);
    int r2;
    if (c->rccl_comm) { if ((r2 = reduce_device(c, LVX_JC_N, LVX_REDUCE_SUM))) return r2; }
    else {
      LVX_HIP(c, hipMemcpyAsync(hm.data(), msg, (size_t)LVX_JC_N * 8, hipMemcpyDeviceToHost, st));
      LVX_HIP(c, hipStreamSynchronize(st));
      if ((r2 = reduce(c, hm.data(), LVX_JC_N, LVX_REDUCE_SUM))) return r2;
      LVX_HIP(c, hipMemcpyAsync(msg, hm.data(), (size_t)LVX_JC_N * 8, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_joint_cov_shared, dim3(1), dim3(CCOV_NT), 0, st, (const double*)msg, (const double*)keep, lmd, 1.0 / opt->radius, (const double*)(w.scale + (nb + nh)), free_mask, rec);
    LVX_HIP(c, hipGetLastError());
    LVX_HIP(c, hipMemcpyAsync(h.data(), rec, (size_t)LVX_JREC_N * 8, hipMemcpyDeviceToHost, st));
    LVX_HIP(c, hipStreamSynchronize(st));
    return leave_together(c, tail[8], lrc);
  };
  bool bcr_used = false;
  if ((rc = run(false, &bcr_used))) return rc;
  if (tail[9] > 0.0 && (tail[7] > 0.0 || tail[2] == 2.0)) {   // decided on reduced words: every rank repeats, the ones that were sequential already included
    if (bcr_used) ++c->solver_fallbacks;
    if ((rc = run(true, &bcr_used))) return rc;
  }
  if (tail[2] == 3.0) return fail(c, LVX_E_ARG, "lvx_calibration_covariance_shared: a shared extrinsic scalar is locked on some ranks and free on others");
  if ((rc = cov_status(c, tail, tail[7] > 0.0, h[LVX_JREC_W]))) return rc;
  std::memset(out, 0, sizeof *out);
  cov_free_index(free_mask, out);
  for (int a = 0; a < LVX_N_SHARED; ++a) if (free_mask >> (LVX_NPRIV + a) & 1u) out->shared_free_slot[out->n_shared_free++] = a;
  std::memcpy(out->cov, h.data() + LVX_JREC_COV, sizeof out->cov);
  std::memcpy(out->sigma, h.data() + LVX_JREC_SIG, sizeof out->sigma);
  std::memcpy(out->info_eig, h.data() + LVX_JREC_W, sizeof out->info_eig);
  std::memcpy(out->info_vec, h.data() + LVX_JREC_V, sizeof out->info_vec);
  std::memcpy(out->own_info, h.data() + LVX_JREC_OWN, sizeof out->own_info);
  std::memcpy(out->scale, h.data() + LVX_JREC_SCALE, sizeof out->scale);
  out->radius = opt->radius; out->sweeps = (int32_t)tail[1]; out->n_hub_eliminated = nh; out->world = (int32_t)tail[6];
  return LVX_OK;
}

// Collectives of the joint loop: one after the first evaluation, then exactly TWO per iteration —
//   R1 [S | rhs | votes] inside solve_step_device (the reduced 14 x 14 system),
//   R2 after the candidate evaluation: [g.delta, delta^T H delta, y^T D^2 y, candidate cost, step norm^2, x norm^2, error votes | the candidate's joint block].
// (R1 and R2 cannot merge: the candidate is a function of the reduced system's solution.)  The candidate is evaluated WITH its normal equations: an accepted step — the
// rule — needs nothing more (the reference's loop evaluates the Jacobian only after acceptance; here acceptance is what a second pass and two more reductions used to
// follow), a rejected one restores the normal equations of x with one more pass and no reduction (every rank rejects together).
int lvx_lm_solve_shared(lvx_ctx* c, double* state, const lvx_lm_options* opt_in, lvx_allreduce_fn fn, void* user, lvx_lm_summary* sum) {
  if (!c || !state) return LVX_E_ARG;
  lvx_lm_options o; lvx_lm_default_options(&o); if (opt_in) o = *opt_in;
  LVX_HIP(c, hipSetDevice(c->device));
  HookScope hook(c, fn, user);
  const bool joint = is_joint(c);
  int rc;
  int lerr = ensure_layout(c);
  SolveWork w;
  if (!lerr) lerr = solver_alloc(c, w, /*will_inplace=*/!joint && c->nb > 0);   // (matters only with free landmarks: see w.inplace below)
  if (lerr && !joint) return lerr;
  // box constraints (free inverse depths: rho >= 0; a free sensor time offset: |tau| <= max) make the problem constrained in Ceres' sense: projected start point,
  // projected gradient norm, projected Armijo line search on every trust-region step.  In the JOINT solve (round 5) the problem is constrained when ANY rank's is
  // (a vote that rides on the first reduction); cost, directional derivatives and trial costs of the search are summed over the ranks, so every rank contracts by the
  // same factor — one more reduction per iteration to decide on the search, one per trial.
  const bool free_rho = c->L > 0 && c->rep.n + c->cs.n > 0 && !(c->locks & LVX_LOCK_LANDMARKS);
  const bool free_tau = (!(c->locks & LVX_LOCK_LIDAR_TAU) && c->surf.n + c->cs.n + c->lp.n > 0) || (!(c->locks & LVX_LOCK_CAM_TAU) && c->rep.n + c->cs.n > 0);
  w.constrained = !lerr && (free_rho || free_tau);   // this rank's own view: its start point and its private gradient entries are projected
  double cons_votes = w.constrained ? 1.0 : 0.0;
  if (!lerr && !joint && w.lm && c->nb > 0) { w.inplace = true; w.Hs = (const double*)c->d_Hb.p; w.Bs = (const double*)c->d_Bd.p; c->p_Hs = w.Hs; }
  const size_t sbytes = (size_t)lvx_state_size(c) * 8;
  c->lm_cost.clear(); c->lm_radius.clear(); c->lm_accept.clear();
  LmRun r(c, w, o);
  lvx_lm_summary& s = r.s;
  bool gconv = false;
  if (!lerr) {
    LVX_HIP(c, hipMemcpyAsync(r.x, state, sbytes, hipMemcpyHostToDevice, r.st));
    if (w.constrained) {   // TrustRegionMinimizer::IterationZero: x <- Plus(x, 0), the start point projected onto the box
      LVX_HIP(c, hipMemsetAsync(w.delta, 0, (size_t)lvx_tangent_size(c) * 8, r.st));
      lerr = try_step(r, r.x, LVX_OK, &r.cost, nullptr);
    } else lerr = lvx_evaluate_d(c, r.x, LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, &r.cost);
  }
  if ((rc = post_eval(c, w, true, o.jacobi_scaling, o.min_lm_diagonal, o.max_lm_diagonal, &r.cost, o.gradient_tolerance, &gconv, lerr, &cons_votes))) return rc;
  r.ls_on = cons_votes > 0.0;
  s.initial_cost = r.cost;
  if (gconv) { s.termination = LVX_LM_GRADIENT_TOLERANCE; }
  // oracle/lm.py::lm_solve, line for line: solve, try the step, search if constrained, reduce, classify, act
  while (s.termination == LVX_LM_NO_CONVERGENCE) {
    if (r.it >= o.max_iterations) { s.termination = LVX_LM_MAX_ITERATIONS; break; }
    ++r.it;
    double m[3]; bool notpd = false;
    if ((rc = solve_step_device(c, w, r.tr.radius, m, &notpd, r.pending))) return rc;
    r.pending = LVX_OK; r.restored = false;
    if (w.inplace) r.acc_is_x = false;   // the landmark elimination ran on the band / border rows themselves
    // candidate x (+) delta: cost AND normal equations (they replace those of x in the accumulators; the model terms of x were taken by solve_step_device)
    double r2[7 + LVX_JB_N] = {m[0], m[1], m[2], 0, 0, 0, 0}, h[6] = {0, 0, 0, 0, 0, 0};
    lerr = LVX_OK;
    bool cand_ne = false;
    EvalLocal ev;
    if (!notpd) {
      double cand = 0;
      bool unevaluable = false, ev_done = false, searched = false;   // (unevaluable: cand = INFINITY, a rejected step)
      lerr = try_step(r, r.xt, LVX_OK, &cand, h, &unevaluable, joint ? nullptr : &ev, &ev_done);
      cand_ne = true; r.acc_is_x = false;
      if (r.ls_on && (rc = line_search(r, m[0], lerr, &cand, h, &searched))) return rc;
      if (!lerr && std::isfinite(cand) && (searched || !ev_done)) lerr = local_after_eval(c, w, &ev);   // the candidate's diagonal / gradient: used if the step is accepted (w.lmd, the damping of x, stays)
      r2[3] = cand; r2[4] = h[0]; r2[5] = h[1];
    }
    if ((rc = reduce_candidate(r, lerr, ev, h, r2))) return rc;
    const double model = -r2[0] - 0.5 * r2[1], cand = r2[3];
    if (!TrustRegion::step_valid(notpd, model)) {   // TrustRegionMinimizer::HandleInvalidStep + LevenbergMarquardtStrategy::StepIsInvalid
      if (o.verbose) fprintf(stderr, "[lvx lm] it %3d invalid step: %s model_cost_change %.6e g.delta %.6e\n", r.it, notpd ? "not positive definite" : "model", model, r2[0]);
      if (!r.tr.StepIsInvalid()) { s.termination = LVX_LM_FAILURE; break; }
      r.record(-1);
      if (cand_ne || w.inplace) r.restore_x();
      continue;
    }
    double rho;
    const StepVerdict verdict = r.tr.classify(r.cost, cand, model, std::sqrt(r2[4]), std::sqrt(r2[5]), &rho);
    if (verdict == STEP_PARAMETER_TOLERANCE || verdict == STEP_FUNCTION_TOLERANCE) {   // tested before the step is accepted or rejected: the solve returns without applying it (trust_region_minimizer.cc)
      s.termination = verdict == STEP_PARAMETER_TOLERANCE ? LVX_LM_PARAMETER_TOLERANCE : LVX_LM_FUNCTION_TOLERANCE;
      r.record(0);
      break;
    }
    if (verdict == STEP_ACCEPT) {
      std::swap(c->d_state.p, c->d_state_try.p); r.x = (double*)c->d_state.p; r.xt = (double*)c->d_state_try.p;
      r.cost = cand; s.successful_steps++; r.acc_is_x = true;
      bool gc = false;
      if ((rc = apply_diag(c, w, false, o.jacobi_scaling, o.min_lm_diagonal, o.max_lm_diagonal, ev, joint ? r2 + 7 : nullptr, o.gradient_tolerance, &gc))) return rc;
      r.tr.StepAccepted(rho);
      r.record(1);
      if (gc) { s.termination = LVX_LM_GRADIENT_TOLERANCE; break; }
    } else {
      const bool above_min = r.tr.StepRejected();   // (the LM diagonal of x is reused)
      r.record(0);
      if (!above_min) { s.termination = LVX_LM_MIN_RADIUS; break; }
      r.restore_x();
    }
    if (o.verbose) fprintf(stderr, "[lvx lm] it %3d cost %.9e radius %.3e rho %.3f\n", r.it, r.cost, r.tr.radius, rho);
  }
  s.iterations = r.it; s.final_cost = r.cost; s.final_radius = r.tr.radius;
  if (joint && r.restored) {   // the loop ended (iteration cap) right behind a rejected step: every rank is here (same decisions), the restore's outcome is voted so that all return together
    double v = r.pending ? 1.0 : 0.0;
    if ((rc = reduce(c, &v, 1, LVX_REDUCE_SUM))) return rc;
    if ((rc = leave_together(c, v, r.pending))) return rc;
  }
  if (!r.acc_is_x) c->last_what &= ~LVX_EVAL_NORMAL_EQ;   // a tolerance test ended the loop on a candidate that was not applied: its normal equations are not those of the returned state
  LVX_HIP(c, hipMemcpyAsync(state, r.x, sbytes, hipMemcpyDeviceToHost, r.st));
  LVX_HIP(c, hipStreamSynchronize(r.st));
  if (sum) *sum = s;
  return r.pending ? r.pending : LVX_OK;
}
int lvx_lm_solve(lvx_ctx* c, double* state, const lvx_lm_options* opt_in, lvx_lm_summary* sum) {
  return lvx_lm_solve_shared(c, state, opt_in, nullptr, nullptr, sum);
}

int lvx_lm_get_history(lvx_ctx* c, int max_n, double* cost, double* radius, int32_t* accepted) {
  if (!c) return LVX_E_ARG;
  const int n = std::min<int>(max_n, (int)c->lm_cost.size());
  for (int i = 0; i < n; ++i) { if (cost) cost[i] = c->lm_cost[i]; if (radius) radius[i] = c->lm_radius[i]; if (accepted) accepted[i] = c->lm_accept[i]; }
  return n;
}

// ---- RCCL transport of the joint solve ----
int lvx_rccl_unique_id(lvx_ctx* c, void* id128) {
  if (!c || !id128) return LVX_E_ARG;
  RcclApi* api = rccl_api(c); if (!api) return LVX_E_COMM;
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return fail(c, LVX_E_COMM, "ncclGetUniqueId failed");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id128, &id, 128);
  return LVX_OK;
}
int lvx_rccl_init(lvx_ctx* c, const void* id128, int rank, int world) {
  if (!c || !id128 || rank < 0 || world < 1 || rank >= world) return LVX_E_ARG;
  LVX_HIP(c, hipSetDevice(c->device));
  RcclApi* api = rccl_api(c); if (!api) return LVX_E_COMM;
  if (c->rccl_comm) { api->CommDestroy((ncclComm_t)c->rccl_comm); c->rccl_comm = nullptr; }
  ncclUniqueId id; std::memcpy(&id, id128, 128);
  ncclComm_t comm = nullptr;
  const ncclResult_t r = api->CommInitRank(&comm, world, id, rank);
  if (r != ncclSuccess) return fail(c, LVX_E_COMM, std::string("ncclCommInitRank: ") + (api->GetErrorString ? api->GetErrorString(r) : "error"));
  int rc = dev_alloc(c, c->d_comm, LVX_COMM_BUF * 8); if (rc) { api->CommDestroy(comm); return rc; }
  c->rccl_comm = comm; c->comm_rank = rank; c->comm_world = world;
  return LVX_OK;
}
int lvx_rccl_finalize(lvx_ctx* c) {
  if (!c) return LVX_E_ARG;
  if (c->rccl_comm) { RcclApi* api = rccl_api(c); if (api) api->CommDestroy((ncclComm_t)c->rccl_comm); c->rccl_comm = nullptr; }
  return LVX_OK;
}
// in-place all-reduce of a caller's DEVICE buffer over the installed communicator, queued on the context's stream (bench.py --gpus N: the per-step reduction of the
// exported border block goes through the library's own transport)
int lvx_rccl_allreduce_d(lvx_ctx* c, double* buf_d, int n, int op) {
  if (!c || !buf_d || n < 0 || (op != LVX_REDUCE_SUM && op != LVX_REDUCE_MAX)) return LVX_E_ARG;
  if (!c->rccl_comm) return fail(c, LVX_E_STATE, "lvx_rccl_allreduce_d: no communicator (lvx_rccl_init)");
  if (n == 0) return LVX_OK;
  RcclApi* api = rccl_api(c); if (!api) return LVX_E_COMM;
  const ncclResult_t r = api->AllReduce(buf_d, buf_d, (size_t)n, ncclDouble, op == LVX_REDUCE_SUM ? ncclSum : ncclMax, (ncclComm_t)c->rccl_comm, c->stream);
  c->n_collectives++;
  if (r != ncclSuccess) return fail(c, LVX_E_COMM, std::string("ncclAllReduce: ") + (api->GetErrorString ? api->GetErrorString(r) : "error"));
  return LVX_OK;
}
int lvx_joint_shared_count(lvx_ctx* c) { return c ? c->last_ns : 0; }
int64_t lvx_collective_count(lvx_ctx* c, int reset) { if (!c) return 0; const int64_t n = c->n_collectives; if (reset) c->n_collectives = 0; return n; }

}  // extern "C"
