// lvx_symeig.h — eigen-decomposition of a small symmetric matrix by cyclic Jacobi rotations, host- and device-callable.  k_calib_cov (lvx_solver.hip) runs it on the
// scaled marginal information of the calibration scalars (at most 22 x 22, in LDS) with the threads of its workgroup as lanes; tests/native/symeig_host_check.cpp builds
// the same header with g++ (one lane, no barrier) and the CPU suite compares it with LAPACK.
//
// Why Jacobi: the matrix is D B D with a well-conditioned B and a diagonal D that spans many decades (a scalar no row touches keeps the LM floor 1e-6 / radius beside
// eigenvalues of order one).  One-sided reductions to tridiagonal form lose the small eigenvalues to eps * |A|; Jacobi with the RELATIVE threshold
//   rotate (p, q)  iff  |a_pq| > eps * sqrt(a_pp a_qq)
// and the diagonal updated as a_pp - t a_pq, a_qq + t a_pq determines every eigenvalue to a few eps of ITSELF (Demmel & Veselic 1992).
//
// Order: a sweep is the round-robin tournament over m = n rounded up to even players: m - 1 rounds of m / 2 disjoint pairs.  The rotations of a round commute, so a
// round is four phases with a barrier behind each:
//   0  lane per pair: c, s and the two new diagonal entries from (a_pp, a_qq, a_pq)                          -> cs[4 l ..]
//   A  lane per (pair, row i):    columns p, q of A and of V rotated
//   B  lane per (pair, column j): rows p, q of A rotated
//   C  lane per pair: a_pq = a_qp = 0 and the diagonal entries of phase 0 (not what A and B left there: c^2 a_pp - 2 c s a_pq + s^2 a_qq cancels)
// Before every sweep each lane evaluates the stopping rule over all pairs itself (231 of them at n = 22): the result is uniform without a reduction.
// The arithmetic does not depend on the number of lanes: one lane on the host performs the same operations on the same operands as 256 on the device.
#pragma once
#include "lvx_math.h"

namespace lvx {

#define LVX_SYMEIG_MAX 22                      // largest n (the calibration scalars)
#define LVX_SYMEIG_CS (4 * (LVX_SYMEIG_MAX / 2))   // doubles of the rotation scratch
#define LVX_SYMEIG_EPS 2.220446049250313e-16

// pair l of round r among m (even) players, p < q; a pair with q >= n (the bye of an odd n) is skipped by the caller
LVX_HD void symeig_pair(int r, int l, int m, int* p, int* q) {
  const int k = m - 1;
  int a, b;
  if (l == 0) { a = k; b = r % k; }
  else { a = (r + l) % k; b = (r + k - l) % k; }
  *p = a < b ? a : b; *q = a < b ? b : a;
}
// |a_pq| / sqrt(a_pp a_qq); a non-positive diagonal product under a non-zero entry counts as infinite (the pair is rotated, the caller sees the eigenvalue's sign)
LVX_HD double symeig_ratio(double app, double aqq, double apq) {
  const double a = fabs(apq);
  if (a == 0.0) return 0.0;
  const double d = app * aqq;
  return d > 0.0 ? a / sqrt(d) : 1e300;
}
// max over p < q of the ratio: the off-diagonal measure of the stopping rule
LVX_HD double symeig_off(const double* A, int lda, int n) {
  double m = 0.0;
  for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) { const double v = symeig_ratio(A[p * lda + p], A[q * lda + q], A[q * lda + p]); m = v > m ? v : m; }
  return m;
}
struct SymeigNoSync { LVX_HD void operator()() const {} };

// A [n][lda] symmetric, both triangles filled; V [n][ldv] is set to the identity here.  On return the diagonal of A holds the eigenvalues (unsorted), the columns of V the
// unit eigenvectors, *sweeps the sweeps that were run and *off the last off-diagonal measure.  Returns 0 when the stopping rule held for every pair, 1 when max_sweeps
// sweeps did not reach it.  Every lane of the group calls with the same arguments but `lane`; sync() is the group's barrier (with memory visibility of A, V, cs).
template <class Sync>
LVX_HD int symeig_jacobi(double* A, int lda, int n, double* V, int ldv, double* cs, int max_sweeps, int lane, int nlanes, Sync sync, int* sweeps, double* off) {
  const int m = (n + 1) & ~1, half = m / 2;
  for (int e = lane; e < n * n; e += nlanes) V[(e / n) * ldv + e % n] = (e / n == e % n) ? 1.0 : 0.0;
  sync();
  int sw = 0;
  double o = 0.0;
  for (;;) {
    o = symeig_off(A, lda, n);
    if (o <= LVX_SYMEIG_EPS || sw >= max_sweeps) break;
    ++sw;
    for (int r = 0; r < m - 1; ++r) {
      for (int l = lane; l < half; l += nlanes) {   // phase 0
        int p, q; symeig_pair(r, l, m, &p, &q);
        double c = 1.0, s = 0.0, dp = 0.0, dq = 0.0;
        if (q < n) {
          const double app = A[p * lda + p], aqq = A[q * lda + q], apq = A[q * lda + p];
          dp = app; dq = aqq;
          if (symeig_ratio(app, aqq, apq) > LVX_SYMEIG_EPS) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t); s = t * c;
            dp = app - t * apq; dq = aqq + t * apq;
          }
        }
        cs[4 * l] = c; cs[4 * l + 1] = s; cs[4 * l + 2] = dp; cs[4 * l + 3] = dq;
      }
      sync();
      for (int e = lane; e < half * n; e += nlanes) {   // phase A
        const int l = e / n, i = e % n;
        int p, q; symeig_pair(r, l, m, &p, &q);
        const double c = cs[4 * l], s = cs[4 * l + 1];
        if (q < n && s != 0.0) {
          const double ap = A[i * lda + p], aq = A[i * lda + q];
          A[i * lda + p] = c * ap - s * aq; A[i * lda + q] = s * ap + c * aq;
          const double vp = V[i * ldv + p], vq = V[i * ldv + q];
          V[i * ldv + p] = c * vp - s * vq; V[i * ldv + q] = s * vp + c * vq;
        }
      }
      sync();
      for (int e = lane; e < half * n; e += nlanes) {   // phase B
        const int l = e / n, j = e % n;
        int p, q; symeig_pair(r, l, m, &p, &q);
        const double c = cs[4 * l], s = cs[4 * l + 1];
        if (q < n && s != 0.0) {
          const double ap = A[p * lda + j], aq = A[q * lda + j];
          A[p * lda + j] = c * ap - s * aq; A[q * lda + j] = s * ap + c * aq;
        }
      }
      sync();
      for (int l = lane; l < half; l += nlanes) {   // phase C
        int p, q; symeig_pair(r, l, m, &p, &q);
        if (q < n && cs[4 * l + 1] != 0.0) { A[p * lda + q] = 0.0; A[q * lda + p] = 0.0; A[p * lda + p] = cs[4 * l + 2]; A[q * lda + q] = cs[4 * l + 3]; }
      }
      sync();
    }
  }
  *sweeps = sw; *off = o;
  return o <= LVX_SYMEIG_EPS ? 0 : 1;
}

// order[0..n): the indices of w ascending (ties by index): insertion sort, for one lane
LVX_HD void symeig_order(const double* w, int stride, int n, int* order) {
  for (int i = 0; i < n; ++i) {
    int k = i;
    while (k > 0 && w[order[k - 1] * stride] > w[i * stride]) { order[k] = order[k - 1]; --k; }
    order[k] = i;
  }
}

}  // namespace lvx
