// lvx_rotinit.h — sensor-to-IMU rotation from odometry: InertialInitializer::EstimateRotation (src/lvi_exc/src/core/inertial_initializer.cpp:26-81), the step
// CalibrHelperLVI::Initialization (src/lvi_exc/src/core/calib_helper_lvi.cpp:44-96) runs on the odometry poses so far after Solve #0, for every prefix of a list and every
// time shift of a list at once.  Host-callable (tests/native/rotinit_host_check.cpp builds it with g++); the library runs it inside the kernels of lvx_rotinit.hip only.
//
// One pair (i = j - 1, j) of consecutive odometry poses and a shift tau of the odometry stamps:
//   d_i = q(t_i + tau)* (x) q(t_j + tau)          the SO3 spline itself, not re-signed (:41-44)
//   d_s = q'_i* (x) q'_j, w >= 0                   the odometry quaternions, normalised on the way in; the sign is what the reference's Matrix3d -> Quaterniond
//                                                   conversion yields for trace > 0 (:46-49)
//   delta = 180 / pi |angle(d_s) - angle(d_i)|,   angle(q) = 2 atan2(|vec|, |w|) (Eigen 3.3 AngleAxis, :51-53);   huber = delta > huber_deg ? huber_deg / delta : 1
//   A = huber (L(d_s) - R(d_i))                   LeftQuatMatrix / RightQuatMatrix (include/utils/math_utils.h:144-165; component order x, y, z, w), :56-58
// and the pair contributes the ten unique entries of A^T A, in the order (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3): the right singular vectors of the
// stacked A (:64-70) are the eigenvectors of sum A^T A, its singular values the roots of the eigenvalues.  x = the eigenvector of the smallest eigenvalue = q_ItoS
// (q_LtoI = conj(x), calib_helper_lvi.cpp:67-68).
//
// Which pairs count, per shift:
//   * the first j whose t_j + tau >= MaxTime (:39-40), or is not finite, ends the list: that pair and all later ones are dropped;
//   * DEVIATION: a pair one of whose two evaluation times lies outside [MinTime, MaxTime) — in practice t_i + tau < MinTime — is skipped and counted in n_skipped; the
//     reference's Evaluate would throw std::range_error, which with a list of shifts must not kill the call;
//   * a pair whose spline window holds a control quaternion that fails logq's unit check is skipped and counted in n_skipped too; the caller reports RES_NONUNIT.
//
// Sums, in ONE order that both builds follow.  Pair p = j - 1 lies in tile p / 64 and in segment k, the first k with p < prefix_len[k] - 1 (prefix k covers pairs
// j = 1 .. prefix_len[k] - 1).  A PIECE is the set of pairs of one tile in one segment; its ten sums are formed over the 64 lanes of the tile — a lane outside the piece,
// skipped or dropped holds +0.0 — by the halving tree of rot_tile_sum (lane l += lane l + 32, then + 16, ... + 1).  Prefix k is the running sum, started at +0.0, of the
// pieces of the segments 0 .. k in the order of their pairs (rot_prefix_sum): a later prefix is an earlier one plus the pieces between them, added one by one.
// The first dropped pair of a tile drops the rest of ITS tile inside the piece sums; rot_prefix_sum stops after the first tile that holds one.
//
// Solve: cyclic Jacobi on the symmetric 4 x 4 sum, ROT_SWEEPS sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a rotation skipped where the off-diagonal entry is exactly
// zero; only + - * / sqrt, so that both builds (no FP contraction) give the same bits.
#pragma once
#include "lvx_traj.h"

namespace lvx {

#define LVX_ROT_TILE 64
enum { ROT_COUNTED = 0, ROT_SKIPPED = 1, ROT_NONUNIT = 2, ROT_DROPPED = 3 };
enum { ROT_NSUM = 10, ROT_REC = 12, ROT_SWEEPS = 12 };   // a piece record: ten sums | counted pairs | skipped pairs

struct RotOptions { double huber_deg; int32_t min_pairs; int32_t reserved; double min_sigma; };                       // = lvx_rotinit_options
struct RotResult { double q_ItoS_xyzw[4]; double sigma[4]; int32_t n_poses, n_pairs, n_skipped, ok; };                // = lvx_rotinit_result

// sin, cos and atan2 from + - * / alone.  The math library's are not the same function on the two sides (the device library's and glibc's results differ in the last
// bit for some arguments, which nine ulp of the quaternion later showed), so the records of the two builds can only be the same bits if neither calls it.  Polynomials
// and break points of FDLIBM (k_sin.c, k_cos.c, s_atan.c, e_atan2.c; errors below 1 ulp there, below 2 ulp in this plainer form).
LVX_HD double rot_ksin(double x) {   // |x| <= pi / 4
  const double z = x * x, v = z * x;
  const double r = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  return x + v * (-1.66666666666666324348e-01 + z * r);
}
LVX_HD double rot_kcos(double x) {   // |x| <= pi / 4
  const double z = x * x, ax = fabs(x);
  const double r = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 +
                   z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  if (ax < 0.3) return 1.0 - (0.5 * z - z * r);
  const double qx = ax > 0.78125 ? 0.28125 : 0.25;
  return (1.0 - qx) - ((0.5 * z - qx) - z * r);
}
// x in [0, 5 pi / 4] (a half angle times a basis value <= 1 never leaves [0, pi]); beyond, the library's functions answer
LVX_HD void rot_sincos(double x, double* s, double* c) {
  const double pio2_hi = 1.57079632673412561417e+00, pio2_lo = 6.07710050650619224932e-11;   // pi / 2 = hi + lo, hi with 33 bits: x - hi is exact for x in [pi / 4, pi]
  if (x <= 0.78539816339744828) { *s = rot_ksin(x); *c = rot_kcos(x); }
  else if (x <= 2.3561944901923448) { const double r = (x - pio2_hi) - pio2_lo; *s = rot_kcos(r); *c = -rot_ksin(r); }
  else if (x <= 3.9269908169872414) { const double r = (x - 2.0 * pio2_hi) - 2.0 * pio2_lo; *s = -rot_ksin(r); *c = -rot_kcos(r); }
  else { *s = sin(x); *c = cos(x); }
}
LVX_HD double rot_atan_pos(double x) {   // x >= 0
  double hi, lo;
  int id = -1;
  if (x < 0.4375) { hi = 0.0; lo = 0.0; }
  else if (x < 0.6875) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; }
  else if (x < 1.1875) { id = 1; x = (x - 1.0) / (x + 1.0); hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; }
  else if (x < 2.4375) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; }
  else { id = 3; x = -1.0 / x; hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; }
  const double z = x * x, w = z * z;
  const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 + w * (6.66107313738753120669e-02 +
                    w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
  const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 +
                    w * -3.65315727442169155270e-02))));
  if (id < 0) return x - x * (s1 + s2);
  return hi - ((x * (s1 + s2) - lo) - x);
}
LVX_HD double rot_atan2_pos(double y, double x) {   // y >= 0: the angle in [0, pi]
  if (x == 0.0) return y == 0.0 ? 0.0 : 1.57079632679489655800e+00;
  const double z = rot_atan_pos(fabs(y / x));
  return x > 0.0 ? z : 3.1415926535897931160e+00 - (z - 1.2246467991473531772e-16);
}
// logq_half / expq_half of lvx_math.h (quaternion_math.h:16-89) on those
LVX_HD v3 rot_logq_half(quat q, bool* ok) {
  const double qn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  if (fabs(qn - 1.0) > 1e-5) *ok = false;
  const double v2 = q.x * q.x + q.y * q.y + q.z * q.z;
  double k = 1.0;
  if (v2 > 1e-16) { const double vn = sqrt(v2); k = rot_atan2_pos(vn, q.w) / vn; }
  return mk(q.x * k, q.y * k, q.z * k);
}
LVX_HD quat rot_expq_half(v3 v) {
  const double v2 = v.x * v.x + v.y * v.y + v.z * v.z;
  double ka = 1.0, kv = 1.0;
  if (v2 > 1e-16) { const double vn = sqrt(v2); double s; rot_sincos(vn, &s, &ka); kv = s / vn; }
  return mkq(ka, kv * v.x, kv * v.y, kv * v.z);
}
// orientation of the spline at tt: RES_OK, RES_RANGE or RES_NONUNIT.  The cumulative form of so3_eval (lvx_math.h; uniform_so3_spline_trajectory.h:46-125), value only.
LVX_HD int rot_orientation(const SplineRef& sp, double tt, quat* q) {
  KnotRef k;
  if (!traj_knot(sp.t0, sp.dt, sp.n, tt, &k)) return RES_RANGE;
  quat c[4]; load_so3_cp(sp, k.i0, c);
  const double u = k.u, u2 = u * u, u3 = u2 * u;
  const double B[4] = {1.0, 5.0 / 6.0 + u * (3.0 / 6.0) + u2 * (-3.0 / 6.0) + u3 * (1.0 / 6.0), 1.0 / 6.0 + u * (3.0 / 6.0) + u2 * (3.0 / 6.0) + u3 * (-2.0 / 6.0), u3 * (1.0 / 6.0)};
  bool ok = true;
  quat r = c[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) r = qmul(r, rot_expq_half(B[j] * rot_logq_half(qmul(qconj(c[j - 1]), c[j]), &ok)));
  if (!ok) return RES_NONUNIT;
  *q = r;
  return RES_OK;
}
LVX_HD double rot_angle(quat q) { return 2.0 * rot_atan2_pos(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), fabs(q.w)); }

// the pair (t_i, q'_i), (t_j, q'_j) under the shift tau: its status and, when counted, the ten entries
LVX_HD int rot_pair(const SplineRef& sp, double ti, double tj, double tau, quat qsi, quat qsj, double huber_deg, double a10[ROT_NSUM]) {
  const double tti = ti + tau, ttj = tj + tau;
  const double tmax = sp.t0 + (double)(sp.n - 3) * sp.dt;
  if (!(ttj < tmax) || !(ttj >= -1.7976931348623157e308)) return ROT_DROPPED;
  quat qi, qj;
  const int si = rot_orientation(sp, tti, &qi), sj = rot_orientation(sp, ttj, &qj);
  if (si == RES_RANGE || sj == RES_RANGE) return ROT_SKIPPED;
  if (si != RES_OK || sj != RES_OK) return ROT_NONUNIT;
  const quat b = qmul(qconj(qi), qj);
  quat a = qmul(qconj(qnormalized(qsi)), qnormalized(qsj));
  if (a.w < 0.0) { a.x = -a.x; a.y = -a.y; a.z = -a.z; a.w = -a.w; }
  const double delta = 180.0 / 3.14159265358979323846 * fabs(rot_angle(a) - rot_angle(b));
  const double h = delta > huber_deg ? huber_deg / delta : 1.0;
  const double dw = a.w - b.w, sx = a.x + b.x, sy = a.y + b.y, sz = a.z + b.z, dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  const double A[4][4] = {{h * dw, h * -sz, h * sy, h * dx}, {h * sz, h * dw, h * -sx, h * dy}, {h * -sy, h * sx, h * dw, h * dz}, {h * -dx, h * -dy, h * -dz, h * dw}};
  int e = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) a10[e++] = ((A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c]) + A[3][r] * A[3][c];
  return ROT_COUNTED;
}

// the prefix list: NULL = one prefix of all n poses; an entry is read clamped to [1, n]
struct RotPrefixes { const int32_t* len; int n_prefix, n; };
LVX_HD int rot_prefix_len(const RotPrefixes& P, int k) {
  const int v = P.len ? P.len[k] : P.n;
  return v < 1 ? 1 : (v > P.n ? P.n : v);
}
LVX_HD int rot_num_prefixes(const RotPrefixes& P) { return P.len ? P.n_prefix : 1; }
// segment of pair p: the first k with p < prefix_len[k] - 1; the number of prefixes if there is none
LVX_HD int rot_segment_of(const RotPrefixes& P, int p) {
  int lo = 0, hi = rot_num_prefixes(P);
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (p < rot_prefix_len(P, mid) - 1) hi = mid; else lo = mid + 1; }
  return lo;
}
LVX_HD int rot_num_tiles(int n) { return n > 1 ? (n - 1 + LVX_ROT_TILE - 1) / LVX_ROT_TILE : 1; }
LVX_HD int rot_num_slots(const RotPrefixes& P) { return rot_num_tiles(P.n) + rot_num_prefixes(P); }
LVX_HD int rot_slot(int tile, int segment) { return tile + segment; }   // pieces in pair order step the tile, the segment or both: the sum is unique

// the halving tree over the 64 lanes of a tile (the host form; the kernel does the same additions with lane shuffles)
inline double rot_tile_sum(double v[LVX_ROT_TILE]) {
  for (int s = LVX_ROT_TILE / 2; s > 0; s >>= 1) for (int l = 0; l < s; ++l) v[l] = v[l] + v[l + s];
  return v[0];
}

// prefix k of one shift: pieces [slots][ROT_REC], first dropped pair of every tile (tile_drop[tile]: lane 0 .. 63, or 64 for none)
LVX_HD void rot_prefix_sum(const RotPrefixes& P, int k, const double* pieces, const int32_t* tile_drop, double sum[ROT_REC]) {
#pragma unroll
  for (int e = 0; e < ROT_REC; ++e) sum[e] = 0.0;
  int p = 0, last_tile = 0x7fffffff;   // last_tile: the first tile that holds a dropped pair; its pieces carry their pairs before it, later tiles nothing
  for (int seg = 0; seg <= k; ++seg) {
    const int end = rot_prefix_len(P, seg) - 1;
    while (p < end) {
      const int tile = p / LVX_ROT_TILE;
      if (tile > last_tile) return;
      const double* r = pieces + (size_t)ROT_REC * rot_slot(tile, seg);
#pragma unroll
      for (int e = 0; e < ROT_REC; ++e) sum[e] = sum[e] + r[e];
      if (tile_drop[tile] < LVX_ROT_TILE) last_tile = tile;
      p = (tile + 1) * LVX_ROT_TILE < end ? (tile + 1) * LVX_ROT_TILE : end;
    }
  }
}

// one Jacobi rotation of the pair (P, Q): A <- J^T A J, V <- V J
template <int P, int Q>
LVX_HD void rot_jacobi_step(double A[4][4], double V[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const double akp = A[k][P], akq = A[k][Q]; A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { const double apk = A[P][k], aqk = A[Q][k]; A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { const double vkp = V[k][P], vkq = V[k][Q]; V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq; }
}
template <int I, int J>
LVX_HD void rot_order(double lam[4], double V[4][4]) {   // descending; equal values keep their order
  if (lam[I] < lam[J]) {
    const double t = lam[I]; lam[I] = lam[J]; lam[J] = t;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double v = V[k][I]; V[k][I] = V[k][J]; V[k][J] = v; }
  }
}
// eigenvalues (descending) and eigenvectors (columns of V) of the symmetric matrix with the upper triangle s10
LVX_HD void rot_eigen4(const double s10[ROT_NSUM], double lam[4], double V[4][4]) {
  double A[4][4];
  int e = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) { A[r][c] = s10[e]; A[c][r] = s10[e]; ++e; }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ROT_SWEEPS; ++sweep) {
    rot_jacobi_step<0, 1>(A, V); rot_jacobi_step<0, 2>(A, V); rot_jacobi_step<0, 3>(A, V);
    rot_jacobi_step<1, 2>(A, V); rot_jacobi_step<1, 3>(A, V); rot_jacobi_step<2, 3>(A, V);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) lam[k] = A[k][k];
  rot_order<0, 1>(lam, V); rot_order<1, 2>(lam, V); rot_order<2, 3>(lam, V);   // bubble sort: three passes
  rot_order<0, 1>(lam, V); rot_order<1, 2>(lam, V);
  rot_order<0, 1>(lam, V);
}

// the result record of one (shift, prefix) from its sums: :60-80.  Fewer than min_pairs pairs: ok = 0, identity, zero sigmas (the reference returns before the SVD)
LVX_HD void rot_solve(const double sum[ROT_REC], int n_poses, const RotOptions& opt, RotResult* r) {
  r->n_poses = n_poses; r->n_pairs = (int32_t)sum[ROT_NSUM]; r->n_skipped = (int32_t)sum[ROT_NSUM + 1]; r->ok = 0;
  r->q_ItoS_xyzw[0] = 0.0; r->q_ItoS_xyzw[1] = 0.0; r->q_ItoS_xyzw[2] = 0.0; r->q_ItoS_xyzw[3] = 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) r->sigma[k] = 0.0;
  if (r->n_pairs < opt.min_pairs) return;
  double lam[4], V[4][4];
  rot_eigen4(sum, lam, V);
#pragma unroll
  for (int k = 0; k < 4; ++k) r->sigma[k] = sqrt(lam[k] > 0.0 ? lam[k] : 0.0);
  double x[4] = {V[0][3], V[1][3], V[2][3], V[3][3]};
  const double nrm = sqrt(((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]);
  // sign: w >= 0; w == 0: the first non-zero component positive
  const double lead = x[3] != 0.0 ? x[3] : (x[0] != 0.0 ? x[0] : (x[1] != 0.0 ? x[1] : x[2]));
  const double sg = lead < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) r->q_ItoS_xyzw[k] = sg * x[k] / nrm;
  r->ok = r->sigma[2] > opt.min_sigma ? 1 : 0;
}

}  // namespace lvx
