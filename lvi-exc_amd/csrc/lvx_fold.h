// lvx_fold.h — one entry of the folded dense border block in closed form, host- and device-callable (k_fold_all of lvx_eval.hip; tests/native/fold_host_check.cpp
// holds it against the sequential in-place fold of k_fold_border_dense).
//
// The pseudo pose variables of set s (6 rows at pp + 6 s) fold back onto its hub control points: x_pseudo = M_s x_hub.  With U[k][x] = M_s[p][c] at (pseudo index
// k = 6 s + p, hub row x = hrow_s[c]; 0 for a dead column, a set that is off and everywhere else) the two sets' folds, one after the other, are
//   C' = (I + U^T) C (I + U) = C + U^T C + C U + U^T C U
// because U_0 U_1 = 0 (a pseudo row is no hub row) — shared hub rows included.  S: the entry's own value, R[k][x] = C[pp + k][x]: the SYMMETRIC pseudo rows, n wide.
// ONE fixed order of summation: S, then the pseudo index ascending in each of the three terms.
#pragma once
#include "lvx_math.h"

namespace lvx {

#define LVX_FOLD_NP 12   // pseudo rows: 2 sets x 6

LVX_HD double fold_dense_entry(int a, int b, double S, const double* R, const double* U, int n, int pp) {
  // every operand is read first (the device reads LDS: 48 independent loads instead of a chain of load, compare, branch); a zero of U still adds nothing
  double ua[LVX_FOLD_NP], ub[LVX_FOLD_NP], ra[LVX_FOLD_NP], rb[LVX_FOLD_NP];
  bool hub_a = false, hub_b = false;
  for (int k = 0; k < LVX_FOLD_NP; ++k) { ua[k] = U[k * n + a]; ub[k] = U[k * n + b]; ra[k] = R[k * n + a]; rb[k] = R[k * n + b]; hub_a = hub_a || ua[k] != 0.0; hub_b = hub_b || ub[k] != 0.0; }
  double v = S;
  for (int k = 0; k < LVX_FOLD_NP; ++k) v = ua[k] != 0.0 ? v + ua[k] * rb[k] : v;
  for (int k = 0; k < LVX_FOLD_NP; ++k) v = ub[k] != 0.0 ? v + ra[k] * ub[k] : v;
  if (hub_a && hub_b) {
    for (int k = 0; k < LVX_FOLD_NP; ++k) {
      double t = 0.0;
      for (int l = 0; l < LVX_FOLD_NP; ++l) t = ub[l] != 0.0 ? t + R[k * n + pp + l] * ub[l] : t;
      v = ua[k] != 0.0 ? v + ua[k] * t : v;
    }
  }
  return v;
}
// the gradient's entry x: g' = g + U^T g_pseudo
LVX_HD double fold_dense_grad(int x, double S, const double* gp, const double* U, int n) {
  double v = S;
  for (int k = 0; k < LVX_FOLD_NP; ++k) { const double u = U[k * n + x]; if (u != 0.0) v += u * gp[k]; }
  return v;
}

}  // namespace lvx
