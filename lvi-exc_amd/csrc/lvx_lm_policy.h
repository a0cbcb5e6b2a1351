// lvx_lm_policy.h — every decision of the Levenberg-Marquardt loop that needs no device: the trust-region schedule and the projected Armijo line search, host only.
// lvx_lm_solve_shared (lvx_solver.hip) supplies the numbers (costs, model terms, norms, directional derivatives — sums over the ranks in a joint solve) and carries
// out what is decided here; tests/native/lm_policy_host_check.cpp builds the same header with g++ and the CPU suite holds it against oracle/lm.py (lm_solve,
// projected_line_search) decision by decision.  Restated from Ceres' public semantics (TrustRegionMinimizer, LevenbergMarquardtStrategy, ArmijoLineSearch): PARITY
// UNPINNED, see DESIGN.md.  No HIP, no context, no I/O.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/lvx.h"

namespace lvx {

// Ceres' defaults, by the names of Solver::Options
constexpr double kSufficientDecrease = 1e-4;        // line_search_sufficient_function_decrease
constexpr double kMaxContraction = 1e-3;            // max_line_search_step_contraction: a trial is at least this fraction of the last one
constexpr double kMinContraction = 0.6;             // min_line_search_step_contraction: ... and at most this fraction
constexpr double kMinLineSearchStep = 1e-9;         // min_line_search_step_size (against step * ||direction||_inf)
constexpr int kMaxLineSearchTrials = 20;            // max_num_line_search_step_size_iterations
constexpr int kMaxConsecutiveInvalidSteps = 5;      // max_num_consecutive_invalid_steps

// ---- trust region (TrustRegionMinimizer::Minimize's tests in their order; LevenbergMarquardtStrategy's radius) ----
enum StepVerdict { STEP_PARAMETER_TOLERANCE, STEP_FUNCTION_TOLERANCE, STEP_ACCEPT, STEP_REJECT };

struct TrustRegion {
  double radius, decrease_factor = 2.0;
  int invalid = 0;   // consecutive invalid steps
  double max_radius, min_radius, min_relative_decrease, function_tolerance, parameter_tolerance;

  explicit TrustRegion(const lvx_lm_options& o)
      : radius(o.initial_radius), max_radius(o.max_radius), min_radius(o.min_radius), min_relative_decrease(o.min_relative_decrease),
        function_tolerance(o.function_tolerance), parameter_tolerance(o.parameter_tolerance) {}

  // a step whose model cost change is not positive and finite (the factorisation failed, or the model did)
  static bool step_valid(bool notpd, double model) { return !notpd && std::isfinite(model) && model > 0.0; }
  // HandleInvalidStep + StepIsInvalid: the radius is halved; false at the fifth in a row (the solve fails, the radius stays)
  bool StepIsInvalid() {
    if (++invalid >= kMaxConsecutiveInvalidSteps) return false;
    radius *= 0.5;
    return true;
  }
  // a valid candidate.  Both tolerances are tested before the step is applied: either ends the solve at x, not at the candidate.  *rho: the step quality (ACCEPT / REJECT)
  StepVerdict classify(double cost, double cand, double model, double step_norm, double x_norm, double* rho) {
    invalid = 0;
    *rho = 0.0;
    if (step_norm <= parameter_tolerance * (x_norm + parameter_tolerance)) return STEP_PARAMETER_TOLERANCE;
    const double cost_change = cost - cand;
    if (std::fabs(cost_change) <= function_tolerance * cost) return STEP_FUNCTION_TOLERANCE;
    *rho = cost_change / model;
    return *rho > min_relative_decrease ? STEP_ACCEPT : STEP_REJECT;
  }
  void StepAccepted(double rho) {
    radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3));
    radius = std::min(max_radius, radius); decrease_factor = 2.0;
  }
  // false: the radius fell under min_radius (Ceres: CONVERGENCE, "minimum trust region radius reached")
  bool StepRejected() {
    radius = radius / decrease_factor; decrease_factor *= 2.0;
    return !(radius < min_radius);
  }
};

// ---- projected Armijo line search of a constrained problem (TrustRegionMinimizer::DoLineSearch) ----
struct LsSample { double x, f, df; bool has_df; };
// coefficients (highest power first) of the lowest-degree polynomial through the samples: Gaussian elimination with partial pivoting, the same operations as
// oracle/lm.py::interpolating_polynomial
inline std::vector<double> poly_fit(const std::vector<LsSample>& sm) {
  int n = 0; for (const auto& q : sm) n += 1 + (q.has_df ? 1 : 0);
  std::vector<double> A((size_t)n * n, 0.0), b(n, 0.0);
  int r = 0;
  for (const auto& q : sm) {
    for (int k = 0; k < n; ++k) A[(size_t)r * n + k] = std::pow(q.x, n - 1 - k);
    b[r++] = q.f;
    if (q.has_df) { for (int k = 0; k < n; ++k) A[(size_t)r * n + k] = (n - 1 - k > 0) ? (n - 1 - k) * std::pow(q.x, n - 2 - k) : 0.0; b[r++] = q.df; }
  }
  for (int k = 0; k < n; ++k) {
    int piv = k; for (int i = k + 1; i < n; ++i) if (std::fabs(A[(size_t)i * n + k]) > std::fabs(A[(size_t)piv * n + k])) piv = i;
    if (piv != k) { for (int j = 0; j < n; ++j) std::swap(A[(size_t)k * n + j], A[(size_t)piv * n + j]); std::swap(b[k], b[piv]); }
    for (int i = k + 1; i < n; ++i) { const double m = A[(size_t)i * n + k] / A[(size_t)k * n + k]; for (int j = k; j < n; ++j) A[(size_t)i * n + j] -= m * A[(size_t)k * n + j]; b[i] -= m * b[k]; }
  }
  std::vector<double> c(n, 0.0);
  for (int k = n - 1; k >= 0; --k) { double t = b[k]; for (int j = k + 1; j < n; ++j) t -= A[(size_t)k * n + j] * c[j]; c[k] = t / A[(size_t)k * n + k]; }
  return c;
}
// argmin on [lo, hi]: 2001 uniform samples, then 60 golden-section steps on the best bracket (oracle/lm.py::minimize_polynomial)
inline double poly_argmin(const std::vector<double>& c, double lo, double hi) {
  auto val = [&](double x) { double v = 0.0; for (double a : c) v = v * x + a; return v; };
  const int n = 2000; double best = 0.0; int bi = 0;
  for (int i = 0; i <= n; ++i) { const double v = val(lo + (hi - lo) * i / n); if (i == 0 || v < best) { best = v; bi = i; } }
  double a = lo + (hi - lo) * std::max(bi - 1, 0) / n, b = lo + (hi - lo) * std::min(bi + 1, n) / n;
  const double g = 0.6180339887498949;
  double x1 = b - g * (b - a), x2 = a + g * (b - a), f1 = val(x1), f2 = val(x2);
  for (int it = 0; it < 60; ++it) {
    if (f1 <= f2) { b = x2; x2 = x1; f2 = f1; x1 = b - g * (b - a); f1 = val(x1); }
    else { a = x1; x1 = x2; f1 = f2; x2 = a + g * (b - a); f2 = val(x2); }
  }
  return 0.5 * (a + b);
}

// The search along a step whose full length (1: cost f1, directional derivative g1) is already evaluated, from (0: f0, g0); dinf: ||step||_inf.
//   while (s.next(&a)) { evaluate at a; if (s.report(f, df, unevaluable)) -> a is the step; }   -> otherwise no step satisfies Armijo: the full step stays
struct ArmijoSearch {
  double f0, g0, dinf;
  LsSample prev{0, 0, 0, false}, cur;
  bool have_prev = false;
  int trial = 0;      // trials fitted so far
  double step = 1.0;  // what the last next() gave

  // the full step stays when it decreases the cost by kSufficientDecrease of the linear prediction m0 = g . delta — the rule
  static bool needed(double cost, double cand, double m0) { return std::isfinite(cand) && m0 < 0.0 && cand > cost + kSufficientDecrease * m0; }

  ArmijoSearch(double f0_, double g0_, double f1, double g1, double dinf_) : f0(f0_), g0(g0_), dinf(dinf_), cur{1.0, f1, g1, true} {}

  // the next trial step: the minimiser of the polynomial through (0, the last sample but one, the last sample), within [kMaxContraction, kMinContraction] x the last
  // step.  false: every trial is spent (*a untouched), or the step fell under kMinLineSearchStep (ArmijoLineSearch gives up; *a is that step)
  bool next(double* a) {
    if (trial >= kMaxLineSearchTrials) return false;
    ++trial;
    std::vector<LsSample> sm{{0.0, f0, g0, true}};
    if (have_prev) sm.push_back(prev);
    sm.push_back(cur);
    *a = step = poly_argmin(poly_fit(sm), kMaxContraction * cur.x, kMinContraction * cur.x);
    return !(step * dinf < kMinLineSearchStep);
  }
  bool armijo(double f) const { return f <= f0 + kSufficientDecrease * step * g0; }
  // the trial's cost and directional derivative (df is read only when the test fails).  true: Armijo holds at the step next() gave.  A trial that cannot be
  // evaluated contracts again without a new sample
  bool report(double f, double df, bool unevaluable) {
    if (unevaluable) { cur.x = step; return false; }
    if (armijo(f)) return true;
    prev = cur; have_prev = true; cur = LsSample{step, f, df, true};
    return false;
  }
};

}  // namespace lvx
