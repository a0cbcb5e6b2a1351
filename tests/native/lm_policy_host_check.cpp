// Host build of lvi-exc_amd/csrc/lvx_lm_policy.h (g++, no HIP): a C ABI over the trust-region schedule and the Armijo search lvx_lm_solve_shared decides with, for
// tests/test_lm_policy_host.py to hold against oracle/lm.py.  Built as a shared object: g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared.
#include <cstdint>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_lm_policy.h"

extern "C" {

// the named constants, in the header's order
void lp_constants(double* d4, int32_t* i2) {
  d4[0] = lvx::kSufficientDecrease; d4[1] = lvx::kMaxContraction; d4[2] = lvx::kMinContraction; d4[3] = lvx::kMinLineSearchStep;
  i2[0] = lvx::kMaxLineSearchTrials; i2[1] = lvx::kMaxConsecutiveInvalidSteps;
}

// poly_fit of n samples (x, f, df; has_df[i] == 0: value only) -> coef (highest power first); returns the number of coefficients
int lp_poly_fit(int n, const double* x, const double* f, const double* df, const int32_t* has_df, double* coef) {
  std::vector<lvx::LsSample> sm;
  for (int i = 0; i < n; ++i) sm.push_back(lvx::LsSample{x[i], f[i], df[i], has_df[i] != 0});
  const std::vector<double> c = lvx::poly_fit(sm);
  for (size_t k = 0; k < c.size(); ++k) coef[k] = c[k];
  return (int)c.size();
}
double lp_poly_argmin(int n, const double* coef, double lo, double hi) { return lvx::poly_argmin(std::vector<double>(coef, coef + n), lo, hi); }

int lp_search_needed(double cost, double cand, double m0) { return lvx::ArmijoSearch::needed(cost, cand, m0) ? 1 : 0; }
void* lp_search_new(double f0, double g0, double f1, double g1, double dinf) { return new lvx::ArmijoSearch(f0, g0, f1, g1, dinf); }
int lp_search_next(void* s, double* a) { return ((lvx::ArmijoSearch*)s)->next(a) ? 1 : 0; }
int lp_search_report(void* s, double f, double df, int unevaluable) { return ((lvx::ArmijoSearch*)s)->report(f, df, unevaluable != 0) ? 1 : 0; }
int lp_search_trials(void* s) { return ((lvx::ArmijoSearch*)s)->trial; }
void lp_search_free(void* s) { delete (lvx::ArmijoSearch*)s; }

void* lp_tr_new(const lvx_lm_options* o) { return new lvx::TrustRegion(*o); }
double lp_tr_radius(void* t) { return ((lvx::TrustRegion*)t)->radius; }
int lp_tr_step_valid(int notpd, double model) { return lvx::TrustRegion::step_valid(notpd != 0, model) ? 1 : 0; }
int lp_tr_invalid(void* t) { return ((lvx::TrustRegion*)t)->StepIsInvalid() ? 1 : 0; }
// 0 parameter tolerance, 1 function tolerance, 2 accept, 3 reject
int lp_tr_classify(void* t, double cost, double cand, double model, double step_norm, double x_norm, double* rho) {
  return (int)((lvx::TrustRegion*)t)->classify(cost, cand, model, step_norm, x_norm, rho);
}
void lp_tr_accepted(void* t, double rho) { ((lvx::TrustRegion*)t)->StepAccepted(rho); }
int lp_tr_rejected(void* t) { return ((lvx::TrustRegion*)t)->StepRejected() ? 1 : 0; }
void lp_tr_free(void* t) { delete (lvx::TrustRegion*)t; }

}  // extern "C"
