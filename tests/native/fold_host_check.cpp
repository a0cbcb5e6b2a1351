// tests/native/fold_host_check.cpp — TEST-ONLY stand-alone host program: the closed form of the folded dense border block (lvi-exc_amd/csrc/lvx_fold.h, what a replica
// block of k_fold_all applies to each of its entries) against the sequential in-place fold of k_fold_border_dense (rows then columns, set 0 then set 1), on random
// symmetric blocks.  Cases: both sets with shared hub rows, disjoint hub rows, partly overlapping hub rows, dead columns, one set off, both off.  Nothing here is linked
// into liblvx.so.  g++ -O2 -std=c++17 fold_host_check.cpp (it also runs clean under -fsanitize=address,undefined); exit status 0 and "fold_host_check: OK" on success.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_fold.h"

using namespace lvx;

struct Set { int ok; double M[6][24]; int hrow[24]; };

// k_fold_border_dense on the full symmetric block Cf [n][n] and g [n]
static void sequential(std::vector<double>& Cf, std::vector<double>& g, int n, int pp, const Set* sets) {
  for (int s = 0; s < 2; ++s) {
    if (sets[s].ok != 1) continue;
    const int p0 = pp + 6 * s;
    const Set& S = sets[s];
    std::vector<double> add((size_t)24 * n);
    for (int c = 0; c < 24; ++c) for (int col = 0; col < n; ++col) { double v = 0.0; for (int p = 0; p < 6; ++p) v += S.M[p][c] * Cf[(size_t)(p0 + p) * n + col]; add[(size_t)c * n + col] = v; }
    for (int c = 0; c < 24; ++c) if (S.hrow[c] >= 0) for (int col = 0; col < n; ++col) Cf[(size_t)S.hrow[c] * n + col] += add[(size_t)c * n + col];
    for (int c = 0; c < 24; ++c) if (S.hrow[c] >= 0) { double v = 0.0; for (int p = 0; p < 6; ++p) v += S.M[p][c] * g[p0 + p]; g[S.hrow[c]] += v; }
    for (int c = 0; c < 24; ++c) for (int row = 0; row < n; ++row) { double v = 0.0; for (int p = 0; p < 6; ++p) v += Cf[(size_t)row * n + p0 + p] * S.M[p][c]; add[(size_t)c * n + row] = v; }
    for (int c = 0; c < 24; ++c) if (S.hrow[c] >= 0) for (int row = 0; row < n; ++row) Cf[(size_t)row * n + S.hrow[c]] += add[(size_t)c * n + row];
  }
}

static int run_case(const char* name, int n, int first0, int first1, int ok0, int ok1, unsigned dead0, unsigned dead1, unsigned seed) {
  const int pp = n - LVX_FOLD_NP;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> ud(-1.0, 1.0);
  // a positive semi-definite block J^T J of 3 n random rows, as the evaluator's is
  std::vector<double> J((size_t)3 * n * n), Cf((size_t)n * n, 0.0), g(n);
  for (double& v : J) v = ud(rng);
  for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) { double v = 0.0; for (int r = 0; r < 3 * n; ++r) v += J[(size_t)r * n + a] * J[(size_t)r * n + b]; Cf[(size_t)a * n + b] = v; }
  for (int a = 0; a < n; ++a) for (int b = 0; b < a; ++b) Cf[(size_t)b * n + a] = Cf[(size_t)a * n + b];
  for (double& v : g) v = ud(rng);
  Set sets[2];
  for (int s = 0; s < 2; ++s) {
    sets[s].ok = s == 0 ? ok0 : ok1;
    for (int p = 0; p < 6; ++p) for (int c = 0; c < 24; ++c) sets[s].M[p][c] = ud(rng);
    for (int c = 0; c < 24; ++c) sets[s].hrow[c] = (((s == 0 ? dead0 : dead1) >> c) & 1u) ? -1 : (s == 0 ? first0 : first1) + c;   // 4 control points x 6, consecutive border rows
  }
  // closed form from the lower triangle (the device's storage): symmetric pseudo rows R, U, then entry by entry
  std::vector<double> R((size_t)LVX_FOLD_NP * n), U((size_t)LVX_FOLD_NP * n, 0.0), gp(LVX_FOLD_NP);
  for (int k = 0; k < LVX_FOLD_NP; ++k) for (int x = 0; x < n; ++x) R[(size_t)k * n + x] = x <= pp + k ? Cf[(size_t)(pp + k) * n + x] : Cf[(size_t)x * n + pp + k];
  for (int k = 0; k < LVX_FOLD_NP; ++k) gp[k] = g[pp + k];
  for (int s = 0; s < 2; ++s) if (sets[s].ok == 1) for (int p = 0; p < 6; ++p) for (int c = 0; c < 24; ++c) if (sets[s].hrow[c] >= 0) U[(size_t)(6 * s + p) * n + sets[s].hrow[c]] = sets[s].M[p][c];
  std::vector<double> Cc((size_t)n * n, 0.0), gc2(n);
  for (int a = 0; a < n; ++a) for (int b = 0; b <= a; ++b) Cc[(size_t)a * n + b] = fold_dense_entry(a, b, Cf[(size_t)a * n + b], R.data(), U.data(), n, pp);
  for (int x = 0; x < n; ++x) gc2[x] = fold_dense_grad(x, g[x], gp.data(), U.data(), n);
  sequential(Cf, g, n, pp, sets);
  double mx = 0.0, mg = 0.0, dC = 0.0, dg = 0.0, asym = 0.0;
  for (int a = 0; a < n; ++a) for (int b = 0; b <= a; ++b) {
    mx = std::fmax(mx, std::fabs(Cf[(size_t)a * n + b])); dC = std::fmax(dC, std::fabs(Cf[(size_t)a * n + b] - Cc[(size_t)a * n + b]));
    asym = std::fmax(asym, std::fabs(Cf[(size_t)a * n + b] - Cf[(size_t)b * n + a]));
  }
  for (int x = 0; x < n; ++x) { mg = std::fmax(mg, std::fabs(g[x])); dg = std::fmax(dg, std::fabs(g[x] - gc2[x])); }
  // every entry is a sum of at most 1 + 12 + 12 + 144 products of magnitude <= max|C'|: 169 roundings of 1.1e-16 at the very most, 1e-13 with room
  const bool ok = dC <= 1e-13 * mx && dg <= 1e-13 * mg && asym <= 1e-13 * mx;
  std::printf("%-28s n %3d: max|C'| %.3e  closed - sequential %.2e (rel %.2e)  gradient %.2e (rel %.2e)  sequential asymmetry %.2e  %s\n", name, n, mx, dC, dC / mx, dg, dg / mg, asym,
              ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  bad += run_case("shared hub rows", 64, 6, 6, 1, 1, 0u, 0u, 1);
  bad += run_case("disjoint hub rows", 76, 0, 30, 1, 1, 0u, 0u, 2);
  bad += run_case("overlapping hub rows", 70, 6, 18, 1, 1, 0u, 0u, 3);
  bad += run_case("shared, dead positions", 64, 12, 12, 1, 1, 0x1c71c7u, 0x1c71c7u, 4);      // columns 0-2 of every control point dead (positions locked)
  bad += run_case("shared, different dead", 61, 3, 3, 1, 1, 0x00003fu, 0xfc0000u, 5);
  bad += run_case("set 1 off", 64, 6, 6, 1, 0, 0u, 0u, 6);
  bad += run_case("set 0 off", 64, 6, 6, 0, 1, 0u, 0u, 7);
  bad += run_case("both off", 40, 0, 0, 0, -3, 0u, 0u, 8);
  bad += run_case("smallest border", 36, 0, 0, 1, 1, 0u, 0u, 9);
  std::printf(bad ? "fold_host_check: %d FAILED\n" : "fold_host_check: OK\n", bad);
  return bad ? 1 : 0;
}
