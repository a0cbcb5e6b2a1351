// The lane-split hub pose of k_clear (lvx_resid.h: hub_lanes_pairs / hub_lanes_coefs / hub_lanes_knots / hub_lanes_matrix) run as loops over "lanes" on the host, against the one-lane
// evaluation it replaces: pose_eval<true> / pose_eval<true, true> + hub_matrix.  The expressions were kept, so every output must have the SAME VALUE (compared with ==:
// a zero may change its sign); the program prints the worst absolute difference it saw (expected 0) and fails on the first value that differs.
// Cases: random control points; u at 0, at 1 - 1e-12 and mid-interval; a control-point pair with |Omega| near zero (below and above logq's 1e-16 switch on |v|^2), one on
// either side of the series switch of so3_Jr_inv / so3_Jr (|2 Omega|^2 = 2.5e-3), large rotations; a non-unit control point (status, as pose_eval reports it).
// Build: g++ -O2 -std=c++17 tests/native/hub_lanes_host_check.cpp -o hub_lanes_host_check   (tests/test_hub_lanes_host.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_resid.h"

using namespace lvx;

static double worst = 0.0;
static long long compared = 0, differing = 0;

static void cmp(const char* what, int cs, double a, double b) {
  ++compared;
  if (a == b) return;
  const double d = std::fabs(a - b);
  if (!(d <= worst)) worst = d;
  if (differing++ < 10) std::printf("  case %d %s: lanes %.17g one lane %.17g\n", cs, what, a, b);
}
static void cmp_m3(const char* what, int cs, const m3& a, const m3& b) { for (int i = 0; i < 9; ++i) cmp(what, cs, a.a[i], b.a[i]); }
static void cmp_v3(const char* what, int cs, v3 a, v3 b) { cmp(what, cs, a.x, b.x); cmp(what, cs, a.y, b.y); cmp(what, cs, a.z, b.z); }

template <bool NEED_V>
static bool lanes_eval(const SplineRef& sp, const KnotRef& k, PoseEval* out, double M[6][24]) {
  HubLanes X;
  std::memset(&X, 0, sizeof X);
  for (int lane = 0; lane < 64; ++lane) hub_lanes_pairs<NEED_V>(sp, k, lane, &X, out);
  if (!hub_lanes_ok(&X)) return false;
  for (int lane = 0; lane < 64; ++lane) hub_lanes_coefs(lane, &X);
  for (int lane = 0; lane < 64; ++lane) hub_lanes_knots<NEED_V>(lane, &X, out);
  for (int lane = 0; lane < 64; ++lane) hub_lanes_matrix(lane, &X, M);
  return true;
}

template <bool NEED_V>
static void one(int cs, const SplineRef& sp, const KnotRef& k, bool expect_ok) {
  PoseEval a, b;
  double Ma[6][24], Mb[6][24];
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b); std::memset(Ma, 0, sizeof Ma); std::memset(Mb, 0, sizeof Mb);
  const bool ok_a = lanes_eval<NEED_V>(sp, k, &a, Ma);
  const bool ok_b = pose_eval<true, NEED_V>(sp, k, &b);
  if (ok_a != ok_b || ok_b != expect_ok) { std::printf("  case %d: status lanes %d one lane %d expected %d\n", cs, (int)ok_a, (int)ok_b, (int)expect_ok); ++differing; return; }
  if (!ok_b) return;
  hub_matrix(b, Mb);
  cmp("k.i0", cs, a.k.i0, b.k.i0); cmp("k.u", cs, a.k.u, b.k.u);
  cmp_v3("p", cs, a.p, b.p);
  for (int j = 0; j < 4; ++j) cmp("Bp", cs, a.Bp[j], b.Bp[j]);
  cmp("q.x", cs, a.so3.q.x, b.so3.q.x); cmp("q.y", cs, a.so3.q.y, b.so3.q.y); cmp("q.z", cs, a.so3.q.z, b.so3.q.z); cmp("q.w", cs, a.so3.q.w, b.so3.q.w);
  for (int j = 0; j < 4; ++j) cmp_m3("dxi", cs, a.so3.dxi[j], b.so3.dxi[j]);
  if (NEED_V) { cmp_v3("v", cs, a.v, b.v); cmp_v3("w_body", cs, a.so3.w_body, b.so3.w_body); }
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 24; ++c) cmp("M", cs, Ma[r][c], Mb[r][c]);
}

int main() {
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const int n = 8;
  const double us[] = {0.0, 1.0 - 1e-12, 0.5, 0.123456789, 0.987};
  // |Omega| of the pair (i0 + 1, i0 + 2); the other pairs are random up to `big`
  const double mids[] = {-1.0 /* random */, 0.0, 5e-9, 2e-8, 1e-4, 0.02499, 0.025, 0.02501, 0.3, 1.4};
  int cs = 0;
  for (double mid : mids)
    for (double big : {0.05, 0.6})
      for (int rep = 0; rep < 4; ++rep) {
        std::vector<double> r3(3 * n), so3(4 * n);
        for (double& x : r3) x = 5.0 * U(rng);
        quat q = mkq(U(rng), U(rng), U(rng), U(rng));
        { const double s = 1.0 / std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w); q = mkq(q.w * s, q.x * s, q.y * s, q.z * s); }
        for (int i = 0; i < n; ++i) {
          so3[4 * i] = q.x; so3[4 * i + 1] = q.y; so3[4 * i + 2] = q.z; so3[4 * i + 3] = q.w;
          v3 ax = mk(U(rng), U(rng), U(rng));
          const double an = std::sqrt(dot(ax, ax));
          const double mag = (mid >= 0.0 && i == 3) ? mid : big * std::fabs(U(rng));      // pair (3, 4) = (i0 + 1, i0 + 2) for i0 = 2
          q = qmul(q, expq_half((mag / an) * ax));
          const double s = 1.0 / std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);   // keep |q| = 1 to rounding over the chain
          q = mkq(q.w * s, q.x * s, q.y * s, q.z * s);
        }
        const SplineRef sp{100.0, 0.02, n, r3.data(), so3.data()};
        for (double u : us) {
          const KnotRef k{2, u};
          one<false>(cs, sp, k, true);
          one<true>(cs, sp, k, true);
          ++cs;
        }
        if (rep == 0) {   // a non-unit control point inside the four knots
          for (int c = 0; c < 4; ++c) so3[4 * 4 + c] *= 1.01;
          one<false>(cs, sp, KnotRef{2, 0.5}, false);
          one<true>(cs, sp, KnotRef{2, 0.5}, false);
          ++cs;
        }
      }
  std::printf("hub_lanes_host_check: %d cases, %lld values compared, %lld differ, worst |difference| %.3e\n", cs, compared, differing, worst);
  if (differing) { std::printf("hub_lanes_host_check: FAILED\n"); return 1; }
  std::printf("hub_lanes_host_check: OK\n");
  return 0;
}
