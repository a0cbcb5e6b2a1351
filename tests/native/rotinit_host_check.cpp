// tests/native/rotinit_host_check.cpp — TEST-ONLY host build of the rotation initialisation (lvi-exc_amd/csrc/lvx_rotinit.h), so that the CPU suite (-m "not gpu") can hold
// it against a numpy restatement of InertialInitializer::EstimateRotation without a GPU, and the GPU suite can hold the device records against these bit for bit.  Not a
// CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2 -ffp-contract=off, as the device translation unit is.
#include <algorithm>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_rotinit.h"

using namespace lvx;

extern "C" int rh_sizes(int* options, int* result) { *options = (int)sizeof(RotOptions); *result = (int)sizeof(RotResult); return ROT_REC; }

// What the two kernels do, tile by tile: results [n_tau][n_prefix], first_ok [n_tau].  prefix_len NULL: one prefix of n; tau NULL: one shift of 0.  Returns RES_NONUNIT if
// a pair met a non-unit control quaternion, else 0; -1: a bad prefix list.
extern "C" int rh_estimate(const double* state, int N, double t0, double dt, int n, const double* t, const double* q, int n_prefix, const int* prefix_len, int n_tau,
                           const double* tau, double huber_deg, int min_pairs, double min_sigma, RotResult* results, int* first_ok) {
  if (!prefix_len || n_prefix == 0) { prefix_len = nullptr; n_prefix = 0; }
  if (!tau || n_tau == 0) { tau = nullptr; n_tau = 0; }
  for (int k = 0; k < n_prefix; ++k) if (prefix_len[k] < 1 || prefix_len[k] > n || (k > 0 && prefix_len[k] < prefix_len[k - 1])) return -1;
  const SplineRef sp{t0, dt, N, state, state + 3 * (size_t)N};
  const RotPrefixes P{prefix_len, n_prefix, n};
  const RotOptions opt{huber_deg, min_pairs, 0, min_sigma};
  const int n_tiles = rot_num_tiles(n), n_seg = rot_num_prefixes(P), n_pairs = n - 1, n_shift = tau ? n_tau : 1;
  std::vector<double> pieces((size_t)rot_num_slots(P) * ROT_REC);
  std::vector<int32_t> tile_drop((size_t)n_tiles);
  int flag = 0;
  for (int s = 0; s < n_shift; ++s) {
    std::fill(pieces.begin(), pieces.end(), -7.0);   // a piece nobody wrote must not be read
    for (int tile = 0; tile < n_tiles; ++tile) {
      double a10[LVX_ROT_TILE][ROT_NSUM] = {};
      int status[LVX_ROT_TILE], seg[LVX_ROT_TILE], drop = LVX_ROT_TILE;
      for (int l = 0; l < LVX_ROT_TILE; ++l) {
        const int p = tile * LVX_ROT_TILE + l;
        status[l] = -1; seg[l] = n_seg;
        if (p >= n_pairs) continue;
        status[l] = rot_pair(sp, t[p], t[p + 1], tau ? tau[s] : 0.0, load_q(q + 4 * (size_t)p), load_q(q + 4 * (size_t)(p + 1)), opt.huber_deg, a10[l]);
        seg[l] = rot_segment_of(P, p);
        if (status[l] == ROT_NONUNIT) flag = RES_NONUNIT;
        if (status[l] == ROT_DROPPED && l < drop) drop = l;
      }
      tile_drop[tile] = drop;
      for (int k = seg[0]; k <= (seg[LVX_ROT_TILE - 1] < n_seg - 1 ? seg[LVX_ROT_TILE - 1] : n_seg - 1); ++k) {
        double v[ROT_REC][LVX_ROT_TILE];
        bool any = false;
        for (int l = 0; l < LVX_ROT_TILE; ++l) {
          const bool in = seg[l] == k, live = l < drop;
          const bool counted = in && live && status[l] == ROT_COUNTED, skipped = in && live && (status[l] == ROT_SKIPPED || status[l] == ROT_NONUNIT);
          any = any || in;
          for (int e = 0; e < ROT_NSUM; ++e) v[e][l] = counted ? a10[l][e] : 0.0;
          v[ROT_NSUM][l] = counted ? 1.0 : 0.0; v[ROT_NSUM + 1][l] = skipped ? 1.0 : 0.0;
        }
        if (!any) continue;
        for (int e = 0; e < ROT_REC; ++e) pieces[(size_t)ROT_REC * rot_slot(tile, k) + e] = rot_tile_sum(v[e]);
      }
    }
    int first = -1;
    for (int k = 0; k < n_seg; ++k) {
      double sum[ROT_REC];
      rot_prefix_sum(P, k, pieces.data(), tile_drop.data(), sum);
      RotResult* r = results + (size_t)s * n_seg + k;
      rot_solve(sum, rot_prefix_len(P, k), opt, r);
      if (r->ok && first < 0) first = k;
    }
    first_ok[s] = first;
  }
  return flag;
}

// the eigen-solver alone: upper triangle in, eigenvalues (descending) and eigenvectors (row-major, columns) out
extern "C" void rh_eigen4(const double* s10, double* lam, double* V16) {
  double V[4][4];
  rot_eigen4(s10, lam, V);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) V16[4 * r + c] = V[r][c];
}

// the header's own sin / cos / atan2 (no math-library call), for the accuracy check: out = [sin x, cos x, atan2(y, w)] per entry, x and y >= 0
extern "C" void rh_trig(int n, const double* x, const double* y, const double* w, double* out) {
  for (int i = 0; i < n; ++i) { rot_sincos(x[i], &out[3 * i], &out[3 * i + 1]); out[3 * i + 2] = rot_atan2_pos(y[i], w[i]); }
}
