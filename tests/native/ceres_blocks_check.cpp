// Test driver for the per-block route of lvi-exc_amd/host/lvx_ceres_shim.hpp (JacobianRows::kBlocks) without a device: random per-block records
// (include/lvx.h, lvx_jacobian_blocks) for every block of a problem, the same values expanded into the 64-wide debug rows of LVX_EVAL_JACOBIAN
// (columns from lvx_jacobian_block_cols), both scattered through LvxRowBlock::Evaluate — the ambient blocks must be bitwise identical.
#include <cstring>
#include <random>
#include <vector>

#include "lvx_ceres_shim.hpp"

using namespace lvx_host;

namespace {
// knots of the block's trajectory segments, in parameter order (the SO3 blocks), split into runs of consecutive knots
std::vector<std::vector<int>> segments_of(const BlockSpec& b, int N) {
  std::vector<std::vector<int>> segs;
  for (const auto& p : b.params) {
    if (!p.quat || p.tangent_off < 0 || p.tangent_off >= 6 * N) continue;
    const int k = p.tangent_off / 6;
    if (segs.empty() || segs.back().back() + 1 != k) segs.emplace_back();
    segs.back().push_back(k);
  }
  return segs;
}
}  // namespace

extern "C" {

// Returns 0 when every block's residuals and ambient Jacobian blocks agree bitwise between the two routes; *n_shared: blocks whose two poses share knots,
// *n_skipped: blocks with (-1, -1, -1) keys.  tau_free: records of the free-offset widths for the surfel / reprojection / camera-surfel families.
int blocks_scatter_compare(const double* state, double t0, double dt, int n_knots, int n_landmarks, double readout, unsigned locks,
                           int n_imu, const double* t_imu, int has_prior, double prior_t, int n_surf, const double* surf_t, double t_map,
                           int n_rep, const int* rep_lm, const double* rep_t0, const double* lm_t0, int n_cs, const int* cs_lm,
                           int tau_free, unsigned seed, int* n_shared, int* n_skipped) {
  try {
    const int N = n_knots;
    BlockLayout lay(t0, dt, N, n_landmarks, readout, 1e-3, locks);
    std::vector<BlockSpec> specs;
    for (int i = 0; i < n_imu; ++i) specs.push_back(lay.Gyro(i, t_imu[i]));
    if (!(locks & LVX_LOCK_R3)) for (int i = 0; i < n_imu; ++i) specs.push_back(lay.Accel(i, t_imu[i]));
    if (has_prior) specs.push_back(lay.Prior(prior_t));
    for (int i = 0; i < n_surf; ++i) specs.push_back(lay.Surfel(i, t_map, surf_t[i]));
    for (int i = 0; i < n_rep; ++i) specs.push_back(lay.Reproj(i, lm_t0[rep_lm[i]], rep_t0[i], rep_lm[i]));
    for (int i = 0; i < n_cs; ++i) specs.push_back(lay.CamSurf(i, t_map, lm_t0[cs_lm[i]], cs_lm[i]));
    const int nrs[LVX_NUM_FAM] = {3, 3, 1, 1, 2, 1};
    const int base_w[LVX_NUM_FAM] = {15, 29, 12, 54, 55, 60};
    int64_t cnt[LVX_NUM_FAM] = {n_imu, (locks & LVX_LOCK_R3) ? 0 : n_imu, has_prior ? 1 : 0, n_surf, n_rep, n_cs};
    int64_t row0[LVX_NUM_FAM + 1] = {0};
    for (int f = 0; f < LVX_NUM_FAM; ++f) row0[f + 1] = row0[f] + cnt[f] * nrs[f];
    const int64_t nres = row0[LVX_NUM_FAM];
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> res((size_t)nres);
    for (auto& v : res) v = U(rng);
    std::vector<int32_t> keys[LVX_NUM_FAM];
    std::vector<double> vals[LVX_NUM_FAM];
    int W[LVX_NUM_FAM];
    for (int f = 0; f < LVX_NUM_FAM; ++f) {
      W[f] = base_w[f] + ((tau_free && f >= LVX_FAM_SURFEL) ? 1 : 0);
      keys[f].assign((size_t)cnt[f] * 3, -1);
      vals[f].resize((size_t)cnt[f] * nrs[f] * W[f]);
      for (auto& v : vals[f]) v = U(rng);
    }
    *n_shared = 0; *n_skipped = 0;
    for (const BlockSpec& b : specs) {
      int32_t* k = keys[b.family].data() + 3 * (size_t)b.index;
      if (rng() % 23 == 0) { ++*n_skipped; continue; }   // not evaluated
      const auto segs = segments_of(b, N);
      if (segs.empty()) return -2;
      auto pick = [&](const std::vector<int>& s) { return s.front() + (int)(rng() % (uint64_t)(s.size() - 3)); };
      k[0] = pick(segs.front());
      if (b.family >= LVX_FAM_SURFEL) {
        k[1] = pick(segs.back());
        if (segs.size() == 1 && rng() % 2) k[1] = k[0];   // both poses in one interval
        if (b.family == LVX_FAM_REPROJ && rng() % 2) std::swap(k[0], k[1]);
        if (std::abs(k[1] - k[0]) < 4) ++*n_shared;
      }
      if (b.family == LVX_FAM_REPROJ) k[2] = b.params.back().tangent_off - 6 * N - 22;
    }
    // the same values as debug rows
    std::vector<int32_t> dcols((size_t)nres * LVX_JAC_WIDTH, -1);
    std::vector<double> dvals((size_t)nres * LVX_JAC_WIDTH, 0.0);
    for (int f = 0; f < LVX_NUM_FAM; ++f)
      for (int64_t i = 0; i < cnt[f]; ++i) {
        const int32_t* k = keys[f].data() + 3 * i;
        if (k[0] < 0) continue;
        int32_t cols[LVX_JAC_WIDTH];
        if (lvx_jacobian_block_cols(f, N, W[f], k, cols) != LVX_OK) return -3;
        for (int a = 0; a < nrs[f]; ++a) {
          const int64_t row = row0[f] + i * nrs[f] + a;
          for (int c = 0; c < W[f]; ++c) { dcols[row * LVX_JAC_WIDTH + c] = cols[c]; dvals[row * LVX_JAC_WIDTH + c] = vals[f][(i * nrs[f] + a) * W[f] + c]; }
        }
      }
    lvx_jacobian_blocks views[LVX_NUM_FAM];
    for (int f = 0; f < LVX_NUM_FAM; ++f) views[f] = lvx_jacobian_blocks{cnt[f], nrs[f], W[f], keys[f].data(), vals[f].data(), nullptr, nullptr};
    LvxEvaluationCallback cbd(JacobianRows::kDebugRows, N, row0), cbb(JacobianRows::kBlocks, N, row0);
    cbd.Provide(state, res.data(), dcols.data(), dvals.data(), nullptr);
    cbb.Provide(state, res.data(), nullptr, nullptr, views);
    double plane_dummy[3] = {0, 0, 1};
    for (const BlockSpec& sp : specs) {
      LvxRowBlock bd(&cbd, sp), bb(&cbb, sp);
      const auto& sizes = bd.parameter_block_sizes();
      const int nr = sp.num_residuals;
      std::vector<const double*> params(sizes.size());
      std::vector<std::vector<double>> jd(sizes.size()), jb(sizes.size());
      std::vector<double*> pd(sizes.size()), pb(sizes.size());
      for (size_t q = 0; q < sizes.size(); ++q) {
        params[q] = sp.params[q].state_off >= 0 ? state + sp.params[q].state_off : plane_dummy;
        const bool constant = sp.params[q].tangent_off < 0;
        jd[q].assign((size_t)nr * sizes[q], 7.0); jb[q].assign((size_t)nr * sizes[q], -7.0);   // (different garbage: every entry must be written)
        pd[q] = constant ? nullptr : jd[q].data(); pb[q] = constant ? nullptr : jb[q].data();
      }
      double rd[4], rb[4];
      if (!bd.Evaluate(params.data(), rd, pd.data())) return -4;
      if (!bb.Evaluate(params.data(), rb, pb.data())) return -5;
      if (std::memcmp(rd, rb, sizeof(double) * nr) != 0) return -6;
      for (size_t q = 0; q < sizes.size(); ++q)
        if (pd[q] && std::memcmp(jd[q].data(), jb[q].data(), sizeof(double) * jd[q].size()) != 0) return 1000 * sp.family + (int)q + 1;
    }
    return 0;
  } catch (const std::exception&) { return -1; }
}

// the seam on a device: every block of the problem loaded in ctx through the shim in blocks mode (PrepareForEvaluation requests LVX_EVAL_JACOBIAN_BLOCKS),
// ambient Jacobian blocks scattered into a dense [n_residuals x n_state] matrix (row order = lvx residual order).  Returns 0, or a negative code.
int shim_check_all_blocks(lvx_ctx* ctx, const double* state, int n_state, double t0, double dt, int n_knots, int n_landmarks, double readout, unsigned locks,
                          int n_imu, const double* t_imu, int has_prior, double prior_t, int n_surf, const double* surf_t, double t_map,
                          int n_rep, const int* rep_lm, const double* rep_t0, const double* lm_t0, int n_cs, const int* cs_lm,
                          double* out_residuals, double* out_J) {
  try {
    BlockLayout lay(t0, dt, n_knots, n_landmarks, readout, 1e-3, locks);
    std::vector<double> st(state, state + n_state);
    LvxEvaluationCallback cb(ctx, [&](double* s) { std::memcpy(s, st.data(), sizeof(double) * st.size()); }, JacobianRows::kBlocks);
    std::vector<BlockSpec> specs;
    for (int i = 0; i < n_imu; ++i) specs.push_back(lay.Gyro(i, t_imu[i]));
    if (!(locks & LVX_LOCK_R3)) for (int i = 0; i < n_imu; ++i) specs.push_back(lay.Accel(i, t_imu[i]));
    if (has_prior) specs.push_back(lay.Prior(prior_t));
    for (int i = 0; i < n_surf; ++i) specs.push_back(lay.Surfel(i, t_map, surf_t[i]));
    for (int i = 0; i < n_rep; ++i) specs.push_back(lay.Reproj(i, lm_t0[rep_lm[i]], rep_t0[i], rep_lm[i]));
    for (int i = 0; i < n_cs; ++i) specs.push_back(lay.CamSurf(i, t_map, lm_t0[cs_lm[i]], cs_lm[i]));
    ceres::EvaluationCallback* ecb = &cb;
    ecb->PrepareForEvaluation(/*evaluate_jacobians*/ true, /*new_evaluation_point*/ true);
    if (!cb.ok() || !cb.have_jacobians()) return -100;
    int64_t row0[LVX_NUM_FAM + 1];
    if (lvx_get_family_rows(ctx, row0) != LVX_OK) return -101;
    double plane_dummy[3] = {0, 0, 1};
    for (const BlockSpec& sp : specs) {
      LvxRowBlock blk(&cb, sp);
      const auto& sizes = blk.parameter_block_sizes();
      const int nr = sp.num_residuals;
      std::vector<const double*> params(sizes.size());
      std::vector<std::vector<double>> jbuf(sizes.size());
      std::vector<double*> jac(sizes.size());
      for (size_t k = 0; k < sizes.size(); ++k) {
        params[k] = sp.params[k].state_off >= 0 ? st.data() + sp.params[k].state_off : plane_dummy;
        jbuf[k].assign((size_t)nr * sizes[k], 0.0);
        jac[k] = sp.params[k].tangent_off < 0 ? nullptr : jbuf[k].data();
      }
      double r[4];
      if (!blk.Evaluate(params.data(), r, jac.data())) return -103;
      const int64_t row = row0[sp.family] + (int64_t)sp.index * nr;
      for (int a = 0; a < nr; ++a) {
        out_residuals[row + a] = r[a];
        for (size_t k = 0; k < sizes.size(); ++k) if (jac[k]) for (int c = 0; c < sizes[k]; ++c) out_J[(row + a) * (int64_t)n_state + sp.params[k].state_off + c] += jbuf[k][(size_t)a * sizes[k] + c];
      }
    }
    return 0;
  } catch (const std::exception&) { return -1; }
}

}  // extern "C"
