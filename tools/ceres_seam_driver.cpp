// Driver of tools/ceres_seam_bench.py: one evaluation + host rows + scatter of every block through LvxRowBlock::Evaluate (lvi-exc_amd/host/lvx_ceres_shim.hpp,
// compiled against the stand-in interfaces of tests/native/mock_ceres), for either route of the Jacobian rows, timed phase by phase.
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "lvx_ceres_shim.hpp"

using namespace lvx_host;

namespace {
double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
struct Seam {
  std::vector<BlockSpec> specs;
  int skipped = 0;
};
}  // namespace

extern "C" {

void* seam_create(double t0, double dt, int n_knots, int n_landmarks, double readout, unsigned locks, int n_imu, const double* t_imu, int has_prior, double prior_t,
                  int n_surf, const double* surf_t, double t_map, int n_rep, const int* rep_lm, const double* rep_t0, const double* lm_t0, int n_cs, const int* cs_lm) {
  auto* s = new Seam();
  BlockLayout lay(t0, dt, n_knots, n_landmarks, readout, 1e-3, locks);
  auto add = [&](auto make) { try { s->specs.push_back(make()); } catch (const std::exception&) { ++s->skipped; } };   // (spans the reference would reject)
  for (int i = 0; i < n_imu; ++i) add([&] { return lay.Gyro(i, t_imu[i]); });
  if (!(locks & LVX_LOCK_R3)) for (int i = 0; i < n_imu; ++i) add([&] { return lay.Accel(i, t_imu[i]); });
  if (has_prior) add([&] { return lay.Prior(prior_t); });
  for (int i = 0; i < n_surf; ++i) add([&] { return lay.Surfel(i, t_map, surf_t[i]); });
  for (int i = 0; i < n_rep; ++i) add([&] { return lay.Reproj(i, lm_t0[rep_lm[i]], rep_t0[i], rep_lm[i]); });
  for (int i = 0; i < n_cs; ++i) add([&] { return lay.CamSurf(i, t_map, lm_t0[cs_lm[i]], cs_lm[i]); });
  return s;
}
int seam_blocks(void* h, int* skipped) { auto* s = (Seam*)h; *skipped = s->skipped; return (int)s->specs.size(); }
void seam_destroy(void* h) { delete (Seam*)h; }

// one repetition of a route (blocks != 0: LVX_EVAL_JACOBIAN_BLOCKS + records, else LVX_EVAL_JACOBIAN + debug rows):
// out = {evaluate ms (lvx_evaluate: the pass, residuals on the host), exposed copy ms (the rows reach the host), scatter ms (every block's Evaluate), bytes moved D2H}
int seam_run(void* h, lvx_ctx* ctx, const double* state, int blocks, double* out) {
  auto* s = (Seam*)h;
  lvx_layout lo;
  if (lvx_get_layout(ctx, &lo) != LVX_OK) return -1;
  int64_t row0[LVX_NUM_FAM + 1];
  if (lvx_get_family_rows(ctx, row0) != LVX_OK) return -2;
  static std::vector<double> res, vals;
  static std::vector<int32_t> cols;
  res.resize((size_t)lo.n_residuals);
  const uint32_t what = LVX_EVAL_COST | LVX_EVAL_RESIDUALS | (blocks ? LVX_EVAL_JACOBIAN_BLOCKS : LVX_EVAL_JACOBIAN);
  double cost = 0;
  auto t = std::chrono::steady_clock::now();
  if (lvx_evaluate(ctx, state, what, &cost, res.data()) != LVX_OK) return -3;
  out[0] = ms_since(t);
  t = std::chrono::steady_clock::now();
  lvx_jacobian_blocks views[LVX_NUM_FAM];
  double bytes = 0;
  if (blocks) {
    for (int f = 0; f < LVX_NUM_FAM; ++f) {
      if (lvx_get_jacobian_blocks(ctx, f, &views[f]) != LVX_OK) return -4;
      bytes += (double)views[f].n_blocks * (12.0 + 8.0 * views[f].rows_per_block * views[f].width);
    }
  } else {
    cols.resize((size_t)lo.n_residuals * LVX_JAC_WIDTH); vals.resize((size_t)lo.n_residuals * LVX_JAC_WIDTH);
    if (lvx_get_jacobian(ctx, cols.data(), vals.data()) != LVX_OK) return -5;
    bytes = (double)lo.n_residuals * LVX_JAC_WIDTH * 12.0;
  }
  out[1] = ms_since(t);
  out[3] = bytes;
  LvxEvaluationCallback cb(blocks ? JacobianRows::kBlocks : JacobianRows::kDebugRows, lo.n_knots, row0);
  cb.Provide(state, res.data(), blocks ? nullptr : cols.data(), blocks ? nullptr : vals.data(), blocks ? views : nullptr);
  std::vector<std::unique_ptr<LvxRowBlock>> fns;
  fns.reserve(s->specs.size());
  for (const BlockSpec& sp : s->specs) fns.emplace_back(new LvxRowBlock(&cb, sp));   // (built once per Problem in a real host: not timed)
  std::vector<double> jb(64 * 4 * 3);
  std::vector<double*> jac(64);
  std::vector<const double*> par(64, state);
  double r[4], sink = 0;
  t = std::chrono::steady_clock::now();
  for (size_t b = 0; b < fns.size(); ++b) {
    const BlockSpec& sp = s->specs[b];
    const size_t np = sp.params.size();
    if (np > 64) return -6;
    for (size_t k = 0; k < np; ++k) jac[k] = sp.params[k].tangent_off < 0 ? nullptr : jb.data() + 12 * k;
    if (!fns[b]->Evaluate(par.data(), r, jac.data())) return -7;
    sink += jb[0];
  }
  out[2] = ms_since(t);
  static volatile double keep;
  keep = sink;
  return 0;
}

// the pinned device -> host rate of one large hipMemcpyAsync (GB/s, best of 5), measured beside the routes
double seam_pinned_d2h_gbs(size_t bytes) {
  void *d = nullptr, *h = nullptr;
  hipStream_t st = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess || hipStreamCreate(&st) != hipSuccess) return -1.0;
  double best = 0.0;
  for (int r = 0; r < 6; ++r) {
    const auto t = std::chrono::steady_clock::now();
    if (hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1.0;
    const double ms = ms_since(t);
    if (r > 0 && bytes / ms / 1e6 > best) best = bytes / ms / 1e6;
  }
  (void)hipStreamDestroy(st); (void)hipHostFree(h); (void)hipFree(d);
  return best;
}

}  // extern "C"
