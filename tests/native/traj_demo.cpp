// tests/native/traj_demo.cpp — the trajectory queries through the C++ free functions of lvi-exc_amd/host/lvx_calibrate.hpp (SampleTrajectory, ComparePoses) on a context
// of its own.  Input: a binary file of doubles [N, t0, dt, frame, align, n_times, n_poses | state (7 N + 32) | times | poses: stamp_ns, p (3), q w x y z (4)].  Prints
// every number with 17 significant digits, one line per sample; tests/test_gpu_traj.py compares the text with what the Python binding returns.
#include <cstdio>
#include <vector>

#include "lvx_calibrate.hpp"

int main(int argc, char** argv) {
  using namespace lvx_host;
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  double h[7];
  if (std::fread(h, 8, 7, f) != 7) return 2;
  const int N = (int)h[0], frame = (int)h[3], align = (int)h[4], nt = (int)h[5], np = (int)h[6];
  std::vector<double> state((size_t)7 * N + 32), t((size_t)nt), poses((size_t)np * 8);
  if (std::fread(state.data(), 8, state.size(), f) != state.size() || std::fread(t.data(), 8, t.size(), f) != t.size() || std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 2;
  std::fclose(f);
  lvx_ctx* ctx = nullptr;
  if (lvx_create(&ctx, 0, 0) != LVX_OK) return 3;
  if (lvx_set_spline(ctx, h[1], h[2], N) != LVX_OK) return 3;
  const TrajectorySamples s = SampleTrajectory(ctx, state, frame, t);
  for (size_t i = 0; i < s.t.size(); ++i) {
    std::printf("sample %d", s.valid[i]);
    for (const std::vector<double>* a : {&s.position, &s.velocity, &s.acceleration, &s.angular_velocity}) if (!a->empty()) for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*a)[3 * i + k]);
    for (int k = 0; k < 4; ++k) std::printf(" %.17g", s.orientation_xyzw[4 * i + k]);
    std::printf("\n");
  }
  std::vector<PoseStamped> ps((size_t)np);
  for (int i = 0; i < np; ++i) {
    const double* r = &poses[(size_t)8 * i];
    ps[i].stamp_ns = (int64_t)r[0]; ps[i].p = {r[1], r[2], r[3]}; ps[i].q_wxyz = {r[4], r[5], r[6], r[7]};
  }
  const PoseComparison c = ComparePoses(ctx, state, frame, ps, align);
  std::printf("errors %d %d\n", c.errors.n, c.errors.n_valid);
  for (const lvx_err_summary* e : {&c.errors.abs_trans, &c.errors.abs_rot, &c.errors.rel_trans, &c.errors.rel_rot}) std::printf("summary %.17g %.17g %.17g %d %d\n", e->rmse, e->mean, e->max, e->argmax, e->n);
  for (int i = 0; i < np; ++i) std::printf("abs %.17g %.17g\n", c.abs_trans[i], c.abs_rot[i]);
  lvx_destroy(ctx);
  return 0;
}
