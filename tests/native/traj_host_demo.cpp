// The host-side pieces of the trajectory queries in lvi-exc_amd/host/lvx_calibrate.hpp that need no device: PublishTrajectory's sampling loop (SampleTimes) and the LOAM
// pose file writer (WritePoseFile) read back by ReadPoseGT.  Prints what tests/test_traj_host.py compares.
#include <cstdio>

#include "lvx_calibrate.hpp"

int main(int argc, char** argv) {
  using namespace lvx_host;
  if (argc < 2) return 2;
  const double cases[4][3] = {{100.0, 101.5, 0.05}, {100.0, 100.5, 0.07}, {100.0, 100.0, 0.05}, {0.1, 0.1 + 3 * 0.3, 0.3}};
  for (const auto& c : cases) {
    const std::vector<double> t = SampleTimes(c[0], c[1], c[2]);
    std::printf("times %zu %.17g %.17g\n", t.size(), t.empty() ? 0.0 : t.front(), t.empty() ? 0.0 : t.back());
  }
  // doubles that need all 17 digits, a non-unit quaternion, a negative zero, a denormal-scale value
  const std::vector<int64_t> stamps = {1403636579763555584LL, 1403636579813555456LL, 1403636580763555584LL};
  const std::vector<double> p = {0.1, -1.0 / 3.0, 2.0 / 7.0, 1e-300, 123456.789012345678, -0.0, 3.141592653589793, 2.718281828459045, 1.4142135623730951};
  const std::vector<double> q = {0.1, 0.2, 0.3, 0.9, -0.5, 0.5, -0.5, 0.5, 1.0 / 3.0, 2.0 / 3.0, 1e-17, 0.7071067811865476};
  if (!WritePoseFile(argv[1], stamps, p, q)) return 1;
  LoamPoses lp;
  if (!ReadPoseGT(argv[1], &lp)) return 1;
  bool same = lp.all.size() == stamps.size();
  for (size_t i = 0; same && i < stamps.size(); ++i) {
    same = lp.all[i].stamp_ns == stamps[i];
    for (int k = 0; k < 3; ++k) same = same && lp.all[i].p[k] == p[3 * i + k];
    for (int k = 0; k < 3; ++k) same = same && lp.all[i].q_wxyz[1 + k] == q[4 * i + k];
    same = same && lp.all[i].q_wxyz[0] == q[4 * i + 3];
  }
  std::printf("roundtrip %zu %d\n", lp.all.size(), same ? 1 : 0);
  if (WritePoseFile(argv[1], stamps, p, p)) return 1;   // sizes that do not match are refused
  return 0;
}
