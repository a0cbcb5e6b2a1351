// Drives lvx_host::Calibrator::RunLidarPoses (lvi-exc_amd/host/lvx_calibrate.hpp) — Solve #0, then trajInitFromLidarPose on the LOAM pose file — on an IMU stream
// and a pose file, no scans.  Usage: lidarpos_demo in.bin out.bin poses.txt
// in.bin (doubles): t0 dt n_knots | state | imu_t | gyro | acc, every array with its length in front.
// stdout per stage: `stage <name> <iterations> <termination> <n_lidar_poses> <outliers before> <outliers after>`, then `accepted <0/1 ...>` and `cost <%.17g ...>`;
// out.bin: the state after Solve #0, then the final state.
#include <cstdio>
#include <fstream>

#include "lvx_calibrate.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s in.bin out.bin poses.txt\n", argv[0]); return 2; }
  try {
    std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
    const std::streamsize bytes = f.tellg(); f.seekg(0);
    std::vector<double> d((size_t)bytes / 8);
    f.read(reinterpret_cast<char*>(d.data()), bytes);
    size_t o = 0;
    auto next = [&]() { return d.at(o++); };
    auto vec = [&]() { const size_t n = (size_t)next(); std::vector<double> v(d.begin() + o, d.begin() + o + n); o += n; return v; };
    lvx_host::CalibrateInput in;
    lvx_host::CalibrateOptions opt;
    in.t0 = next(); in.dt = next(); in.n_knots = (int)next();
    opt.verbose = 0; opt.keep_history = true; opt.error_statistics = true;
    in.camera.rows = 480; in.camera.cols = 640; in.camera.readout = 0.0; in.camera.fx = in.camera.fy = 500; in.camera.cx = 320; in.camera.cy = 240;
    std::vector<double> state = vec();
    in.imu_t = vec(); in.gyro = vec(); in.acc = vec();
    if (!lvx_host::ReadPoseGT(argv[3], &in.loam)) throw std::runtime_error(std::string("cannot read pose file ") + argv[3]);
    lvx_host::Calibrator cal(0, in, opt);
    const std::vector<lvx_host::StageReport> rep = cal.RunLidarPoses(&state);
    std::ofstream g(argv[2], std::ios::binary);
    for (const lvx_host::StageReport& r : rep) {
      std::printf("stage %s %d %d %d %lld %lld\naccepted", r.name.c_str(), r.lm.iterations, r.lm.termination, r.n_lidar_poses, (long long)r.lidar_pos_before.n_outliers, (long long)r.lidar_pos_after.n_outliers);
      for (int a : r.accepted) std::printf(" %d", a);
      std::printf("\ncost");
      for (double c : r.cost_history) std::printf(" %.17g", c);
      std::printf("\n");
    }
    if (rep.size() != 2) throw std::runtime_error("expected two stage reports");
    g.write(reinterpret_cast<const char*>(rep[1].state_in.data()), (std::streamsize)rep[1].state_in.size() * 8);
    g.write(reinterpret_cast<const char*>(state.data()), (std::streamsize)state.size() * 8);
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
