// Drives lvx_host::Calibrator (lvi-exc_amd/host/lvx_calibrate.hpp) through Solve #0 and the rotation initialisation on a recorded-sequence stand-in without scans: the
// IMU stream, the scans' header stamps and a LOAM pose file.  Usage: rotinit_demo in.bin out.bin poses.txt
// in.bin (doubles): t0 dt n_knots init_lidar_rotation | camera (12) | state | imu_t | gyro | acc | lm_uv | lm_t0 | scan_stamps, every array with its length in front.
// stdout: one line `stage <name>` per report of Run, and for the "Initialization" report `init <prefix index> <n_poses> <n_pairs> <n_skipped> <ok> q (4) sigma (4)`;
// out.bin: the state Run left.
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
    opt.init_lidar_rotation = next() != 0; opt.solve0_so3_from_gyro = true; opt.refine_iterations = 0; opt.lvi_stage = false; opt.verbose = 0;
    in.camera.rows = (int)next(); in.camera.cols = (int)next(); in.camera.readout = next(); in.camera.fx = next(); in.camera.fy = next(); in.camera.cx = next(); in.camera.cy = next();
    in.camera.k1 = next(); in.camera.k2 = next(); in.camera.p1 = next(); in.camera.p2 = next(); in.camera.k3 = next();
    std::vector<double> state = vec();
    in.imu_t = vec(); in.gyro = vec(); in.acc = vec(); in.lm_uv = vec(); in.lm_t0 = vec(); in.scan_stamps = vec();
    if (!lvx_host::ReadPoseGT(argv[3], &in.loam)) throw std::runtime_error(std::string("cannot read pose file ") + argv[3]);
    lvx_host::Calibrator cal(0, in, opt);
    const std::vector<lvx_host::StageReport> rep = cal.Run(&state);
    for (const lvx_host::StageReport& r : rep) {
      std::printf("stage %s\n", r.name.c_str());
      if (r.name != "Initialization") continue;
      std::printf("init %d %d %d %d %d", r.init_prefix, r.init.n_poses, r.init.n_pairs, r.init.n_skipped, r.init.ok);
      for (int k = 0; k < 4; ++k) std::printf(" %.17g", r.init.q_ItoS_xyzw[k]);
      for (int k = 0; k < 4; ++k) std::printf(" %.17g", r.init.sigma[k]);
      std::printf("\n");
    }
    std::ofstream g(argv[2], std::ios::binary);
    g.write(reinterpret_cast<const char*>(state.data()), (std::streamsize)state.size() * 8);
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
