// Drives lvx_host::Calibrator (lvi-exc_amd/host/lvx_calibrate.hpp) with CalibrateOptions::lidar_odometry and NO pose file: Solve #0, the LiDAR odometry over the raw scans
// (RunLidarOdometry), the first map from its poses and one surfel solve.  Usage: odometry_demo in.bin scans.bin out.bin
// in.bin (doubles): t0 dt n_knots H W | camera (12) | state | imu_t | gyro | acc | lm_uv | lm_t0 | scan_stamps, every array with its length in front;
// scans.bin: the raw scans [n_scans][H * W] lvx_point_xyzit.
// stdout: `stage <name>` per report of Run, `keys <n_key>`, `firstmap <flag per scan>` (the key scans of the first-map association);
// out.bin (doubles): pose16 [n][16] as Calibrator::odometry() holds them | per scan is_key, n_src, iterations | per scan stamp_ns, p (3), q w x y z of odometry().loam.all.
#include <cstdio>
#include <fstream>

#include "lvx_calibrate.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s in.bin scans.bin out.bin\n", argv[0]); return 2; }
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
    in.t0 = next(); in.dt = next(); in.n_knots = (int)next(); in.H = (int)next(); in.W = (int)next();
    opt.lidar_odometry = true; opt.solve0_so3_from_gyro = true; opt.refine_iterations = 1; opt.lvi_stage = false; opt.verbose = 0;
    in.camera.rows = (int)next(); in.camera.cols = (int)next(); in.camera.readout = next(); in.camera.fx = next(); in.camera.fy = next(); in.camera.cx = next(); in.camera.cy = next();
    in.camera.k1 = next(); in.camera.k2 = next(); in.camera.p1 = next(); in.camera.p2 = next(); in.camera.k3 = next();
    std::vector<double> state = vec();
    in.imu_t = vec(); in.gyro = vec(); in.acc = vec(); in.lm_uv = vec(); in.lm_t0 = vec(); in.scan_stamps = vec();
    in.map_time = in.scan_stamps.empty() ? 0.0 : in.scan_stamps.front();
    std::ifstream g(argv[2], std::ios::binary);
    if (!g) throw std::runtime_error(std::string("cannot open ") + argv[2]);
    const size_t HW = (size_t)in.H * in.W;
    in.scans.assign(in.scan_stamps.size(), std::vector<lvx_point_xyzit>(HW));
    for (auto& s : in.scans) g.read(reinterpret_cast<char*>(s.data()), (std::streamsize)(HW * sizeof(lvx_point_xyzit)));
    if (!g) throw std::runtime_error("scans.bin is too short");
    lvx_host::Calibrator cal(0, in, opt);
    for (const lvx_host::StageReport& r : cal.Run(&state)) std::printf("stage %s\n", r.name.c_str());
    const lvx_host::LidarOdometry& od = cal.odometry();
    std::printf("keys %d\nfirstmap", (int)od.n_key);
    for (int32_t k : cal.key_scans()) std::printf(" %d", (int)k);
    std::printf("\n");
    std::vector<double> out = od.pose16;
    for (const lvx_odom_step& s : od.steps) { out.push_back(s.is_key); out.push_back(s.n_src); out.push_back(s.iterations); }
    for (const lvx_host::PoseStamped& ps : od.loam.all) {
      out.push_back((double)ps.stamp_ns);
      out.insert(out.end(), ps.p.begin(), ps.p.end()); out.insert(out.end(), ps.q_wxyz.begin(), ps.q_wxyz.end());
    }
    std::ofstream h(argv[3], std::ios::binary);
    h.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size() * 8);
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
