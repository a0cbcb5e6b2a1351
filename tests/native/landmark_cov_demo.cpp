// lvx_host::Calibrator with CalibrateOptions::landmark_covariance on a problem file of tests/native/calibrate_demo.cpp's format (tests/test_gpu_pipeline.py::_write):
// every stage's landmark sigmas, and the final state.  Usage: landmark_cov_demo in.bin <0|1>     (0: the option off)
// stdout, per stage:
//   STAGE <name> has <0|1> n <landmarks> n_valid <k> radius <r>
//   SIGMA_REL <the smallest and the largest sigma_rho / |rho| over the valid landmarks, %.17g>
//   the line of lvx_host::FormatLandmarkUncertainty
//   END
// then   STATE <the final state as hex doubles>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "lvx_calibrate.hpp"

static std::vector<double> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  const std::streamsize n = f.tellg(); f.seekg(0);
  std::vector<double> v((size_t)n / 8);
  f.read(reinterpret_cast<char*>(v.data()), n);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s problem.bin <0|1>\n", argv[0]); return 2; }
  try {
    const std::vector<double> d = read_all(argv[1]);
    size_t o = 0;
    auto next = [&]() { return d.at(o++); };
    auto vec = [&]() { const size_t n = (size_t)next(); std::vector<double> v(d.begin() + o, d.begin() + o + n); o += n; return v; };
    lvx_host::CalibrateInput in;
    lvx_host::CalibrateOptions opt;
    in.t0 = next(); in.dt = next(); in.n_knots = (int)next(); in.map_time = next(); in.H = (int)next(); in.W = (int)next();
    const int n_scans = (int)next();
    opt.refine_iterations = (int)next(); opt.lvi_stage = next() != 0; opt.camera_surfel_stage = next() != 0; opt.downsample_step = (int)next(); opt.solve0_so3_from_gyro = next() != 0;
    in.camera.rows = (int)next(); in.camera.cols = (int)next(); in.camera.readout = next(); in.camera.fx = next(); in.camera.fy = next(); in.camera.cx = next(); in.camera.cy = next();
    in.camera.k1 = next(); in.camera.k2 = next(); in.camera.p1 = next(); in.camera.p2 = next(); in.camera.k3 = next();
    std::vector<double> state = vec();
    in.imu_t = vec(); in.gyro = vec(); in.acc = vec();
    in.lm_uv = vec(); in.lm_t0 = vec();
    { const std::vector<double> ol = vec(); in.obs_landmark.assign(ol.begin(), ol.end()); }
    in.obs_uv = vec(); in.obs_t0 = vec();
    for (int s = 0; s < n_scans; ++s) {
      const std::vector<double> xyz = vec(), ts = vec();
      std::vector<lvx_point_xyzit> pts((size_t)in.H * in.W);
      for (size_t i = 0; i < pts.size(); ++i) { std::memset(&pts[i], 0, sizeof(pts[i])); pts[i].x = (float)xyz[3 * i]; pts[i].y = (float)xyz[3 * i + 1]; pts[i].z = (float)xyz[3 * i + 2]; pts[i].timestamp = ts[i]; }
      in.scans.push_back(std::move(pts));
    }
    opt.landmark_covariance = std::atoi(argv[2]) != 0;
    opt.verbose = 0;
    lvx_host::Calibrator cal(0, in, opt);
    const auto rep = cal.Run(&state);
    for (const auto& r : rep) {
      const lvx_host::LandmarkUncertainty& u = r.landmark_sigma;
      int nv = 0;
      double lo = 1e300, hi = -1e300;
      for (size_t i = 0; i < u.valid.size(); ++i) if (u.valid[i]) { ++nv; const double rel = u.sigma_rho[i] / std::fabs(u.rho[i]); lo = std::min(lo, rel); hi = std::max(hi, rel); }
      std::printf("STAGE %s has %d n %d n_valid %d radius %.17g\nSIGMA_REL %.17g %.17g\n%sEND\n", r.name.c_str(), r.has_landmark_sigma ? 1 : 0, (int)u.valid.size(), nv, u.radius,
                  nv ? lo : 0.0, nv ? hi : 0.0, r.has_landmark_sigma ? lvx_host::FormatLandmarkUncertainty(u).c_str() : "");
    }
    std::printf("STATE");
    for (double v : state) std::printf(" %a", v);
    std::printf("\n");
    return 0;
  } catch (const std::range_error& e) { std::fprintf(stderr, "range_error: %s\n", e.what()); return 4;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
