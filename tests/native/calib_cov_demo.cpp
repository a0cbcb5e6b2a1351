// lvx_host::Calibrator with CalibrateOptions::covariance on a problem file of tests/native/calibrate_demo.cpp's format (tests/test_gpu_pipeline.py::_write): every stage's
// record, raw and as lvx_host::FormatCalibrationUncertainty prints it.  Usage: calib_cov_demo in.bin
// stdout, per stage:
//   STAGE <name> has <0|1> n_free <k> radius <r> free <c ...>
//   SIGMA <22 values, %.17g>
//   EIG <n_free values>
//   VEC0 <n_free values: the eigenvector of the smallest eigenvalue over free>
//   the formatted lines
//   END
#include <cstdio>
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
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin\n", argv[0]); return 2; }
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
    opt.covariance = true;
    opt.verbose = 0;
    lvx_host::Calibrator cal(0, in, opt);
    const auto rep = cal.Run(&state);
    for (const auto& r : rep) {
      const lvx_calib_cov& c = r.covariance;
      std::printf("STAGE %s has %d n_free %d radius %.17g free", r.name.c_str(), r.has_covariance ? 1 : 0, (int)c.n_free, c.radius);
      for (int k = 0; k < c.n_free; ++k) std::printf(" %d", (int)c.free_index[k]);
      std::printf("\nSIGMA");
      for (int k = 0; k < 22; ++k) std::printf(" %.17g", c.sigma[k]);
      std::printf("\nEIG");
      for (int k = 0; k < c.n_free; ++k) std::printf(" %.17g", c.info_eig[k]);
      std::printf("\nVEC0");
      for (int k = 0; k < c.n_free; ++k) std::printf(" %.17g", c.info_vec[k * 22]);
      std::printf("\n%sEND\n", r.has_covariance ? lvx_host::FormatCalibrationUncertainty(c).c_str() : "");
    }
    return 0;
  } catch (const std::range_error& e) { std::fprintf(stderr, "range_error: %s\n", e.what()); return 4;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
