// lvx_host::Calibrator::ProjectionUncertainty on a problem file of tests/native/calibrate_demo.cpp's format (tests/test_gpu_pipeline.py::_write): the stages run, the
// normal equations are evaluated at the final state, and every `step`-th point of the map cloud is carried into two images (1 s and 3 s behind the map time) with
// its pixel covariance.
// Usage: projcov_demo in.bin step
// stdout:
//   POINTS n <points> n_projected <k> radius <r>
//   the line of lvx_host::FormatProjectionUncertainty
//   P <index in map> <image> <u v> <sigma u v> <sigma_max>     (hex doubles), one per projected point
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
  if (argc < 3) { std::fprintf(stderr, "usage: %s problem.bin step\n", argv[0]); return 2; }
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
    opt.verbose = 0;
    lvx_host::Calibrator cal(0, in, opt);
    cal.Run(&state);
    double cost = 0;
    lvx_host::ThrowOnError(cal.context(), lvx_evaluate(cal.context(), state.data(), LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, &cost, nullptr));
    std::vector<int32_t> index;
    const lvx_host::PixelUncertainty u = cal.ProjectionUncertainty({in.map_time + 1.0, in.map_time + 3.0}, &index, std::atoi(argv[2]));
    size_t np = 0;
    for (uint8_t s : u.status) np += s == 2;
    std::printf("POINTS n %zu n_projected %zu radius %.17g\n%s", u.status.size(), np, u.radius, lvx_host::FormatProjectionUncertainty(u).c_str());
    for (size_t i = 0; i < u.status.size(); ++i)
      if (u.status[i] == 2) std::printf("P %d %d %a %a %a %a %a\n", index[i], u.image[i], u.uv[2 * i], u.uv[2 * i + 1], u.sigma[2 * i], u.sigma[2 * i + 1], u.sigma_max[i]);
    return 0;
  } catch (const std::range_error& e) { std::fprintf(stderr, "range_error: %s\n", e.what()); return 4;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
