// lvx_host::Calibrator::MapPointCovariance on a problem file of tests/native/calibrate_demo.cpp's format (tests/test_gpu_pipeline.py::_write): the stages run, the normal
// equations are evaluated at the final state, and every `step`-th point of raw scan `scan` is carried into the map with its covariance.
// Usage: ptcov_demo in.bin scan step
// stdout:
//   POINTS n <points> n_valid <k> radius <r>
//   the line of lvx_host::FormatMapPointUncertainty
//   P <index in scan> <valid> <p_M x y z> <sigma x y z> <sigma_max>     (hex doubles), one per point
//   REVERSED <1 when the same points in reverse order through lvx_host::MapPointCovariance return the same bits>
//   STATE <the final state as hex doubles>
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
  if (argc < 4) { std::fprintf(stderr, "usage: %s problem.bin scan step\n", argv[0]); return 2; }
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
    const lvx_host::MapPointUncertainty u = cal.MapPointCovariance(std::atoi(argv[2]), &index, std::atoi(argv[3]));
    size_t nv = 0;
    for (uint8_t v : u.valid) nv += v;
    std::printf("POINTS n %zu n_valid %zu radius %.17g\n%s", u.valid.size(), nv, u.radius, lvx_host::FormatMapPointUncertainty(u).c_str());
    for (size_t i = 0; i < u.valid.size(); ++i)
      std::printf("P %d %d %a %a %a %a %a %a %a\n", index[i], (int)u.valid[i], u.point[3 * i], u.point[3 * i + 1], u.point[3 * i + 2], u.sigma[3 * i], u.sigma[3 * i + 1], u.sigma[3 * i + 2], u.sigma_max[i]);
    // the same points in reverse order, through the free function
    const size_t n = index.size();
    const std::vector<lvx_point_xyzit>& raw = in.scans.at((size_t)std::atoi(argv[2]));
    std::vector<double> pts(3 * n), t(n);
    for (size_t i = 0; i < n; ++i) { const lvx_point_xyzit& p = raw[(size_t)index[n - 1 - i]]; pts[3 * i] = p.x; pts[3 * i + 1] = p.y; pts[3 * i + 2] = p.z; t[i] = p.timestamp; }
    const lvx_host::MapPointUncertainty v = lvx_host::MapPointCovariance(cal.context(), pts, t);
    bool same = v.valid.size() == n;
    for (size_t i = 0; same && i < n; ++i)
      same = v.valid[i] == u.valid[n - 1 - i] && std::memcmp(&v.cov[9 * i], &u.cov[9 * (n - 1 - i)], 72) == 0 && std::memcmp(&v.point[3 * i], &u.point[3 * (n - 1 - i)], 24) == 0 &&
             std::memcmp(&v.sigma_max[i], &u.sigma_max[n - 1 - i], 8) == 0;
    std::printf("REVERSED %d\nSTATE", same ? 1 : 0);
    for (double x : state) std::printf(" %a", x);
    std::printf("\n");
    return 0;
  } catch (const std::range_error& e) { std::fprintf(stderr, "range_error: %s\n", e.what()); return 4;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
