// tests/native/error_stats_demo.cpp — TEST-ONLY driver of the host side of the error statistics (lvi-exc_amd/host: FormatErrorStatistics,
// TrajectoryEstimator::ErrorStatistics, CalibrateOptions::error_statistics).  Modes:
//   format                          no device: a hand-filled lvx_error_stats through FormatErrorStatistics, the text on stdout
//   estimator problem.bin out.bin   the problem of tests/test_gpu_error_stats.py built measurement by measurement, ErrorStatistics() at its state: out.bin = the
//                                   lvx_error_stats bytes; the formatted lines on stdout
//   calibrate sequence.bin out.bin  the file format of calibrate_demo; out.bin (doubles) = n_stages | per stage: has_stats, cost before, cost after, lm.initial_cost,
//                                   lm.final_cost, blocks before, blocks evaluated before
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "lvx_calibrate.hpp"
#include "lvx_estimator.hpp"

static std::vector<double> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  const std::streamsize n = f.tellg(); f.seekg(0);
  std::vector<double> v((size_t)n / 8);
  f.read(reinterpret_cast<char*>(v.data()), n);
  return v;
}

static int run_format() {
  lvx_error_stats st{};
  auto fill = [](lvx_family_stats& f, int64_t n, double a, double b, double c, bool sgn) {
    f.n_blocks = n; f.n_evaluated = n;
    const double v[3] = {a, b, c};
    for (int k = 0; k < 3; ++k) { (sgn ? f.sum : f.sum_abs)[k] = v[k] * (double)n; }
  };
  fill(st.fam[LVX_FAM_GYRO], 4000, 0.00123456789, 0.5, 12.25, false);
  fill(st.fam[LVX_FAM_ACCEL], 4000, 0.25, 0.0625, 1e-7, false);
  fill(st.fam[LVX_FAM_SURFEL], 123456, 0.015625, 0, 0, false);
  fill(st.fam[LVX_FAM_REPROJ], 200, -0.75, 1.5, 0, true);
  st.fam[LVX_FAM_REPROJ].sum_abs[0] = 1e9;   // the camera line must not read the absolute sums
  std::cout << lvx_host::FormatErrorStatistics("Before optimization", st);
  lvx_error_stats none{};
  none.fam[LVX_FAM_GYRO].n_blocks = 8; none.fam[LVX_FAM_GYRO].n_evaluated = 8; none.fam[LVX_FAM_GYRO].sum_abs[1] = 16.0;
  none.fam[LVX_FAM_REPROJ].n_blocks = 2; none.fam[LVX_FAM_REPROJ].n_evaluated = 2; none.fam[LVX_FAM_REPROJ].sum[0] = 3.0; none.fam[LVX_FAM_REPROJ].sum[1] = -1.0;
  std::cout << lvx_host::FormatErrorStatistics("After optimization", none, 5.0);
  return 0;
}

static int run_estimator(const char* pin, const char* pout) {
  const std::vector<double> d = read_all(pin);
  size_t o = 0;
  auto next = [&]() { return d.at(o++); };
  auto vec = [&]() { const size_t n = (size_t)next(); std::vector<double> v(d.begin() + o, d.begin() + o + n); o += n; return v; };
  const double t0 = next(), dt = next(); const int n_knots = (int)next(); const unsigned locks = (unsigned)next();
  lvx_pinhole cam{};
  cam.rows = (int)next(); cam.cols = (int)next(); cam.readout = next(); cam.fx = next(); cam.fy = next(); cam.cx = next(); cam.cy = next();
  cam.k1 = next(); cam.k2 = next(); cam.p1 = next(); cam.p2 = next(); cam.k3 = next();
  const double w_gyro = next(), w_acc = next(), t_map = next(), huber_surf = next(), w_surf = next(), huber_rep = next(), w_rep = next(), huber_cs = next(), w_cs = next();
  const double prior_t = next(), pq0 = next(), pq1 = next(), pq2 = next(), pq3 = next(), prior_w = next();
  std::vector<double> state = vec(), t_imu = vec(), gyro = vec(), acc = vec(), planes = vec(), surf_pt = vec(), surf_t = vec(), surf_plane = vec(),
                      lm_uv = vec(), lm_t0 = vec(), rep_lm = vec(), rep_uv = vec(), rep_t0 = vec(), cs_lm = vec(), cs_plane = vec();
  lvx_host::TrajectoryEstimator est(0, t0, dt, n_knots, &state);
  est.SetCamera(cam);
  est.Lock(locks);
  for (size_t i = 0; i < t_imu.size(); ++i) {
    est.AddMeasurement(lvx_host::GyroscopeMeasurement{t_imu[i], {gyro[3 * i], gyro[3 * i + 1], gyro[3 * i + 2]}}, w_gyro);
    est.AddMeasurement(lvx_host::AccelerometerMeasurement{t_imu[i], {acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]}}, w_acc);
  }
  est.AddMeasurement(lvx_host::OrientationMeasurement{prior_t, {pq0, pq1, pq2, pq3}, prior_w});
  std::vector<std::array<double, 3>> pl(planes.size() / 3);
  for (size_t i = 0; i < pl.size(); ++i) pl[i] = {planes[3 * i], planes[3 * i + 1], planes[3 * i + 2]};
  est.SetPlanes(pl);
  for (size_t i = 0; i < surf_t.size(); ++i)
    est.AddMeasurement(lvx_host::LiDARSurfelPoint{{surf_pt[3 * i], surf_pt[3 * i + 1], surf_pt[3 * i + 2]}, (int32_t)surf_plane[i], surf_t[i]}, t_map, huber_surf, w_surf);
  std::vector<std::array<double, 2>> uv(lm_t0.size());
  for (size_t i = 0; i < uv.size(); ++i) uv[i] = {lm_uv[2 * i], lm_uv[2 * i + 1]};
  est.SetLandmarks(uv, lm_t0);
  for (size_t i = 0; i < rep_t0.size(); ++i)
    est.AddMeasurement(lvx_host::StaticRsCameraMeasurement{(int32_t)rep_lm[i], {rep_uv[2 * i], rep_uv[2 * i + 1]}, rep_t0[i]}, huber_rep, w_rep);
  for (size_t i = 0; i < cs_lm.size(); ++i) est.AddMeasurement(lvx_host::CameraSurfelLandmark{(int32_t)cs_lm[i], (int32_t)cs_plane[i]}, t_map, huber_cs, w_cs);
  const lvx_error_stats st = est.ErrorStatistics();
  std::cout << lvx_host::FormatErrorStatistics("Before optimization", st, w_rep);
  std::ofstream f(pout, std::ios::binary);
  f.write(reinterpret_cast<const char*>(&st), sizeof(st));
  return 0;
}

static int run_calibrate(const char* pin, const char* pout) {
  const std::vector<double> d = read_all(pin);
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
  opt.error_statistics = true; opt.verbose = 0;
  lvx_host::Calibrator cal(0, in, opt);
  const auto rep = cal.Run(&state);
  std::vector<double> out;
  out.push_back((double)rep.size());
  for (const auto& r : rep) {
    int64_t nb = 0, ne = 0;
    for (int f = 0; f < LVX_NUM_FAM; ++f) { nb += r.stats_before.fam[f].n_blocks; ne += r.stats_before.fam[f].n_evaluated; }
    out.push_back(r.has_stats ? 1.0 : 0.0); out.push_back(r.stats_before.cost); out.push_back(r.stats_after.cost); out.push_back(r.lm.initial_cost); out.push_back(r.lm.final_cost);
    out.push_back((double)nb); out.push_back((double)ne);
    std::cout << r.name << "\n" << lvx_host::FormatErrorStatistics("Before optimization", r.stats_before) << lvx_host::FormatErrorStatistics("After optimization", r.stats_after);
  }
  std::ofstream f(pout, std::ios::binary);
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size() * 8);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "format")) return run_format();
    if (argc >= 4 && !std::strcmp(argv[1], "estimator")) return run_estimator(argv[2], argv[3]);
    if (argc >= 4 && !std::strcmp(argv[1], "calibrate")) return run_calibrate(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s format | estimator problem.bin out.bin | calibrate sequence.bin out.bin\n", argv[0]);
    return 2;
  } catch (const std::range_error& e) { std::fprintf(stderr, "range_error: %s\n", e.what()); return 4;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
